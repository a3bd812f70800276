"""The KPlanes encoding restated in plain numpy: per level the K = D (D - 1) / 2 dense 2-D grids over the axis pairs (a, b), a < b, each a
2-D DenseGrid level with Linear interpolation, multiplied or summed per feature.  W is the working precision: float64 is the reference
(R64); float32 with one rounding to the output precision is Rh, the yardstick for what fp32 arithmetic can deliver.  The function is DEFINED
on the grid's pos_fract, a float32 fmaf: cell and fraction come from that float in every working precision (fract=F64 lifts this, for
finite differences).  Each plane value is a chain of fused multiply-adds; float32 restates them with one rounding each."""
import ctypes
import ctypes.util

import numpy as np

F32, F64 = np.float32, np.float64
LIBM = ctypes.CDLL(ctypes.util.find_library("m"))  # the level scales are the C library's floats: log2f(1.02) is not the rounded log2
for function in (LIBM.exp2f, LIBM.log2f):
    function.restype, function.argtypes = ctypes.c_float, [ctypes.c_float]


def fma(a, b, c):
    """a * b + c rounded once to a's type (the product of two float32 is exact in float64)"""
    return (a.astype(F64) * b + c).astype(a.dtype)


class KPlanes:
    def __init__(self, n_dims, cfg, fract=F32):
        self.fract = fract
        self.D, self.L, self.F = n_dims, cfg.get("n_levels", 4), cfg.get("n_features_per_level", 2)
        self.product = cfg.get("reduction", "Product").lower() == "product"
        self.planes = [(a, b) for a in range(n_dims) for b in range(a + 1, n_dims)]
        self.K = len(self.planes)
        log2_scale = F32(LIBM.log2f(F32(cfg.get("per_level_scale", 2.0))))  # exp2f(l * log2f(per_level_scale)) * base_resolution - 1, as the grid
        self.scales = [F32(F32(F32(LIBM.exp2f(F32(F32(l) * log2_scale))) * F32(cfg.get("base_resolution", 64))) - F32(1)) for l in range(self.L)]
        self.R = [int(np.ceil(s)) + 1 for s in self.scales]
        self.entries = [(r * r + 7) // 8 * 8 for r in self.R]
        self.offsets = np.concatenate([[0], np.cumsum([self.K * e for e in self.entries])])  # in entries
        self.n_output_dims, self.n_params = self.L * self.F, int(self.offsets[-1]) * self.F

    def cell(self, x, level, W=F64):
        """pos_fract: -> cell [n, D] int64, fraction [n, D] W"""
        p = (x.astype(F64) * F64(self.scales[level]) + 0.5).astype(self.fract).astype(W)
        cell = np.floor(p)
        return cell.astype(np.int64), p - cell

    def corners(self, cell, pos, k, level):
        """plane k -> entries [n, 4] (within the plane) and weights [n, 4] of its corners, in the grid's corner order"""
        (a, b), R, one = self.planes[k], self.R[level], pos.dtype.type(1)
        idx = np.stack([((cell[:, a] + (c & 1)) + (cell[:, b] + (c >> 1)) * R) % 2 ** 32 % self.entries[level] for c in range(4)], axis=1)
        w = np.stack([(pos[:, a] if c & 1 else one - pos[:, a]) * (pos[:, b] if c & 2 else one - pos[:, b]) for c in range(4)], axis=1)
        return idx, w

    def table(self, params, level, W):
        return params.astype(W)[self.offsets[level] * self.F:self.offsets[level + 1] * self.F].reshape(self.K, self.entries[level], self.F)

    def level_terms(self, x, params, level, W=F64):
        """per plane: (entries [n, 4], weights [n, 4], corner values [n, 4, F], value P [n, F], majorant sum|w v| [n, F])"""
        cell, pos = self.cell(x, level, W)
        out = []
        for k in range(self.K):
            idx, w = self.corners(cell, pos, k, level)
            v = self.table(params, level, W)[k][idx] if params is not None else np.zeros(idx.shape + (self.F,), W)
            P, M = np.zeros((x.shape[0], self.F), W), np.zeros((x.shape[0], self.F), W)
            for c in range(4):
                P, M = fma(w[:, c, None], v[:, c], P), M + np.abs(w[:, c, None] * v[:, c])
            out.append((idx, w, v, P, M))
        return out, pos

    def reduce_others(self, values, k):
        """the factor the other planes put on plane k's gradient: their product, or 1 for Sum"""
        other = np.ones_like(values[0])
        for q in range(self.K):
            if self.product and q != k:
                other = other * values[q]
        return other

    def forward(self, x, params, W=F64, out_dtype=None):
        """[n, L*F]; params: the values the kernel reads (half or float)"""
        y = np.zeros((x.shape[0], self.L, self.F), W)
        for l in range(self.L):
            terms, _ = self.level_terms(x, params, l, W)
            acc = terms[0][3]
            for k in range(1, self.K):
                acc = acc * terms[k][3] if self.product else acc + terms[k][3]
            y[:, l] = acc
        y = y.reshape(x.shape[0], -1)
        return y if out_dtype is None else y.astype(out_dtype)

    def min_fraction(self, x):
        """[n]: the smallest distance of a fraction from 0 and 1 over all levels and dimensions (0 on a cell boundary, where dy/dx jumps)"""
        return np.min([np.minimum(pos, 1 - pos).min(axis=1) for pos in (self.cell(x, l)[1] for l in range(self.L))], axis=0)

    def dy_dx(self, x, params, W=F64):
        """[n, L*F, D], analytic"""
        out = np.zeros((x.shape[0], self.L, self.F, self.D), W)
        for l in range(self.L):
            terms, pos = self.level_terms(x, params, l, W)
            for k, (a, b) in enumerate(self.planes):
                v, other = terms[k][2], self.reduce_others([t[3] for t in terms], k) * W(self.scales[l])
                pa, pb = pos[:, a, None], pos[:, b, None]
                out[:, l, :, a] += other * ((1 - pb) * (v[:, 1] - v[:, 0]) + pb * (v[:, 3] - v[:, 2]))
                out[:, l, :, b] += other * ((1 - pa) * (v[:, 2] - v[:, 0]) + pa * (v[:, 3] - v[:, 1]))
        return out.reshape(x.shape[0], -1, self.D)

    def backward_input(self, x, params, dy, W=F64):
        """dL/dx [n, D] for dL/dy [n, >= L*F] (padding columns are ignored)"""
        return np.einsum("nk,nkd->nd", dy[:, :self.n_output_dims].astype(W), self.dy_dx(x, params, W))

    def param_gradient_terms(self, x, params, dy, W=F64, each=None):
        """per parameter, summed in fp64: S the sum of the contributions dL/dy_f * [product of the other planes' values] * w_corner formed in W
        (each: rounded to that type first, as the half kernel rounds them), A the sum of their magnitudes, Abar the same with every plane
        value replaced by its majorant sum|w v|, k their count"""
        S, A, Abar, K = (np.zeros((self.offsets[-1], self.F), t) for t in (F64, F64, F64, np.int64))
        g = dy[:, :self.n_output_dims].astype(W).reshape(x.shape[0], self.L, self.F)
        for l in range(self.L):
            terms, _ = self.level_terms(x, params if self.product else None, l, W)
            for k in range(self.K):
                idx, w = terms[k][0] + self.offsets[l] + k * self.entries[l], terms[k][1]
                G, Gbar = g[:, l] * self.reduce_others([t[3] for t in terms], k), np.abs(g[:, l]) * self.reduce_others([t[4] for t in terms], k)
                for c in range(4):
                    contribution = G * w[:, c, None]
                    contribution = (contribution if each is None else contribution.astype(each)).astype(F64)
                    np.add.at(S, idx[:, c], contribution)
                    np.add.at(A, idx[:, c], np.abs(contribution))
                    np.add.at(Abar, idx[:, c], (Gbar * w[:, c, None]).astype(F64))
                    np.add.at(K, idx[:, c], 1)
        return S.ravel(), A.ravel(), Abar.ravel(), K.ravel()
