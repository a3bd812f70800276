"""The TensoRF encoding restated in plain numpy.  A level's output is one mode (CP) or three (VM); a mode is a product of FACTORS: VM mode k
is the plane over KPlanes' axis pair k times the line over the remaining axis 2 - k, CP's single mode the D lines, left to right.  A factor's
value is a chain of fused multiply-adds over its taps (a plane's four corners in the grid's order, a line's two entries: fma(w, v1, (1 - w) v0)
is that chain on two taps).  W is the working precision as in kplanes_reference.py, whose pos_fract and plane corners these are."""
import numpy as np

from kplanes_reference import F32, F64, LIBM, KPlanes, fma


class TensoRF:
    cell, corners, min_fraction = KPlanes.cell, KPlanes.corners, KPlanes.min_fraction

    def __init__(self, n_dims, cfg, fract=F32):
        self.fract, self.D, self.L, self.F = fract, n_dims, cfg.get("n_levels", 1), cfg.get("n_components", 16)
        self.cp = cfg.get("decomposition", "VM").upper() == "CP"
        self.planes, self.n_lines, self.n_modes = [(0, 1), (0, 2), (1, 2)], (n_dims if self.cp else 3), (1 if self.cp else 3)
        log2_scale = F32(LIBM.log2f(F32(cfg.get("per_level_scale", 2.0))))
        self.scales = [F32(F32(F32(LIBM.exp2f(F32(F32(l) * log2_scale))) * F32(cfg.get("base_resolution", 128))) - F32(1)) for l in range(self.L)]
        self.R = [int(np.ceil(s)) + 1 for s in self.scales]
        self.entries = [(r * r + 7) // 8 * 8 for r in self.R]  # of a plane
        self.line_entries = [(r + 7) // 8 * 8 for r in self.R]
        self.offsets = np.concatenate([[0], np.cumsum([self.n_lines * n if self.cp else 3 * (e + n) for e, n in zip(self.entries, self.line_entries)])])  # in entries
        self.n_output_dims, self.n_params = self.L * self.n_modes * self.F, int(self.offsets[-1]) * self.F

    def factors(self, x, params, level, W=F64):
        """per mode the list of its factors: (entries [n, taps] counted from the first level's, weights [n, taps], value [n, F], majorant
        sum|w v| [n, F], [(axis, d value / d cell coordinate [n, F])])"""
        cell, pos = self.cell(x, level, W)
        one, n_line = pos.dtype.type(1), self.line_entries[level]
        table = params.astype(W)[self.offsets[level] * self.F:self.offsets[level + 1] * self.F].reshape(-1, self.F)

        def factor(idx, w, slopes):
            v, value, major = table[idx], np.zeros((x.shape[0], self.F), W), np.zeros((x.shape[0], self.F), W)
            for t in range(idx.shape[1]):
                value, major = fma(w[:, t, None], v[:, t], value), major + np.abs(w[:, t, None] * v[:, t])
            return idx + self.offsets[level], w, value, major, slopes(v)

        def line(k, axis, first):
            idx = np.stack([(cell[:, axis] + q) % 2 ** 32 % n_line for q in range(2)], axis=1) + first + k * n_line
            return factor(idx, np.stack([one - pos[:, axis], pos[:, axis]], axis=1), lambda v: [(axis, v[:, 1] - v[:, 0])])

        if self.cp:
            return [[line(d, d, 0) for d in range(self.D)]]
        modes = []
        for k, (a, b) in enumerate(self.planes):
            idx, w = self.corners(cell, pos, k, level)
            pa, pb = pos[:, a, None], pos[:, b, None]
            plane = factor(idx + k * self.entries[level], w, lambda v: [(a, (1 - pb) * (v[:, 1] - v[:, 0]) + pb * (v[:, 3] - v[:, 2])), (b, (1 - pa) * (v[:, 2] - v[:, 0]) + pa * (v[:, 3] - v[:, 1]))])
            modes.append([plane, line(k, 2 - k, 3 * self.entries[level])])
        return modes

    @staticmethod
    def others(values, j):
        """the product of every value but the j-th, left to right"""
        out = np.ones_like(values[0])
        for q, v in enumerate(values):
            out = out * v if q != j else out
        return out

    def forward(self, x, params, W=F64, out_dtype=None):
        """[n, L * modes * F]; params: the values the kernel reads (half or float)"""
        y = np.stack([self.others([f[2] for f in mode], -1) for l in range(self.L) for mode in self.factors(x, params, l, W)], axis=1).reshape(x.shape[0], -1)
        return y if out_dtype is None else y.astype(out_dtype)

    def dy_dx(self, x, params, W=F64):
        """[n, L * modes * F, D], analytic"""
        out = np.zeros((x.shape[0], self.L, self.n_modes, self.F, self.D), W)
        for l in range(self.L):
            for k, mode in enumerate(self.factors(x, params, l, W)):
                for j, f in enumerate(mode):
                    for axis, slope in f[4]:
                        out[:, l, k, :, axis] += self.others([g[2] for g in mode], j) * slope * W(self.scales[l])
        return out.reshape(x.shape[0], -1, self.D)

    def backward_input(self, x, params, dy, W=F64):
        """dL/dx [n, D] for dL/dy [n, >= width] (padding columns are ignored)"""
        return np.einsum("nk,nkd->nd", dy[:, :self.n_output_dims].astype(W), self.dy_dx(x, params, W))

    def param_gradient_terms(self, x, params, dy, W=F64, each=None):
        """per parameter, summed in fp64: S the sum of the contributions dL/dy_f * [product of the mode's other factors] * w_tap formed in W
        (each: rounded to that type first, as the half kernel rounds them), A the sum of their magnitudes, Abar the same with every factor
        value replaced by its majorant, k their count"""
        S, A, Abar, K = (np.zeros((self.offsets[-1], self.F), t) for t in (F64, F64, F64, np.int64))
        g = dy[:, :self.n_output_dims].astype(W).reshape(x.shape[0], self.L, self.n_modes, self.F)
        for l in range(self.L):
            for k, mode in enumerate(self.factors(x, params, l, W)):
                for j, (idx, w, _, _, _) in enumerate(mode):
                    G, Gbar = g[:, l, k] * self.others([f[2] for f in mode], j), np.abs(g[:, l, k]) * self.others([f[3] for f in mode], j)
                    for t in range(idx.shape[1]):
                        contribution = G * w[:, t, None]
                        contribution = (contribution if each is None else contribution.astype(each)).astype(F64)
                        np.add.at(S, idx[:, t], contribution)
                        np.add.at(A, idx[:, t], np.abs(contribution))
                        np.add.at(Abar, idx[:, t], (Gbar * w[:, t, None]).astype(F64))
                        np.add.at(K, idx[:, t], 1)
        return S.ravel(), A.ravel(), Abar.ravel(), K.ravel()
