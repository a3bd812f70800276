"""The reference's grid encoding for any number of input dimensions from 1 to 7, restated in numpy (encodings/grid.h:49-650 and
:668-730, common_device.h:631-718 and :825-868, pcg32.h).  The CPU oracle stops at four dimensions; tests/test_grid_nd_reference.py pins
this restatement to it, bit for bit, where both exist, and the tests of the 1-, 5-, 6- and 7-dimensional kernels compare against it.

Arithmetic.  Every fp32 operation of the kernels is one numpy float32 operation (numpy never contracts).  A fused multiply-add is formed in
float64 -- the product of two floats or halves is exact there -- and the sum is rounded TO ODD before the one rounding to the target type,
so that no double rounding can occur (Boldo & Melquiond, "Emulation of a FMA and correctly rounded sums").  Conversions float64 -> float32
-> float16 by astype round to nearest even, as the hardware does.  Integer index arithmetic wraps in uint32.  No GPU in here."""
import numpy as np

F16, F32, F64, U32, U64 = np.float16, np.float32, np.float64, np.uint32, np.uint64
MAX_DIMS = 7
DIMS_MESSAGE = "GridEncoding: number of input dims must be 2 or 3."
GRID_TYPE = {"hash": 0, "dense": 1, "tiled": 2}
HASH_TYPE = {"prime": 0, "coherentprime": 1, "reversedprime": 2, "rng": 3}
INTERP = {"nearest": 0, "linear": 1, "smoothstep": 2}
PRIMES = {  # common_device.h:645-661
    0: [1958374283, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737],
    1: [1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737],
    2: [2165219737, 1434869437, 2097192037, 3674653429, 805459861, 2654435761, 1958374283],
}
PRODUCT_FP32, PRODUCT_SCRATCH32, PRODUCT_HALF = 0, 1, 2  # how a gradient contribution is formed (oracle.PRODUCT_*)
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------------ arithmetic helpers
def fma(a, b, c, dtype):
    """round_dtype(a * b + c) with one rounding; a, b, c float32 or float16 arrays"""
    p = np.asarray(a, dtype=F64) * np.asarray(b, dtype=F64)  # exact: at most 48 significant bits
    c = np.broadcast_to(np.asarray(c, dtype=F64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: s + err == p + c exactly
    even = (s.view(np.int64) & 1) == 0
    with np.errstate(over="ignore"):
        s = np.where(even & (err > 0), np.nextafter(s, np.inf), np.where(even & (err < 0), np.nextafter(s, -np.inf), s))  # round to odd
    return s.astype(dtype)


def _pcg32_advanced(step):
    """state of pcg32{1337} after advance(step) (pcg32.h:40-60, :145-166); step: uint64 array"""
    mult, inc = 0x5851F42D4C957F2D, 3
    state = (0 * mult + inc) & M64
    state = (state + 1337) & M64
    state = (state * mult + inc) & M64
    acc_mult = np.ones(step.shape, dtype=U64)
    acc_plus = np.zeros(step.shape, dtype=U64)
    cur_mult, cur_plus = mult, inc
    with np.errstate(over="ignore"):
        for k in range(64):
            bit = ((step >> U64(k)) & U64(1)).astype(bool)
            acc_mult = np.where(bit, acc_mult * U64(cur_mult), acc_mult)
            acc_plus = np.where(bit, acc_plus * U64(cur_mult) + U64(cur_plus), acc_plus)
            cur_plus = ((cur_mult + 1) * cur_plus) & M64
            cur_mult = (cur_mult * cur_mult) & M64
        return acc_mult * U64(state) + acc_plus


def _pcg32_output(old):
    """next_uint()'s output for the state it starts from (pcg32.h:72-78)"""
    xorshifted = (((old >> U64(18)) ^ old) >> U64(27)).astype(U32)
    rot = (old >> U64(59)).astype(U32)
    return (xorshifted >> rot) | (xorshifted << ((~rot + U32(1)) & U32(31)))


def random_val(idx):
    """random_val(1337, idx) (common_device.h:333-337): pcg32{1337}, advance(idx), next_float()"""
    bits = (_pcg32_output(_pcg32_advanced(np.asarray(idx, dtype=U64))) >> U32(9)) | U32(0x3F800000)
    return bits.view(F32) - F32(1.0)


def half_bits(a):
    return np.ascontiguousarray(a, dtype=F32).astype(F16).view(np.uint16)


class _G:
    """the fields tests/grid_reference.py reads from an oracle encoding's .g"""


class GridND:
    def __init__(self, n_in, cfg):
        F = cfg.get("n_features_per_level", 2)
        if F not in (1, 2, 4, 8):
            raise RuntimeError("GridEncoding: n_features_per_level must be 1, 2, 4, or 8.")
        otype = str(cfg.get("otype", "Grid")).lower()
        default_type = "tiled" if otype == "tiledgrid" else ("dense" if otype == "densegrid" else "hash")
        n_levels = cfg.get("n_levels", 16)
        if not 1 <= n_in <= MAX_DIMS:
            raise RuntimeError(DIMS_MESSAGE)
        self.n_in, self.F, self.n_levels = n_in, F, n_levels
        self.grid_type = GRID_TYPE[str(cfg.get("type", default_type)).lower()]
        self.hash_type = HASH_TYPE[str(cfg.get("hash", "CoherentPrime")).lower()]
        self.interpolation = INTERP[str(cfg.get("interpolation", "Linear")).lower()]
        self.stochastic = bool(cfg.get("stochastic_interpolation", False))
        base = cfg.get("base_resolution", 16)
        log2_hashmap_size = cfg.get("log2_hashmap_size", 19)
        if "per_level_scale" in cfg:
            pls = F32(cfg["per_level_scale"])
        elif self.grid_type == GRID_TYPE["dense"]:
            pls = F32(np.exp(F64(F32(F32(np.log(F64(F32(256.0) / F32(base)))) / F32(n_levels - 1)))))
        else:
            pls = F32(2.0)
        # grid.h:692-718 with common_device.h:709-718
        log2_scale = F32(np.log2(F64(pls)))
        self.scales, self.resolutions, self.sizes, self.strides, self.hashed = [], [], [], [], []
        offsets = [0]
        for level in range(n_levels):
            scale = F32(F32(F32(np.exp2(F64(F32(F32(level) * log2_scale)))) * F32(base)) - F32(1.0))
            resolution = (int(np.ceil(scale)) + 1) & M32
            max_params = M32 // 2
            if float(resolution) ** n_in > float(F32(max_params)):  # std::pow((float)resolution, N_POS_DIMS): double arithmetic
                size = max_params
            else:
                size = (resolution ** n_in) & M32  # powi: uint32 products
            size = ((size + 7) // 8 * 8) & M32
            if self.grid_type == GRID_TYPE["tiled"]:
                size = min(size, (base ** n_in) & M32)
            elif self.grid_type == GRID_TYPE["hash"]:
                size = min(size, 1 << log2_hashmap_size)
            # grid_index's stride loop (common_device.h:692-704), evaluated once: early exit and wrap-around included
            stride, strides = 1, [0] * n_in
            for d in range(n_in):
                if not stride <= size:
                    break
                strides[d] = stride
                stride = (stride * resolution) & M32
            self.scales.append(scale)
            self.resolutions.append(resolution)
            self.sizes.append(size)
            self.strides.append(strides)
            self.hashed.append(self.grid_type == GRID_TYPE["hash"] and size < stride)
            offsets.append((offsets[-1] + size) & M32)  # (uint32, as m_offset_table)
        self.offsets = np.array(offsets, dtype=U32)
        self.n_output_dims = n_levels * F
        self.n_to_pad = 0
        self.n_params = offsets[-1] * F
        self.g = _G()
        self.g.n_features_per_level, self.g.n_levels, self.g.interpolation = F, n_levels, self.interpolation

    @property
    def padded_output_width(self):
        return self.n_output_dims + self.n_to_pad

    # -------------------------------------------------------------------------------------------------- indexing
    def index(self, level, cell):
        """grid_index (common_device.h:690-707); cell: list of D uint32 arrays"""
        D = self.n_in
        with np.errstate(over="ignore"):
            if self.hashed[level]:
                if self.hash_type == HASH_TYPE["rng"]:  # :663-676
                    bits = 64 // D
                    step = np.zeros(cell[0].shape, dtype=U64)
                    for d in range(D):
                        step = step ^ (cell[d].astype(U64) << U64(d * bits))
                    index = _pcg32_output(_pcg32_advanced(step))
                else:
                    index = np.zeros(cell[0].shape, dtype=U32)
                    for d in range(D):
                        index = index ^ (cell[d] * U32(PRIMES[self.hash_type][d]))
            else:
                index = np.zeros(cell[0].shape, dtype=U32)
                for d in range(D):
                    index = index + cell[d] * U32(self.strides[level][d])
        return index % U32(self.sizes[level])

    def fractions(self, level, x, dtype=F32):
        """pos_fract with both derivatives (common_device.h:825-868): cell, pos, d pos, d2 pos per dimension.  dtype float64: the same
        cell and fraction (the fp32 ones, exactly), smoothstep and its derivatives in float64."""
        scale = self.scales[level]
        cell, pos, d1, d2 = [], [], [], []
        for d in range(self.n_in):
            p = fma(scale, x[:, d], F32(0.5), F32)
            tmp = np.floor(p)
            cell.append((tmp.astype(np.int64) & M32).astype(U32))  # (uint32_t)(int)tmp
            p = (p - tmp).astype(dtype)
            if self.interpolation == INTERP["smoothstep"]:
                one, two, three, six, twelve = (dtype(v) for v in (1.0, 2.0, 3.0, 6.0, 12.0))
                d2.append(six - twelve * p)
                d1.append(six * p * (one - p))
                pos.append(p * p * (three - two * p))
            else:
                d2.append(np.zeros_like(p))
                d1.append(np.ones_like(p))
                pos.append(p)
        return cell, pos, d1, d2

    def _corner(self, cell, pos, code, first, skip=None):
        """the corner whose bit d says cell_d + 1: (cell coordinates, product over the dimensions in order starting from `first`)"""
        local, w = [], first
        one = pos[0].dtype.type(1.0)
        with np.errstate(over="ignore"):
            for d in range(self.n_in):
                up = (code >> d) & 1
                local.append(cell[d] + U32(1) if up else cell[d])
                if d != skip:
                    w = w * (pos[d] if up else one - pos[d])
        return local, w

    @staticmethod
    def _expand(idx, k):
        """D-bit corner code of pair idx (the dimensions but k, in order), bit k clear"""
        return (idx & ((1 << k) - 1)) | ((idx >> k) << (k + 1))

    # -------------------------------------------------------------------------------------------------- forward (grid.h:49-212)
    def forward(self, x, params, want_dy_dx=False):
        """params: float16 or float32 array [n_params]; returns (out [n][padded] of the same type, dy_dx float32 [n][L * F][D] or None)"""
        x = np.ascontiguousarray(x, dtype=F32)
        T = params.dtype.type
        assert T in (F16, F32)
        n, D, F, L = x.shape[0], self.n_in, self.F, self.n_levels
        out = np.zeros((n, self.padded_output_width), dtype=T)
        dy_dx = np.zeros((n, L * F, D), dtype=F32) if want_dy_dx else None
        for level in range(L):
            table = params[int(self.offsets[level]) * F:int(self.offsets[level + 1]) * F].reshape(-1, F)
            cell, pos, d1, _ = self.fractions(level, x)
            if self.interpolation == INTERP["nearest"]:
                out[:, level * F:(level + 1) * F] = table[self.index(level, cell)]
                continue
            acc = np.zeros((n, F), dtype=T)
            for code in range(1 << D):
                local, w = self._corner(cell, pos, code, F32(1.0))
                acc = fma(w.astype(T)[:, None], table[self.index(level, local)], acc, T)
            out[:, level * F:(level + 1) * F] = acc
            if want_dy_dx:  # grid.h:172-211
                for gd in range(D):
                    grads = np.zeros((n, F), dtype=F32)
                    for idx in range(1 << (D - 1)):
                        code = self._expand(idx, gd)
                        local, w = self._corner(cell, pos, code, self.scales[level], skip=gd)
                        left = table[self.index(level, local)].astype(F32)
                        local[gd] = cell[gd] + U32(1)
                        right = table[self.index(level, local)].astype(F32)
                        w = np.broadcast_to(np.asarray(w, dtype=F32), (n,))
                        grads = grads + w[:, None] * (right - left) * d1[gd][:, None]
                    dy_dx[:, level * F:(level + 1) * F, gd] = grads
        return out, dy_dx

    def backward_input(self, dy_dx, dL_dy):
        """kernel_grid_backward_input (grid.h:323-349): dL/dx in fp32, features in order"""
        n = dL_dy.shape[0]
        result = np.zeros((n, self.n_in), dtype=F32)
        for k in range(self.n_output_dims):
            result = result + dL_dy[:, k].astype(F32)[:, None] * dy_dx[:, k, :]
        return result

    # -------------------------------------------------------------------------------------------------- parameter gradients (grid.h:215-320)
    def contributions(self, x, dL_dy, product):
        """every gradient contribution as the kernels form it: (parameter index int64 [m], value float64 [m]).  PRODUCT_HALF: (half)weight *
        dL/dy in fp16; PRODUCT_SCRATCH32: weight * (float)dL/dy in fp32 (dL/dy half); PRODUCT_FP32: weight * dL/dy in fp32.  With
        stochastic_interpolation: dL/dy itself on the corner drawn per (sample, level) (grid.h:284-298)."""
        x = np.ascontiguousarray(x, dtype=F32)
        assert dL_dy.dtype.type == (F32 if product == PRODUCT_FP32 else F16)
        n, D, F = x.shape[0], self.n_in, self.F
        keys, values = [], []

        def add(level, local, w):
            g = dL_dy[:, level * F:(level + 1) * F]
            w = np.broadcast_to(np.asarray(w, dtype=F32), (n,))
            if product == PRODUCT_HALF:
                term = (w.astype(F16).astype(F32)[:, None] * g.astype(F32)).astype(F16)  # the fp32 product of two halves is exact
            else:
                term = w[:, None] * g.astype(F32)
            base = int(self.offsets[level]) * F
            k = base + self.index(level, local).astype(np.int64)[:, None] * F + np.arange(F)[None, :]
            keys.append(k.reshape(-1))
            values.append(term.astype(F64).reshape(-1))

        for level in range(self.n_levels):
            cell, pos, _, _ = self.fractions(level, x)
            if self.interpolation == INTERP["nearest"]:
                add(level, cell, F32(1.0))
            elif self.stochastic:
                with np.errstate(over="ignore"):
                    sample = random_val((np.arange(n, dtype=U32) + U32(level) * U32(n)).astype(U64))
                    local = [np.where(sample >= pos[d], cell[d], cell[d] + U32(1)) for d in range(D)]
                add(level, local, F32(1.0))
            else:
                for code in range(1 << D):
                    local, w = self._corner(cell, pos, code, F32(1.0))
                    add(level, local, w)
        return np.concatenate(keys), np.concatenate(values)

    def backward_terms(self, x, dL_dy, product):
        """per parameter: the sum of its contributions, the sum of their magnitudes, their count (tests/grid_reference.py's bounds)"""
        k, v = self.contributions(x, dL_dy, product)
        s, a, hits = np.zeros(self.n_params), np.zeros(self.n_params), np.zeros(self.n_params, dtype=U32)
        np.add.at(s, k, v)
        np.add.at(a, k, np.abs(v))
        np.add.at(hits, k, 1)
        nz = np.abs(v[v != 0])
        return {"sum": s, "abs_sum": a, "hits": hits, "min_nonzero": float(nz.min()) if nz.size else float("inf")}

    def backward_exact(self, x, dL_dy):
        """the exact sum of the fp16 products per parameter, rounded to half once: the deterministic route's result (half bits)"""
        k, v = self.contributions(x, dL_dy, PRODUCT_HALF)
        fixed = np.zeros(self.n_params, dtype=np.int64)
        np.add.at(fixed, k, np.round(v * 2.0 ** 24).astype(np.int64))  # halves are multiples of 2^-24: exact
        assert np.all(np.abs(fixed) < 2 ** 52)
        return (fixed.astype(F64) * 2.0 ** -24).astype(F16).view(np.uint16)

    # -------------------------------------------------------------------------------------------------- second order (grid.h:352-650)
    def second_order(self, x, v, dL_dy, params, mode):
        """backward_backward_input for v = dL_ddLdx.  mode "r64": float64 throughout on the given parameters and dL/dy (the truth);
        "rh": fp32 in the kernels' operation order, rounded to the storage type wherever the kernels store -- dL_ddLdy, the gradient
        products and every addition into the gradient table (sample order stands in for the atomics' order).  Returns (dL_ddLdy
        [n][padded], dL/dgrid [n_params], dL_dx [n][D]) as float64 arrays."""
        x = np.ascontiguousarray(x, dtype=F32)
        T = params.dtype.type
        exact = mode == "r64"
        W = F64 if exact else F32
        n, D, F, L = x.shape[0], self.n_in, self.F, self.n_levels
        FT = min(F, 2)
        store = (lambda a: a) if exact else (lambda a: a.astype(T).astype(W))
        v = v.astype(W)
        pw, dyw = params.astype(W), dL_dy.astype(W)
        ddy = np.zeros((n, self.padded_output_width), dtype=W)
        dx = np.zeros((n, D), dtype=W)
        keys, values = [], []
        nearest, smooth = self.interpolation == INTERP["nearest"], self.interpolation == INTERP["smoothstep"]
        for level in range(L if not nearest else 0):
            table = pw[int(self.offsets[level]) * F:int(self.offsets[level + 1]) * F].reshape(-1, F)
            cell, pos, d1, d2 = self.fractions(level, x, W)
            scale = W(self.scales[level])
            g = dyw[:, level * F:(level + 1) * F]
            base = int(self.offsets[level]) * F
            for gd in range(D):
                # dL_ddLdy = J v (grid.h:626-650) from dy_dx (:172-211)
                jac = np.zeros((n, F), dtype=W)
                grad_in = scale * v[:, gd] * d1[gd]
                for idx in range(1 << (D - 1)):
                    code = self._expand(idx, gd)
                    local, w = self._corner(cell, pos, code, scale, skip=gd)
                    il = self.index(level, local)
                    local[gd] = cell[gd] + U32(1)
                    ir = self.index(level, local)
                    w = np.broadcast_to(np.asarray(w, dtype=W), (n,))
                    jac = jac + w[:, None] * (table[ir] - table[il]) * d1[gd][:, None]
                    # d/dgrid (grid.h:352-454): -weight on the left corner, +weight on the right one
                    _, wg = self._corner(cell, pos, code, grad_in, skip=gd)
                    for entry, sign in ((il, -1.0), (ir, 1.0)):
                        weight = W(sign) * wg
                        if exact:
                            term = weight[:, None] * g
                        elif T == F16 and F > 1:
                            term = (weight.astype(F16).astype(F32)[:, None] * g).astype(F16).astype(W)
                        else:
                            term = weight[:, None] * g
                        keys.append((base + entry.astype(np.int64)[:, None] * F + np.arange(F)[None, :]).reshape(-1))
                        values.append(term.reshape(-1))
                ddy[:, level * F:(level + 1) * F] = ddy[:, level * F:(level + 1) * F] + jac * v[:, gd][:, None]
            # d/dx (grid.h:456-624): per feature group, gradient dimension, corner pair
            for feature in range(0, F, FT):
                gy = g[:, feature:feature + FT]

                def calc(entry, weight):
                    r = np.zeros(n, dtype=W)
                    for f in range(FT):
                        r = r + table[entry, feature + f] * gy[:, f] * weight
                    return r

                for gd in range(D):
                    grad_out = np.zeros(n, dtype=W)
                    diag = scale * scale * v[:, gd] * d2[gd]
                    for idx in range(1 << (D - 1)):
                        if smooth:
                            code = self._expand(idx, gd)
                            local, w = self._corner(cell, pos, code, diag, skip=gd)
                            grad_out = grad_out + calc(self.index(level, local), -w)
                            local[gd] = cell[gd] + U32(1)
                            grad_out = grad_out + calc(self.index(level, local), w)
                        for og in range(D - 1):
                            rog = og + 1 if og >= gd else og
                            code = self._expand(idx, rog)
                            w = scale * scale * v[:, rog] * d1[rog] * d1[gd]
                            local = []
                            with np.errstate(over="ignore"):
                                for d in range(D):
                                    up = (code >> d) & 1
                                    local.append(cell[d] + U32(1) if up else cell[d])
                                    if d == rog:
                                        continue
                                    if d == gd:
                                        w = w if up else w * W(-1.0)
                                    else:
                                        w = w * (pos[d] if up else W(1.0) - pos[d])
                            grad_out = grad_out + calc(self.index(level, local), -w)
                            local[rog] = cell[rog] + U32(1)
                            grad_out = grad_out + calc(self.index(level, local), w)
                    dx[:, gd] = dx[:, gd] + grad_out
        ddy = store(ddy)
        grad = np.zeros(self.n_params, dtype=F64)
        if keys:
            k, val = np.concatenate(keys), np.concatenate(values)
            if exact:
                np.add.at(grad, k, val.astype(F64))
            else:
                GT = F16 if (T == F16 and F > 1) else F32  # grid.h:660: one feature per level accumulates in fp32
                grad = ordered_sum(k, val, self.n_params, GT).astype(F64)
                if T == F16 and F == 1:
                    grad = grad.astype(F16).astype(F64)
        return ddy.astype(F64), grad, dx.astype(F64)


def ordered_sum(keys, values, n, dtype):
    """per key the sum of its values in the order given, every addition rounded to dtype"""
    order = np.argsort(keys, kind="stable")
    k, v = keys[order], values[order].astype(dtype)
    first = np.r_[True, k[1:] != k[:-1]]
    start = np.flatnonzero(first)
    rank = np.arange(k.size) - np.repeat(start, np.diff(np.r_[start, k.size]))
    acc = np.zeros(n, dtype=dtype)
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(int(rank.max()) + 2)) if k.size else [0]
    for r in range(len(bounds) - 1):
        sel = by_rank[bounds[r]:bounds[r + 1]]
        acc[k[sel]] = (acc[k[sel]] + v[sel]).astype(dtype)
    return acc
