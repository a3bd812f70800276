"""The PermutoGrid encoding restated in plain numpy: the permutohedral lattice lookup of Adams, Baek and Davis (2010) per level, value,
analytic dy/dx and the parameter-gradient contributions.  W is the working precision: float64 is the reference (R64), float32 with one
rounding to the output precision is Rh, the yardstick for what fp32 arithmetic can deliver.  No cleverness: arrays are indexed by rank."""
import numpy as np

PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737)  # the grid's CoherentPrime hash
F32, F64 = np.float32, np.float64


class Permuto:
    def __init__(self, n_dims, cfg):
        self.D, self.L, self.F = n_dims, cfg.get("n_levels", 16), cfg.get("n_features_per_level", 2)
        self.T = 1 << cfg.get("log2_hashmap_size", 19)
        self.n_output_dims, self.n_params = self.L * self.F, self.L * self.T * self.F
        log2_scale = F32(np.log2(F64(F32(cfg.get("per_level_scale", 2.0)))))  # float, as the grid computes its scale (without the - 1)
        self.scales = [F32(F32(np.exp2(F64(F32(F32(l) * log2_scale)))) * F32(cfg.get("base_resolution", 16))) for l in range(self.L)]

    def simplex(self, x, level, W=F64):
        """-> rem0 [n, D+1] (W, integer-valued), rank [n, D+1] int, b [n, D+1] W: steps 1 - 5 of the recipe"""
        n, D, N = x.shape[0], self.D, self.D + 1
        p = x.astype(W) * W(self.scales[level])
        E, sm = np.zeros((n, N), W), np.zeros(n, W)
        for i in range(D, 0, -1):  # elevate
            cf = p[:, i - 1] * W(1.0 / np.sqrt((i * (i + 1))))
            E[:, i] = sm - W(i) * cf
            sm = sm + cf
        E[:, 0] = sm
        v = E / W(N)
        up, down = np.ceil(v) * W(N), np.floor(v) * W(N)
        rem0 = np.where(up - E < E - down, up, down)
        total = (rem0 / W(N)).sum(axis=1).astype(np.int64)
        rank = np.zeros((n, N), np.int64)
        for i in range(N):
            for j in range(i + 1, N):
                lt = E[:, i] - rem0[:, i] < E[:, j] - rem0[:, j]
                rank[:, i] += lt
                rank[:, j] += ~lt
        s = total[:, None]
        dec, inc = (s > 0) & (rank >= N - s), (s < 0) & (rank < -s)  # fix-up
        rem0 = rem0 + W(N) * (inc.astype(W) - dec.astype(W))
        rank = rank + s + N * (inc.astype(np.int64) - dec.astype(np.int64))
        b, rows = np.zeros((n, N + 1), W), np.arange(n)
        for i in range(N):
            d = (E[:, i] - rem0[:, i]) / W(N)
            b[rows, D - rank[:, i]] += d
            b[rows, D + 1 - rank[:, i]] -= d
        b[:, 0] += W(1) + b[:, N]
        return rem0, rank, b[:, :N]

    def keys(self, rem0, rank, r):
        """the D + 1 integer key components of vertex r"""
        return rem0.astype(np.int64) + r - (self.D + 1) * (rank > self.D - r)

    def indices(self, rem0, rank):
        """[n, D+1]: table entry of every vertex (first D key components, int32 -> uint32, hashed, masked)"""
        out = np.zeros(rank.shape, np.int64)
        for r in range(self.D + 1):
            k = self.keys(rem0, rank, r) & 0xFFFFFFFF
            h = np.zeros(rank.shape[0], np.int64)
            for i in range(self.D):
                h ^= (k[:, i] * PRIMES[i]) & 0xFFFFFFFF
            out[:, r] = h & (self.T - 1)
        return out

    def forward(self, x, params, W=F64, out_dtype=None):
        """[n, L*F]; params: the values the kernel reads (half or float), any shape of L*T*F elements"""
        table = params.astype(W).reshape(self.L, self.T, self.F)
        y = np.zeros((x.shape[0], self.L, self.F), W)
        for l in range(self.L):
            rem0, rank, b = self.simplex(x, l, W)
            idx = self.indices(rem0, rank)
            for r in range(self.D + 1):
                y[:, l] += b[:, r, None] * table[l, idx[:, r]]
        y = y.reshape(x.shape[0], -1)
        return y if out_dtype is None else y.astype(out_dtype)

    def min_weight(self, x):
        """[n]: the smallest barycentric weight over all levels (0 on a simplex face, where dy/dx jumps)"""
        return np.min([self.simplex(x, l)[2].min(axis=1) for l in range(self.L)], axis=0)

    def dy_dx(self, x, params, W=F64):
        """[n, L*F, D], analytic: b is affine in E inside a simplex, E is linear in x"""
        D, N = self.D, self.D + 1
        table = params.astype(W).reshape(self.L, self.T, self.F)
        elev = np.zeros((N, D), W)  # dE_i / dp_j
        for j in range(D):
            elev[:j + 1, j] = 1
            elev[j + 1, j] = -(j + 1)
            elev[:, j] *= W(1.0 / np.sqrt((j + 1) * (j + 2)))
        out, rows = np.zeros((x.shape[0], self.L, self.F, D), W), np.arange(x.shape[0])
        for l in range(self.L):
            rem0, rank, _ = self.simplex(x, l, W)
            idx = self.indices(rem0, rank)
            db_dE = np.zeros((x.shape[0], N, N), W)  # [., r, i]
            for i in range(N):
                db_dE[rows, D - rank[:, i], i] += W(1) / W(N)
                db_dE[rows, (D + 1 - rank[:, i]) % N, i] -= W(1) / W(N)  # (b[D+1] is folded into b[0])
            db_dx = (db_dE @ elev) * W(self.scales[l])  # [n, r, D]
            out[:, l] = np.einsum("nrf,nrd->nfd", table[l, idx], db_dx)
        return out.reshape(x.shape[0], -1, D)

    def backward_input(self, x, params, dy, W=F64):
        """dL/dx [n, D] for dL/dy [n, >= L*F] (padding columns are ignored)"""
        return np.einsum("nk,nkd->nd", dy[:, :self.n_output_dims].astype(W), self.dy_dx(x, params, W))

    def param_gradient_terms(self, x, dy, W=F64):
        """per parameter, summed in fp64: (S the sum of the contributions dL/dy * b formed in W, the sum of their magnitudes, their count)"""
        S, A, K = (np.zeros((self.L, self.T, self.F), t) for t in (F64, F64, np.int64))
        g = dy[:, :self.n_output_dims].astype(W).reshape(x.shape[0], self.L, self.F)
        for l in range(self.L):
            rem0, rank, b = self.simplex(x, l, W)
            idx = self.indices(rem0, rank)
            for r in range(self.D + 1):
                c = (g[:, l] * b[:, r, None]).astype(F64)
                np.add.at(S[l], idx[:, r], c)
                np.add.at(A[l], idx[:, r], np.abs(c))
                np.add.at(K[l], idx[:, r], 1)
        return S.ravel(), A.ravel(), K.ravel()
