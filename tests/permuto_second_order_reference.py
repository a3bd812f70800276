"""The PermutoGrid second-order pass restated in plain numpy on permuto_reference.Permuto.  The weights b are affine in x inside a simplex,
so with v [n, D] and d = dL/dy: Q = <v, J^T d> has no Hessian term, dQ/dx = 0, the tangent is t = J v = sum_r beta_r table[index_r] and
dQ/dparams(index_r, f) = d_f beta_r with beta = db/dx . v.  W is the working precision; in float32 beta is formed in the kernel's order."""
import numpy as np

from permuto_reference import F64, Permuto


class PermutoSecondOrder(Permuto):
    def tangent(self, x, v, params, W=F64, out_dtype=None):
        """J v [n, L*F]"""
        t = np.einsum("nkd,nd->nk", self.dy_dx(x, params, W), v.astype(W))
        return t if out_dtype is None else t.astype(out_dtype)

    def beta(self, x, v, level, W=F64):
        """-> indices [n, D+1], beta [n, D+1] and its majorant (the same formula on magnitudes, every difference a sum): the elevation of
        v * scale, times 1 / (D + 1), sorted by the ranks after the fix-up, differenced as the weights are"""
        D, N, n = self.D, self.D + 1, x.shape[0]
        rem0, rank, _ = self.simplex(x, level, W)
        vs = v.astype(W) * W(self.scales[level])
        out = []
        for sign, p in ((W(-1), vs), (W(1), np.abs(vs))):
            E, sm = np.zeros((n, N), W), np.zeros(n, W)
            for i in range(D, 0, -1):
                cf = p[:, i - 1] * W(1.0 / np.sqrt(i * (i + 1)))
                E[:, i] = sm + sign * (W(i) * cf)
                sm = sm + cf
            E[:, 0] = sm
            s = np.zeros((n, N + 1), W)
            s[np.arange(n)[:, None], rank] = E * (W(1) / W(N))  # sorted by rank: s[rank_i] = d'_i
            s[:, N] = s[:, 0]
            out.append(s[:, D::-1] + sign * s[:, N:0:-1])  # beta_r = s[D - r] - s[D + 1 - r], beta_0 = s[D] - s[0]
        return self.indices(rem0, rank), out[0], out[1]

    def param_gradient_terms(self, x, v, dy, W=F64, each=None):
        """per parameter, summed in fp64: (S the sum of the contributions d_f beta_r formed in W and rounded to `each`, the sum of their
        magnitudes A, of their majorants Abar, their count K)"""
        S, A, Abar, K = (np.zeros((self.L, self.T, self.F), t) for t in (F64, F64, F64, np.int64))
        g = dy[:, :self.n_output_dims].astype(W).reshape(x.shape[0], self.L, self.F)
        for l in range(self.L):
            idx, beta, bar = self.beta(x, v, l, W)
            for r in range(self.D + 1):
                c = g[:, l] * beta[:, r, None]
                c = (c if each is None else c.astype(each)).astype(F64)
                np.add.at(S[l], idx[:, r], c)
                np.add.at(A[l], idx[:, r], np.abs(c))
                np.add.at(Abar[l], idx[:, r], (np.abs(g[:, l]) * bar[:, r, None]).astype(F64))
                np.add.at(K[l], idx[:, r], 1)
        return S.ravel(), A.ravel(), Abar.ravel(), K.ravel()
