"""The TensoRF second-order pass restated in plain numpy on tensorf_reference.TensoRF.  With v [n, D], d = dL/dy and vs = scale * v:
Q = <v, J^T d> = sum_f d_f t_f, t = J v the tangent.  Every mode is a list of factors; factor j with taps of weight w, the product O of the
mode's other factors and S = D_v O, the derivative of that product along vs, gets d_f (O D_v w + w S) on each tap.  VM: a plane's other is its
line (O = V, S = V' vs_c), a line's its plane (O = P, S = DP = vs_a daP + vs_b dbP).  CP: O_i and S_i ride on prefix and suffix products.
W is the working precision; in float32 every operation is the kernels' own, in their order."""
import numpy as np

from tensorf_reference import F64, TensoRF
from kplanes_reference import fma


class TensoRFSecondOrder(TensoRF):
    @staticmethod
    def others_tangent(V, T):
        """([O_i], [S_i]) from the factor values and their derivatives along v: prefix and suffix products carried with their derivatives"""
        n, one, zero = len(V), np.ones_like(V[0]), np.zeros_like(V[0])
        suffix, dsuffix = [one] * n, [zero] * n
        for i in range(n - 2, -1, -1):
            dsuffix[i], suffix[i] = fma(dsuffix[i + 1], V[i + 1], suffix[i + 1] * T[i + 1]), suffix[i + 1] * V[i + 1]
        prefix, dprefix, O, S = one, zero, [], []
        for i in range(n):
            O.append(prefix * suffix[i])
            S.append(fma(dprefix, suffix[i], prefix * dsuffix[i]))
            dprefix, prefix = fma(dprefix, V[i], prefix * T[i]), prefix * V[i]
        return O, S

    def level(self, x, v, params, l, W):
        """per mode: (targets, tangent [n, F], [(axis, dQ/dx per cell and component [n, F])]); a target is a dict of entries idx [n, taps],
        weights w and their derivatives along vs dw [n, taps], O, S [n, F], the majorants dwbar [n, taps], Obar, Sbar [n, F] (every factor value
        replaced by sum|w v|, every difference by the sum of magnitudes) and plane: the contribution is fma(O, dw, w S), else fma(S, w, O dw)"""
        table, vs = params.astype(W).reshape(-1, self.F), W(self.scales[l]) * v.astype(W)
        pos, one, modes = self.cell(x, l, W)[1], W(1), []
        for k, mode in enumerate(self.factors(x, params, l, W)):
            if self.cp:
                c = [table[f[0]] for f in mode]
                dV = [ci[:, 1] - ci[:, 0] for ci in c]
                T = [dV[i] * vs[:, i, None] for i in range(self.D)]
                Tbar = [(np.abs(c[i][:, 1]) + np.abs(c[i][:, 0])) * np.abs(vs[:, i, None]) for i in range(self.D)]
                (O, S), (Obar, Sbar) = self.others_tangent([f[2] for f in mode], T), self.others_tangent([f[3] for f in mode], Tbar)
                targets = [dict(idx=f[0], w=f[1], dw=np.stack([-vs[:, i], vs[:, i]], axis=1), dwbar=np.abs(vs[:, [i, i]]), O=O[i], S=S[i], Obar=Obar[i], Sbar=Sbar[i], plane=False)
                           for i, f in enumerate(mode)]
                t = T[0] * O[0]
                for i in range(1, self.D):
                    t = fma(T[i], O[i], t)
                modes.append((targets, t, [(i, dV[i] * S[i]) for i in range(self.D)]))
                continue
            (a, b), axis, (plane, line) = self.planes[k], 2 - k, mode
            pa, pb, va, vb, vc = pos[:, a, None], pos[:, b, None], vs[:, a, None], vs[:, b, None], vs[:, axis, None]
            c, e, (P, Pbar), (V, Vbar) = table[plane[0]], table[line[0]], plane[2:4], line[2:4]
            M, m = (c[:, 3] - c[:, 2]) - (c[:, 1] - c[:, 0]), np.abs(c)
            dA, dB, dV = fma(pb, M, c[:, 1] - c[:, 0]), fma(pa, (c[:, 3] - c[:, 1]) - (c[:, 2] - c[:, 0]), c[:, 2] - c[:, 0]), e[:, 1] - e[:, 0]
            DP, lvs = fma(vb, dB, va * dA), dV * vc
            DPbar = np.abs(va) * (m[:, 1] + m[:, 0] + pb * m.sum(axis=1)) + np.abs(vb) * (m[:, 2] + m[:, 0] + pa * m.sum(axis=1))  # as dA, dB are formed: d10 + u M
            other = [((pos[:, a] if q & 1 else one - pos[:, a]), (pos[:, b] if q & 2 else one - pos[:, b])) for q in range(4)]
            dw = np.stack([fma((vs[:, b] if q & 2 else -vs[:, b]), other[q][0], (vs[:, a] if q & 1 else -vs[:, a]) * other[q][1]) for q in range(4)], axis=1)
            dwbar = np.stack([np.abs(vs[:, b]) * other[q][0] + np.abs(vs[:, a]) * other[q][1] for q in range(4)], axis=1)
            targets = [dict(idx=plane[0], w=plane[1], dw=dw, dwbar=dwbar, O=V, S=lvs, Obar=Vbar, Sbar=(np.abs(e[:, 1]) + np.abs(e[:, 0])) * np.abs(vc), plane=True),
                       dict(idx=line[0], w=line[1], dw=np.stack([-vs[:, axis], vs[:, axis]], axis=1), dwbar=np.abs(vs[:, [axis, axis]]), O=P, S=DP, Obar=Pbar, Sbar=DPbar, plane=False)]
            modes.append((targets, fma(DP, V, P * lvs), [(a, fma(M * vb, V, dA * lvs)), (b, fma(M * va, V, dB * lvs)), (axis, dV * DP)]))
        return modes

    def tangent(self, x, v, params, W=F64, out_dtype=None):
        """J v [n, L * modes * F]"""
        t = np.stack([mode[1] for l in range(self.L) for mode in self.level(x, v, params, l, W)], axis=1).reshape(x.shape[0], -1)
        return t if out_dtype is None else t.astype(out_dtype)

    def dQ_dx(self, x, v, params, dy, W=F64):
        """[n, D]: per (level, mode) the sum over the components by fused multiply-adds, then fma(scale, ., total)"""
        out, g = np.zeros(x.shape, W), dy[:, :self.n_output_dims].astype(W).reshape(x.shape[0], self.L, self.n_modes, self.F)
        for l in range(self.L):
            for k, (_, _, slopes) in enumerate(self.level(x, v, params, l, W)):
                for axis, q in slopes:
                    dx = np.zeros(x.shape[0], W)
                    for f in range(self.F):
                        dx = fma(g[:, l, k, f], q[:, f], dx)
                    out[:, axis] = fma(np.full_like(dx, self.scales[l]), dx, out[:, axis])
        return out

    def param_gradient_terms(self, x, v, params, dy, W=F64, each=None):
        """tensorf_reference's (S, A, Abar, k) for the contributions d_f (O D_v w + w S) to dQ/dparams"""
        S, A, Abar, K = (np.zeros((self.offsets[-1], self.F), t) for t in (F64, F64, F64, np.int64))
        g = dy[:, :self.n_output_dims].astype(W).reshape(x.shape[0], self.L, self.n_modes, self.F)
        for l in range(self.L):
            for k, (targets, _, _) in enumerate(self.level(x, v, params, l, W)):
                for p in targets:
                    for t in range(p["idx"].shape[1]):
                        w, dw = p["w"][:, t, None], p["dw"][:, t, None]
                        contribution = g[:, l, k] * (fma(p["O"], dw, w * p["S"]) if p["plane"] else fma(p["S"], w, p["O"] * dw))
                        contribution = (contribution if each is None else contribution.astype(each)).astype(F64)
                        np.add.at(S, p["idx"][:, t], contribution)
                        np.add.at(A, p["idx"][:, t], np.abs(contribution))
                        np.add.at(Abar, p["idx"][:, t], (np.abs(g[:, l, k]) * (p["Obar"] * p["dwbar"][:, t, None] + w * p["Sbar"])).astype(F64))
                        np.add.at(K, p["idx"][:, t], 1)
        return S.ravel(), A.ravel(), Abar.ravel(), K.ravel()
