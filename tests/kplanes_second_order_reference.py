"""The KPlanes second-order pass restated in plain numpy on kplanes_reference.KPlanes.  With v [n, D] and d = dL/dy: Q = <v, J^T d> =
sum_f d_f t_f, t = J v the tangent.  Per (level, feature), along vs = scale * v: a plane's slopes da, db, its mixed derivative dc, T = D_v P;
O_k = prod_{q != k} P_q and S_k = D_v O_k = sum_{q != k} T_q prod_{m != k, q} P_m (Sum: 1 and 0).  Then t = sum_k O_k T_k,
dQ/dx_a += scale d_f (O_k vs_b dc_k + S_k da_k) (and b likewise) and dQ/dparams(k, c, f) = d_f (O_k D_v w_c + w_c S_k).  W is the working
precision; in float32 every operation is the kernels' own, in their order."""
import numpy as np

from kplanes_reference import F64, KPlanes, fma


class KPlanesSecondOrder(KPlanes):
    def others(self, P, T):
        """([O_k], [S_k]) from the plane values and their derivatives along v: prefix and suffix products carried with their derivatives"""
        one, zero = np.ones_like(P[0]), np.zeros_like(P[0])
        if not self.product or self.K == 1:
            return [one] * self.K, [zero] * self.K
        suffix, dsuffix = [one] * self.K, [zero] * self.K
        for k in range(self.K - 2, -1, -1):
            dsuffix[k], suffix[k] = fma(dsuffix[k + 1], P[k + 1], suffix[k + 1] * T[k + 1]), suffix[k + 1] * P[k + 1]
        prefix, dprefix, O, S = one, zero, [], []
        for k in range(self.K):
            O.append(prefix * suffix[k])
            S.append(fma(dprefix, suffix[k], prefix * dsuffix[k]))
            dprefix, prefix = fma(dprefix, P[k], prefix * T[k]), prefix * P[k]
        return O, S

    def level(self, x, v, params, l, W):
        """per plane: dict of entries idx [n, 4], weights w and their derivatives along v dw [n, 4], P, da, db, dc, T, O, S [n, F] and the
        majorants Obar, Sbar [n, F], dwbar [n, 4] (every plane value replaced by sum|w v|, every difference by the sum of magnitudes)"""
        terms, pos = self.level_terms(x, params, l, W)
        vs, one, planes = W(self.scales[l]) * v.astype(W), W(1), []
        for k, (a, b) in enumerate(self.planes):
            idx, w, c, P, M = terms[k]
            pa, pb, va, vb = pos[:, a, None], pos[:, b, None], vs[:, a, None], vs[:, b, None]
            dc = (c[:, 3] - c[:, 2]) - (c[:, 1] - c[:, 0])
            da, db = fma(pb, dc, c[:, 1] - c[:, 0]), fma(pa, (c[:, 3] - c[:, 1]) - (c[:, 2] - c[:, 0]), c[:, 2] - c[:, 0])
            m = np.abs(c)
            Tbar = np.abs(va) * (m[:, 1] + m[:, 0] + pb * m.sum(axis=1)) + np.abs(vb) * (m[:, 2] + m[:, 0] + pa * m.sum(axis=1))  # as da, db are formed: d10 + u dc
            other = [((pos[:, a] if i & 1 else one - pos[:, a]), (pos[:, b] if i & 2 else one - pos[:, b])) for i in range(4)]
            dw = np.stack([fma((vs[:, b] if i & 2 else -vs[:, b]), other[i][0], (vs[:, a] if i & 1 else -vs[:, a]) * other[i][1]) for i in range(4)], axis=1)
            dwbar = np.stack([np.abs(vs[:, b]) * other[i][0] + np.abs(vs[:, a]) * other[i][1] for i in range(4)], axis=1)
            planes.append(dict(a=a, b=b, va=va, vb=vb, idx=idx, w=w, dw=dw, dwbar=dwbar, P=P, M=M, da=da, db=db, dc=dc, T=fma(vb, db, va * da), Tbar=Tbar))
        (O, S), (Obar, Sbar) = (self.others([p[values] for p in planes], [p[slopes] for p in planes]) for values, slopes in (("P", "T"), ("M", "Tbar")))
        for k, p in enumerate(planes):
            p.update(O=O[k], S=S[k], Obar=Obar[k], Sbar=Sbar[k])
        return planes

    def tangent(self, x, v, params, W=F64, out_dtype=None):
        """J v [n, L*F]"""
        t = np.zeros((x.shape[0], self.L, self.F), W)
        for l in range(self.L):
            planes = self.level(x, v, params, l, W)
            p, dp = planes[0]["P"], planes[0]["T"]
            for q in planes[1:]:
                p, dp = (p * q["P"], fma(dp, q["P"], p * q["T"])) if self.product else (p, dp + q["T"])
            t[:, l] = dp
        t = t.reshape(x.shape[0], -1)
        return t if out_dtype is None else t.astype(out_dtype)

    def dQ_dx(self, x, v, params, dy, W=F64):
        """[n, D]"""
        out, g = np.zeros(x.shape, W), dy[:, :self.n_output_dims].astype(W).reshape(x.shape[0], self.L, self.F)
        for l in range(self.L):
            dx, planes = np.zeros(x.shape, W), self.level(x, v, params, l, W)
            for f in range(self.F):
                for p in planes:
                    for axis, other, slope in ((p["a"], p["vb"], p["da"]), (p["b"], p["va"], p["db"])):
                        inner = fma(p["O"][:, f], other[:, 0] * p["dc"][:, f], p["S"][:, f] * slope[:, f]) if self.product and self.K > 1 else other[:, 0] * p["dc"][:, f]
                        dx[:, axis] = fma(g[:, l, f], inner, dx[:, axis])
            out = fma(np.full_like(dx, self.scales[l]), dx, out)
        return out

    def param_gradient_terms(self, x, v, params, dy, W=F64, each=None):
        """kplanes_reference's (S, A, Abar, k) for the contributions d_f (O_k D_v w_c + w_c S_k) to dQ/dparams"""
        S, A, Abar, K = (np.zeros((self.offsets[-1], self.F), t) for t in (F64, F64, F64, np.int64))
        g = dy[:, :self.n_output_dims].astype(W).reshape(x.shape[0], self.L, self.F)
        for l in range(self.L):
            for k, p in enumerate(self.level(x, v, params if self.product else None, l, W)):
                idx = p["idx"] + self.offsets[l] + k * self.entries[l]
                for c in range(4):
                    w, dw = p["w"][:, c, None], p["dw"][:, c, None]
                    contribution = g[:, l] * (fma(p["O"], dw, w * p["S"]) if self.product and self.K > 1 else dw)
                    contribution = (contribution if each is None else contribution.astype(each)).astype(F64)
                    np.add.at(S, idx[:, c], contribution)
                    np.add.at(A, idx[:, c], np.abs(contribution))
                    np.add.at(Abar, idx[:, c], (np.abs(g[:, l]) * (p["Obar"] * p["dwbar"][:, c, None] + w * p["Sbar"])).astype(F64))
                    np.add.at(K, idx[:, c], 1)
        return S.ravel(), A.ravel(), Abar.ravel(), K.ravel()
