"""The reverse of a tangent pass through an MLP, restated in torch on the CPU: what tests/test_input_jvp_backward_reference.py pins against
torch.autograd and tests/test_input_jvp_backward_gpu.py measures the library against.

L = sum_t <ubar_t, J(x) v_t> + <obar, f(x)> for f = the MLP with weight matrices Ws [rows][cols] and one activation per layer.

  recipe()    the layer recipe, stated on its own.  With z = W h, zdot_t = W u_t, h' = a(z), u'_t = a'(z) zdot_t and incoming hbar', ubar'_t:
                  eps_t = a'(z) ubar'_t
                  zbar  = a'(z) hbar' + a''(z) sum_t zdot_t ubar'_t
                  hbar  = W^T zbar,  ubar_t = W^T eps_t
                  dW    = zbar^T h + sum_t eps_t^T u_t
              dL/dx = hbar_0 and dL/dv_t = ubar_{0,t}.  fp64, nothing rounded: R64.
  composed()  the same quantities as the library's composed route forms them: the first-order backward pass of obar; then per tangent the
              second-order pass of test_network_second_order._restate (dL_ddLdinput = v_t, dL_doutput = ubar_t) for its weight gradients
              and dS/dinput, and a first-order backward pass of ubar_t for dL/dv_t; gradients accumulate in that order.  half=False: fp64
              (equal to recipe() up to summation order).  half=True: fp32 with a round-to-half wherever the kernels store a half matrix,
              the accumulated gradients included: Rh.
"""
from test_network_second_order import _act, _curved, _d1, _d2, _restate


def _recipe_parts(Ws, acts, x, vs, ubar, obar):
    """recipe() with dW in its two sums: (zbar^T h per layer, sum_t eps_t^T u_t per layer, dL/dx, dL/dv)"""
    import torch

    dt = torch.float64
    Ws = [W.to(dt) for W in Ws]
    K, T = len(Ws), vs.shape[1]
    h, u, z, zdot = [x.to(dt)], [[vs[:, t].to(dt) for t in range(T)]], [], []
    for W, a in zip(Ws, acts):
        z.append(h[-1] @ W.T)
        zdot.append([ut @ W.T for ut in u[-1]])
        h.append(_act(a, z[-1]))
        u.append([_d1(a, z[-1]) * zd for zd in zdot[-1]])
    hbar = torch.zeros_like(h[-1]) if obar is None else obar.to(dt)
    ubars = [ubar[:, t].to(dt) for t in range(T)]
    dW_h, dW_u = [None] * K, [None] * K
    for k in range(K - 1, -1, -1):
        d1, d2 = _d1(acts[k], z[k]), _d2(acts[k], z[k])
        eps = [d1 * ub for ub in ubars]
        zbar = d1 * hbar + d2 * sum(zd * ub for zd, ub in zip(zdot[k], ubars))
        dW_h[k] = zbar.T @ h[k]
        dW_u[k] = sum(e.T @ ut for e, ut in zip(eps, u[k]))
        hbar = zbar @ Ws[k]
        ubars = [e @ Ws[k] for e in eps]
    return dW_h, dW_u, hbar, torch.stack(ubars, dim=1)


def recipe(Ws, acts, x, vs, ubar, obar=None):
    """Ws, x [n][n_in], vs [n][T][n_in], ubar [n][T][n_out], obar [n][n_out] or None -> (dW per layer, dL/dx, dL/dv [n][T][n_in]), fp64"""
    dW_h, dW_u, dx, dv = _recipe_parts(Ws, acts, x, vs, ubar, obar)
    return [a + b for a, b in zip(dW_h, dW_u)], dx, dv


def pass_terms(Ws, acts, x, vs, ubar, obar=None):
    """The term every pass of the composed route adds onto dL_dparams, in fp64 and in the route's order: the first-order pass of obar
    (zbar^T h), then per tangent its bilinear term eps_t^T u_t and, where an activation has curvature, its curvature term (zbar^T h with
    hbar' = 0).  -> a list of per-layer lists; their sum is recipe()'s dW."""
    import torch

    terms = []
    if obar is not None:
        terms.append(_recipe_parts(Ws, acts, x, vs[:, :1], torch.zeros_like(ubar[:, :1]), obar)[0])
    for t in range(vs.shape[1]):
        dW_h, dW_u, _, _ = _recipe_parts(Ws, acts, x, vs[:, t:t + 1], ubar[:, t:t + 1], None)
        terms.append(dW_u)
        if any(_curved(a) for a in acts):
            terms.append(dW_h)
    return terms


def first_order(Ws, acts, x, dy, half):
    """the first-order backward pass: (dW per layer, dL/dx) for dL/dy, with _restate's precision and rounding rule"""
    import torch

    dt = torch.float32 if half else torch.float64
    rh = (lambda t: t.half().to(dt)) if half else (lambda t: t)
    Ws = [W.to(dt) for W in Ws]
    K = len(Ws)
    h, z = [rh(x.to(dt))], []
    for W, a in zip(Ws, acts):
        z.append(rh(h[-1] @ W.T))
        h.append(rh(_act(a, z[-1])))
    aux = [z[k] if _curved(acts[k]) else h[k + 1] for k in range(K)]
    g = dy.to(dt)
    dW = [None] * K
    for k in range(K - 1, -1, -1):
        d = g if acts[k] == "None" and k == K - 1 else rh(g * _d1(acts[k], aux[k]))
        dW[k] = rh(d.T @ h[k])
        g = rh(d @ Ws[k])
    return dW, g


def composed(Ws, acts, x, vs, ubar, obar=None, half=True):
    """(dW per layer, dL/dx, dL/dv) as the composed route adds them up; see the module's docstring"""
    import torch

    dt = torch.float32 if half else torch.float64
    rh = (lambda t: t.half().to(dt)) if half else (lambda t: t)
    T = vs.shape[1]
    dW, dx, dv = None, None, []
    if obar is not None:
        dW, dx = first_order(Ws, acts, x, obar, half)
    for t in range(T):
        _, dW_t, dx_t = _restate(Ws, acts, x, ubar[:, t], vs[:, t], half)
        dW = dW_t if dW is None else [rh(a + b) for a, b in zip(dW, dW_t)]
        dx = dx_t.to(dt) if dx is None else dx + dx_t.to(dt)  # (dL/dinput is added in fp32)
        dv.append(first_order(Ws, acts, x, ubar[:, t], half)[1])
    return dW, dx, torch.stack(dv, dim=1)
