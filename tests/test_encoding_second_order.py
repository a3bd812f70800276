"""Second-order input gradients of the analytic encodings (Frequency, TriangleWave, SphericalHarmonics, Empty) and of the Composite
encoding in its three reductions (backward_backward_input: k_frequency_bwd_bwd_input, k_trianglewave_bwd_bwd_input, k_sh_bwd_bwd_input,
k_composite_reduce_bwd_bwd in k_encodings.hip; CompositeEncoding::backward_backward_input).

With x the input, v = dL_ddLdx and d = dL_dy, per sample:
  t  = dL_ddLdy = J v                       (the encoding's precision; zero in the padding columns)
  dx = dL_dx    = sum_j d_j (Hess y_j) v    (fp32)
Each analytic encoding is restated twice in torch on the CPU:
  R64  fp64 throughout, the mathematical function (the truth);
  Rh   the kernels' precision: fp32 in the kernels' operation order (the library is built without floating-point contraction), rounded to
       half where the kernels store a half; plain fp32 for float32 encodings.
The kernels must be as close to R64 as Rh is, up to a factor 2 (two realisations of the same rounding noise may differ by sqrt(2) in
norm; 2 is that rounded up).  R64's forward is pinned to the oracle, the recipes to torch.autograd's double backward in fp64, and the
Composite to its parts chained by hand from separate tcnn.Encoding modules."""
import ctypes
import math

import numpy as np
import pytest

# the recipes, restated: shared with the first-order per-element tests
from analytic_encoding_reference import _half_ulp, _restate, _triangle_inputs, _width

gpu = pytest.mark.gpu
LOSS_SCALE = 128.0
NOT_IMPLEMENTED = "backward_backward_input_impl: not implemented error"


def _inputs(cfg, n, n_in, pad, seed, half_d=True):
    """x in [0.02, 0.98), v in [-1, 1), d at loss scale (half-representable so that one d serves both precisions)"""
    import torch

    g = torch.Generator().manual_seed(seed)
    x = _triangle_inputs(n, n_in, seed) if cfg["otype"] == "TriangleWave" else torch.rand(n, n_in, generator=g) * 0.96 + 0.02
    v = torch.rand(n, n_in, generator=g) * 2 - 1
    d = ((torch.rand(n, _width(cfg, n_in) + pad, generator=g) * 2 - 1) * (LOSS_SCALE / n)).half().float()
    return x, v, d


# ---------------------------------------------------------------------------------------------------- CPU: R64 is the oracle's function
@pytest.mark.parametrize("kind,n_frequencies", [("frequency", 8), ("trianglewave", 12)])
def test_r64_forward_matches_oracle_periodic(oracle, kind, n_frequencies):
    """|oracle (fp32 arithmetic, stored as half) - R64| <= half an ulp of the half value + the fp32 rounding of the argument:
    2^-23 2^k pi |x| for Frequency; TriangleWave: the argument val = x 2^(k-1) + k/4 enters with slope 4, 4 * 2^-24 |val| for its
    rounding and as much again for the operations after it (val - floor - 0.5 is exact, |.| * 4 - 1 rounds once below 2^-24)."""
    import torch

    n, n_in = 512, 3
    cfg = {"otype": "Frequency" if kind == "frequency" else "TriangleWave", "n_frequencies": n_frequencies}
    x, v, d = _inputs(cfg, n, n_in, 4, seed=2)
    enc = oracle.PeriodicEncoding(n_in, cfg, kind)
    enc.n_to_pad = 4
    out, _ = enc.forward(x.numpy())
    got = torch.from_numpy(oracle.half_to_f32(out)).double()
    want, _, _ = _restate(cfg, x, v, d, 4, "r64")
    per = 2 * n_frequencies if kind == "frequency" else n_frequencies
    k = (torch.arange(n_in * per) % per) // (2 if kind == "frequency" else 1)
    if kind == "frequency":
        arg_error = 2.0 ** -23 * torch.pow(2.0, k.double())[None, :] * math.pi * x.double().repeat_interleave(per, dim=1)
    else:
        val = x.double().repeat_interleave(per, dim=1) * torch.pow(2.0, k.double() - 1)[None, :] + k.double()[None, :] * 0.25
        arg_error = 2.0 ** -22 * val.abs() + 2.0 ** -24
    live = n_in * per
    excess = (got[:, :live] - want[:, :live]).abs() - (_half_ulp(torch.maximum(want[:, :live].abs(), got[:, :live].abs())) + arg_error)
    print(f"{kind}: max excess over the tolerance {float(excess.max()):.3e} (negative: inside)")
    assert float(excess.max()) <= 0
    assert bool((got[:, live:] == 1).all()) and bool((want[:, live:] == 1).all())


@pytest.mark.parametrize("degree", [1, 4, 8])
def test_r64_forward_matches_oracle_spherical_harmonics(oracle, degree):
    """Same rule.  The fp32 part: every value is reached through at most 4 * degree + 8 rounded operations of the recurrences (the
    2 p - 1 of the argument, degree steps of (c, s), degree steps of q with 5 operations each, the normalisation and the final
    product), each within 2^-24 of a quantity no larger than the largest value of the row (or 1): (4 degree + 8) 2^-24 max(1, row max)."""
    import torch

    n = 512
    cfg = {"otype": "SphericalHarmonics", "degree": degree}
    x, v, d = _inputs(cfg, n, 3, 3, seed=4)
    enc = oracle.SphericalHarmonicsEncoding(3, cfg)
    enc.n_to_pad = 3
    out, _ = enc.forward(x.numpy())
    got = torch.from_numpy(oracle.half_to_f32(out)).double()
    want, _, _ = _restate(cfg, x, v, d, 3, "r64")
    fp32 = (4 * degree + 8) * 2.0 ** -24 * want[:, 3:].abs().max(dim=1, keepdim=True).values.clamp_min(1.0)
    excess = (got[:, 3:] - want[:, 3:]).abs() - (_half_ulp(torch.maximum(want[:, 3:].abs(), got[:, 3:].abs())) + fp32)
    print(f"degree {degree}: max excess over the tolerance {float(excess.max()):.3e} (negative: inside)")
    assert float(excess.max()) <= 0
    assert bool((got[:, :3] == 1).all()) and bool((want[:, :3] == 1).all())  # the padding comes first


# ---------------------------------------------------------------------------------------------------- CPU: the recipes are right
def _close(got, want, what):
    import torch

    err, norm = float(torch.linalg.norm(got - want)), float(torch.linalg.norm(want))
    print(f"{what}: |recipe - autograd| = {err:.3e}, |autograd| = {norm:.3e}")
    assert err <= 1e-10 * norm, (what, err, norm)


ANALYTIC = [("frequency_8", {"otype": "Frequency", "n_frequencies": 8}), ("trianglewave_12", {"otype": "TriangleWave", "n_frequencies": 12}),
            ("sh_1", {"otype": "SphericalHarmonics", "degree": 1}), ("sh_4", {"otype": "SphericalHarmonics", "degree": 4}),
            ("sh_8", {"otype": "SphericalHarmonics", "degree": 8}), ("empty", {"otype": "Empty"})]


@pytest.mark.parametrize("cfg", [c for _, c in ANALYTIC[:5]], ids=[i for i, _ in ANALYTIC[:5]])
def test_encoding_recipe_matches_autograd_double_backward(cfg):
    """R64's t and dx against torch.autograd in fp64: S = <v, dL/dx> differentiated with respect to dL/dy and x.  TriangleWave: the
    inputs avoid every kink, so autograd's sign (of |.|) is the kernel's (of floor(2 val))."""
    import torch

    n, pad = 64, 2
    x, v, d = _inputs(cfg, n, 3, pad, seed=6)
    _, t, dx = _restate(cfg, x, v, d, pad, "r64")
    if cfg == ANALYTIC[2][1]:  # degree 1: a constant, nothing for autograd to differentiate
        assert not t.any() and not dx.any()
        return
    xp = x.double().requires_grad_(True)
    dp = d.double().requires_grad_(True)
    y, _, _ = _restate(cfg, xp, v, d, pad, "r64")
    (gx,) = torch.autograd.grad(y, xp, grad_outputs=dp, create_graph=True)
    got_t, got_dx = torch.autograd.grad((gx * v.double()).sum(), [dp, xp], allow_unused=True)
    _close(t, got_t, "dL_ddLdy")
    if cfg["otype"] == "TriangleWave":
        assert not dx.any() and (got_dx is None or not got_dx.any())
    else:
        _close(dx, got_dx, "dL_dx")


class _SinePart:
    """A parametric stand-in for a nested encoding, y = sin(x W) on the input columns `cols`, with the three passes a nested
    encoding provides (written out by hand: they are what the Composite recipe calls, autograd sees only forward)"""

    def __init__(self, cols, W):
        self.cols, self.W = cols, W

    def forward(self, xs):
        import torch

        return torch.sin(xs @ self.W)

    def backward(self, xs, q):
        import torch

        qc = q * torch.cos(xs @ self.W)
        return qc @ self.W.T, xs.T @ qc

    def backward_backward_input(self, xs, vs, d):
        import torch

        z, zdot = xs @ self.W, vs @ self.W
        t = torch.cos(z) * zdot
        if d is None:
            return t, None, None
        r = -torch.sin(z) * zdot * d
        return t, r @ self.W.T, xs.T @ r + vs.T @ (torch.cos(z) * d)


def _chain(reduction, parts, x, v, d, up, store):
    """CompositeEncoding::backward_backward_input from its parts.  `up`: to the dtype the reductions compute in; `store`: to the
    dtype (and rounding) the encoding stores.  Returns dL_ddLdy, dL_dx, the parts' parameter gradients as (second-order pass,
    first-order pass on q or None) pairs."""
    import torch

    n = x.shape[0]
    dx = torch.zeros_like(x)
    xs = [x[:, p.cols].contiguous() for p in parts]
    vs = [v[:, p.cols].contiguous() for p in parts]
    ys = [p.forward(a) for p, a in zip(parts, xs)]
    ts, grads = [], []
    if reduction == "Concatenation":
        col = 0
        for p, a, b, y in zip(parts, xs, vs, ys):
            w = y.shape[1]
            t, dxi, gp = p.backward_backward_input(a, b, d[:, col:col + w].contiguous())
            dx[:, p.cols] = dxi
            ts.append(t)
            grads.append((gp, None))
            col += w
        return torch.cat(ts, dim=1), dx, grads
    if reduction == "Sum":
        total = torch.zeros_like(up(ys[0]))
        for p, a, b in zip(parts, xs, vs):
            t, dxi, gp = p.backward_backward_input(a, b, d)
            dx[:, p.cols] = dxi
            total = total + up(t)
            grads.append((gp, None))
        return store(total), dx, grads
    assert reduction == "Product"
    K = len(parts)
    for i, (p, a, b) in enumerate(zip(parts, xs, vs)):
        g = up(d)
        for k in range(K):  # the product of the other factors, multiplied up in nesting order
            if k != i:
                g = g * up(ys[k])
        t, dxi, gp = p.backward_backward_input(a, b, store(g))
        dx[:, p.cols] = dxi
        ts.append(t)
        grads.append([gp, None])

    def partial(i, skip):  # t_i times every factor outside `skip`, in nesting order
        term = up(ts[i])
        for m in range(K):
            if m not in skip:
                term = term * up(ys[m])
        return term

    total = torch.zeros_like(up(ys[0]))
    for i in range(K):
        total = total + partial(i, (i,))
    dx_more = torch.zeros_like(x)
    for k in range(K):
        inner = torch.zeros_like(up(ys[0]))
        for i in range(K):
            if i != k:
                inner = inner + partial(i, (i, k))
        dxk, gk = parts[k].backward(xs[k], store(up(d) * inner))
        dx_more[:, parts[k].cols] = dxk
        grads[k][1] = gk
    return store(total), dx + dx_more, [tuple(g) for g in grads]


@pytest.mark.parametrize("reduction", ["Concatenation", "Sum", "Product"])
def test_composite_recipe_matches_autograd_double_backward(reduction):
    """The Composite recipe in fp64 on three parametric parts (disjoint input slices, one dim that no part reads) against
    torch.autograd: dS/d(dL_dy), dS/dx and dS/dW of every part -- for the Product this covers the q_k pass"""
    import torch

    g = torch.Generator().manual_seed(8)
    n, w = 48, 5
    slices = [slice(0, 3), slice(3, 5), slice(6, 9)]  # dim 5 is read by nobody
    Ws = [torch.randn(s.stop - s.start, w, generator=g, dtype=torch.float64) for s in slices]
    x = torch.rand(n, 9, generator=g, dtype=torch.float64)
    v = torch.rand(n, 9, generator=g, dtype=torch.float64) * 2 - 1
    d = torch.rand(n, w * (3 if reduction == "Concatenation" else 1), generator=g, dtype=torch.float64) * 2 - 1
    same = lambda t: t  # noqa: E731
    ddy, dx, grads = _chain(reduction, [_SinePart(s, W) for s, W in zip(slices, Ws)], x, v, d, same, same)

    xp, dp = x.clone().requires_grad_(True), d.clone().requires_grad_(True)
    Wp = [W.clone().requires_grad_(True) for W in Ws]
    ys = [torch.sin(xp[:, s] @ W) for s, W in zip(slices, Wp)]
    y = torch.cat(ys, dim=1) if reduction == "Concatenation" else (ys[0] + ys[1] + ys[2] if reduction == "Sum" else ys[0] * ys[1] * ys[2])
    (gx,) = torch.autograd.grad(y, xp, grad_outputs=dp, create_graph=True)
    got = torch.autograd.grad((gx * v).sum(), [dp, xp] + Wp)
    _close(ddy, got[0], "dL_ddLdy")
    _close(dx, got[1], "dL_dx")
    assert not dx[:, 5].any() and not got[1][:, 5].any()
    for k, (a, b) in enumerate(grads):
        assert (b is not None) == (reduction == "Product")
        _close(a if b is None else a + b, got[2 + k], f"dL_dW[{k}]")


# ---------------------------------------------------------------------------------------------------- GPU helpers
def _bits(t):
    import torch

    return t.view(torch.int16 if t.dtype == torch.half else torch.int32)


def _native_second_order(tcnn, n_in, cfg, dtype, x, v, d, params=None):
    """(module, context, x, params, d on the device, (dL_ddLdy, dL_dparams, dL_dx)) of one bwd_bwd_input call on a tcnn.Encoding"""
    import torch

    enc = tcnn.Encoding(n_in, cfg, dtype=dtype)
    native = enc.native_tcnn_module
    xt = x.cuda().requires_grad_(True)
    if params is None:
        params = torch.zeros(native.n_params(), dtype=dtype, device="cuda")
    pt = params.clone().requires_grad_(True)
    dt = d.to(dtype).cuda().requires_grad_(True)
    ctx, y = native.fwd(xt, pt)
    return native, ctx, xt, pt, dt, y, native.bwd_bwd_input(ctx, xt, pt, v.cuda(), dt)


# ---------------------------------------------------------------------------------------------------- 1. single encodings
@gpu
@pytest.mark.parametrize("precision", ["half", "float32"])
@pytest.mark.parametrize("cfg", [c for _, c in ANALYTIC], ids=[i for i, _ in ANALYTIC])
def test_analytic_encoding_second_order_matches_restatement(tcnn, cfg, precision):
    import torch

    n, n_in = 4096, 3
    dtype = torch.half if precision == "half" else torch.float32
    x, v, d = _inputs(cfg, n, n_in, 0, seed=12)
    native, ctx, xt, pt, dt, y, (ddy, dparams, dx) = _native_second_order(tcnn, n_in, cfg, dtype, x, v, d)
    assert ddy.dtype == dtype and ddy.shape == (n, _width(cfg, n_in)) and dx.dtype == torch.float32 and dparams.numel() == 0
    y64, t64, dx64 = _restate(cfg, x, v, d, 0, "r64")
    yh, th, dxh = _restate(cfg, x, v, d, 0, "half" if precision == "half" else "f32")
    failures = []
    for what, ours, h, ref in (("forward", y, yh, y64), ("dL_ddLdy", ddy, th, t64), ("dL_dx", dx, dxh, dx64)):
        ours, h = ours.detach().cpu().double(), h.double()
        e_ours, e_h, norm = float(torch.linalg.norm(ours - ref)), float(torch.linalg.norm(h - ref)), float(torch.linalg.norm(ref))
        print(f"{cfg} {precision} {what:9s} |ours-R64| {e_ours:.3e}  |Rh-R64| {e_h:.3e}  |R64| {norm:.3e}")
        if not e_ours <= 2 * e_h:
            failures.append((what, e_ours, e_h))
        if not bool((ours[ref == 0] == 0).all()):
            failures.append((what, "nonzero where R64 is exactly zero"))
    assert not failures, failures
    if cfg["otype"] in ("TriangleWave", "Empty") or cfg == ANALYTIC[2][1]:
        assert not _bits(dx).any()  # all bits zero
    else:
        assert float(dx.abs().sum()) > 0 and float(ddy.float().abs().sum()) > 0

    # two runs give the same bits
    ddy2, _, dx2 = native.bwd_bwd_input(ctx, xt, pt, v.cuda(), dt)
    assert torch.equal(_bits(ddy2), _bits(ddy)) and torch.equal(_bits(dx2), _bits(dx))
    # only what is asked for comes back
    ddy3, dparams3, dx3 = native.bwd_bwd_input(ctx, xt, pt.detach(), v.cuda(), dt.detach())
    assert ddy3 is None and dparams3 is None and torch.equal(_bits(dx3), _bits(dx))
    ddy4, dparams4, dx4 = native.bwd_bwd_input(ctx, xt.detach(), pt.detach(), v.cuda(), dt)
    assert dx4 is None and dparams4 is None and torch.equal(_bits(ddy4), _bits(ddy))


GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5, "interpolation": "Smoothstep"}
GRID_B = {**GRID, "base_resolution": 5, "log2_hashmap_size": 11}
GRID_F8 = {**GRID, "n_levels": 1, "n_features_per_level": 8}


PADDED = [("frequency_3", {"otype": "Frequency", "n_frequencies": 3}), ("trianglewave_12", {"otype": "TriangleWave", "n_frequencies": 12}),
          ("sh_1", {"otype": "SphericalHarmonics", "degree": 1}), ("sh_3", {"otype": "SphericalHarmonics", "degree": 3})]


@gpu
@pytest.mark.parametrize("precision", ["half", "float32"])
@pytest.mark.parametrize("cfg", [c for _, c in PADDED], ids=[i for i, _ in PADDED])
def test_padding_columns_of_the_tangent_are_zero_bits(tcnn, cfg, precision):
    """A nested encoding is padded so that the next one starts at a multiple of ITS alignment: in front of a grid with 8 features per
    level the encoding under test (18, 36, 1, 9 columns) is padded to a multiple of 8.  Its padding columns hold ones in the output and
    zero bits in dL_ddLdy; its live columns are those of the encoding on its own."""
    import torch

    n, n_in = 1024, 3
    dtype = torch.half if precision == "half" else torch.float32
    w = _width(cfg, n_in)
    pw = -(-w // 8) * 8
    assert pw > w
    composite = {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, **cfg}, {"n_dims_to_encode": 3, **GRID_F8}]}
    x, v, d = _inputs(cfg, n, n_in, 0, seed=16)
    g = torch.Generator().manual_seed(17)
    x6 = torch.cat([x, torch.rand(n, 3, generator=g) * 0.96 + 0.02], dim=1)
    v6 = torch.cat([v, torch.rand(n, 3, generator=g) * 2 - 1], dim=1)
    first = cfg["otype"] == "SphericalHarmonics"  # its padding comes first
    live = slice(pw - w, pw) if first else slice(0, w)
    pad = slice(0, pw - w) if first else slice(w, pw)
    d6 = ((torch.rand(n, pw + 8, generator=g) * 2 - 1) * (LOSS_SCALE / n)).half().float()
    d6[:, live] = d
    enc = tcnn.Encoding(6, composite, dtype=dtype)
    assert enc.n_output_dims == pw + 8
    params = ((torch.rand(enc.native_tcnn_module.n_params(), device="cuda") * 2 - 1)).to(dtype)
    _, _, _, _, _, y, (ddy, _, dx) = _native_second_order(tcnn, 6, composite, dtype, x6, v6, d6, params)
    assert bool((y[:, pad] == 1).all()) and not _bits(ddy[:, pad].contiguous()).any()
    _, _, _, _, _, _, (alone_ddy, _, alone_dx) = _native_second_order(tcnn, n_in, cfg, dtype, x, v, d)
    assert torch.equal(_bits(ddy[:, live].contiguous()), _bits(alone_ddy)) and torch.equal(_bits(dx[:, :3].contiguous()), _bits(alone_dx))
    if cfg["otype"] != "TriangleWave" and cfg != ANALYTIC[2][1]:
        assert float(alone_dx.abs().sum()) > 0 and float(alone_ddy.float().abs().sum()) > 0
    assert float(ddy[:, pw:].float().abs().sum()) > 0 and float(dx[:, 3:].abs().sum()) > 0  # the grid behind it did its part


@gpu
def test_empty_encoding_pads_with_a_zero_tangent(tcnn):
    """Empty has no columns of its own; as the last nested encoding of a model's input layer it absorbs the padding (ones).  With a
    zero tangent there, Composite[Frequency on 3 dims, Empty on the 4th] -> CutlassMLP gives bit for bit what Frequency -> CutlassMLP
    gives (Frequency pads its own 12 columns to 16 the same way), and the 4th input dim gets zero bits."""
    import torch

    from test_network_second_order import _net_cfg

    torch.manual_seed(19)
    n = 1024
    freq = {"otype": "Frequency", "n_frequencies": 2}
    net_cfg = _net_cfg(64, 2, "Softplus")
    with_empty = tcnn.NetworkWithInputEncoding(4, 1, {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, **freq}, {"otype": "Empty"}]}, net_cfg).native_tcnn_module
    plain = tcnn.NetworkWithInputEncoding(3, 1, freq, net_cfg).native_tcnn_module
    assert with_empty.hyperparams()["encoding"]["nested"][1]["otype"] == "Empty" and with_empty.n_params() == plain.n_params()
    p = ((torch.rand(plain.n_params(), device="cuda") * 2 - 1) * 0.25).half().requires_grad_(True)
    x = (torch.rand(n, 4, device="cuda") * 0.96 + 0.02)
    v = torch.rand(n, 4, device="cuda") * 2 - 1
    dy = ((torch.rand(n, 16, device="cuda") * 2 - 1) * (LOSS_SCALE / n)).half().requires_grad_(True)
    x4 = x.clone().requires_grad_(True)
    x3 = x[:, :3].contiguous().requires_grad_(True)
    ctx4, y4 = with_empty.fwd(x4, p)
    ctx3, y3 = plain.fwd(x3, p)
    assert torch.equal(y4, y3)
    ddy4, g4, dx4 = with_empty.bwd_bwd_input(ctx4, x4, p, v, dy)
    ddy3, g3, dx3 = plain.bwd_bwd_input(ctx3, x3, p, v[:, :3].contiguous(), dy)
    assert torch.equal(_bits(ddy4), _bits(ddy3)) and torch.equal(_bits(g4), _bits(g3))
    assert torch.equal(_bits(dx4[:, :3].contiguous()), _bits(dx3)) and not _bits(dx4[:, 3].contiguous()).any()
    assert float(ddy3.float().abs().sum()) > 0 and float(dx3.abs().sum()) > 0 and float(g3.float().abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------- 2. Composite against its parts
class _NativePart:
    """One tcnn.Encoding on the input columns `cols` with its own parameters: the nested encoding of a Composite, as a module"""

    def __init__(self, tcnn, cols, cfg, dtype, params):
        import torch

        self.cols = cols
        self.enc = tcnn.Encoding(cols.stop - cols.start, cfg, dtype=dtype)
        self.native = self.enc.native_tcnn_module
        assert self.native.n_params() == params.numel()
        self.params = params.clone().requires_grad_(params.numel() > 0)
        self.dtype = dtype
        self.torch = torch

    def forward(self, xs):
        self.x = xs.clone().requires_grad_(True)
        self.ctx, self.y = self.native.fwd(self.x, self.params)
        return self.y

    def backward(self, xs, q):
        dx, gp = self.native.bwd(self.ctx, self.x, self.params, self.y, q.contiguous())
        return dx, gp

    def backward_backward_input(self, xs, vs, d):
        t, gp, dx = self.native.bwd_bwd_input(self.ctx, self.x, self.params, vs, d.contiguous().requires_grad_(True))
        return t, dx, gp


def _untouched_parameters(tcnn, cfg, xs):
    """Which parameters of a grid no sample touches: the float32 form of the grid, first-order gradient of sum(y).  The interpolation
    weights are non-negative, so with dL_dy = 1 nothing cancels and nothing underflows: a parameter is touched exactly where that
    gradient is nonzero.  (A zero in a half gradient proves nothing: touched parameters cancel or round to zero there, differently
    from run to run with the order of the atomics.)"""
    import torch

    native = tcnn.Encoding(xs.shape[1], cfg, dtype=torch.float32).native_tcnn_module
    p = torch.zeros(native.n_params(), device="cuda").requires_grad_(True)
    ctx, y = native.fwd(xs.contiguous(), p)
    _, g = native.bwd(ctx, xs.contiguous(), p, y, torch.ones_like(y))
    return g == 0


FREQ3 = {"otype": "Frequency", "n_frequencies": 3}
SH3 = {"otype": "SphericalHarmonics", "degree": 3}
COMPOSITES = [
    # (id, reduction, [(input columns, nested config)])
    ("concat_grid_frequency_sh", "Concatenation", [(slice(0, 3), GRID), (slice(3, 6), FREQ3), (slice(6, 9), SH3)]),
    ("sum_two_grids", "Sum", [(slice(0, 3), GRID), (slice(3, 6), GRID_B)]),
    ("product_two_grids", "Product", [(slice(0, 3), GRID), (slice(3, 6), GRID_B)]),
    ("product_grid_frequency", "Product", [(slice(0, 3), GRID), (slice(3, 5), {"otype": "Frequency", "n_frequencies": 2})]),  # 8 columns each
]


def _composite_cfg(reduction, nested):
    return {"otype": "Composite", "reduction": reduction,
            "nested": [{"n_dims_to_encode": c.stop - c.start, "dims_to_encode_begin": c.start, **cfg} for c, cfg in nested]}


def _composite_case(tcnn, reduction, nested, n, dtype, seed):
    import torch

    torch.manual_seed(seed)
    n_in = max(c.stop for c, _ in nested)
    cfg = _composite_cfg(reduction, nested)
    enc = tcnn.Encoding(n_in, cfg, dtype=dtype)
    native = enc.native_tcnn_module
    params = (torch.rand(native.n_params(), device="cuda") * 2 - 1).to(dtype)
    x = torch.rand(n, n_in, device="cuda") * 0.96 + 0.02
    v = torch.rand(n, n_in, device="cuda") * 2 - 1
    d = ((torch.rand(n, enc.n_output_dims, device="cuda") * 2 - 1) * (LOSS_SCALE / n)).to(dtype)
    return enc, native, params, x, v, d


@gpu
@pytest.mark.parametrize("precision", ["half", "float32"])
@pytest.mark.parametrize("case", COMPOSITES, ids=[c[0] for c in COMPOSITES])
def test_composite_matches_parts_chained_by_hand(tcnn, case, precision):
    """dL_ddLdy and dL_dx bit for bit (the reductions restated in torch on the device: fp32 sums and products in nesting order, one
    rounding per stored value), the grids' parameter gradients within 2e-2 in norm (packed-fp16 atomics, the bound of
    test_composition_matches_hand_assembled_pipeline), zeros where no sample touches a parameter"""
    import torch

    _, reduction, nested = case
    dtype = torch.half if precision == "half" else torch.float32
    n = 1024
    enc, native, params, x, v, d = _composite_case(tcnn, reduction, nested, n, dtype, seed=21)
    xt, pt, dt = x.clone().requires_grad_(True), params.clone().requires_grad_(True), d.clone().requires_grad_(True)
    ctx, y = native.fwd(xt, pt)
    ddy, dparams, dx = native.bwd_bwd_input(ctx, xt, pt, v, dt)

    parts, off = [], 0
    for cols, cfg in nested:
        k = tcnn.Encoding(cols.stop - cols.start, cfg, dtype=dtype).native_tcnn_module.n_params()
        parts.append(_NativePart(tcnn, cols, cfg, dtype, params[off:off + k]))
        off += k
    assert off == params.numel()
    want_ddy, want_dx, grads = _chain(reduction, parts, x, v, d, lambda t: t.float(), lambda t: t.to(dtype))
    assert torch.equal(_bits(ddy), _bits(want_ddy))
    assert torch.equal(_bits(dx), _bits(want_dx))
    assert float(ddy.float().abs().sum()) > 0 and float(dx.abs().sum()) > 0
    off = 0
    for part, (a, b) in zip(parts, grads):
        k = part.params.numel()
        if k == 0:
            continue
        got = dparams[off:off + k].float()
        want = a.float() if b is None else a.float() + b.float()
        untouched = _untouched_parameters(tcnn, nested[parts.index(part)][1], x[:, part.cols])
        assert 0 < int(untouched.sum()) < k
        err, norm = float(torch.linalg.norm(got - want)), float(torch.linalg.norm(want))
        print(f"{case[0]} {precision} parameters [{off}, {off + k}): |ours - chained| / |chained| = {err / norm:.3e}; untouched {int(untouched.sum())} of {k}")
        assert norm > 0 and err <= 2e-2 * norm
        assert bool((got[untouched] == 0).all())
        off += k

    # determinism outside the grids' scatter, and only what is asked for
    ddy2, _, dx2 = native.bwd_bwd_input(ctx, xt, pt, v, dt)
    assert torch.equal(_bits(ddy2), _bits(ddy)) and torch.equal(_bits(dx2), _bits(dx))
    ddy3, dparams3, dx3 = native.bwd_bwd_input(ctx, xt, pt.detach(), v, dt.detach())
    assert ddy3 is None and dparams3 is None and torch.equal(_bits(dx3), _bits(dx))
    ddy4, dparams4, dx4 = native.bwd_bwd_input(ctx, xt.detach(), pt.detach(), v, dt)
    assert dx4 is None and dparams4 is None and torch.equal(_bits(ddy4), _bits(ddy))


@gpu
def test_composite_input_dims_nobody_reads_and_max_level(tcnn):
    """An input dim outside every nested slice gets zero bits in dL_dx; a nested grid sees the module's max_level in the second-order
    pass as in the first-order ones (levels beyond it: zero tangent, zero gradient)"""
    import torch

    nested = [(slice(0, 3), GRID), (slice(4, 7), FREQ3)]  # dim 3 is read by nobody
    n = 1024
    enc, native, params, x, v, d = _composite_case(tcnn, "Concatenation", nested, n, torch.half, seed=23)
    xt, pt, dt = x.clone().requires_grad_(True), params.clone().requires_grad_(True), d.clone().requires_grad_(True)
    ctx, _ = native.fwd(xt, pt)
    ddy, dparams, dx = native.bwd_bwd_input(ctx, xt, pt, v, dt)
    assert not _bits(dx[:, 3].contiguous()).any() and float(dx[:, :3].abs().sum()) > 0 and float(dx[:, 4:].abs().sum()) > 0

    part = _NativePart(tcnn, slice(0, 3), GRID, torch.half, params)
    native.set_max_level(0.5)  # 0.5 * 4 levels: levels 0..2 stay on (a level l is cut when l >= max_level * n_levels + 1e-3), the fourth is cut
    part.native.set_max_level(0.5)
    ctx, _ = native.fwd(xt, pt)
    ddy_cut, dparams_cut, dx_cut = native.bwd_bwd_input(ctx, xt, pt, v, dt)
    part.forward(x[:, :3].contiguous())
    t, dx_part, g_part = part.backward_backward_input(None, v[:, :3].contiguous(), d[:, :8].contiguous())
    assert torch.equal(_bits(ddy_cut[:, :8].contiguous()), _bits(t)) and torch.equal(_bits(dx_cut[:, :3].contiguous()), _bits(dx_part))
    assert not _bits(ddy_cut[:, 6:8].contiguous()).any() and float(ddy[:, 6:8].float().abs().sum()) > 0
    assert torch.equal(_bits(ddy_cut[:, :6].contiguous()), _bits(ddy[:, :6].contiguous()))
    assert torch.equal(_bits(ddy_cut[:, 8:].contiguous()), _bits(ddy[:, 8:].contiguous()))  # the Frequency part has no levels to cut
    err, norm = float(torch.linalg.norm(dparams_cut.float() - g_part.float())), float(torch.linalg.norm(g_part.float()))
    assert norm > 0 and err <= 2e-2 * norm and bool((dparams_cut[g_part == 0] == 0).all())


# ---------------------------------------------------------------------------------------------------- 3. gradient modes through the C ABI
def _bbi_mode(native, ctx, x, params, v, dy, grads, mode):
    import torch

    from tinycudann import _C

    n = x.shape[0]
    ddy = torch.zeros((n, native.n_output_dims()), dtype=dy.dtype, device="cuda")
    dx = torch.zeros_like(x)
    _C.check(_C.lib.tcnn_module_backward_backward_input_mode(native._h, torch.cuda.current_stream().cuda_stream, ctx._h, n, v.data_ptr(), x.data_ptr(), dy.data_ptr(),
                                                             grads.data_ptr(), ddy.data_ptr(), dx.data_ptr(), params.data_ptr(), ctypes.c_int(mode)))
    torch.cuda.synchronize()
    return ddy, dx


@gpu
@pytest.mark.parametrize("case", [COMPOSITES[0], COMPOSITES[3]], ids=[COMPOSITES[0][0], COMPOSITES[3][0]])
def test_composite_gradient_modes_through_c_abi(tcnn, case):
    """Overwrite ignores what the gradient buffer holds; Accumulate twice doubles the gradient -- within the bounds of
    test_gradient_modes_through_c_abi (2e-2 in norm: the grid's packed-fp16 atomics).  The Product case accumulates its q pass
    onto the second-order gradients inside one call in either mode."""
    import torch

    from tinycudann.native import GRADIENT_ACCUMULATE, GRADIENT_OVERWRITE

    _, reduction, nested = case
    enc, native, params, x, v, d = _composite_case(tcnn, reduction, nested, 1024, torch.half, seed=27)
    x.requires_grad_(True)
    ctx, _ = native.fwd(x, params.clone().requires_grad_(True))

    clean = torch.zeros_like(params)
    ddy, dx = _bbi_mode(native, ctx, x, params, v, d, clean, GRADIENT_OVERWRITE)
    poisoned = torch.full_like(params, 777.0)
    ddy2, dx2 = _bbi_mode(native, ctx, x, params, v, d, poisoned, GRADIENT_OVERWRITE)
    norm = float(torch.linalg.norm(clean.float()))
    assert norm > 0
    assert float(torch.linalg.norm(poisoned.float() - clean.float())) <= 2e-2 * norm and float(poisoned.float().abs().max()) < 700
    assert torch.equal(ddy2, ddy) and torch.equal(dx2, dx)

    twice = torch.zeros_like(params)
    _bbi_mode(native, ctx, x, params, v, d, twice, GRADIENT_ACCUMULATE)
    once = twice.clone()
    _bbi_mode(native, ctx, x, params, v, d, twice, GRADIENT_ACCUMULATE)
    assert float(torch.linalg.norm(once.float() - clean.float())) <= 2e-2 * norm
    assert float(torch.linalg.norm(twice.float() - 2 * clean.float())) <= 2e-2 * 2 * norm


# ---------------------------------------------------------------------------------------------------- 4. behind a network
@gpu
@pytest.mark.parametrize("act", ["Softplus", "ReLU"])
def test_composite_behind_network_matches_hand_assembled_pipeline(tcnn, act):
    """NetworkWithInputEncoding(6 -> 1, Composite[HashGrid, Frequency], CutlassMLP 64 x 2) against the Composite as a tcnn.Encoding
    and a tcnn.Network chained by hand: the criteria of test_composition_matches_hand_assembled_pipeline.  (8 + 24 = 32 encoded
    columns: the model adds no padding, so the hand-made zero padding of that helper is empty.)"""
    import torch

    from test_network_second_order import _composed_by_hand, _net_cfg

    torch.manual_seed(3)
    n, n_in, n_out = 1024, 6, 1
    enc_cfg = _composite_cfg("Concatenation", [(slice(0, 3), GRID), (slice(3, 6), {"otype": "Frequency", "n_frequencies": 4})])
    net_cfg = _net_cfg(64, 2, act)
    model = tcnn.NetworkWithInputEncoding(n_in, n_out, enc_cfg, net_cfg)
    native = model.native_tcnn_module
    n_net = 32 * 64 + 64 * 64 + 64 * 16
    n_enc = native.n_params() - n_net
    assert n_enc == tcnn.Encoding(3, GRID).native_tcnn_module.n_params()
    p_net = ((torch.rand(n_net, device="cuda") * 2 - 1) * 0.25).half()
    p_enc = (torch.rand(n_enc, device="cuda") * 2 - 1).half()
    x = torch.rand(n, n_in, device="cuda") * 0.96 + 0.02
    v = torch.rand(n, n_in, device="cuda") * 2 - 1
    dy = ((torch.rand(n, 16, device="cuda") * 2 - 1) * (LOSS_SCALE / n)).half()

    xt = x.clone().requires_grad_(True)
    pt = torch.cat([p_net, p_enc]).requires_grad_(True)
    ctx, _ = native.fwd(xt, pt)
    ddy, dparams, dx = native.bwd_bwd_input(ctx, xt, pt, v, dy.clone().requires_grad_(True))

    want_ddy, want_net, want_enc, _, want_dx, curved = _composed_by_hand(tcnn, enc_cfg, net_cfg, n_in, n_out, x, v, dy, p_net, p_enc)
    assert curved == (act == "Softplus")
    assert torch.equal(ddy.view(torch.int16), want_ddy.view(torch.int16))
    assert torch.equal(dx.view(torch.int32), want_dx.view(torch.int32))
    assert torch.equal(dparams[:n_net].view(torch.int16), want_net.view(torch.int16))
    got_enc = dparams[n_net:].float()
    err, norm = float(torch.linalg.norm(got_enc - want_enc)), float(torch.linalg.norm(want_enc))
    print(f"encoding slice: |ours - composed| / |composed| = {err / norm:.3e}")
    assert norm > 0 and err <= 2e-2 * norm
    untouched = _untouched_parameters(tcnn, GRID, x[:, :3])  # (the helper's own mask reads zeros of half sums, which also arise by cancellation)
    assert 0 < int(untouched.sum()) < n_enc and bool((got_enc[untouched] == 0).all())
    assert float(dx[:, :3].abs().sum()) > 0 and float(dx[:, 3:].abs().sum()) > 0 and float(ddy.float().abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------- 5. through PyTorch
@gpu
def test_composite_double_backward_through_torch(tcnn):
    """The eikonal pattern of test_encoding_double_backward_through_torch on an fp32 Composite (Smoothstep grid + Frequency + SH):
    y = enc(x); g = d(sum w y)/dx with create_graph; loss = <g, c>; d loss / dx against central differences of g, d loss / d params
    along a random direction, same thresholds"""
    import torch

    torch.manual_seed(0)
    cfg = _composite_cfg("Concatenation", [(slice(0, 3), GRID), (slice(3, 6), FREQ3), (slice(6, 9), SH3)])
    enc = tcnn.Encoding(9, cfg, dtype=torch.float32)
    with torch.no_grad():
        enc.params.copy_(torch.rand_like(enc.params) * 2 - 1)
    n = 256
    x0 = torch.rand(n, 9, device="cuda") * 0.9 + 0.05
    w = (torch.rand(enc.n_output_dims, device="cuda") - 0.5).requires_grad_(True)
    c = torch.rand(n, 9, device="cuda") - 0.5

    def grad_of(x):
        (g,) = torch.autograd.grad((enc(x).float() * w).sum(), x, create_graph=True)
        return g

    x = x0.clone().requires_grad_(True)
    loss = (grad_of(x) * c).sum()
    gx, gp, gw = torch.autograd.grad(loss, [x, enc.params, w])

    eps = 1e-3
    fd = torch.zeros_like(x0)
    for k in range(9):
        e = torch.zeros(9, device="cuda")
        e[k] = eps
        gp_ = grad_of((x0 + e).requires_grad_(True)).detach()
        gm_ = grad_of((x0 - e).requires_grad_(True)).detach()
        fd[:, k] = ((gp_ - gm_) * c).sum(1) / (2 * eps)
    for name, cols in (("grid", slice(0, 3)), ("frequency", slice(3, 6)), ("sh", slice(6, 9))):
        err = (fd[:, cols] - gx[:, cols]).abs().max(1).values / (gx[:, cols].abs().max() + 1e-12)
        print(f"{name}: median relative difference to central differences {float(err.median()):.3e}")
        assert (err < 3e-2).float().mean() > 0.85, (name, float(err.median()))
        assert float(gx[:, cols].abs().sum()) > 0

    direction = torch.randn_like(enc.params)
    h = 1e-2
    with torch.no_grad():
        base = enc.params.clone()
        enc.params.copy_(base + h * direction)
    lp = (grad_of(x0.clone().requires_grad_(True)).detach() * c).sum()
    with torch.no_grad():
        enc.params.copy_(base - h * direction)
    lm = (grad_of(x0.clone().requires_grad_(True)).detach() * c).sum()
    with torch.no_grad():
        enc.params.copy_(base)
    fd_dir, an_dir = float((lp - lm) / (2 * h)), float((gp * direction).sum())
    assert abs(fd_dir - an_dir) <= 2e-2 * abs(an_dir) + 1e-3, (fd_dir, an_dir)
    assert gw.shape == w.shape and float(gw.abs().sum()) > 0


@gpu
def test_sdf_fit_with_eikonal_term_through_composite(tcnn):
    """[p, p] -> Composite[HashGrid, Frequency(6)] -> CutlassMLP 64 x 2 Softplus fitted to a sphere's signed distance plus
    0.1 * eikonal with Adam: every loss finite, and | |grad f| - 1 | over a fixed probe set lower at the end than at the start (a
    sanity condition, not a measurement)"""
    import torch

    from test_network_second_order import _net_cfg

    torch.manual_seed(0)
    grid = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 4, "per_level_scale": 1.5, "interpolation": "Smoothstep"}
    enc = _composite_cfg("Concatenation", [(slice(0, 3), grid), (slice(3, 6), {"otype": "Frequency", "n_frequencies": 6})])
    model = tcnn.NetworkWithInputEncoding(6, 1, enc, _net_cfg(64, 2, "Softplus"))
    opt = torch.optim.Adam(model.parameters(), lr=2e-3, eps=1e-15)
    probe = torch.rand(4096, 3, device="cuda") * 0.9 + 0.05

    def field(p):
        return model(torch.cat([p, p], dim=1)).float()[:, 0]

    def eikonal_error(points):
        p = points.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(field(p).sum(), p, create_graph=True)
        return (g.norm(dim=1) - 1).abs().mean().detach()

    before = float(eikonal_error(probe))
    for step in range(300):
        pts = torch.rand(4096, 3, device="cuda") * 0.9 + 0.05
        sdf = (pts - 0.5).norm(dim=1) - 0.3
        p = pts.clone().requires_grad_(True)
        f = field(p)
        (g,) = torch.autograd.grad(f.sum(), p, create_graph=True)
        loss = ((f - sdf) ** 2).mean() + 0.1 * ((g.norm(dim=1) - 1) ** 2).mean()
        assert bool(torch.isfinite(loss)), (step, float(loss))
        opt.zero_grad()
        loss.backward()
        opt.step()
    after = float(eikonal_error(probe))
    print(f"mean | |grad f| - 1 | over the probe set: {before:.4f} before, {after:.4f} after 300 steps")
    assert after < before


# ---------------------------------------------------------------------------------------------------- 6. boundaries
@gpu
def test_composites_with_oneblob_still_raise_and_leave_the_module_usable(tcnn):
    import torch

    from test_network_second_order import _net_cfg

    with_oneblob = _composite_cfg("Concatenation", [(slice(0, 3), GRID), (slice(3, 8), {"otype": "OneBlob", "n_bins": 4})])
    x = (torch.rand(256, 8, device="cuda") * 0.9 + 0.05).requires_grad_(True)
    for make in (lambda: tcnn.Encoding(8, with_oneblob), lambda: tcnn.Encoding(8, {"otype": "OneBlobFrequency", "n_frequencies": 4, "n_bins": 4}),
                 lambda: tcnn.Encoding(8, {"otype": "NRC", "n_frequencies": 4, "n_bins": 4}),
                 lambda: tcnn.NetworkWithInputEncoding(8, 1, with_oneblob, _net_cfg(64, 2, "Softplus")),
                 lambda: tcnn.NetworkWithInputEncoding(8, 1, {"otype": "OneBlobFrequency"}, _net_cfg(64, 2, "Softplus"))):
        module = make()
        native = module.native_tcnn_module
        p = module.params.detach().half().requires_grad_(True)
        ctx, out = native.fwd(x, p)
        dy = torch.rand_like(out)
        before = native.bwd(ctx, x, p, out, dy)
        with pytest.raises(RuntimeError, match=NOT_IMPLEMENTED):
            native.bwd_bwd_input(ctx, x, p, torch.rand_like(x), dy.clone().requires_grad_(True))
        # the module and the context are as they were: the first-order pass gives what it gave (dL_dinput has no atomics)
        after = native.bwd(ctx, x, p, out, dy)
        assert torch.equal(after[0], before[0]) and bool(torch.isfinite(after[1].float()).all())
        ctx2, out2 = native.fwd(x, p)
        assert torch.equal(out2, out)


@gpu
def test_context_without_input_gradients_is_rejected(tcnn):
    """backward()'s message for a context whose forward pass did not prepare input gradients; the next valid call is right"""
    import torch

    from test_network_second_order import _net_cfg

    torch.manual_seed(9)
    enc_cfg = _composite_cfg("Concatenation", [(slice(0, 3), GRID), (slice(3, 6), {"otype": "Frequency", "n_frequencies": 4})])
    model = tcnn.NetworkWithInputEncoding(6, 1, enc_cfg, _net_cfg(64, 2, "Softplus"))
    native = model.native_tcnn_module
    p = model.params.detach().half().requires_grad_(True)
    x = torch.rand(256, 6, device="cuda") * 0.9 + 0.05
    v = torch.rand_like(x)
    ctx_no_input, out = native.fwd(x, p)  # the input does not require a gradient: no input gradients prepared
    dy = torch.rand_like(out).requires_grad_(True)
    with pytest.raises(RuntimeError, match="input gradients were not prepared"):
        native.bwd_bwd_input(ctx_no_input, x.clone().requires_grad_(True), p, v, dy)
    xg = x.clone().requires_grad_(True)
    ctx, _ = native.fwd(xg, p)
    first = native.bwd_bwd_input(ctx, xg, p, v, dy)
    model2 = tcnn.NetworkWithInputEncoding(6, 1, enc_cfg, _net_cfg(64, 2, "Softplus"))  # a module that never saw the rejected call
    ctx2, _ = model2.native_tcnn_module.fwd(xg, p)
    second = model2.native_tcnn_module.bwd_bwd_input(ctx2, xg, p, v, dy)
    assert torch.equal(first[0], second[0]) and torch.equal(first[2], second[2]) and float(first[2].abs().sum()) > 0
