"""Training through input_jvp on the GPU: tcnn_module_input_jvp_forward / _backward -- the gradients of
L = sum_t <dL_djvp_t, J(x) v_t> + <dL_doutput, f(x)> by parameters, input and tangents -- and tcnn.Module.input_jvp(differentiable=True).

1. The composed route ("two-pass") gives, for modules that have a second-order pass, the bits of the public calls chained by hand in the
   route's order: forward(prepare_input_gradients); backward(dL_doutput) if there is one; per tangent backward_backward_input_mode(
   dL_ddLdinput = v_t, dL_doutput = dL_djvp_t) -- TCNN_GRADIENT_ACCUMULATE once something was written -- with dL_dinput added in fp32, and
   backward(dL_doutput = dL_djvp_t) for dL_dtangents[:, t].  A grid's parameter gradients are packed-half atomics in arbitrary order in its
   second-order kernel: tests/test_grid_second_order.py holds one run within 2e-2 (norm) of the fp32 sum, so two runs -- the call and the
   hand-made chain -- lie within twice that of each other.  (Measured: 6e-4 to 9e-4.  No element-wise claim: three or more contributions
   that cancel to an exact zero in one order leave a rounding residue in another.)
2. Half fused-shape networks (the nine shapes of tests/test_input_jvp_gpu.py, restated) on the route the plan names: jvp and output have
   input_jvp's and inference's bits; every layer's dL_dparams, dL_dinput and each dL_dtangents[:, t] meet ||ours - R64|| <= 2 ||Rh - R64||
   with the guard ||Rh - R64|| <= 0.05 ||R64|| (R64, Rh: tests/input_jvp_backward_reference.py; the factor 2 is
   tests/test_network_second_order.py's); piecewise linear networks have all-zero bits in the tangents' dL_dinput; two runs give the same
   bits; rows keep their bits at another batch position; Accumulate onto zeros is Overwrite, and onto a known buffer, with dL_doutput
   given, it is Overwrite plus the buffer within the rounding of the route's stores (_check_accumulate).
3. FullyFusedMLP and OneBlob modules are served, and their backward_backward_input still raises; the trainer pair is the module pair.
4. tcnn.Network through autograd against an fp32 torch model, and a fit through input_jvp(differentiable=True) alone.
"""
import ctypes

import pytest

from input_jvp_backward_reference import composed, pass_terms, recipe
from test_input_gradient_gpu import HASH, _create_network, _create_nwie, _net, _params, _same_bits, _x
from test_input_jvp_gpu import _composite, _gained_params, _half_network, _make, _tangents
from test_network_second_order import _act, _acts, _d1

pytestmark = pytest.mark.gpu

IGNORE, OVERWRITE, ACCUMULATE = 0, 1, 2
NOT_IMPLEMENTED = "not implemented error"


def _cotangents(native, n, n_tangents, seed, scale=None):
    """dL_djvp [n][T][padded outputs] and dL_doutput [n][padded outputs] in the module's output precision"""
    import torch
    from tinycudann.modules import _torch_precision

    dtype = _torch_precision(native.output_precision())
    g = torch.Generator().manual_seed(seed)
    s = 128.0 / n if scale is None else scale
    pw = native.n_output_dims()
    ubar = ((torch.rand(n, n_tangents, pw, generator=g) * 2 - 1) * s).to(dtype).cuda().contiguous()
    obar = ((torch.rand(n, pw, generator=g) * 2 - 1) * s).to(dtype).cuda().contiguous()
    return ubar, obar


def _bbi(native, ctx, x, params, v, dy, grads, mode):
    """tcnn_module_backward_backward_input_mode asked for dL_dinput and, by mode, the parameter gradients"""
    import torch
    from tinycudann import _C

    dx = torch.empty_like(x)
    _C.check(_C.lib.tcnn_module_backward_backward_input_mode(native._h, torch.cuda.current_stream().cuda_stream, ctx._h, x.shape[0], v.data_ptr(), x.data_ptr(), dy.data_ptr(),
                                                             grads.data_ptr() if mode != IGNORE else None, None, dx.data_ptr(), params.data_ptr(), ctypes.c_int(mode)))
    return dx


def _chain_by_hand(native, x, params, v, ubar, obar, grads, mode):
    """the public calls in the composed route's order -> (dL_dparams, dL_dinput, dL_dtangents); grads: the buffer Accumulate adds to"""
    import torch

    n, T = v.shape[0], v.shape[1]
    has_params = mode != IGNORE and params.numel() > 0
    if not has_params:
        mode = IGNORE  # (no buffer to name)
    xg = x.detach().clone().requires_grad_(True)
    ctx, out = native.fwd(xg, params.detach().requires_grad_(True))
    first, dx = True, None
    if obar is not None:
        assert mode != ACCUMULATE  # (tcnn_module_backward overwrites)
        dx, grads = native.bwd(ctx, xg, params.detach().requires_grad_(has_params), out, obar)
        first = False
    elif mode == OVERWRITE:
        grads = torch.empty_like(params)
    dv = torch.empty_like(v)
    for t in range(T):
        u = ubar[:, t].contiguous()
        dx_t = _bbi(native, ctx, x, params, v[:, t].contiguous(), u, grads, mode if first or mode == IGNORE else ACCUMULATE)
        dx = dx_t if first else dx + dx_t
        first = False
        dv[:, t] = native.bwd(ctx, xg, params.detach(), out, u)[0]
    return grads, dx, dv


def _call(native, x, params, v, ubar, obar=None, accumulate_onto=None, want_params=True, want_input=True, want_tangents=True):
    ctx, jvp, out = native.input_jvp_fwd(x, params, v, want_output=True)
    return native.input_jvp_bwd(ctx, x, params, v, ubar, obar, want_params, want_input, want_tangents, dL_dparams=accumulate_onto)


# ------------------------------------------------------------------------------------------------------------ 1. composed == chained by hand
COMPOSED_MODULES = [
    ("grid_softplus_64x2", "nwie", {"n_in": 3, "n_out": 3, "enc": HASH, "net": _net(64, 2, "Softplus", otype="CutlassMLP")}),
    ("composite_sum", "encoding", {"n_in": 6, "enc": _composite("Sum")}),
    ("frequency", "encoding", {"n_in": 3, "enc": {"otype": "Frequency", "n_frequencies": 4}}),
    ("tanh_48x3_fp32", "network", {"n_in": 5, "n_out": 3, "net": _net(48, 3, "Tanh", otype="CutlassMLP"), "fp32": True}),
    ("sine_32x2", "network", {"n_in": 5, "n_out": 3, "net": _net(32, 2, "Sine", otype="CutlassMLP")}),
]


def _grid_params(tcnn, native, kind, c):
    """how many of the module's trailing parameters belong to a grid (their second-order gradients are unordered atomics)"""
    from tinycudann import _C
    from tinycudann.modules import _create

    if kind == "network":
        return 0
    return _create(_C.lib.tcnn_create_encoding, c["n_in"], _C.to_json_bytes(c["enc"]), _C.Precision.Fp16).n_params()


@pytest.mark.parametrize("mode", ["overwrite", "accumulate"])
@pytest.mark.parametrize("n_tangents", [1, 3])
@pytest.mark.parametrize("case", COMPOSED_MODULES, ids=[c[0] for c in COMPOSED_MODULES])
def test_composed_route_is_the_public_calls_chained_by_hand(tcnn, case, n_tangents, mode):
    import torch

    _, kind, c = case
    native = _make(tcnn, kind, c)
    assert native.last_input_jvp_backward_route() == "none"
    params = _gained_params(tcnn, native, kind, c)
    n, n_in = 512, c["n_in"]
    x, v = _x(n, n_in), _tangents(n, n_tangents, n_in, seed=31 + n_tangents)
    ubar, obar = _cotangents(native, n, n_tangents, seed=41)
    n_grid = _grid_params(tcnn, native, kind, c)
    known = None
    if mode == "accumulate":  # onto a known buffer, without dL_doutput: the chain is the second-order pass's own Accumulate mode
        known = ((torch.rand(params.shape, generator=torch.Generator().manual_seed(3)) * 2 - 1) * 0.25).to(params.dtype).cuda()
        obar = None
    before = params.clone()

    ctx, jvp, out = native.input_jvp_fwd(x, params, v, want_output=True)
    want_jvp, want_out = native.input_jvp(x, params, v, want_output=True)
    assert _same_bits(jvp, want_jvp) and _same_bits(out, want_out) and _same_bits(out, native.fwd(x, params)[1])
    got_p, got_x, got_v = native.input_jvp_bwd(ctx, x, params, v, ubar, obar, dL_dparams=None if known is None else known.clone())
    assert native.last_input_jvp_backward_route() == "two-pass"
    want_p, want_x, want_v = _chain_by_hand(native, x, params, v, ubar, obar, None if known is None else known.clone(), OVERWRITE if known is None else ACCUMULATE)

    assert _same_bits(got_x, want_x), float((got_x - want_x).abs().max())
    assert _same_bits(got_v, want_v), float((got_v - want_v).abs().max())
    n_net = native.n_params() - n_grid
    if native.n_params():
        assert _same_bits(got_p[:n_net], want_p[:n_net])
        a, b = got_p[n_net:].double(), want_p[n_net:].double()
        if known is not None:
            a, b = a - known[n_net:].double(), b - known[n_net:].double()
        if n_grid:
            print(case[0], n_tangents, mode, "grid gradients |ours - chain| / |chain| =", float(torch.linalg.norm(a - b)) / float(torch.linalg.norm(b)))
            assert float(torch.linalg.norm(b)) > 0 and float(torch.linalg.norm(a - b)) <= 2 * 2e-2 * float(torch.linalg.norm(b))
    assert bool(got_x.isfinite().all()) and bool(got_v.isfinite().all()) and bool((got_v != 0).any())
    assert _same_bits(params, before)  # parameters are read only

    # only what is asked for is computed, and asking for less changes no bit of the rest
    only_v = native.input_jvp_bwd(ctx, x, params, v, ubar, obar, want_params=False, want_input=False)
    assert only_v[0] is None and only_v[1] is None and _same_bits(only_v[2], got_v)
    only_x = native.input_jvp_bwd(ctx, x, params, v, ubar, obar, want_params=False, want_tangents=False)
    assert only_x[0] is None and only_x[2] is None and _same_bits(only_x[1], got_x)


def test_max_level_in_force_applies_to_both_calls(tcnn):
    c = {"n_in": 3, "n_out": 3, "enc": HASH, "net": _net(64, 2, "Softplus", otype="CutlassMLP")}
    native = _make(tcnn, "nwie", c)
    params = _gained_params(tcnn, native, "nwie", c)
    n = 256
    x, v = _x(n, 3), _tangents(n, 1, 3)
    ubar, _ = _cotangents(native, n, 1, seed=5)
    results = []
    for level in (1000.0, 0.5):
        native.set_max_level(level)
        ctx, jvp, _ = native.input_jvp_fwd(x, params, v)
        assert _same_bits(jvp, native.input_jvp(x, params, v)[0])
        got = native.input_jvp_bwd(ctx, x, params, v, ubar, want_params=False)
        want = _chain_by_hand(native, x, params, v, ubar, None, None, IGNORE)
        assert _same_bits(got[1], want[1]) and _same_bits(got[2], want[2])
        results.append((jvp, got[2]))
    native.set_max_level(1000.0)
    assert not _same_bits(results[0][0], results[1][0]) and not _same_bits(results[0][1], results[1][1])  # the setting applies


# ------------------------------------------------------------------------------------------------------------ 2. half fused-shape networks
# (id, inputs, width, hidden, outputs, activation): FUSED_SHAPES of tests/test_input_jvp_gpu.py
FUSED_SHAPES = [
    ("relu_16x1_1_output", 3, 16, 1, 1, "ReLU"),
    ("relu_64x2_16_outputs", 3, 64, 2, 16, "ReLU"),
    ("relu_128x4_20_outputs_32_inputs", 32, 128, 4, 20, "ReLU"),
    ("relu_32x4_20_outputs", 3, 32, 4, 20, "ReLU"),
    ("softplus_16x1_16_outputs_32_inputs", 32, 16, 1, 16, "Softplus"),
    ("softplus_64x2_20_outputs", 3, 64, 2, 20, "Softplus"),
    ("softplus_128x4_1_output", 3, 128, 4, 1, "Softplus"),
    ("softplus_32x4_16_outputs", 3, 32, 4, 16, "Softplus"),
    ("leaky_64x2_3_outputs", 3, 64, 2, 3, "LeakyReLU"),
]


def _plan_route(width, hidden, act, n, n_tangents):
    """mlp_input_jvp_backward_plan for a half fused-shape network: no class is fused (tests/test_input_jvp_backward_plan.py holds the table)"""
    return "two-pass"


def _criterion(name, ours, r64, rh):
    import torch

    e_ours, e_h, norm = float(torch.linalg.norm(ours - r64)), float(torch.linalg.norm(rh - r64)), float(torch.linalg.norm(r64))
    print(f"{name}: |ours-R64|/|R64| {e_ours / max(norm, 1e-300):.3e}  |Rh-R64|/|R64| {e_h / max(norm, 1e-300):.3e}  ratio {e_ours / max(e_h, 1e-300):.3f}")
    assert norm > 0 and e_h <= 0.05 * norm, (name, e_h / norm)  # the restatement alone: the bar cannot hide a wrong result
    assert e_ours <= 2 * e_h, (name, e_ours, e_h)


def _padded(x, width, value):
    import torch

    return torch.cat([x, torch.full(tuple(x.shape[:-1]) + (width - x.shape[-1],), value, dtype=x.dtype)], dim=-1)


def _check_criterion(name, Ws, acts, x, v, ubar, obar, got, n_in):
    """got = (dL_dparams, dL_dinput or None, dL_dtangents) of a bare network behind the Identity encoding: the input padded with ones, the
    tangents with zeros"""
    import torch

    n_in_padded = Ws[0].shape[1]
    xp, vp = _padded(x, n_in_padded, 1.0), _padded(v, n_in_padded, 0.0)
    ub, ob = ubar.cpu(), None if obar is None else obar.cpu()
    r64 = recipe(Ws, acts, xp, vp, ub, ob)
    rh = composed(Ws, acts, xp, vp, ub, ob, half=True)
    off = 0
    for k, W in enumerate(Ws):
        ours = got[0][off:off + W.numel()].reshape(W.shape).cpu().double()
        off += W.numel()
        _criterion(f"{name} dL_dparams[{k}]", ours, r64[0][k], rh[0][k].double())
    if got[1] is not None:
        if r64[1].any():
            _criterion(f"{name} dL_dinput", got[1].cpu().double(), r64[1][:, :n_in], rh[1][:, :n_in].double())
        else:
            assert not got[1].view(torch.int32).any()
    for t in range(v.shape[1]):
        _criterion(f"{name} dL_dtangents[:, {t}]", got[2][:, t].cpu().double(), r64[2][:, t, :n_in], rh[2][:, t, :n_in].double())


def _check_accumulate(name, native, ctx, Ws, acts, x, v, xc, vc, params, ubar, obar, overwritten):
    """Accumulate onto a known non-zero buffer, with dL_doutput given, against Overwrite plus that buffer.  The issue's "to one rounding" is
    the fused kernel's; on the composed route N passes store dL_dparams -- one for dL_doutput, per tangent one for the bilinear term and,
    where an activation has curvature, one for the curvature term -- and each store rounds its running sum to half once, on either path:
    an error of at most 2^-11 times that sum's magnitude.  Every running sum is bounded, element by element, by S = |buffer| + the sum of
    the passes' |terms|; the terms come from the fp64 restatement (input_jvp_backward_reference.pass_terms: nothing of the code under test),
    taken 25 % larger because the kernels' terms are those only up to half rounding (the criterion's guard holds them within 5 % in norm).
    So |accumulated - (overwritten + buffer)| <= 2 N 2^-11 * 1.25 S, plus a half subnormal per store.  Overwriting instead of accumulating
    in any pass would miss by that pass's share of |buffer| (0.125 on average), about a hundred bounds."""
    import torch

    n_in_padded = Ws[0].shape[1]
    terms = pass_terms(Ws, acts, _padded(x, n_in_padded, 1.0), _padded(v, n_in_padded, 0.0), ubar.cpu(), obar.cpu())
    n_passes = len(terms)
    known = ((torch.rand(params.shape, generator=torch.Generator().manual_seed(77)) * 2 - 1) * 0.25).half().cuda()
    acc = native.input_jvp_bwd(ctx, xc, params, vc, ubar, obar, dL_dparams=known.clone())[0]
    off, worst = 0, 0.0
    for k, W in enumerate(Ws):
        sl = slice(off, off + W.numel())
        off += W.numel()
        S = known[sl].double().abs().cpu() + sum(term[k].abs() for term in terms).reshape(-1)
        bound = 2 * n_passes * (2.0 ** -11 * 1.25 * S + 2.0 ** -25)
        miss = (acc[sl].double() - (overwritten[sl].double() + known[sl].double())).abs().cpu()
        worst = max(worst, float((miss / bound).max()))
        assert bool((miss <= bound).all()), (name, k, float((miss / bound).max()))
    assert bool(((acc.float() - overwritten.float()).abs() > 0.01).any())  # (the buffer is in the result)
    print(f"{name} accumulate onto a buffer, {n_passes} stores: largest miss / bound {worst:.3f}")


@pytest.mark.parametrize("case", FUSED_SHAPES, ids=[c[0] for c in FUSED_SHAPES])
def test_fused_shapes_meet_the_contract(tcnn, case):
    import torch

    name, n_in, width, hidden, n_out, act = case
    n_in_padded, pad_out = -(-n_in // 16) * 16, -(-n_out // 16) * 16
    Ws = _half_network(n_in_padded, width, hidden, pad_out, seed=3)
    acts = _acts(hidden, act, "None")
    native = _create_network(tcnn, n_in, n_out, _net(width, hidden, act))
    params = torch.cat([W.reshape(-1) for W in Ws]).cuda().contiguous()
    assert native.n_params() == params.numel() and native.n_output_dims() == pad_out
    g = torch.Generator().manual_seed(17)
    n = 512
    x = (torch.rand(n, n_in, generator=g) * 2 - 1).half().float()
    xc = x.cuda()
    inference = native.fwd(xc, params)[1]
    for T in (1, 3, 4):
        v = (torch.rand(n, T, n_in, generator=g) * 2 - 1).half().float()
        vc = v.cuda().contiguous()
        ubar, obar = _cotangents(native, n, T, seed=50 + T)
        ctx, jvp, out = native.input_jvp_fwd(xc, params, vc, want_output=True)
        assert _same_bits(out, inference) and _same_bits(jvp, native.input_jvp(xc, params, vc)[0])
        got = native.input_jvp_bwd(ctx, xc, params, vc, ubar, obar)
        assert native.last_input_jvp_backward_route() == _plan_route(width, hidden, act, n, T)
        _check_criterion(f"{name} T={T}", Ws, acts, x, v, ubar, obar, got, n_in)
        # the tangents' own dL_dinput (no dL_doutput): zero bits for piecewise linear networks, else by the criterion
        alone = native.input_jvp_bwd(ctx, xc, params, vc, ubar, None)
        if act in ("ReLU", "LeakyReLU"):
            assert not alone[1].view(torch.int32).any()
        else:
            _check_criterion(f"{name} T={T} tangents alone", Ws, acts, x, v, ubar, None, alone, n_in)
        # two runs, the same bits
        again = native.input_jvp_bwd(ctx, xc, params, vc, ubar, obar)
        assert all(_same_bits(a, b) for a, b in zip(again, got))
        # rows 0 .. 255 moved to rows 256 .. 511 of another call, behind other rows
        moved_x = torch.cat([(torch.rand(256, n_in, generator=g) * 2 - 1), x[:256]]).cuda().contiguous()
        moved_v = torch.cat([(torch.rand(256, T, n_in, generator=g) * 2 - 1), v[:256]]).cuda().contiguous()
        moved_u, moved_o = torch.cat([ubar[256:], ubar[:256]]).contiguous(), torch.cat([obar[256:], obar[:256]]).contiguous()
        moved_ctx = native.input_jvp_fwd(moved_x, params, moved_v)[0]
        moved = native.input_jvp_bwd(moved_ctx, moved_x, params, moved_v, moved_u, moved_o, want_params=False)
        assert _same_bits(moved[1][256:], got[1][:256]) and _same_bits(moved[2][256:], got[2][:256])
        # Accumulate onto zeros is Overwrite, bit for bit (every pass rounds the same sums); onto a known buffer it adds, within the route's bound
        acc = native.input_jvp_bwd(ctx, xc, params, vc, ubar, obar, dL_dparams=torch.zeros_like(params))[0]
        assert _same_bits(acc, got[0])
        _check_accumulate(f"{name} T={T}", native, ctx, Ws, acts, x, v, xc, vc, params, ubar, obar, got[0])


# ------------------------------------------------------------------------------------------------------------ 3. FullyFusedMLP and OneBlob
def test_fully_fused_mlp_is_served_and_keeps_no_second_order_pass(tcnn):
    import torch

    n_in, width, hidden, n_out, act = 3, 64, 2, 3, "Softplus"
    Ws = _half_network(16, width, hidden, 16, seed=5)
    native = _create_network(tcnn, n_in, n_out, _net(width, hidden, act, otype="FullyFusedMLP"))
    params = torch.cat([W.reshape(-1) for W in Ws]).cuda().contiguous()
    g = torch.Generator().manual_seed(19)
    n, T = 512, 3
    x = (torch.rand(n, n_in, generator=g) * 2 - 1).half().float()
    v = (torch.rand(n, T, n_in, generator=g) * 2 - 1).half().float()
    ubar, obar = _cotangents(native, n, T, seed=61)
    got = _call(native, x.cuda(), params, v.cuda().contiguous(), ubar, obar)
    assert native.last_input_jvp_backward_route() == "two-pass"
    _check_criterion("fully_fused_64x2", Ws, _acts(hidden, act, "None"), x, v, ubar, obar, got, n_in)
    ctx = native.input_jvp_fwd(x.cuda(), params, v.cuda().contiguous())[0]
    _check_accumulate("fully_fused_64x2", native, ctx, Ws, _acts(hidden, act, "None"), x, v, x.cuda(), v.cuda().contiguous(), params, ubar, obar, got[0])
    xg = x.cuda().requires_grad_(True)
    ctx, out = native.fwd(xg, params.requires_grad_(True))
    with pytest.raises(RuntimeError, match=NOT_IMPLEMENTED):
        native.bwd_bwd_input(ctx, xg, params, v[:, 0].cuda().contiguous(), ubar[:, 0].contiguous().requires_grad_(True))


def test_oneblob_in_front_is_served_for_parameters_and_tangents(tcnn):
    import torch
    from tinycudann import _C
    from tinycudann.modules import _create

    n_in, width, hidden, n_out, act, n_bins = 2, 64, 2, 3, "Softplus", 16
    enc = {"otype": "OneBlob", "n_bins": n_bins}
    native = _create_nwie(tcnn, n_in, n_out, enc, _net(width, hidden, act, otype="FullyFusedMLP"))
    encoding = _create(_C.lib.tcnn_create_encoding, n_in, _C.to_json_bytes(enc), _C.Precision.Fp16)
    enc_w = encoding.n_output_dims()
    assert enc_w == n_in * n_bins
    Ws = _half_network(enc_w, width, hidden, 16, seed=7)
    params = torch.cat([W.reshape(-1) for W in Ws]).cuda().contiguous()
    assert native.n_params() == params.numel()
    g = torch.Generator().manual_seed(23)
    n, T = 512, 3
    x = torch.rand(n, n_in, generator=g).cuda().contiguous()
    v = (torch.rand(n, T, n_in, generator=g) * 2 - 1).cuda().contiguous()
    ubar, obar = _cotangents(native, n, T, seed=67)
    no_params = torch.empty(0, dtype=torch.half, device="cuda")
    ctx, jvp, out = native.input_jvp_fwd(x, params, v, want_output=True)
    assert _same_bits(jvp, native.input_jvp(x, params, v)[0])
    with pytest.raises(RuntimeError, match="input_jvp_backward: dL_dinput not implemented for NetworkWithInputEncoding"):
        native.input_jvp_bwd(ctx, x, params, v, ubar, obar)
    assert native.last_input_jvp_backward_route() == "none"  # a refused call is no call
    got_p, none, got_v = native.input_jvp_bwd(ctx, x, params, v, ubar, obar, want_input=False)
    assert none is None and native.last_input_jvp_backward_route() == "two-pass"
    # the network's part by the criterion, on the encoded input and the encoded tangents the encoding itself gives
    e = encoding.fwd(x, no_params)[1].cpu()
    t = encoding.input_jvp(x, no_params, v)[0].cpu()
    assert e.shape == (n, enc_w) and t.shape == (n, T, enc_w)
    acts = _acts(hidden, act, "None")
    r64 = recipe(Ws, acts, e, t, ubar.cpu(), obar.cpu())
    rh = composed(Ws, acts, e, t, ubar.cpu(), obar.cpu(), half=True)
    off = 0
    for k, W in enumerate(Ws):
        _criterion(f"oneblob_64x2 dL_dparams[{k}]", got_p[off:off + W.numel()].reshape(W.shape).cpu().double(), r64[0][k], rh[0][k].double())
        off += W.numel()
    # dL_dtangents[:, t] = J^T dL_djvp_t: bit for bit the first-order backward pass, which a OneBlob module has.  (That holds it to more
    # than the R64 / Rh criterion would: the pass itself -- the fused MLP backward kernel and OneBlob's backward_input -- is pinned
    # against the oracle in tests/test_gpu_parity.py and tests/test_more_encodings.py.)
    xg = x.clone().requires_grad_(True)
    fctx, fout = native.fwd(xg, params)
    for k in range(T):
        want = native.bwd(fctx, xg, params, fout, ubar[:, k].contiguous())[0]
        assert _same_bits(got_v[:, k].contiguous(), want) and bool((want != 0).any())
    with pytest.raises(RuntimeError, match=NOT_IMPLEMENTED):
        native.bwd_bwd_input(fctx, xg, params.requires_grad_(True), v[:, 0].contiguous(), ubar[:, 0].contiguous().requires_grad_(True))


def test_trainer_pair_is_the_module_pair_on_the_training_parameters(tcnn):
    """tcnn_trainer_input_jvp_forward / _backward (what NetworkWithInputEncoding<T>::input_jvp_forward / _backward of the C++ headers call):
    the module pair's bits on the trainer's training parameters, the parameter gradients in the buffer optimizer_step reads, Overwrite
    and Accumulate.  (A Frequency encoding: no grid atomics, so every bit is determined.)"""
    import torch
    from tinycudann.native import GRADIENT_ACCUMULATE, GRADIENT_OVERWRITE

    enc = {"otype": "Frequency", "n_frequencies": 4}
    cfg = {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2}, "encoding": enc, "network": _net(64, 2, "Softplus")}
    trainer = tcnn.Trainer(3, 3, cfg, seed=1337)
    n, T = 512, 3
    x, target = _x(n, 3), _x(n, 3, seed=5)
    for _ in range(3):  # (so that the parameters are not the initial ones)
        trainer.training_step(x, target)
    params = trainer.params().clone().contiguous()
    v = _tangents(n, T, 3)
    native = _create_nwie(tcnn, 3, 3, enc, cfg["network"])
    ubar, obar = _cotangents(native, n, T, seed=71)

    ctx, jvp, out = trainer.input_jvp_forward(x, v, want_output=True)
    mctx, want_jvp, want_out = native.input_jvp_fwd(x, params, v, want_output=True)
    assert _same_bits(jvp, want_jvp) and _same_bits(out, want_out) and _same_bits(trainer.params(), params)
    dx, dv = trainer.input_jvp_backward(ctx, x, v, ubar, obar, gradient_mode=GRADIENT_OVERWRITE)
    want_p, want_x, want_v = native.input_jvp_bwd(mctx, x, params, v, ubar, obar)
    first = trainer.param_gradients().clone()
    assert _same_bits(first, want_p) and _same_bits(dx, want_x) and _same_bits(dv, want_v) and bool((want_p != 0).any())
    # Accumulate: onto what the buffer holds
    dx2, none = trainer.input_jvp_backward(ctx, x, v, ubar, None, want_tangents=False, gradient_mode=GRADIENT_ACCUMULATE)
    want_p2, want_x2, _ = native.input_jvp_bwd(mctx, x, params, v, ubar, None, want_tangents=False, dL_dparams=first.clone())
    assert none is None and _same_bits(trainer.param_gradients(), want_p2) and _same_bits(dx2, want_x2) and not _same_bits(want_p2, first)
    assert _same_bits(trainer.params(), params)  # parameters are read only
    # the buffer is the one optimizer_step reads: a step moves the parameters
    trainer.optimizer_step(1.0)
    assert not _same_bits(trainer.params(), params)


# ------------------------------------------------------------------------------------------------------------ 4. PyTorch
def _torch_mlp(Ws, act):
    def f(inp):
        h = inp
        for k, W in enumerate(Ws):
            h = h @ W.T
            if k < len(Ws) - 1:
                h = _act(act, h)
        return h
    return f


def test_module_input_jvp_differentiable_against_an_fp32_torch_model(tcnn):
    """tcnn.Network(3 -> 3, 64 x 2 Softplus), n = 300, T = 3, loss = mean(jvp^2) + mean(output^2): .grad of params, x and tangents against an
    fp32 torch MLP on the same half weights through torch.func.jvp, relative to the distance between that model and its own half-rounded
    restatement (the loss-scaled half cotangents included), factor 2"""
    import torch

    n, T, n_in, n_out, width, hidden, act = 300, 3, 3, 3, 64, 2, "Softplus"
    net = tcnn.Network(n_in, n_out, _net(width, hidden, act, otype="FullyFusedMLP"))
    Ws = _half_network(16, width, hidden, 16, seed=9)
    with torch.no_grad():
        net.params.copy_(torch.cat([W.reshape(-1) for W in Ws]).float())
    g = torch.Generator().manual_seed(29)
    x0 = (torch.rand(n, n_in, generator=g) * 2 - 1).half().float()
    v0 = (torch.rand(n, T, n_in, generator=g) * 2 - 1).half().float()

    x = x0.cuda().requires_grad_(True)
    v = v0.cuda().requires_grad_(True)
    jvp, out = net.input_jvp(x, v, return_output=True, differentiable=True)
    assert jvp.shape == (n, T, n_out) and out.shape == (n, n_out) and jvp.requires_grad and out.requires_grad
    loss = (jvp.float() ** 2).mean() + (out.float() ** 2).mean()
    loss.backward()
    assert net.native_tcnn_module.last_input_jvp_backward_route() == "two-pass"
    ours = (net.params.grad.cpu().double(), x.grad.cpu().double(), v.grad.cpu().double())

    # the fp32 model
    Wf = [W.float().requires_grad_(True) for W in Ws]
    xf = _padded(x0, 16, 1.0).requires_grad_(True)
    vf = _padded(v0, 16, 0.0).requires_grad_(True)
    f = _torch_mlp(Wf, act)
    jv = []
    for t in range(T):
        o, j = torch.func.jvp(f, (xf,), (vf[:, t],))
        jv.append(j[:, :n_out])
    loss32 = (torch.stack(jv, dim=1) ** 2).mean() + (o[:, :n_out] ** 2).mean()
    g32 = torch.autograd.grad(loss32, [xf, vf] + Wf)
    ref = (torch.cat([w.reshape(-1) for w in g32[2:]]).double(), g32[0][:, :n_in].double(), g32[1][:, :, :n_in].double())

    # its half-rounded restatement: forward and tangents rounded where the kernels store halves, the loss in fp32 on those, the cotangents
    # at the module's loss scale rounded to half, the composed route's roundings, the gradients divided by the loss scale
    acts = _acts(hidden, act, "None")
    rh = lambda a: a.half().float()
    h, us = rh(_padded(x0, 16, 1.0)), [rh(_padded(v0[:, t], 16, 0.0)) for t in range(T)]
    for W, a in zip(Ws, acts):
        z = rh(h @ W.float().T)
        us = [rh(_d1(a, z) * (u @ W.float().T)) for u in us]
        h = rh(_act(a, z))
    scale = net.loss_scale
    ubar = torch.zeros(n, T, 16)
    ubar[:, :, :n_out] = torch.stack(us, dim=1)[:, :, :n_out] * (2.0 / (n * T * n_out))
    obar = torch.zeros(n, 16)
    obar[:, :n_out] = h[:, :n_out] * (2.0 / (n * n_out))
    dW, dx, dv = composed(Ws, acts, _padded(x0, 16, 1.0), _padded(v0, 16, 0.0), (ubar * scale).half(), (obar * scale).half(), half=True)
    restated = (torch.cat([w.reshape(-1) for w in dW]).double() / scale, dx[:, :n_in].double() / scale, dv[:, :, :n_in].double() / scale)
    for what, a, b, c in zip(("params.grad", "x.grad", "tangents.grad"), ours, ref, restated):
        _criterion("torch " + what, a, b, c)

    # differentiable=False is the call of before: outside autograd, the same bits
    plain = net.input_jvp(x, v)
    assert not plain.requires_grad and _same_bits(plain, jvp.detach())
    plain, plain_out = net.input_jvp(x, v, return_output=True)
    assert not plain.requires_grad and not plain_out.requires_grad and _same_bits(plain_out, out.detach())
    # first order only: a backward pass through the backward pass raises
    jvp2 = net.input_jvp(x, v, differentiable=True)
    (gx,) = torch.autograd.grad((jvp2.float() ** 2).mean(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    # a loss on the output alone runs no pass per tangent: the gradients are forward()'s, bit for bit, and the tangents' are zero
    net.params.grad, x.grad, v.grad = None, None, None
    _, out_only = net.input_jvp(x, v, return_output=True, differentiable=True)
    (out_only.float() ** 2).mean().backward()
    by_jvp = (net.params.grad.clone(), x.grad.clone(), v.grad.clone())
    net.params.grad, x.grad = None, None
    (net(x).float() ** 2).mean().backward()
    assert _same_bits(by_jvp[0], net.params.grad) and _same_bits(by_jvp[1], x.grad) and not by_jvp[2].any()
    # a 2-D tangent means T = 1; only what requires grad receives one
    flat = net.input_jvp(x.detach(), v0[:, 0].cuda(), differentiable=True)
    assert flat.shape == (n, n_out) and flat.requires_grad
    net.params.grad = None
    flat.float().sum().backward()
    assert net.params.grad is not None and bool(net.params.grad.isfinite().all())


def test_fit_a_derivative_through_input_jvp_alone(tcnn):
    """200 Adam steps of 256 points on FullyFusedMLP 32 x 2 Tanh: d/dx of the network is fitted to the derivative of sin(3 x), and nothing
    else enters the loss"""
    import torch

    torch.manual_seed(0)
    net = tcnn.Network(1, 1, _net(32, 2, "Tanh", otype="FullyFusedMLP"))
    optimizer = torch.optim.Adam(net.parameters(), lr=1e-2)
    ones = torch.ones(256, 1, device="cuda")
    losses = []
    for step in range(200):
        x = torch.rand(256, 1, device="cuda")
        jvp = net.input_jvp(x, ones, differentiable=True)
        loss = ((jvp.float() - 3 * torch.cos(3 * x)) ** 2).mean()
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu()
    print("derivative loss: first", float(losses[0]), "last", float(losses[-1]))
    assert bool(losses.isfinite().all())
    assert float(losses[-1]) < 0.1 * float(losses[0])
