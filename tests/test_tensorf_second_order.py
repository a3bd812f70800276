"""The TensoRF second-order pass and tangent (k_tensorf.hip: k_tensorf_tangent, k_tensorf_bwdbwd_input, k_tensorf_bwdbwd, k_tensorf_bwdbwd_f32;
opt-in by "second_order": true) against tests/tensorf_second_order_reference.py, on test_tensorf_encoding's shapes, interior rows and
yardsticks: tangent and dQ/dx by ||ours - R64|| <= 2 ||Rh - R64||, dQ/dparams per parameter (test_second_order says what m is)."""
import numpy as np
import pytest

from grid_reference import gamma, to_device
from tensorf_reference import F32, F64
from tensorf_second_order_reference import TensoRFSecondOrder
from test_tensorf_encoding import BACKWARD_CASES, N_ROWS, case_id, cfg, inputs, within_yardstick

CUTLASS = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
_DIRECTIONS = {}


def on(c):
    return {**c, "second_order": True}


def direction(D):
    """v = dL_ddLdx, uniform in [-1, 1], computed once per D"""
    if D not in _DIRECTIONS:
        _DIRECTIONS[D] = np.random.RandomState(41 + D).uniform(-1, 1, (N_ROWS, D)).astype(F32)
    return _DIRECTIONS[D]


def run(tcnn, D, c, x, params, dy, v, fp32=False):
    """C ABI forward + backward_backward_input of the encoding module -> (dL_ddLdy, dL/dx, dL/dparams) as numpy"""
    import torch

    T = F32 if fp32 else np.float16
    native = (tcnn.Encoding(D, c, dtype=torch.float32) if fp32 else tcnn.Encoding(D, c)).native_tcnn_module
    xt, pt, dyt = (to_device(a).requires_grad_(True) for a in (x, params.astype(T), dy.astype(T)))
    ctx, _ = native.fwd(xt, pt)
    t, dp, dx = native.bwd_bwd_input(ctx, xt, pt, to_device(v), dyt)
    return t.cpu().numpy(), dx.cpu().numpy(), dp.cpu().numpy()


@pytest.mark.parametrize("D,decomposition", [(3, "VM"), (2, "CP"), (4, "CP")])
def test_reference_against_differences(D, decomposition):
    """the float64 reference's tangent, dQ/dx and dQ/dparams against central differences of the forward pass along v and of
    Q = <v, backward_input(x, params, d)> (fractions in float64; a step along one random direction of the parameters: Q is a polynomial in them)"""
    c = cfg(decomposition, 2)
    _, xi, params, dy = inputs(D, c, True)
    ref, xi, v, h, rs = TensoRFSecondOrder(D, c, fract=F64), xi.astype(F64), direction(D).astype(F64), 1e-6, np.random.RandomState(3)

    def Q(x, p):
        return np.sum(v * ref.backward_input(x, p, dy), axis=1)

    t = ref.tangent(xi, v, params)
    assert np.abs((ref.forward(xi + h * v, params) - ref.forward(xi - h * v, params)) / (2 * h) - t).max() <= 1e-6 * np.abs(t).max()
    assert np.abs(np.sum(dy * t, axis=1) - Q(xi, params)).max() <= 1e-12 * np.abs(t).max()
    dx = ref.dQ_dx(xi, v, params, dy)
    for d in range(D):
        step = h * np.eye(D)[d]
        assert np.abs((Q(xi + step, params) - Q(xi - step, params)) / (2 * h) - dx[:, d]).max() <= 1e-6 * np.abs(dx).max()
    S, r = ref.param_gradient_terms(xi, v, params, dy)[0], rs.uniform(-1, 1, ref.n_params)
    assert abs((Q(xi, params + h * r).sum() - Q(xi, params - h * r).sum()) / (2 * h) - S @ r) <= 1e-6 * np.abs(S) @ np.abs(r)


@pytest.mark.gpu
@pytest.mark.parametrize("D,c", BACKWARD_CASES, ids=case_id)
def test_second_order(tcnn, D, c):
    """m, the fp32 roundings behind one contribution of k_tensorf_bwdbwd relative to its majorant, counted from its code.  vs = scale * v is
    1, 1 - u is 1, a difference of two entries 1 (on the sum of their magnitudes), a line value 3 and a plane value 7 (test_backward).
    VM, a plane's corner, (half)(g * fmaf(V, D_v w, w * (V' * vs_c))): D_v w = fmaf(+-vs_b, wa, +-vs_a * wb) is 3 for the product and 1 for
    the fma, 4, so V D_v w carries 7; w is 3 and V' * vs_c is 3, their product 7; the fma and the multiply by g: m = 9.  VM, a line's entry,
    (half)(g * fmaf(DP, w, P * +-vs_c)): a slope daP = fmaf(u, M, v1 - v0) is 1 for the difference, 3 for M and 1: 4 on (|v1| + |v0|) +
    u sum|v|; DP = fmaf(vs_b, dbP, vs_a * daP) is 1 + 4 + 1 per term and 1: 7, times w: 8; P * vs_c is 7 + 1 + 1 = 9; the fma and g:
    m = 11.  CP, (half)(g * fmaf(S_i, w, O_i * +-vs_i)): O_i is D - 1 line values and at most D - 1 multiplies, 4 (D - 1), times vs_i:
    4 D - 2; a term of S_i = D_v O_i is one V_j' * vs_j (3) and D - 2 line values, 3 (D - 1), and passes at most D - 2 multiplies of its
    suffix or prefix, the multiply by V_j' vs_j, D - 2 fused steps and the last two operations, 2 D - 1: 5 D - 4, times w: 5 D - 3, the
    larger; the fma and g: m = 5 D - 1.  The test holds every parameter to the larger count of its decomposition."""
    ref, x, params, dy = inputs(D, c, True)
    so, v = TensoRFSecondOrder(D, c), direction(D)
    m = 5 * D - 1 if so.cp else 11
    S, A, Abar, K = so.param_gradient_terms(x, v, params, dy)
    bound = 2.0 ** -11 * (A + np.abs(S)) + m * 2.0 ** -24 * Abar + (K + 1) * 2.0 ** -25
    rh = so.param_gradient_terms(x, v, params, dy, F32, np.float16)[0].astype(np.float16)  # the float32 reference, rounded as the kernel rounds
    assert np.all(np.abs(rh.astype(F64) - S) <= bound), "the float32 reference misses the bound: the inputs do not suit it"
    t, dx, dp = run(tcnn, D, on(c), x, params, dy, v)
    within_yardstick(t[:, :so.n_output_dims], so.tangent(x, v, params), so.tangent(x, v, params, F32, np.float16), f"{D}-D {case_id(c)} tangent")
    within_yardstick(dx, so.dQ_dx(x, v, params, dy), so.dQ_dx(x, v, params, dy, F32), f"{D}-D {case_id(c)} dQ/dx")
    err = np.abs(dp.astype(F64) - S)
    print(f"dQ/dparams: largest error / bound = {np.max(err / bound):.3f}; {np.count_nonzero(K)} of {K.size} parameters touched")
    assert np.all(err <= bound) and np.any(dp != 0) and not np.any(dp.view(np.uint16)[K == 0]) and not np.any(t[:, so.n_output_dims:])
    for what, first, second in zip(("tangent", "dQ/dx", "dQ/dparams"), (t, dx, dp), run(tcnn, D, on(c), x, params, dy, v)):
        assert np.array_equal(first.view(np.uint8), second.view(np.uint8)), f"two runs differ: {what}"


@pytest.mark.gpu
def test_fp32_module(tcnn):
    D, c = 3, cfg("VM", 4)
    _, x, params, dy = inputs(D, c, True)
    so, v = TensoRFSecondOrder(D, c), direction(D)
    t, dx, dp = run(tcnn, D, on(c), x, params, dy, v, fp32=True)
    within_yardstick(t[:, :so.n_output_dims], so.tangent(x, v, params), so.tangent(x, v, params, F32), "fp32 tangent")
    within_yardstick(dx, so.dQ_dx(x, v, params, dy), so.dQ_dx(x, v, params, dy, F32), "fp32 dQ/dx")
    S, _, Abar, K = so.param_gradient_terms(x, v, params, dy, F32)
    assert np.all(np.abs(dp.astype(F64) - S) <= gamma(np.maximum(K - 1, 0), 2.0 ** -24) * Abar) and np.any(dp != 0)


@pytest.mark.gpu
def test_many_directions_are_one_direction_each(tcnn):
    """input_jvp's one k_tensorf_tangent launch for 3 directions against the single-direction second-order call, bit for bit: behind a
    CutlassMLP (48 wide: the network's two-pass route, whose contract this is) and on the bare encoding"""
    from test_input_gradient_gpu import _create_nwie, _net, _params, _same_bits
    from test_input_jvp_gpu import _second_order_tangent, _tangents

    D, c = 3, cfg("VM", 2)
    _, x, params, dy = inputs(D, c, True)
    xt, v = to_device(x), _tangents(N_ROWS, 3, D)
    native = _create_nwie(tcnn, D, 3, on(c), _net(48, 2, otype="CutlassMLP"))
    p = _params(native).clone()
    p[native.n_params() - params.size:] = to_device(params.astype(np.float16))  # (the encoding's parameters lie behind the network's)
    jvp = native.input_jvp(xt, p, v)[0]
    assert native.last_input_jvp_route() == "two-pass"
    for k in range(3):
        assert _same_bits(jvp[:, k, :].contiguous(), _second_order_tangent(native, xt, p, v[:, k, :])) and bool(jvp[:, k, :].any())
    bare = tcnn.Encoding(D, on(c)).native_tcnn_module.input_jvp(xt, to_device(params.astype(np.float16)), v[:, :2].contiguous())[0].cpu().numpy()
    for k in range(2):
        want = run(tcnn, D, on(c), x, params, dy, v[:, k].cpu().numpy())[0]
        assert np.array_equal(bare[:, k].view(np.uint16), want.view(np.uint16)) and np.any(bare[:, k] != 0)


@pytest.mark.gpu
def test_composite(tcnn):
    """Composite[VM F = 2 on 3 dims (18 columns, padded to the 8 the next TensoRF asks for: 24), CP on 2, Identity on 1]: the nested columns
    and gradients are the stand-alone modules' bits, the tangent's padding columns exactly zero (the forward pass pads with ones)"""
    ca, cb, rs = cfg("VM", 2), cfg("CP", 8, L=1, base=5), np.random.RandomState(9)
    (_, xa, pa, dya), (_, xb, pb, dyb), va, vb = inputs(3, ca, True), inputs(2, cb, True), direction(3), direction(2)
    (ta, dxa, dpa), (tb, dxb, dpb) = run(tcnn, 3, on(ca), xa, pa, dya, va), run(tcnn, 2, on(cb), xb, pb, dyb, vb)
    composite = {"otype": "Composite", "nested": [dict(on(ca), n_dims_to_encode=3), dict(on(cb), n_dims_to_encode=2), {"otype": "Identity", "n_dims_to_encode": 1}]}
    last = lambda: rs.uniform(0.1, 0.9, (N_ROWS, 1)).astype(F32)  # noqa: E731
    dy6 = np.concatenate([dya, np.zeros((N_ROWS, 6), F32), dyb, last()], axis=1)
    ct, cdx, cdp = run(tcnn, 6, composite, np.concatenate([xa, xb, last()], axis=1), np.concatenate([pa, pb]), dy6, np.concatenate([va, vb, last()], axis=1))
    assert ct.shape[1] == 24 + 8 + 1 and not np.any(ct[:, 18:24]) and np.any(ct[:, 32:] != 0)
    assert np.array_equal(ct[:, :18].view(np.uint16), ta.view(np.uint16)) and np.array_equal(ct[:, 24:32].view(np.uint16), tb.view(np.uint16))
    assert np.array_equal(cdx[:, :5], np.concatenate([dxa, dxb], axis=1)) and np.array_equal(cdp.view(np.uint16), np.concatenate([dpa, dpb]).view(np.uint16))


@pytest.mark.gpu
def test_torch_double_backward(tcnn):
    """torch.autograd.grad(create_graph=True) on tcnn.Encoding at loss_scale 1 returns the native call's bits"""
    import torch

    D, c = 3, cfg("VM", 16, L=1, base=5)
    _, x, params, dy = inputs(D, c, True)
    v = direction(D)
    _, dx, dp = run(tcnn, D, on(c), x, params, dy, v)
    enc = tcnn.Encoding(D, on(c))
    with torch.no_grad():
        enc.params.copy_(to_device(params.astype(np.float16)))
    enc.loss_scale = 1.0
    xt = to_device(x).requires_grad_(True)
    (gx,) = torch.autograd.grad(enc(xt), xt, to_device(dy.astype(np.float16)), create_graph=True)
    (gx * to_device(v)).sum().backward()
    assert np.array_equal(xt.grad.cpu().numpy(), dx) and np.array_equal(enc.params.grad.cpu().numpy(), dp.astype(F32)) and np.any(dx != 0) and np.any(dp != 0)


@pytest.mark.gpu
def test_eikonal_step(tcnn):
    """TensoRF VM in front of a CutlassMLP: the double backward of an eikonal loss runs, with finite, non-zero gradients"""
    import torch

    c = cfg("VM", 4)
    model = tcnn.NetworkWithInputEncoding(3, 1, on(c), CUTLASS)
    xt = to_device(inputs(3, c, True)[1]).requires_grad_(True)
    (gx,) = torch.autograd.grad(model(xt).float().sum(), xt, create_graph=True)
    ((gx.norm(dim=1) - 1) ** 2).mean().backward()
    n_enc = tcnn.Encoding(3, c).params.numel()
    for g in (xt.grad, model.params.grad, model.params.grad[-n_enc:]):
        assert bool(torch.all(torch.isfinite(g))) and bool(torch.any(g != 0))


@pytest.mark.gpu
def test_the_switch(tcnn):
    c = cfg("VM", 2)
    with pytest.raises(RuntimeError, match="TensoRF: second_order must be true or false"):
        tcnn.Encoding(3, dict(c, second_order="yes"))
    assert tcnn.Encoding(3, on(c)).native_tcnn_module.hyperparams()["second_order"] is True
    assert "second_order" not in tcnn.Encoding(3, c).native_tcnn_module.hyperparams()
    _, x, params, dy = inputs(3, c, True)
    with pytest.raises(RuntimeError, match="not implemented"):
        run(tcnn, 3, c, x, params, dy, direction(3))
