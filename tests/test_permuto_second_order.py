"""The PermutoGrid second-order pass and tangent (k_permuto.hip: k_permuto_tangent, k_permuto_bwdbwd, k_permuto_bwdbwd_f32; opt-in by
"second_order": true) against tests/permuto_second_order_reference.py, on test_permuto_encoding's shapes, interior rows and yardsticks:
the tangent by ||ours - R64|| <= 2 ||Rh - R64||, dQ/dx exactly zero, dQ/dparams per parameter (test_second_order says what m is)."""
import numpy as np
import pytest

from grid_reference import gamma, to_device
from permuto_reference import F32, F64
from permuto_second_order_reference import PermutoSecondOrder
from test_permuto_encoding import BACKWARD_CASES, N_ROWS, case_id, cfg, inputs, within_yardstick

CUTLASS = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
_DIRECTIONS = {}


def on(c):
    return dict(c, second_order=True)


def direction(D):
    """v = dL_ddLdx, uniform in [-1, 1], computed once per D"""
    if D not in _DIRECTIONS:
        _DIRECTIONS[D] = np.random.RandomState(41 + D).uniform(-1, 1, (N_ROWS, D)).astype(F32)
    return _DIRECTIONS[D]


def run(tcnn, D, c, x, params, dy, v, fp32=False):
    """C ABI forward + backward_backward_input of the encoding module -> (dL_ddLdy, dL/dx, dL/dparams) as numpy"""
    import torch

    T = F32 if fp32 else np.float16
    native = (tcnn.Encoding(D, on(c), dtype=torch.float32) if fp32 else tcnn.Encoding(D, on(c))).native_tcnn_module
    xt, pt, dyt = (to_device(a).requires_grad_(True) for a in (x, params.astype(T), dy.astype(T)))
    ctx, _ = native.fwd(xt, pt)
    t, dp, dx = native.bwd_bwd_input(ctx, xt, pt, to_device(v), dyt)
    return t.cpu().numpy(), dx.cpu().numpy(), dp.cpu().numpy()


@pytest.mark.parametrize("D", [2, 3, 7])
def test_reference_against_differences(D):
    """the float64 reference's tangent against central differences of the forward pass along v (interior rows: the step stays inside the
    simplex), <d, t> = <v, backward_input>, and dQ/dparams against a difference of Q along one random parameter direction (Q is linear)"""
    c = cfg(2)
    _, xi, params, dy = inputs(D, c, True)
    ref, xi, v, h, rs = PermutoSecondOrder(D, c), xi.astype(F64), direction(D).astype(F64), 1e-6, np.random.RandomState(3)

    def Q(p):
        return np.sum(v * ref.backward_input(xi, p, dy))

    t = ref.tangent(xi, v, params)
    assert np.abs((ref.forward(xi + h * v, params) - ref.forward(xi - h * v, params)) / (2 * h) - t).max() <= 1e-6 * np.abs(t).max()
    assert abs(np.sum(dy * t) - Q(params)) <= 1e-12 * np.abs(dy * t).sum()
    S, r = ref.param_gradient_terms(xi, v, dy)[0], rs.uniform(-1, 1, ref.n_params)
    assert abs((Q(params + h * r) - Q(params - h * r)) / (2 * h) - S @ r) <= 1e-6 * np.abs(S) @ np.abs(r)


@pytest.mark.gpu
@pytest.mark.parametrize("D,c", BACKWARD_CASES, ids=case_id)
def test_second_order(tcnn, D, c):
    """m, the fp32 roundings behind one contribution (half)(g * beta_r) of k_permuto_bwdbwd relative to its majorant, counted from
    weight_tangent: cf = (v * scale) * SF is 2 and SF's own rounding, 3; E'_i = sm - i * cf takes at most D - 1 additions into sm, the
    multiplication by i and the subtraction, D + 1; times 1 / (D + 1), rounded itself, 2; a selected s'[k] is one d' (the other terms are
    zeros), 0; beta_r = s' - s', 1; times g (a half, exact), 1: m = D + 8."""
    ref, x, params, dy = inputs(D, c, True)
    so, v, m = PermutoSecondOrder(D, c), direction(D), D + 8
    S, A, Abar, K = so.param_gradient_terms(x, v, dy)
    bound = 2.0 ** -11 * (A + np.abs(S)) + m * 2.0 ** -24 * Abar + (K + 1) * 2.0 ** -25
    rh = so.param_gradient_terms(x, v, dy, F32, np.float16)[0].astype(np.float16)  # the float32 reference, rounded as the kernel rounds
    assert np.all(np.abs(rh.astype(F64) - S) <= bound), "the float32 reference misses the bound: the inputs do not suit it"
    p = params.astype(np.float16)
    t, dx, dp = run(tcnn, D, c, x, params, dy, v)
    within_yardstick(t[:, :so.n_output_dims], so.tangent(x, v, p), so.tangent(x, v, p, F32, np.float16), f"{D}-D {case_id(c)} tangent")
    err = np.abs(dp.astype(F64) - S)
    print(f"dQ/dparams: largest error / bound = {np.max(err / bound):.3f}; {np.count_nonzero(K)} of {K.size} parameters touched")
    assert not np.any(t[:, so.n_output_dims:]) and not np.any(dx)
    assert np.all(err <= bound) and np.any(dp != 0) and not np.any(dp.view(np.uint16)[K == 0])
    for what, first, second in zip(("tangent", "dQ/dx", "dQ/dparams"), (t, dx, dp), run(tcnn, D, c, x, params, dy, v)):
        assert np.array_equal(first.view(np.uint8), second.view(np.uint8)), f"two runs differ: {what}"


@pytest.mark.gpu
def test_fp32_module(tcnn):
    D, c = 3, cfg(2)
    _, x, params, dy = inputs(D, c, True)
    so, v = PermutoSecondOrder(D, c), direction(D)
    t, dx, dp = run(tcnn, D, c, x, params, dy, v, fp32=True)
    within_yardstick(t, so.tangent(x, v, params), so.tangent(x, v, params, F32), "fp32 tangent")
    S, _, Abar, K = so.param_gradient_terms(x, v, dy, F32)
    assert np.all(np.abs(dp.astype(F64) - S) <= gamma(np.maximum(K - 1, 0), 2.0 ** -24) * Abar) and np.any(dp != 0) and not np.any(dx)


@pytest.mark.gpu
def test_many_directions_are_one_direction_each(tcnn):
    """input_jvp's one k_permuto_tangent launch for 3 directions against the single-direction second-order call, bit for bit: behind a
    CutlassMLP (48 wide: the network's two-pass route, whose contract this is) and on the bare encoding"""
    from test_input_gradient_gpu import _create_nwie, _net, _params, _same_bits
    from test_input_jvp_gpu import _second_order_tangent, _tangents

    D, c = 7, cfg(2)
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
        want = run(tcnn, D, c, x, params, dy, v[:, k].cpu().numpy())[0]
        assert np.array_equal(bare[:, k].view(np.uint16), want.view(np.uint16)) and np.any(bare[:, k] != 0)


@pytest.mark.gpu
def test_torch_double_backward(tcnn):
    """torch.autograd.grad(create_graph=True) on tcnn.Encoding at loss_scale 1: a zero input gradient and the native call's parameter bits"""
    import torch

    D, c = 3, cfg(2)
    _, x, params, dy = inputs(D, c, True)
    v = direction(D)
    _, _, dp = run(tcnn, D, c, x, params, dy, v)
    enc = tcnn.Encoding(D, on(c))
    with torch.no_grad():
        enc.params.copy_(to_device(params.astype(np.float16)))
    enc.loss_scale = 1.0
    xt = to_device(x).requires_grad_(True)
    (gx,) = torch.autograd.grad(enc(xt), xt, to_device(dy.astype(np.float16)), create_graph=True)
    (gx * to_device(v)).sum().backward()
    assert not bool(torch.any(xt.grad)) and np.array_equal(enc.params.grad.cpu().numpy(), dp.astype(F32)) and np.any(dp != 0)


@pytest.mark.gpu
def test_eikonal_step(tcnn):
    """PermutoGrid in front of a CutlassMLP: the double backward of an eikonal loss runs, with finite, non-zero gradients"""
    import torch

    model = tcnn.NetworkWithInputEncoding(3, 1, on(cfg(2)), CUTLASS)
    xt = to_device(inputs(3, cfg(2), True)[1]).requires_grad_(True)
    (gx,) = torch.autograd.grad(model(xt).float().sum(), xt, create_graph=True)
    ((gx.norm(dim=1) - 1) ** 2).mean().backward()
    n_enc = tcnn.Encoding(3, cfg(2)).params.numel()
    for g in (xt.grad, model.params.grad, model.params.grad[-n_enc:]):
        assert bool(torch.all(torch.isfinite(g))) and bool(torch.any(g != 0))


@pytest.mark.gpu
def test_the_switch(tcnn):
    with pytest.raises(RuntimeError, match="PermutoGrid: second_order must be true or false"):
        tcnn.Encoding(3, dict(cfg(2), second_order="yes"))
    for value in (True, False):
        assert tcnn.Encoding(3, dict(cfg(2), second_order=value)).native_tcnn_module.hyperparams()["second_order"] is value
