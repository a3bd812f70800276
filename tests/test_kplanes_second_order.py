"""The KPlanes second-order pass and tangent (k_kplanes.hip: k_kplanes_tangent, k_kplanes_bwdbwd_input, k_kplanes_bwdbwd, k_kplanes_bwdbwd_f32)
against tests/kplanes_second_order_reference.py, on test_kplanes_encoding's shapes and yardsticks: tangent and dQ/dx by
||ours - R64|| <= 2 ||Rh - R64||, dQ/dparams per parameter (test_second_order says what m is)."""
import numpy as np
import pytest

from grid_reference import gamma, to_device
from kplanes_reference import F32, F64
from kplanes_second_order_reference import KPlanesSecondOrder
from test_kplanes_encoding import BACKWARD_CASES, N_ROWS, case_id, cfg, inputs, within_yardstick

_DIRECTIONS = {}


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


@pytest.mark.parametrize("D,reduction", [(2, "Product"), (3, "Product"), (4, "Sum"), (4, "Product")])
def test_reference_against_differences(D, reduction):
    """the float64 reference's tangent, dQ/dx and dQ/dparams against central differences of the forward pass along v and of
    Q = <v, backward_input(x, params, d)> (fractions in float64; a step along one random direction of the parameters: Q is a polynomial in them)"""
    c = cfg(2, reduction)
    _, xi, params, dy = inputs(D, c, True)
    ref, xi, v, h, rs = KPlanesSecondOrder(D, c, fract=F64), xi.astype(F64), direction(D).astype(F64), 1e-6, np.random.RandomState(3)

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
    """m, the fp32 roundings behind one contribution (half)(g * fma(O_k, D_v w_c, w_c * S_k)) of k_kplanes_bwdbwd relative to its majorant,
    counted from its code.  vs = scale * v is 1, 1 - u is 1: D_v w_c = fma(+-vs_b, wa, +-vs_a * wb) is 3 per term and 1 for the fma: 4.
    Sum: times g, m = 5.  Product: a plane value is 7 and O_k, K - 1 of them and at most K - 1 multiplies, 8 (K - 1) (test_backward); a
    slope da = fma(u, dc, v1 - v0) is 1 for the difference, 3 for dc and 1: 4 on (|v1| + |v0|) + u sum|v|; T = fma(vs_b, db, vs_a * da) is
    1 + 4 + 1 per term and 1: 7; a term of S_k is one T and K - 2 plane values, 7 (K - 1), and passes at most K - 2 multiplies of its
    suffix or prefix, the multiply by T, K - 2 fused steps and the last two operations: 2 K - 1; S_k: 9 K - 8.  The weight is 3.  The two
    terms of the fma: 8 (K - 1) + 4 and 3 + 9 K - 8 + 1; the larger, the fma and the multiply by g: m = 9 K - 2."""
    ref, x, params, dy = inputs(D, c, True)
    so, v = KPlanesSecondOrder(D, c), direction(D)
    m = 9 * so.K - 2 if so.product and so.K > 1 else 5
    S, A, Abar, K = so.param_gradient_terms(x, v, params, dy)
    bound = 2.0 ** -11 * (A + np.abs(S)) + m * 2.0 ** -24 * Abar + (K + 1) * 2.0 ** -25
    rh = so.param_gradient_terms(x, v, params, dy, F32, np.float16)[0].astype(np.float16)  # the float32 reference, rounded as the kernel rounds
    assert np.all(np.abs(rh.astype(F64) - S) <= bound), "the float32 reference misses the bound: the inputs do not suit it"
    t, dx, dp = run(tcnn, D, c, x, params, dy, v)
    within_yardstick(t[:, :so.n_output_dims], so.tangent(x, v, params), so.tangent(x, v, params, F32, np.float16), f"{D}-D {case_id(c)} tangent")
    within_yardstick(dx, so.dQ_dx(x, v, params, dy), so.dQ_dx(x, v, params, dy, F32), f"{D}-D {case_id(c)} dQ/dx")
    err = np.abs(dp.astype(F64) - S)
    print(f"dQ/dparams: largest error / bound = {np.max(err / bound):.3f}; {np.count_nonzero(K)} of {K.size} parameters touched")
    assert np.all(err <= bound) and np.any(dp != 0) and not np.any(dp.view(np.uint16)[K == 0]) and not np.any(t[:, so.n_output_dims:])
    for what, first, second in zip(("tangent", "dQ/dx", "dQ/dparams"), (t, dx, dp), run(tcnn, D, c, x, params, dy, v)):
        assert np.array_equal(first.view(np.uint8), second.view(np.uint8)), f"two runs differ: {what}"


@pytest.mark.gpu
def test_input_jvp_is_the_tangent(tcnn):
    """native.input_jvp with two tangents: each is the dL_ddLdy of a backward_backward_input call, bit for bit"""
    D, c = 4, cfg(8, "Product")
    _, x, params, dy = inputs(D, c, True)
    vs = np.stack([direction(D), direction(D)[::-1]], axis=1)
    xt, pt = to_device(x), to_device(params.astype(np.float16))
    jvp = tcnn.Encoding(D, c).native_tcnn_module.input_jvp(xt, pt, to_device(vs))[0].cpu().numpy()
    for i in range(2):
        assert np.array_equal(jvp[:, i].view(np.uint16), run(tcnn, D, c, x, params, dy, vs[:, i])[0].view(np.uint16)) and np.any(jvp[:, i] != 0)


@pytest.mark.gpu
def test_fp32_module(tcnn):
    D, c = 3, cfg(2, "Product")
    _, x, params, dy = inputs(D, c, True)
    so, v = KPlanesSecondOrder(D, c), direction(D)
    t, dx, dp = run(tcnn, D, c, x, params, dy, v, fp32=True)
    within_yardstick(t, so.tangent(x, v, params), so.tangent(x, v, params, F32), "fp32 tangent")
    within_yardstick(dx, so.dQ_dx(x, v, params, dy), so.dQ_dx(x, v, params, dy, F32), "fp32 dQ/dx")
    S, _, Abar, K = so.param_gradient_terms(x, v, params, dy, F32)
    assert np.all(np.abs(dp.astype(F64) - S) <= gamma(np.maximum(K - 1, 0), 2.0 ** -24) * Abar) and np.any(dp != 0)


@pytest.mark.gpu
def test_torch_double_backward(tcnn):
    """torch.autograd.grad(create_graph=True) on tcnn.Encoding at loss_scale 1 returns the native call's bits"""
    import torch

    D, c = 3, cfg(2, "Product")
    _, x, params, dy = inputs(D, c, True)
    v = direction(D)
    _, dx, dp = run(tcnn, D, c, x, params, dy, v)
    enc = tcnn.Encoding(D, c)
    with torch.no_grad():
        enc.params.copy_(to_device(params.astype(np.float16)))
    enc.loss_scale = 1.0
    xt = to_device(x).requires_grad_(True)
    (gx,) = torch.autograd.grad(enc(xt), xt, to_device(dy.astype(np.float16)), create_graph=True)
    (gx * to_device(v)).sum().backward()
    assert np.array_equal(xt.grad.cpu().numpy(), dx) and np.array_equal(enc.params.grad.cpu().numpy(), dp.astype(F32))


@pytest.mark.gpu
@pytest.mark.parametrize("tail,block", [({"otype": "Frequency", "n_frequencies": 2}, 3), ({"otype": "DenseGrid", "n_levels": 1, "base_resolution": 4}, 4)], ids=["Frequency", "DenseGrid"])
def test_composite(tcnn, tail, block):
    """Composite[KPlanes on 3 dims, `tail` on 1]: no longer refused; the planes' columns (padded to `block` by a grid's alignment of 2)
    are the standalone module's, their padding exactly zero in the tangent"""
    D, c = 3, cfg(1, "Product")
    _, x, params, dy = inputs(D, c, True)
    v, rs = direction(D), np.random.RandomState(9)
    t, dx, dp = run(tcnn, D, c, x, params, dy, v)
    composite = {"otype": "Composite", "nested": [dict(c, n_dims_to_encode=3), dict(tail, n_dims_to_encode=1)]}
    native = tcnn.Encoding(4, composite).native_tcnn_module
    wide = lambda a, n: np.concatenate([a, rs.uniform(0.1, 0.9, (N_ROWS, n)).astype(F32)], axis=1)  # noqa: E731
    tail_params = rs.uniform(-1, 1, native.n_params() - params.size).astype(F32)
    dy4 = np.concatenate([dy, np.zeros((N_ROWS, block - 3), F32), wide(dy[:, :0], native.n_output_dims() - block)], axis=1)
    ct, cdx, cdp = run(tcnn, 4, composite, wide(x, 1), np.concatenate([params, tail_params]), dy4, wide(v, 1))
    assert np.array_equal(ct[:, :3].view(np.uint16), t.view(np.uint16)) and not np.any(ct[:, 3:block]) and np.any(ct[:, block:] != 0)
    assert np.array_equal(cdx[:, :3], dx) and np.array_equal(cdp[:params.size].view(np.uint16), dp.view(np.uint16))


@pytest.mark.gpu
def test_network_with_input_encoding(tcnn):
    """KPlanes in front of a CutlassMLP: the double backward of an eikonal-style loss runs, with finite, non-zero gradients"""
    import torch

    network = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    model = tcnn.NetworkWithInputEncoding(3, 1, cfg(2, "Product"), network)
    xt = to_device(inputs(3, cfg(2, "Product"), True)[1]).requires_grad_(True)
    (gx,) = torch.autograd.grad(model(xt).float().sum(), xt, create_graph=True)
    ((gx.norm(dim=1) - 1) ** 2).mean().backward()
    for g in (xt.grad, model.params.grad):
        assert bool(torch.all(torch.isfinite(g))) and bool(torch.any(g != 0))
