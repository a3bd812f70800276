"""The TensoRF encoding (k_tensorf.hip) against tests/tensorf_reference.py, by the yardsticks of test_kplanes_encoding.py: values and dL/dx
||ours - R64|| <= 2 ||Rh - R64||, Rh the function in float32 rounded once to the output precision; dL/dparams in half per parameter
|got - S| <= 2^-11 (A + |S|) + m 2^-24 Abar + (k + 1) 2^-25 (test_backward says what m is); fp32: gamma(k - 1) Abar at u = 2^-24."""
import numpy as np
import pytest

from grid_reference import edge_x, gamma, to_device
from tensorf_reference import F32, F64, TensoRF

N_ROWS = 768  # the batch granularity times 3


def cfg(decomposition, F, L=3, base=4, scale=1.7):
    return {"otype": "TensoRF", "decomposition": decomposition, "n_components": F, "n_levels": L, "base_resolution": base, "per_level_scale": scale}


# F = 2: a lane's 16-byte chunk holds four (level, mode) units; F = 16, 32: two and four chunks per mode; 48 levels of F = 4: 72 chunks per
# row, a sample's lanes span two waves
CASES = [(3, cfg("VM", 2)), (3, cfg("VM", 16, L=1, base=5)), (3, cfg("VM", 32, L=2)), (3, cfg("VM", 4, L=48, scale=1.02)), (2, cfg("CP", 8)), (4, cfg("CP", 2)), (3, cfg("CP", 16, L=1, base=5))]
# where the accumulators go (k_tensorf_bwd's passes): R = 96: planes in the global scratch, lines in LDS; R = 18: planes alone fill the LDS, the
# lines take a pass of their own; CP at R = 600: a line longer than the LDS holds, two segments.  Every case above: planes and lines together.
BACKWARD_CASES = CASES + [(3, cfg("VM", 16, L=1, base=96)), (3, cfg("VM", 8, L=1, base=18)), (2, cfg("CP", 8, L=1, base=600))]
NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
_INPUTS = {}


def case_id(v):
    return f"{v}d" if isinstance(v, int) else f"{v['decomposition']}-F{v['n_components']}-L{v['n_levels']}-R{v['base_resolution']}"


def inputs(D, c, interior):
    """(reference, x, params, dL/dy), computed once.  x: uniform rows; not interior: also 0, 1, negatives, > 1 (edge_x), rows with
    x_0 = 1.5 / (base_resolution - 1), exactly on a cell boundary of level 0, and rows out to [-1, 2]; interior: every fraction of every level
    at least 1e-3 away from 0 and 1"""
    key = (D, case_id(c), interior)
    if key not in _INPUTS:
        ref, rs = TensoRF(D, c), np.random.RandomState(29 + D)
        x = rs.uniform(0, 1, (4 * N_ROWS, D)).astype(F32)
        if interior:
            x = x[ref.min_fraction(x) >= 1e-3][:N_ROWS]
        else:
            boundary = rs.uniform(0, 1, (32, D)).astype(F32)
            boundary[:, 0] = 1.5 / (c["base_resolution"] - 1)
            x = np.concatenate([x[:N_ROWS - 128], edge_x(64, D), boundary, rs.uniform(-1, 2, (32, D)).astype(F32)])
        assert x.shape == (N_ROWS, D) and (interior or ref.min_fraction(x).min() == 0)
        params = rs.uniform(-1, 1, ref.n_params).astype(np.float16).astype(F32)
        dy = rs.uniform(-1, 1, (N_ROWS, ref.n_output_dims)).astype(np.float16).astype(F32)
        _INPUTS[key] = (ref, x, params, dy)
    return _INPUTS[key]


def within_yardstick(got, r64, rh, what):
    ours, theirs = np.linalg.norm(got.astype(F64) - r64), np.linalg.norm(rh.astype(F64) - r64)
    print(f"{what}: ||ours - R64|| = {ours:.4g}, ||Rh - R64|| = {theirs:.4g}")
    assert np.all(np.isfinite(got)) and np.any(got != 0) and ours <= 2 * theirs, what


def run(tcnn, D, c, x, params, dy, fp32=False):
    """C ABI forward + backward of the encoding module -> (output, dL/dx, dL/dparams) as numpy"""
    import torch

    T = F32 if fp32 else np.float16
    native = (tcnn.Encoding(D, c, dtype=torch.float32) if fp32 else tcnn.Encoding(D, c)).native_tcnn_module
    xt, pt = to_device(x).requires_grad_(True), to_device(params.astype(T)).requires_grad_(True)
    ctx, out = native.fwd(xt, pt)
    dx, dp = native.bwd(ctx, xt, pt, out, to_device(dy.astype(T)))
    return out.cpu().numpy(), dx.cpu().numpy(), dp.cpu().numpy()


@pytest.mark.parametrize("D,decomposition", [(3, "VM"), (2, "CP"), (4, "CP")])
def test_reference_jacobian(D, decomposition):
    """the float64 reference's analytic dy/dx against central differences on interior rows (fractions in float64: nothing quantises the step)"""
    c = cfg(decomposition, 2)
    _, xi, params, _ = inputs(D, c, True)
    ref, xi, h = TensoRF(D, c, fract=F64), xi.astype(F64), 1e-6
    jac = ref.dy_dx(xi, params)
    for d in range(D):
        step = h * np.eye(D)[d]
        assert np.abs((ref.forward(xi + step, params) - ref.forward(xi - step, params)) / (2 * h) - jac[:, :, d]).max() <= 1e-6 * np.abs(jac).max()


@pytest.mark.gpu
@pytest.mark.parametrize("D,c", CASES, ids=case_id)
def test_forward(tcnn, D, c):
    ref, x, params, dy = inputs(D, c, False)
    out, _, _ = run(tcnn, D, c, x, params, dy)
    assert out.shape == (N_ROWS, ref.n_output_dims)  # a stand-alone module is not padded; test_composite has the padding columns
    within_yardstick(out, ref.forward(x, params), ref.forward(x, params, F32, np.float16), f"{D}-D {case_id(c)} output")
    assert np.array_equal(out.view(np.uint16), run(tcnn, D, c, x, params, dy)[0].view(np.uint16)), "two runs differ"


@pytest.mark.gpu
@pytest.mark.parametrize("D,c", BACKWARD_CASES, ids=case_id)
def test_backward(tcnn, D, c):
    """m, the fp32 operations behind one contribution (half)((g * others) * w) of k_tensorf_bwd, counted from its code.  A line value
    fmaf(w, v1, (1 - w) * v0) is 3 roundings relative to its majorant; a plane value is 4 fused multiply-adds on weights (1 - x) * (1 - y) of
    3 operations each: 7 (as KPlanes counts it).  VM, a plane's corner: others = V (3), g * V (1), the corner weight (3), the product (1):
    m = 8.  VM, a line's entry: others = P (7), g * P (1), the weight 1 - w (1), the product (1): m = 10.  CP: others is D - 1 line values
    (3 each) combined by at most D - 1 multiplies (prefix, suffix, prefix * suffix), then g * others, 1 - w and the product:
    m = 4 (D - 1) + 3.  The test holds every parameter to the larger count of its decomposition."""
    ref, x, params, dy = inputs(D, c, True)
    m = 4 * (D - 1) + 3 if ref.cp else 10
    S, A, Abar, K = ref.param_gradient_terms(x, params, dy)
    bound = 2.0 ** -11 * (A + np.abs(S)) + m * 2.0 ** -24 * Abar + (K + 1) * 2.0 ** -25
    rh = ref.param_gradient_terms(x, params, dy, F32, np.float16)[0].astype(np.float16)  # the float32 reference, rounded as the kernel rounds
    assert np.all(np.abs(rh.astype(F64) - S) <= bound), "the float32 reference misses the bound: the inputs do not suit it"
    _, dx, dp = run(tcnn, D, c, x, params, dy)
    within_yardstick(dx, ref.backward_input(x, params, dy), ref.backward_input(x, params, dy, F32), f"{D}-D {case_id(c)} dL/dx")
    err = np.abs(dp.astype(F64) - S)
    print(f"dL/dparams: largest error / bound = {np.max(err / bound):.3f}; {np.count_nonzero(K)} of {K.size} parameters touched")
    assert np.all(err <= bound) and np.any(dp != 0) and not np.any(dp.view(np.uint16)[K == 0])
    again = run(tcnn, D, c, x, params, dy)
    assert np.array_equal(dx.view(np.uint32), again[1].view(np.uint32)) and np.array_equal(dp.view(np.uint16), again[2].view(np.uint16)), "two runs differ"


@pytest.mark.gpu
def test_fp32_module(tcnn):
    D, c = 3, cfg("VM", 4)
    ref, x, params, dy = inputs(D, c, True)
    out, dx, dp = run(tcnn, D, c, x, params, dy, fp32=True)
    within_yardstick(out, ref.forward(x, params), ref.forward(x, params, F32), "fp32 output")
    within_yardstick(dx, ref.backward_input(x, params, dy), ref.backward_input(x, params, dy, F32), "fp32 dL/dx")
    S, _, Abar, K = ref.param_gradient_terms(x, params, dy, F32)
    assert np.all(np.abs(dp.astype(F64) - S) <= gamma(np.maximum(K - 1, 0), 2.0 ** -24) * Abar) and np.any(dp != 0)


@pytest.mark.gpu
def test_composite(tcnn):
    """VM (18 columns, padded with ones to the 8 the next TensoRF asks for), CP and an Identity, each on its slice of 6-D rows"""
    ca, cb = cfg("VM", 2), cfg("CP", 8, L=1, base=5)
    (ra, xa, pa, _), (rb, xb, pb, _), xc = inputs(3, ca, False), inputs(2, cb, False), np.random.RandomState(3).uniform(0, 1, (N_ROWS, 1)).astype(F32)
    composite = {"otype": "Composite", "nested": [dict(ca, n_dims_to_encode=3), dict(cb, n_dims_to_encode=2), {"otype": "Identity", "n_dims_to_encode": 1}]}
    native = tcnn.Encoding(6, composite).native_tcnn_module
    out = native.fwd(to_device(np.concatenate([xa, xb, xc], axis=1)), to_device(np.concatenate([pa, pb]).astype(np.float16)))[1].cpu().numpy()
    assert out.shape == (N_ROWS, 24 + 8 + 1) and np.all(out[:, 18:24] == 1) and np.array_equal(out[:, 32:], xc.astype(np.float16))
    for got, ref, xs, ps in ((out[:, :18], ra, xa, pa), (out[:, 24:32], rb, xb, pb)):
        within_yardstick(got, ref.forward(xs, ps), ref.forward(xs, ps, F32, np.float16), "nested output")


@pytest.mark.gpu
def test_torch_module_and_hyperparams(tcnn):
    """tcnn.Encoding under autograd gives the C ABI call's bits; hyperparams() returns every key"""
    import torch

    D, c = 3, cfg("VM", 16, L=1, base=5, scale=2.0)
    ref, x, params, dy = inputs(D, c, True)
    out, dx, dp = run(tcnn, D, c, x, params, dy)
    enc = tcnn.Encoding(D, {**c, "otype": "tensorf", "decomposition": "vm"})

    def hyperparams(module):
        h = module.native_tcnn_module.hyperparams()
        return {**h, "per_level_scale": round(h["per_level_scale"], 6)}  # (a float in the library)

    assert enc.native_tcnn_module.name() == "TensoRF" and hyperparams(enc) == c
    assert hyperparams(tcnn.Encoding(3, {"otype": "TensoRF"})) == cfg("VM", 16, L=1, base=128, scale=2.0)
    with torch.no_grad():
        enc.params.copy_(to_device(params.astype(np.float16)))
    enc.loss_scale = 1.0  # as the C ABI call above
    xt = to_device(x).requires_grad_(True)
    y = enc(xt)
    y.backward(to_device(dy.astype(np.float16)))
    assert np.array_equal(y.detach().cpu().numpy().view(np.uint16), out.view(np.uint16)) and np.array_equal(xt.grad.cpu().numpy(), dx)
    assert np.array_equal(enc.params.grad.cpu().numpy(), dp.astype(F32))
    for second_order in (lambda: torch.autograd.grad(enc(xt).float().sum(), xt, create_graph=True)[0].sum().backward(), lambda: enc.input_jvp(xt, torch.ones_like(xt))):
        with pytest.raises(RuntimeError, match="not implemented"):
            second_order()


@pytest.mark.gpu
def test_training_reduces_the_loss(tcnn):
    """NetworkWithInputEncoding (VM, F = 16, 64 x 2 FullyFusedMLP, Adam) on a smooth 3-D target; measured: mean of the last ten losses / mean of the first ten = 0.0004"""
    import torch

    model = {"loss": {"otype": "RelativeL2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2}, "encoding": cfg("VM", 16, L=1, base=16, scale=2.0), "network": NETWORK}
    tr = tcnn.create_from_config(3, 1, model).trainer
    gen, losses = torch.Generator(device="cuda").manual_seed(3), []
    for _ in range(100):
        x = torch.rand((4096, 3), device="cuda", generator=gen)
        losses.append(tr.loss(tr.training_step(x, 0.5 + 0.5 * torch.sin(2 * np.pi * x.sum(dim=1, keepdim=True) / 3) * torch.cos(3 * x[:, :1]))))
    print(f"mean of the last ten losses / mean of the first ten = {np.mean(losses[-10:]) / np.mean(losses[:10]):.4f}")
    assert np.all(np.isfinite(losses)) and np.mean(losses[-10:]) < np.mean(losses[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("D,extra,message", [(2, {}, "TensoRF: n_dims_to_encode"), (4, {}, "TensoRF: n_dims_to_encode"), (1, {"decomposition": "CP"}, "TensoRF: n_dims_to_encode"),
                                             (5, {"decomposition": "CP"}, "TensoRF: n_dims_to_encode"), (3, {"n_components": 3}, "TensoRF: n_components"),
                                             (3, {"decomposition": "Tucker"}, "TensoRF: decomposition"), (3, {"base_resolution": 50000}, "TensoRF: base_resolution")])
def test_constructor_refuses(tcnn, D, extra, message):
    with pytest.raises(RuntimeError, match=message):
        tcnn.Encoding(D, dict(cfg("VM", 2), **extra))
