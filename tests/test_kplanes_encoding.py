"""The KPlanes encoding (k_kplanes.hip) against tests/kplanes_reference.py.  Yardstick for values and dL/dx, the project's own (DESIGN.md
"Second-order pass"): ||ours - R64|| <= 2 ||Rh - R64||, Rh the function in float32 rounded once to the output precision.  dL/dparams, half:
per parameter |got - S| <= 2^-11 (A + |S|) + m 2^-24 Abar + (k + 1) 2^-25 (test_backward says what m is).  fp32: the float32
contributions summed in any order, gamma(k - 1) Abar at u = 2^-24."""
import numpy as np
import pytest

from grid_reference import edge_x, gamma, to_device
from kplanes_reference import F32, F64, KPlanes

N_ROWS = 768  # the batch granularity times 3


def cfg(F, reduction, L=3, base=4, scale=1.7):
    return {"otype": "KPlanes", "n_levels": L, "n_features_per_level": F, "base_resolution": base, "per_level_scale": scale, "reduction": reduction}


# every D, every F, both reductions; 70 levels: a sample's levels span two waves; 96^2 entries x 3 planes x 2 x 8 B: does not fit the LDS
CASES = [(2, cfg(1, "Product")), (3, cfg(2, "Product")), (3, cfg(4, "Sum")), (4, cfg(8, "Product")), (4, cfg(2, "Sum")), (3, cfg(2, "Product", L=70, scale=1.02))]
BACKWARD_CASES = CASES + [(3, cfg(2, "Product", L=1, base=96))]
NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
_INPUTS = {}


def case_id(v):
    return f"{v}d" if isinstance(v, int) else f"F{v['n_features_per_level']}-{v['reduction']}-L{v['n_levels']}-R{v['base_resolution']}"


def inputs(D, c, interior):
    """(reference, x, params, dL/dy), computed once.  x: uniform rows; not interior: also 0, 1, negatives, > 1 (edge_x), rows with x_0 = 0.5
    (base_resolution 4: 3 * 0.5 + 0.5 = 2, exactly on a cell boundary of level 0) and rows out to [-1, 2]; interior: every fraction of every
    level at least 1e-3 away from 0 and 1"""
    key = (D, case_id(c), interior)
    if key not in _INPUTS:
        ref, rs = KPlanes(D, c), np.random.RandomState(23 + D)
        x = rs.uniform(0, 1, (4 * N_ROWS, D)).astype(F32)
        if interior:
            x = x[ref.min_fraction(x) >= 1e-3][:N_ROWS]
        else:
            boundary = rs.uniform(0, 1, (32, D)).astype(F32)
            boundary[:, 0] = 0.5
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


@pytest.mark.parametrize("D,reduction", [(2, "Product"), (3, "Product"), (4, "Sum"), (4, "Product")])
def test_reference_jacobian(D, reduction):
    """the float64 reference's analytic dy/dx against central differences on interior rows (fractions in float64: nothing quantises the step)"""
    c = cfg(2, reduction)
    _, xi, params, _ = inputs(D, c, True)
    ref, xi, h = KPlanes(D, c, fract=F64), xi.astype(F64), 1e-6
    jac = ref.dy_dx(xi, params)
    for d in range(D):
        step = h * np.eye(D)[d]
        assert np.abs((ref.forward(xi + step, params) - ref.forward(xi - step, params)) / (2 * h) - jac[:, :, d]).max() <= 1e-6 * np.abs(jac).max()


@pytest.mark.gpu
@pytest.mark.parametrize("fp32", [False, True], ids=["half", "fp32"])
@pytest.mark.parametrize("reduction", ["Product", "Sum"])
def test_one_plane_is_the_dense_grid(tcnn, reduction, fp32):
    """D = 2: the output's bits are the 2-D DenseGrid / Linear output's, on the same parameter vector"""
    c = cfg(2, reduction)
    ref, x, params, dy = inputs(2, c, False)
    dense = {**{k: v for k, v in c.items() if k != "reduction"}, "otype": "DenseGrid", "interpolation": "Linear"}
    ours, theirs = run(tcnn, 2, c, x, params, dy, fp32)[0], run(tcnn, 2, dense, x, params, dy, fp32)[0]
    bits = np.uint32 if fp32 else np.uint16
    print(f"{np.count_nonzero(ours.view(bits) != theirs.view(bits))} of {ours.size} elements differ, by at most {np.abs(ours.astype(F64) - theirs).max():.3g}")
    assert np.array_equal(ours.view(bits), theirs.view(bits))


@pytest.mark.gpu
@pytest.mark.parametrize("D,c", CASES, ids=case_id)
def test_forward(tcnn, D, c):
    ref, x, params, dy = inputs(D, c, False)
    out, _, _ = run(tcnn, D, c, x, params, dy)
    within_yardstick(out, ref.forward(x, params), ref.forward(x, params, F32, np.float16), f"{D}-D {case_id(c)} output")
    assert np.array_equal(out.view(np.uint16), run(tcnn, D, c, x, params, dy)[0].view(np.uint16)), "two runs differ"


@pytest.mark.gpu
@pytest.mark.parametrize("D,c", BACKWARD_CASES, ids=case_id)
def test_backward(tcnn, D, c):
    """m, the fp32 operations behind one contribution (half)(g * (prefix * suffix) * w) of k_kplanes_bwd, counted from its code.  Sum: the
    weight w = (1 - x) * (1 - y) is 3 and the product g * w is 1: m = 4.  Product: each of the K - 1 other plane values is 4 fused
    multiply-adds on weights of 3 operations each -- 7 roundings relative to its majorant; combining them (prefix, suffix, prefix * suffix) is
    at most K - 1 multiplies; g * other, the weight and the last product are 5: m = 8 (K - 1) + 5."""
    ref, x, params, dy = inputs(D, c, True)
    m = 8 * (ref.K - 1) + 5 if ref.product else 4
    S, A, Abar, K = ref.param_gradient_terms(x, params, dy)
    bound = 2.0 ** -11 * (A + np.abs(S)) + m * 2.0 ** -24 * Abar + (K + 1) * 2.0 ** -25
    rh = ref.param_gradient_terms(x, params, dy, F32, np.float16)[0].astype(np.float16)  # the float32 reference, rounded as the kernel rounds
    assert np.all(np.abs(rh.astype(F64) - S) <= bound), "the float32 reference misses the bound: the inputs do not suit it"
    _, dx, dp = run(tcnn, D, c, x, params, dy)
    within_yardstick(dx, ref.backward_input(x, params, dy), ref.backward_input(x, params, dy, F32), f"{D}-D {case_id(c)} dL/dx")
    err = np.abs(dp.astype(F64) - S)
    print(f"dL/dparams: largest error / bound = {np.max(err / bound):.3f}; {np.count_nonzero(K)} of {K.size} parameters touched")
    assert np.all(err <= bound) and np.any(dp != 0) and not np.any(dp.view(np.uint16)[K == 0])
    assert np.array_equal(dp.view(np.uint16), run(tcnn, D, c, x, params, dy)[2].view(np.uint16)), "two runs differ"


@pytest.mark.gpu
def test_fp32_module(tcnn):
    D, c = 3, cfg(2, "Product")
    ref, x, params, dy = inputs(D, c, True)
    out, dx, dp = run(tcnn, D, c, x, params, dy, fp32=True)
    within_yardstick(out, ref.forward(x, params), ref.forward(x, params, F32), "fp32 output")
    within_yardstick(dx, ref.backward_input(x, params, dy), ref.backward_input(x, params, dy, F32), "fp32 dL/dx")
    S, _, Abar, K = ref.param_gradient_terms(x, params, dy, F32)
    assert np.all(np.abs(dp.astype(F64) - S) <= gamma(np.maximum(K - 1, 0), 2.0 ** -24) * Abar) and np.any(dp != 0)


@pytest.mark.gpu
def test_composite_and_trainer_surfaces(tcnn):
    """Nested in a Composite beside a PermutoGrid, each on a slice of wider rows: the planes' 3 columns are padded with ones to the lattice's
    alignment of 8.  Then the trainer's own forms against the C ABI's: SoA input, and GradientMode::Accumulate onto zeros."""
    import torch

    from permuto_reference import Permuto
    from tinycudann.native import GRADIENT_ACCUMULATE, GRADIENT_OVERWRITE, LAYOUT_SOA

    ca, cb = cfg(1, "Product"), {"otype": "PermutoGrid", "n_levels": 5, "n_features_per_level": 8, "log2_hashmap_size": 8, "base_resolution": 2, "per_level_scale": 1.7}
    (ra, xa, pa, _), (_, xb, _, _), rb = inputs(2, ca, False), inputs(3, cfg(2, "Product"), False), Permuto(3, cb)
    pb = np.random.RandomState(5).uniform(-1, 1, rb.n_params).astype(np.float16).astype(F32)
    composite = {"otype": "Composite", "nested": [dict(ca, n_dims_to_encode=2), dict(cb, n_dims_to_encode=3)]}
    out = tcnn.Encoding(5, composite).native_tcnn_module.fwd(to_device(np.concatenate([xa, xb], axis=1)), to_device(np.concatenate([pa, pb]).astype(np.float16)))[1].cpu().numpy()
    assert out.shape == (N_ROWS, 48) and np.all(out[:, 3:8] == 1)
    for got, ref, xs, ps in ((out[:, :3], ra, xa, pa), (out[:, 8:], rb, xb, pb)):
        within_yardstick(got, ref.forward(xs, ps), ref.forward(xs, ps, F32, np.float16), "nested output")

    D, c = 3, cfg(2, "Product")
    ref, x, params, _ = inputs(D, c, False)
    model = {"loss": {"otype": "RelativeL2"}, "optimizer": {"otype": "Adam"}, "encoding": c, "network": NETWORK}

    def step(soa, mode):
        tr = tcnn.Trainer(D, 1, model, seed=7)
        tr.set_params(torch.cat([tr.params()[:-ref.n_params], to_device(params.astype(np.float16))]))
        assert not bool(torch.any(tr.param_gradients()))  # the zeros Accumulate adds onto
        xin, layout = (to_device(x).t().contiguous(), {"input_layout": LAYOUT_SOA}) if soa else (to_device(x), {})
        tr.training_step(xin, to_device(x[:, :1]), run_optimizer=False, gradient_mode=mode, **layout)
        return tr.inference(xin, **layout), tr.param_gradients()[-ref.n_params:].view(torch.int16)

    base = step(False, GRADIENT_OVERWRITE)
    for what, other in (("SoA input", step(True, GRADIENT_OVERWRITE)), ("Accumulate onto zeros", step(False, GRADIENT_ACCUMULATE))):
        assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1]) and bool(torch.any(base[1] != 0)), what


@pytest.mark.gpu
def test_torch_module_and_hyperparams(tcnn):
    """tcnn.Encoding under autograd gives the C ABI call's bits; hyperparams() returns every key"""
    D, c = 4, cfg(2, "Sum")
    ref, x, params, dy = inputs(D, c, True)
    out, dx, dp = run(tcnn, D, c, x, params, dy)
    enc = tcnn.Encoding(D, {**c, "otype": "kplanes", "reduction": "sum"})
    import torch

    def hyperparams(module):
        h = module.native_tcnn_module.hyperparams()
        return {**h, "per_level_scale": round(h["per_level_scale"], 6)}  # (a float in the library)

    assert enc.native_tcnn_module.name() == "KPlanes" and hyperparams(enc) == c
    assert hyperparams(tcnn.Encoding(3, {"otype": "KPlanes"})) == cfg(2, "Product", L=4, base=64, scale=2.0)

    with torch.no_grad():
        enc.params.copy_(to_device(params.astype(np.float16)))
    enc.loss_scale = 1.0  # as the C ABI call above: at the default 128 a contribution (half)(128 g w) is not 128 (half)(g w) where that is subnormal
    xt = to_device(x).requires_grad_(True)
    y = enc(xt)
    y.backward(to_device(dy.astype(np.float16)))
    assert np.array_equal(y.detach().cpu().numpy().view(np.uint16), out.view(np.uint16)) and np.array_equal(xt.grad.cpu().numpy(), dx)
    assert np.array_equal(enc.params.grad.cpu().numpy(), dp.astype(F32))


@pytest.mark.gpu
def test_training_reduces_the_loss(tcnn):
    """4-D, Product: a product of planes drawn as the grid draws its tables (1e-4) would be zero in half, and so would every gradient"""
    import torch

    model = {"loss": {"otype": "RelativeL2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2}, "encoding": cfg(2, "Product", base=8, scale=2.0), "network": NETWORK}
    tr = tcnn.create_from_config(4, 1, model).trainer
    gen, losses = torch.Generator(device="cuda").manual_seed(3), []
    for _ in range(100):
        x = torch.rand((4096, 4), device="cuda", generator=gen)
        losses.append(tr.loss(tr.training_step(x, 0.5 + 0.5 * torch.sin(2 * np.pi * x.sum(dim=1, keepdim=True) / 4) * torch.cos(3 * x[:, :1]))))
    print(f"mean of the last ten losses / mean of the first ten = {np.mean(losses[-10:]) / np.mean(losses[:10]):.4f}")
    assert np.all(np.isfinite(losses)) and np.mean(losses[-10:]) < np.mean(losses[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("D,extra,message", [(1, {}, "KPlanes: n_dims_to_encode"), (5, {}, "KPlanes: n_dims_to_encode"), (3, {"n_features_per_level": 3}, "KPlanes: n_features_per_level"),
                                             (3, {"reduction": "Max"}, "KPlanes: reduction")])
def test_constructor_refuses(tcnn, D, extra, message):
    with pytest.raises(RuntimeError, match=message):
        tcnn.Encoding(D, dict(cfg(2, "Product"), **extra))
