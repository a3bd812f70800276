"""The PermutoGrid encoding (k_permuto.hip) against tests/permuto_reference.py.  Yardstick for values and dL/dx, the project's own (DESIGN.md
"Second-order pass"): ||ours - R64|| <= 2 ||Rh - R64||, Rh the recipe in float32 rounded once to the output precision.  dL/dparams, half:
per parameter |got - S| <= 2^-11 (sum|c| + |S|) + 2^-20 sum|c| + (k + 1) 2^-25 -- every contribution's rounding to half and the final one,
the fp32 weights, subnormal spacing.  fp32: the float32 contributions summed in any order, gamma(k - 1) sum|c| at u = 2^-24."""
import numpy as np
import pytest

from grid_reference import edge_x, to_device
from permuto_reference import F32, F64, Permuto

N_ROWS = 768  # the batch granularity times 3


def cfg(F, L=5, log2_t=8, scale=1.7):
    return {"otype": "PermutoGrid", "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": log2_t, "base_resolution": 2, "per_level_scale": scale}


# (D, config): a diagonal of D x F; 70 levels: a sample's levels span two waves; 2^16 entries: the level does not fit the LDS
CASES = [(2, cfg(1)), (3, cfg(2)), (4, cfg(8)), (7, cfg(2)), (7, cfg(1)), (3, cfg(2, L=70, scale=1.05))]
BACKWARD_CASES = CASES + [(4, cfg(2, log2_t=16))]
_INPUTS = {}


def case_id(v):
    return f"{v}d" if isinstance(v, int) else f"L{v['n_levels']}-F{v['n_features_per_level']}-T{v['log2_hashmap_size']}"


def inputs(D, c, interior):
    """(reference, x, params, dL/dy), computed once.  x: uniform rows; not interior: also 0, 1, negatives, > 1 (edge_x), rows out to [-1, 2]
    and rows ON simplex faces (x_0 = 0: two equal residuals at every level); interior: every level's smallest weight >= 1e-3"""
    key = (D, case_id(c), interior)
    if key not in _INPUTS:
        ref, rs = Permuto(D, c), np.random.RandomState(11 + D)
        x = rs.uniform(0, 1, (2 * N_ROWS, D)).astype(F32)
        if interior:
            x = x[ref.min_weight(x) >= 1e-3][:N_ROWS]
        else:
            face = rs.uniform(0, 1, (32, D)).astype(F32)
            face[:, 0] = 0
            x = np.concatenate([x[:N_ROWS - 128], edge_x(64, D), face, rs.uniform(-1, 2, (32, D)).astype(F32)])
        assert x.shape == (N_ROWS, D) and (interior or ref.min_weight(x).min() <= 1e-12)
        params = rs.uniform(-1, 1, ref.n_params).astype(F32)
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


@pytest.mark.parametrize("D", [2, 3, 7])
def test_reference_properties_and_gradient(D):
    ref, x, params, _ = inputs(D, cfg(2), False)
    for level in range(ref.L):
        rem0, rank, b = ref.simplex(x, level)
        keys = np.stack([ref.keys(rem0, rank, r) for r in range(D + 1)], axis=1)  # [n, vertex, component]
        assert np.abs(b.sum(axis=1) - 1).max() <= 1e-12 and b.min() >= -1e-12 and np.all(keys.sum(axis=2) == 0)
        assert all(len({tuple(k) for k in row}) == D + 1 for row in keys)
    _, xi, _, _ = inputs(D, cfg(2), True)
    xi, jac, h = xi.astype(F64), ref.dy_dx(xi, params), 1e-6
    for d in range(D):
        step = h * np.eye(D)[d]
        assert np.abs((ref.forward(xi + step, params) - ref.forward(xi - step, params)) / (2 * h) - jac[:, :, d]).max() <= 1e-6 * np.abs(jac).max()


@pytest.mark.gpu
@pytest.mark.parametrize("D,c", CASES, ids=case_id)
def test_forward(tcnn, D, c):
    ref, x, params, dy = inputs(D, c, False)
    p = params.astype(np.float16)
    out, _, _ = run(tcnn, D, c, x, params, dy)
    within_yardstick(out, ref.forward(x, p), ref.forward(x, p, F32, np.float16), f"{D}-D {case_id(c)} output")
    assert np.array_equal(out.view(np.uint16), run(tcnn, D, c, x, params, dy)[0].view(np.uint16)), "two runs differ"


@pytest.mark.gpu
@pytest.mark.parametrize("D,c", BACKWARD_CASES, ids=case_id)
def test_backward(tcnn, D, c):
    ref, x, params, dy = inputs(D, c, True)
    p = params.astype(np.float16)
    _, dx, dp = run(tcnn, D, c, x, params, dy)
    within_yardstick(dx, ref.backward_input(x, p, dy), ref.backward_input(x, p, dy, F32), f"{D}-D {case_id(c)} dL/dx")
    S, A, K = ref.param_gradient_terms(x, dy)
    err, bound = np.abs(dp.astype(F64) - S), 2.0 ** -11 * (A + np.abs(S)) + 2.0 ** -20 * A + (K + 1) * 2.0 ** -25
    print(f"dL/dparams: largest error / bound = {np.max(err / bound):.3f}; {np.count_nonzero(K)} of {K.size} parameters touched")
    assert np.all(err <= bound) and np.any(dp != 0) and not np.any(dp.view(np.uint16)[K == 0])
    assert np.array_equal(dp.view(np.uint16), run(tcnn, D, c, x, params, dy)[2].view(np.uint16)), "two runs differ"


@pytest.mark.gpu
def test_fp32_module(tcnn):
    D, c = 3, cfg(2)
    ref, x, params, dy = inputs(D, c, True)
    out, dx, dp = run(tcnn, D, c, x, params, dy, fp32=True)
    within_yardstick(out, ref.forward(x, params), ref.forward(x, params, F32), "fp32 output")
    within_yardstick(dx, ref.backward_input(x, params, dy), ref.backward_input(x, params, dy, F32), "fp32 dL/dx")
    S, A, K = ref.param_gradient_terms(x, dy, F32)
    m = np.maximum(K - 1, 0) * 2.0 ** -24
    assert np.all(np.abs(dp.astype(F64) - S) <= m / (1 - m) * A) and np.any(dp != 0)


@pytest.mark.gpu
def test_composite_padding_and_slices(tcnn):
    """nested in a Composite: the first encoding's 5 columns are padded to the second one's alignment with ones; both read a slice of wider rows"""
    (ra, xa, pa, _), (rb, xb, pb, _) = inputs(2, cfg(1), False), inputs(3, cfg(8), False)
    x, p = np.concatenate([xa, xb], axis=1), np.concatenate([pa, pb]).astype(np.float16)
    composite = {"otype": "Composite", "nested": [dict(cfg(1), n_dims_to_encode=2), dict(cfg(8), n_dims_to_encode=3)]}
    out = tcnn.Encoding(5, composite).native_tcnn_module.fwd(to_device(x), to_device(p))[1].cpu().numpy()
    assert out.shape == (N_ROWS, 48) and np.all(out[:, 5:8] == 1)
    for got, ref, xs, ps in ((out[:, :5], ra, xa, pa), (out[:, 8:], rb, xb, pb)):
        within_yardstick(got, ref.forward(xs, ps.astype(np.float16)), ref.forward(xs, ps.astype(np.float16), F32, np.float16), "nested output")


@pytest.mark.gpu
def test_trainer_layout_and_gradient_mode(tcnn):
    """The C ABI's module calls take AoS rows and overwrite; SoA input and GradientMode::Accumulate are the trainer's.  Each against AoS + Overwrite."""
    import torch

    from tinycudann.native import GRADIENT_ACCUMULATE, GRADIENT_OVERWRITE, LAYOUT_SOA

    D, c = 3, cfg(2)
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


NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
ENC5 = {"otype": "Permutohedral", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}


@pytest.mark.gpu
def test_torch_modules(tcnn):
    import torch

    D, c = 3, cfg(2)
    ref, x, params, dy = inputs(D, c, True)
    out, dx, dp = run(tcnn, D, c, x, params, dy)
    enc = tcnn.Encoding(D, c)
    assert enc.native_tcnn_module.name() == "PermutoGrid" and enc.native_tcnn_module.hyperparams()["hash"] == "CoherentPrime"
    with torch.no_grad():
        enc.params.copy_(to_device(params.astype(np.float16)))
    enc.loss_scale = 1.0  # as the C ABI call above: at the default 128 a contribution (half)(128 g b) is not 128 (half)(g b) where that is subnormal
    xt = to_device(x).requires_grad_(True)
    y = enc(xt)
    y.backward(to_device(dy.astype(np.float16)))
    assert np.array_equal(y.detach().cpu().numpy().view(np.uint16), out.view(np.uint16)) and np.array_equal(xt.grad.cpu().numpy(), dx)
    assert np.array_equal(enc.params.grad.cpu().numpy(), dp.astype(F32))

    # NetworkWithInputEncoding: inference = forward; input_gradient against the reference composed with the network's own input gradient
    ref5, x5, _, _ = inputs(5, {**ENC5, "n_levels": 8}, True)
    model, net = tcnn.NetworkWithInputEncoding(5, 1, ENC5, NETWORK), tcnn.Network(16, 1, NETWORK)
    n_net = net.params.numel()
    assert model.params.numel() == n_net + ref5.n_params
    with torch.no_grad():
        model.params[n_net:].copy_((torch.rand(ref5.n_params, device="cuda") * 2 - 1).half())
        net.params.copy_(model.params[:n_net])
        pe = model.params[n_net:].half()
        encoded = tcnn.Encoding(5, ENC5).native_tcnn_module.fwd(to_device(x5), pe)[1]
        inferred = model(to_device(x5))
    assert torch.equal(inferred, model(to_device(x5).requires_grad_(True)).detach())
    d_enc = (net.input_gradient(encoded.float(), dim=0) * 128).half().float().cpu().numpy() / 128  # dL/dy reaches the encoding as half at the loss scale
    pe = pe.cpu().numpy()
    within_yardstick(model.input_gradient(to_device(x5), dim=0).cpu().numpy(), ref5.backward_input(x5, pe, d_enc), ref5.backward_input(x5, pe, d_enc, F32), "input_gradient")

    native, v = enc.native_tcnn_module, torch.ones((N_ROWS, 1, D), device="cuda")
    with pytest.raises(RuntimeError, match="input_jvp: not implemented for"):
        enc.input_jvp(xt.detach(), v)
    ctx, o = native.fwd(xt, enc.params.detach().half().requires_grad_(True))
    with pytest.raises(RuntimeError, match="backward_backward_input_impl: not implemented error"):
        native.bwd_bwd_input(ctx, xt, enc.params.detach().half().requires_grad_(True), v[:, 0].contiguous(), to_device(dy.astype(np.float16)).requires_grad_(True))


@pytest.mark.gpu
def test_training_reduces_the_loss(tcnn):
    import torch

    model = {"loss": {"otype": "RelativeL2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2}, "encoding": ENC5, "network": NETWORK}
    tr = tcnn.create_from_config(5, 1, model).trainer
    gen, losses = torch.Generator(device="cuda").manual_seed(3), []
    for _ in range(100):
        x = torch.rand((4096, 5), device="cuda", generator=gen)
        losses.append(tr.loss(tr.training_step(x, 0.5 + 0.5 * torch.sin(2 * np.pi * x.sum(dim=1, keepdim=True) / 5) * torch.cos(3 * x[:, :1]))))
    print(f"mean of the last ten losses / mean of the first ten = {np.mean(losses[-10:]) / np.mean(losses[:10]):.4f}")
    assert np.all(np.isfinite(losses)) and np.mean(losses[-10:]) < np.mean(losses[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("D,extra,message", [(3, {"n_features_per_level": 3}, "PermutoGrid: n_features_per_level"), (3, {"hash": "Prime"}, "PermutoGrid: hash must be CoherentPrime, not Prime"),
                                             (1, {}, "PermutoGrid: n_dims_to_encode"), (8, {}, "PermutoGrid: n_dims_to_encode")])
def test_constructor_refuses(tcnn, D, extra, message):
    with pytest.raises(RuntimeError, match=message):
        tcnn.Encoding(D, dict(cfg(2), **extra))
