"""CutlassMLP of any width (multiples of 16 up to 1024), with zero hidden layers and with Sine: the layer-by-layer path (k_mlp_layers.hip,
Network::layerwise) against the CPU oracle, a numpy restatement for Sine, and the fused kernels under TCNN_AMD_MLP_LAYERWISE=1.

CPU tests (creation, parameter counts, error messages) go through the C ABI; every other test is marked gpu."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import CONFIG_C3B
from grad_checks import assert_structural_zeros, assert_weight_grads_close, layer_slices

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(tcnn):
    from tinycudann import _C

    return _C


def _net(width, hidden, act="ReLU", out_act="None", otype="CutlassMLP"):
    return {"otype": otype, "activation": act, "output_activation": out_act, "n_neurons": width, "n_hidden_layers": hidden}


def _create(lib, n_in, n_out, net):
    h = C.c_void_p()
    rc = lib.lib.tcnn_create_network(n_in, n_out, json.dumps(net).encode(), C.byref(h))
    return rc, h


# ---------------------------------------------------------------------------------------------------- CPU: configuration semantics
@pytest.mark.parametrize("n_in,n_out,width,hidden,act", [(32, 3, 48, 2, "ReLU"), (32, 3, 96, 3, "Tanh"), (64, 20, 512, 1, "ReLU"), (32, 3, 64, 0, "None"),
                                                        (16, 16, 128, 0, "ReLU"), (32, 3, 1024, 1, "Sine"), (32, 3, 208, 2, "Sine")])
def test_cutlass_shapes_create(lib, oracle, n_in, n_out, width, hidden, act):
    """n_params and the layer layout follow oracle.Mlp (cutlass_mlp.cu:57-67): with zero hidden layers one [padded_out][in] matrix."""
    net = _net(width, hidden, act)
    rc, h = _create(lib, n_in, n_out, net)
    assert rc == 0, lib.lib.tcnn_last_error()
    ref = oracle.Mlp({**net, "n_input_dims": n_in, "n_output_dims": n_out})
    sizes = ref.layer_sizes()
    assert lib.lib.tcnn_module_n_params(h) == ref.n_params == sum(r * c for r, c in sizes)
    if hidden == 0:
        assert sizes == [(16 * ((n_out + 15) // 16), n_in)]
    hp = json.loads(lib.lib.tcnn_module_hyperparams(h))["network"]
    assert hp == {"otype": "CutlassMLP", "activation": act, "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}
    lib.lib.tcnn_module_destroy(h)


@pytest.mark.parametrize("width", [40, 2048, 8, 0])
def test_cutlass_width_rule(lib, width):
    rc, _ = _create(lib, 32, 3, _net(width, 2))
    assert rc != 0
    assert b"n_neurons must be a multiple of 16 between 16 and 1024" in lib.lib.tcnn_last_error()


def test_fully_fused_messages_unchanged(lib):
    rc, _ = _create(lib, 32, 3, _net(48, 2, otype="FullyFusedMLP"))
    assert rc != 0 and b"only supports 16, 32, 64, and 128 neurons" in lib.lib.tcnn_last_error()
    rc, _ = _create(lib, 32, 3, _net(64, 2, "Sine", otype="FullyFusedMLP"))
    assert rc != 0 and b"Sine activation is not supported" in lib.lib.tcnn_last_error()
    rc, _ = _create(lib, 32, 3, _net(64, 0, otype="FullyFusedMLP"))
    assert rc != 0 and b"requires at least 1 hidden layer" in lib.lib.tcnn_last_error()


# ---------------------------------------------------------------------------------------------------- GPU helpers
def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint16)


def _f32(bits):
    return bits.view(np.float16).astype(np.float32)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


def elem_close(a, b, rtol=1e-2, floor=1e-3):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    bound = rtol * np.abs(b) + floor * max(float(np.max(np.abs(b))), 1e-30)
    return float(np.max(np.abs(a - b) / bound))


def _fwd_bwd(tcnn, net_module, x, n_out, padded, seed=5):
    """torch autograd through a tcnn module: (output, dL/dparams, dL/dx), gradients in loss-scaled units"""
    xt = _t(x).requires_grad_(True)
    out = net_module(xt)
    n = x.shape[0]
    dy = np.random.RandomState(seed).uniform(-1.0, 1.0, (n, n_out)).astype(np.float16).astype(np.float32)
    out.backward(_t(dy.astype(np.float16)).to(out.dtype))
    dy_h = np.zeros((n, padded), dtype=np.float32)
    dy_h[:, :n_out] = dy
    return (out.detach().float().cpu().numpy(), net_module.params.grad.detach().float().cpu().numpy() * 128.0, xt.grad.detach().cpu().numpy() * 128.0, dy_h)


# ---------------------------------------------------------------------------------------------------- GPU: against the oracle
ORACLE_CASES = [
    (32, 3, _net(48, 2, "ReLU")),
    (32, 3, _net(96, 3, "Tanh")),
    (64, 20, _net(192, 2, "ReLU", "Sigmoid")),
    (32, 3, _net(512, 2, "ReLU")),
    (128, 3, _net(80, 1, "Softplus")),
    (16, 3, _net(64, 0, "None")),
    (32, 20, _net(64, 0, "None", "Sigmoid")),
    (32, 3, _net(1024, 1, "ReLU")),
]


# Over 2^16 rows the ReLU flips of _check_dx reach the weight gradients of the two wide, two-hidden-layer ReLU cases (by n_neurons): a flipped
# unit's dL/dhidden of one sample is a whole term of the sum, and 1e-3 of a layer's largest gradient is about one term at this batch size.
# float64 sums against the oracle's fp32 ones exceed the per-layer bar there on the CPU alone, with every input seed tried (1.2-2.4 x in the second
# layer); tests/test_grad_checks.py asserts that, and that every other case -- and these two at 512 rows -- stays below half of it.
FLIPS_EXCEED_THE_BAR_AT_2_16 = (192, 512)


@gpu
@pytest.mark.parametrize("n", [512, (1 << 16) + 256])
@pytest.mark.parametrize("n_in,n_out,net_cfg", ORACLE_CASES)
def test_layerwise_network_matches_oracle(tcnn, oracle, n_in, n_out, net_cfg, n):
    """tcnn.Network (Identity + CutlassMLP, layer by layer) vs the oracle with fp32 accumulation: the bars of
    test_gpu_parity.test_network_forward_backward -- parameters bit-equal, outputs element-wise within 1e-2, gradients within 2e-2."""
    net = tcnn.Network(n_in, n_out, net_cfg, seed=1337)
    ref = oracle.NetworkWithInputEncoding(n_in, n_out, {"otype": "Identity"}, net_cfg)
    params = ref.initialize_params(oracle.Pcg32(1337))
    assert np.array_equal(net.params.detach().cpu().numpy().view(np.uint32), params.view(np.uint32))
    params_h = oracle.half_bits(params)
    x = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in)
    want_out, ctx = ref.forward(x, params_h)
    got, got_dp, got_dx, dy_h = _fwd_bwd(tcnn, net, x, n_out, ref.padded_output_width)
    assert got.shape == (n, n_out)
    assert elem_close(got, _f32(want_out)[:, :n_out]) <= 1.0
    dy_scaled = oracle.half_bits(dy_h.astype(np.float16).astype(np.float32) * 128.0)
    grads32 = np.zeros(ref.n_params, dtype=np.float32)
    grads_h = np.zeros(ref.n_params, dtype=np.uint16)
    want_dx, _ = ref.backward(x, params_h, ctx, want_out, dy_scaled, want_dL_dx=True, grads_half=grads_h, grads_f32=grads32)
    assert rel_err(got_dp, grads32) < 2e-2
    what = f"layer by layer {n_in} -> {n_out} {net_cfg} n = {n}"
    if n <= 512 or net_cfg["n_neurons"] not in FLIPS_EXCEED_THE_BAR_AT_2_16:
        assert_weight_grads_close(got_dp, grads32, layer_slices(ref.network), 2e-2, True, what)  # per layer, per element (grad_checks.weight_grad_ratios)
    assert_structural_zeros(got_dp, grads32, layer_slices(ref.network), what)
    _check_dx(got_dx, want_dx)


def _check_dx(got_dx, want_dx):
    """dL/dx within rel_err 2e-2.  Over 2^16 rows a few samples have a hidden pre-activation within an fp32 rounding of zero, which one
    side passes through ReLU and the other does not (the fp32 sums differ in order): their dL/dx rows differ by a whole unit's share.
    Such rows must be rare (< 1e-3 of them) and the rest must meet the bar; norm-wise the whole matrix is within 1e-2."""
    n = got_dx.shape[0]
    if n <= 512:
        assert rel_err(got_dx, want_dx) < 2e-2
        return
    scale = max(float(np.max(np.abs(want_dx))), 1e-30)
    bad = np.max(np.abs(got_dx.astype(np.float64) - want_dx), axis=1) >= 2e-2 * scale
    assert np.count_nonzero(bad) <= 1e-3 * n
    assert float(np.linalg.norm(got_dx - want_dx)) <= 1e-2 * float(np.linalg.norm(want_dx))


# ---------------------------------------------------------------------------------------------------- GPU: Sine
def _siren_init(oracle, sizes, seed):
    """cutlass_mlp.cu:360-366 / gpu_matrix.h:335-369 restated: per matrix in layout order, the first U(+-30/fan_in), the others
    U(+-sqrt(6/fan_in)), fan_in = cols, the whole padded matrix row-major from one pcg32 stream"""
    rng = oracle.Pcg32(seed)
    out = []
    for l, (r, c) in enumerate(sizes):
        s = np.float32(30.0) / np.float32(c) if l == 0 else np.sqrt(np.float32(6.0) / np.float32(c), dtype=np.float32)
        for _ in range(r * c):
            u = np.float32(rng.next_float())
            out.append(np.float32(np.float32(u * np.float32(2.0)) * s) - s)
    return np.array(out, dtype=np.float32)


def _sine_reference(x_h, params, sizes, n_out_padded):
    """forward with the half pre-activations kept, backward dpre = grad * half(cos(pre)) (cutlass_mlp.cu:101-113); float64 sums"""
    Ws, off = [], 0
    for r, c in sizes:
        Ws.append(params[off:off + r * c].astype(np.float16).astype(np.float64).reshape(r, c))
        off += r * c
    h = x_h.astype(np.float64)
    ins, pres = [], []
    for l, W in enumerate(Ws):
        ins.append(h)
        pre = (h @ W.T).astype(np.float16)
        if l == len(Ws) - 1:
            out = pre
        else:
            pres.append(pre)
            h = np.sin(pre.astype(np.float32)).astype(np.float16).astype(np.float64)

    def backward(dY):
        g = dY.astype(np.float16)
        grads = [None] * len(Ws)
        for l in range(len(Ws) - 1, -1, -1):
            grads[l] = g.astype(np.float64).T @ ins[l]
            d = (g.astype(np.float64) @ Ws[l]).astype(np.float16)
            if l > 0:
                g = (d * np.cos(pres[l - 1].astype(np.float32)).astype(np.float16)).astype(np.float16)
            else:
                dx = d
        return np.concatenate([gr.ravel() for gr in grads]), dx

    return out, backward


@gpu
@pytest.mark.parametrize("width,hidden", [(64, 3), (64, 0), (96, 2)])
def test_sine_network(tcnn, oracle, width, hidden):
    """SIREN init bit for bit, forward against the oracle (its Sine forward is the reference's), gradients against the numpy backward"""
    n_in, n_out, n = 32, 3, 1024
    cfg = _net(width, hidden, "Sine")
    net = tcnn.Network(n_in, n_out, cfg, seed=1337)
    ref = oracle.NetworkWithInputEncoding(n_in, n_out, {"otype": "Identity"}, cfg)
    sizes = ref.network.layer_sizes()
    want_p = _siren_init(oracle, sizes, 1337)
    got_p = net.params.detach().cpu().numpy()
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    params_h = oracle.half_bits(got_p)
    x = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in)
    want_out, _ = ref.forward(x, params_h)
    got, got_dp, got_dx, dy_h = _fwd_bwd(tcnn, net, x, n_out, ref.padded_output_width)
    assert elem_close(got, _f32(want_out)[:, :n_out]) <= 1.0
    x_h = x.astype(np.float16)
    np_out, backward = _sine_reference(x_h, got_p, sizes, ref.padded_output_width)
    assert elem_close(got, np_out[:, :n_out].astype(np.float32)) <= 1.0
    want_dp, want_dx = backward(dy_h * 128.0)
    assert rel_err(got_dp, want_dp) < 2e-2
    assert_weight_grads_close(got_dp, want_dp, layer_slices(ref.network), 2e-2, True, f"Sine {width} x {hidden}")
    assert_structural_zeros(got_dp, want_dp, layer_slices(ref.network), f"Sine {width} x {hidden}")
    assert rel_err(got_dx, want_dx) < 2e-2


@gpu
def test_sine_trainer_learns(tcnn):
    """200 steps of a SIREN (Identity -> 64 x 3 Sine) on a smooth 2-D target: the loss ends below the first step's"""
    cfg = {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-3}, "encoding": {"otype": "Identity"}, "network": _net(64, 3, "Sine")}
    tr = tcnn.Trainer(2, 1, cfg, seed=1337)
    rs = np.random.RandomState(3)
    losses = []
    for _ in range(200):
        x = rs.uniform(0, 1, (4096, 2)).astype(np.float32)
        t = (0.5 + 0.25 * np.sin(4 * x[:, :1]) * np.cos(3 * x[:, 1:])).astype(np.float32)
        ctx = tr.training_step(_t(x), _t(t))
        losses.append(tr.loss(ctx))
    assert tr.last_step_kernel() == "unfused"
    assert np.all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0]


# ---------------------------------------------------------------------------------------------------- GPU: training steps
GRID_96x3 = {**CONFIG_C3B, "network": _net(96, 3, "ReLU")}
IDENTITY_0 = {**CONFIG_C3B, "encoding": {"otype": "Identity"}, "network": _net(64, 0, "None")}


def _step(tcnn, n_in, cfg, x, t, run_optimizer=False):
    tr = tcnn.Trainer(n_in, 3, cfg, seed=1337)
    ctx = tr.training_step(_t(x), _t(t), run_optimizer=run_optimizer)
    return tr, {"kernel": tr.last_step_kernel(), "out": _bits(ctx.output()), "L": ctx.L().cpu().numpy(), "dy": _bits(ctx.dL_doutput()),
                "g": _bits(tr.param_gradients()), "loss": tr.loss(ctx)}


@gpu
@pytest.mark.parametrize("cfg", [GRID_96x3, IDENTITY_0], ids=["hashgrid_96x3", "identity_0hidden"])
def test_training_step_matches_oracle(tcnn, oracle, cfg):
    """Trainer.training_step runs the unfused sequence on the layer-by-layer network; the bars of
    test_training_step_matrix._check_against_oracle"""
    from test_training_step_matrix import _check_against_oracle

    n = 4096
    x, t = oracle.synthetic_batch(n, 2, 3, seed=42)
    ref = oracle.Trainer(2, 3, cfg, seed=1337)
    tr = tcnn.Trainer(2, 3, cfg, seed=1337)
    # the grid's initial entries (U(+-1e-4)) put a 3-hidden-layer network's outputs among fp16 subnormals, where the element-wise bar
    # measures rounding: both sides start from the same larger grid entries instead
    p = _bits(tr.params()).copy()
    n_net = ref.model.network.n_params
    p[n_net:] = oracle.half_bits(np.random.RandomState(1).uniform(-0.5, 0.5, p.size - n_net).astype(np.float32))
    tr.set_params(_t(p.view(np.float16)))
    ref.params = p.copy()
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    want = ref.training_step(x, t, run_optimizer=False, grads_f32=grads32)
    ctx = tr.training_step(_t(x), _t(t), run_optimizer=False)
    got = {"out": _bits(ctx.output()), "L": ctx.L().cpu().numpy(), "dy": _bits(ctx.dL_doutput()), "g": _bits(tr.param_gradients()), "loss": tr.loss(ctx)}
    assert tr.last_step_kernel() == "unfused"
    _check_against_oracle(ref, want, grads32, got, n, 3)


@gpu
def test_loss_curve_tracks_oracle(tcnn, oracle):
    n, steps = 4096, 12
    ref = oracle.Trainer(2, 3, GRID_96x3, seed=1337)
    tr = tcnn.Trainer(2, 3, GRID_96x3, seed=1337)
    losses_ref, losses = [], []
    for s in range(steps):
        x, _ = oracle.synthetic_batch(n, 2, 3, seed=100 + s)
        t = np.stack([np.sin(6.0 * x[:, 0]) * 0.5 + 0.5, x[:, 1] * x[:, 0], np.cos(4.0 * x[:, -1]) * 0.5 + 0.5], axis=1).astype(np.float32)
        losses_ref.append(ref.training_step(x, t)["loss"])
        losses.append(tr.loss(tr.training_step(_t(x), _t(t))))
    losses_ref, losses = np.array(losses_ref), np.array(losses)
    assert losses[-1] < losses[0]
    assert np.all(np.abs(losses - losses_ref) <= 0.05 * np.abs(losses_ref) + 1e-6)


OPTIMIZERS = [
    {"otype": "SGD", "learning_rate": 1e-2, "l2_reg": 1e-4},
    {"otype": "Ema", "decay": 0.9, "nested": {"otype": "ExponentialDecay", "decay_start": 1, "decay_interval": 1, "decay_base": 0.5, "nested": CONFIG_C3B["optimizer"]}},
    {"otype": "Novograd", "learning_rate": 1e-2},
    {"otype": "Lookahead", "alpha": 0.5, "n_steps": 2, "nested": {"otype": "Average", "n_samples": 2, "nested": {"otype": "Batched", "batch_size_multiplier": 2, "nested": CONFIG_C3B["optimizer"]}}},
]


@gpu
@pytest.mark.parametrize("opt", OPTIMIZERS, ids=["sgd", "ema_decay_adam", "novograd", "lookahead_average_batched"])
def test_optimizer_wrappers(tcnn, oracle, opt):
    """every optimizer wrapper over a layer-by-layer network (Identity -> 96 x 2): four steps, losses within 5 % of the oracle's"""
    cfg = {"loss": {"otype": "L2"}, "optimizer": opt, "encoding": {"otype": "Identity"}, "network": _net(96, 2, "ReLU")}
    ref = oracle.Trainer(2, 3, cfg, seed=1337)
    tr = tcnn.Trainer(2, 3, cfg, seed=1337)
    for s in range(4):
        x, t = oracle.synthetic_batch(1024, 2, 3, seed=200 + s)
        want = ref.training_step(x, t)["loss"]
        got = tr.loss(tr.training_step(_t(x), _t(t)))
        assert abs(got - want) <= 0.05 * abs(want) + 1e-6
    assert tr.last_step_kernel() == "unfused"


@gpu
def test_use_inference_params_with_ema(tcnn, oracle):
    from test_training_step_matrix import _check_against_oracle

    cfg = {**GRID_96x3, "optimizer": {"otype": "Ema", "decay": 0.9, "nested": CONFIG_C3B["optimizer"]}}
    n = 256 * 9
    tr = tcnn.Trainer(2, 3, cfg, seed=1337)
    for s in range(3):
        x, t = oracle.synthetic_batch(n, 2, 3, seed=100 + s)
        tr.training_step(_t(x), _t(t))
    ema, p_before = _bits(tr.params_inference()), _bits(tr.params())
    assert not np.array_equal(ema, p_before)
    x, t = oracle.synthetic_batch(n, 2, 3, seed=7)
    ctx = tr.training_step(_t(x), _t(t), run_optimizer=False, use_inference_params=True)
    assert tr.last_step_kernel() == "unfused" and np.array_equal(_bits(tr.params()), p_before)
    ref = oracle.Trainer(2, 3, cfg, seed=1337)
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    ref.params = p_before.copy()
    ref.optimizer.weights_ema[:] = ema
    want = ref.training_step(x, t, run_optimizer=False, grads_f32=grads32, use_inference_params=True)
    got = {"out": _bits(ctx.output()), "L": ctx.L().cpu().numpy(), "dy": _bits(ctx.dL_doutput()), "g": _bits(tr.param_gradients()), "loss": tr.loss(ctx)}
    _check_against_oracle(ref, want, grads32, got, n, 3)
    assert rel_err(tr.inference(_t(x)).cpu().numpy(), ref.model.inference(x, ema)) < 1e-2  # inference runs at the EMA weights


# ---------------------------------------------------------------------------------------------------- GPU: A/B against the fused kernels
@gpu
@pytest.mark.parametrize("width,hidden", [(64, 2), (128, 4)])
def test_layerwise_switch_agrees_with_fused_kernels(tcnn, oracle, monkeypatch, width, hidden):
    """TCNN_AMD_MLP_LAYERWISE=1 on shapes the specialised kernels cover: inference, forward / backward through tcnn.Network and a C3B
    training step agree with the default kernels within the bars of _check_against_unfused"""
    from test_training_step_matrix import _check_against_unfused

    net_cfg = _net(width, hidden, "ReLU", otype="FullyFusedMLP")
    n = 8192
    x = oracle.Pcg32(42).uniform_strided(n * 32).reshape(n, 32)

    def network_run(env):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            net = tcnn.Network(32, 3, net_cfg, seed=1337)
            import torch

            with torch.no_grad():
                inf = net(_t(x)).float().cpu().numpy()
            return (inf,) + _fwd_bwd(tcnn, net, x, 3, 16)[:3]

    a, b = network_run({}), network_run({"TCNN_AMD_MLP_LAYERWISE": "1"})
    for got, ref_ in ((b[0], a[0]), (b[1], a[1])):
        assert float(np.max(np.abs(got - ref_))) <= 4e-3 * max(1.0, float(np.max(np.abs(ref_))))
    for got, ref_ in ((b[2], a[2]), (b[3], a[3])):
        assert float(np.linalg.norm(got - ref_)) <= 5e-3 * float(np.linalg.norm(ref_))

    cfg = {**CONFIG_C3B, "network": net_cfg}
    xs, ts = oracle.synthetic_batch(4096, 2, 3, seed=42)
    with monkeypatch.context() as m:
        m.setenv("TCNN_AMD_FUSED_STEP", "0")
        _, unf = _step(tcnn, 2, cfg, xs, ts)
    with monkeypatch.context() as m:
        m.setenv("TCNN_AMD_MLP_LAYERWISE", "1")
        _, lw = _step(tcnn, 2, cfg, xs, ts)
    assert lw["kernel"] == "unfused"
    _check_against_unfused(lw, unf)


# ---------------------------------------------------------------------------------------------------- GPU: surfaces and determinism
@gpu
@pytest.mark.parametrize("enc,n_in,width", [({"otype": "OneBlob", "n_bins": 32}, 2, 96),
                                            ({"otype": "Composite", "nested": [{"n_dims_to_encode": 1, "otype": "OneBlob", "n_bins": 16},
                                                                               {"otype": "Identity"}]}, 3, 48)],
                         ids=["oneblob64_96x2", "composite_48x2"])
def test_network_with_input_encoding(tcnn, oracle, enc, n_in, width):
    """tcnn.NetworkWithInputEncoding: no fused OneBlob input, the encoding's own kernel writes the batch; against the oracle"""
    net_cfg = _net(width, 2, "ReLU")
    n, n_out = 2048, 3
    mod = tcnn.NetworkWithInputEncoding(n_in, n_out, enc, net_cfg, seed=1337)
    ref = oracle.NetworkWithInputEncoding(n_in, n_out, enc, net_cfg)
    params = ref.initialize_params(oracle.Pcg32(1337))
    assert np.array_equal(mod.params.detach().cpu().numpy().view(np.uint32), params.view(np.uint32))
    params_h = oracle.half_bits(params)
    x = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in)
    want_out, ctx = ref.forward(x, params_h)
    got, got_dp, _, dy_h = _fwd_bwd(tcnn, mod, x, n_out, ref.padded_output_width)
    assert elem_close(got, _f32(want_out)[:, :n_out]) <= 1.0
    dy_scaled = oracle.half_bits(dy_h.astype(np.float16).astype(np.float32) * 128.0)
    grads32 = np.zeros(ref.n_params, dtype=np.float32)
    ref.backward(x, params_h, ctx, want_out, dy_scaled, want_dL_dx=False, grads_f32=grads32)
    assert rel_err(got_dp, grads32) < 2e-2
    assert_weight_grads_close(got_dp, grads32, layer_slices(ref.network), 2e-2, True, f"tcnn.NetworkWithInputEncoding {enc['otype']} -> {width} x 2")
    assert_structural_zeros(got_dp, grads32, layer_slices(ref.network), f"tcnn.NetworkWithInputEncoding {enc['otype']} -> {width} x 2")


@gpu
def test_snapshot_round_trip_of_a_sine_model(tcnn, oracle):
    cfg = {"loss": {"otype": "L2"}, "optimizer": CONFIG_C3B["optimizer"], "encoding": {"otype": "Identity"}, "network": _net(80, 2, "Sine")}
    tr = tcnn.Trainer(2, 3, cfg, seed=1337)
    for s in range(3):
        x, t = oracle.synthetic_batch(1024, 2, 3, seed=300 + s)
        tr.training_step(_t(x), _t(t))
    x, _ = oracle.synthetic_batch(1024, 2, 3, seed=9)
    want = tr.inference(_t(x)).cpu().numpy()
    assert tr.network_hyperparams()["network"] == {"otype": "CutlassMLP", "activation": "Sine", "output_activation": "None", "n_neurons": 80, "n_hidden_layers": 2}
    blob = tr.serialize(serialize_optimizer=True)
    tr2 = tcnn.Trainer(2, 3, cfg, seed=7)
    tr2.deserialize(blob)
    assert np.array_equal(tr2.inference(_t(x)).cpu().numpy().view(np.uint32), want.view(np.uint32))


@gpu
@pytest.mark.parametrize("cfg", [GRID_96x3, {**IDENTITY_0, "network": _net(208, 2, "Sine")}], ids=["hashgrid_96x3", "identity_208x2_sine"])
def test_gradients_are_deterministic(tcnn, oracle, cfg):
    x, t = oracle.synthetic_batch(256 * 33, 2, 3, seed=11)
    _, a = _step(tcnn, 2, cfg, x, t)
    _, b = _step(tcnn, 2, cfg, x, t)
    assert np.any(a["g"] != 0)
    assert np.array_equal(a["g"], b["g"]) and np.array_equal(a["out"], b["out"])
