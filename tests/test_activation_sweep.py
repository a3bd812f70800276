"""Every activation over every finite fp16 input, in each MLP kernel family.

The activation code of mlp_device.h (activation_fwd, activation_bwd, act_d1, act_d2, act_fwd_t, act_bwd_t) is compiled separately into
k_mlp.hip, k_train.hip, k_train_regs.hip and k_mlp_layers.hip, three of them with compiler flags of their own.  Every other test feeds it
pre-activations within about |z| < 4.  Here the 63 488 finite halves go through each activation in each of these files, in the setting of
tests/activation_sweep.py (identity weights: the network's output is the activation of its input, element by element), forward and backward:
expf overflowing to a half infinity, the cancellation in Squareplus for negative arguments, sinf's range reduction up to 65504, Sigmoid and Tanh
in saturation, fp16 subnormals through the MFMA and the half stores, inf * 0 in the backward expressions.

Forward: against the oracle network on the rows whose results are all finite (+0 and -0 equal) -- bit for bit for None, ReLU, LeakyReLU and
Squareplus (*, +, sqrtf and / only), and for the activations that call expf, logf, tanhf or sinf at least 99.9 % of the halves identical and
every other one an adjacent half (the bar of test_losses._assert_fused_loss_close).  Backward: dL/dinput against the elementwise
orc_activation_backward(dL/dy, the kernel's OWN forward output), bit for bit, but for Softplus (an expf in the derivative) and a Sine layer of the
layer-by-layer path (differentiated from the stored pre-activation: hmul(dL/dy, half(cosf(z))) in numpy), which take the 99.9 % bar.  (Softplus' and Sigmoid'' cancel near zero, 1 - expf(-10 y) and 1 - 2 s: mlp_device.h evaluates expf
there by expf_near_zero, correctly rounded like the host's, or its last bit would show as 2 and 8 half steps.)  On the
other rows the class (finite, +inf, -inf, NaN) of every element is the oracle network's.  Two runs agree bit for bit, and inference returns the
training forward's bits on every row.

Covered, each asserted by Trainer.last_step_kernel: the unfused sequence k_mlp_fwd -> k_act_bwd_output -> k_mlp_bwd (widths 16, 32, 256; 64 and
128 under TCNN_AMD_FUSED_STEP=0), train<64,1,8,8>, train<128,1,8,16> and train_regw of k_train.hip (/act, and /relu for a ReLU
hidden layer), regs of k_train_regs.hip (ReLU and None: all it accepts), the layer-by-layer path of k_mlp_layers.hip (CutlassMLP 48 and 512
wide, Sine hidden layers included), Trainer.inference_half on each of them, tcnn.Network's inference and forward (64 and 48 wide), and the
second-order epilogues of k_mlp_layers.hip (act_d1, act_d2) through backward_backward_input.

train_regw takes two hidden layers only, so a hidden activation A reaches the output as A(A(x)): device and host libm differ in the last bit of
the first application and the second magnifies it, which no bar on single roundings describes.  It runs the exact hidden activations (both
applications are then the oracle's, bit for bit) and every output activation behind two None layers.

NOT reachable in this setting: r32, r32a, r32w and regs_fast (a grid input, and a loss instead of an external dL/dy), r32ob and train_ob (a
OneBlob input).  The fp32 networks (k_layer_gemm<float>, k_mlp_layers.hip) have a sweep of their own, over a wide float32 range and with a per-element yardstick of
another kind (candidate sets): tests/test_activation_sweep_f32.py.  Not covered: weight gradients, which are sums of wide-range terms here and are
held by test_weight_gradients_exact.py.
"""
import numpy as np
import pytest

import activation_sweep as sw
from grad_checks import layer_slices

gpu = pytest.mark.gpu

FUSED_ACTIVATIONS = [a for a in sw.ACTIVATIONS if a != "Sine"]  # FullyFusedMLP takes no Sine hidden layer
R0 = {"TCNN_AMD_MLP_REGS": "0", "TCNN_AMD_MLP_REGW": "0"}
FUSED_CASES = sw.cases(FUSED_ACTIVATIONS)
LAYER_CASES = sw.cases()
REGS_CASES = [("ReLU", "None"), ("None", "None")]
REGW_CASES = sw.cases([a for a in FUSED_ACTIVATIONS if a in sw.EXACT])


def _v(nb, nw, maxt):
    return {**R0, "TCNN_AMD_MLP_VARIANT": f"{nb},{nw},{maxt}"}


# (id, width, hidden layers, environment, kernel, cases)
PATHS = [
    ("unfused16", 16, 1, {}, "unfused", FUSED_CASES),
    ("unfused32", 32, 1, {}, "unfused", FUSED_CASES),
    ("unfused64", 64, 1, {"TCNN_AMD_FUSED_STEP": "0"}, "unfused", FUSED_CASES),
    ("unfused128", 128, 1, {"TCNN_AMD_FUSED_STEP": "0"}, "unfused", FUSED_CASES),
    ("unfused256", 256, 1, {}, "unfused", FUSED_CASES),
    ("train64", 64, 1, _v(1, 8, 8), "train<64,1,8,8>/act", FUSED_CASES),
    ("train128", 128, 1, _v(1, 8, 16), "train<128,1,8,16>/act", FUSED_CASES),
    ("regw", 64, 2, {"TCNN_AMD_MLP_REGS": "0"}, "train_regw/act", REGW_CASES),
    ("regs", 64, 1, {}, "regs", REGS_CASES),
    ("layers48", 48, 1, {}, "unfused", LAYER_CASES),
    ("layers512", 512, 1, {}, "unfused", LAYER_CASES),
]
RUNS = [(p, c) for p in PATHS for c in p[5]]
ALL_CASES = sorted({(p[2], c) for p, c in RUNS})  # (hidden layers, case)


def _kernel_name(path, case):
    """a ReLU hidden layer runs the /relu instance of k_train.hip's kernels, every other activation (chosen at run time) the /act one"""
    return path[4].replace("/act", "/relu") if case[0] == "ReLU" else path[4]


def _layerwise(path):
    return path[0].startswith("layers")


def _forward_is_exact(case):
    return sw.curved(case) in sw.EXACT


def _backward_is_exact(path, case):
    return not (sw.curved(case) == "Softplus" or (case[0] == "Sine" and _layerwise(path)))


def _backward_yardstick(oracle, path, case, got_out):
    """dL/dinput from the kernel's own forward output, element by element (with two hidden layers: through the oracle's first application,
    which an exact activation shares with the kernel)"""
    dy, a = sw.dy_bits(), sw.curved(case)
    if case[0] == "Sine" and _layerwise(path):
        return sw.sine_backward_from_preactivation(dy, sw.sweep_bits())
    g = sw.elementwise_backward(oracle, a, dy, got_out)
    if path[2] == 2 and case[0] != "None":
        g = sw.elementwise_backward(oracle, a, g, sw.elementwise_forward(oracle, a, sw.sweep_bits()))
    return g


# ---------------------------------------------------------------------------------------------------- CPU: the setting itself
def test_the_sweep_holds_every_finite_half_once():
    x = sw.sweep_bits()
    v = x.ravel()[:63488]
    assert np.array_equal(np.sort(v), np.sort(np.concatenate([np.arange(0x0000, 0x7C00), np.arange(0x8000, 0xFC00)]).astype(np.uint16)))
    assert not np.any(x.ravel()[63488:]) and np.all(np.diff(sw.ordered(v)) >= 0) and np.all(sw.classes(x) == sw.FINITE)
    assert np.array_equal(sw.sweep_x().astype(np.float16).view(np.uint16), x)  # the cast to float32 and back is exact


def test_dL_dy_stays_in_range():
    for n_out in (16, 5):
        dy = sw.dy_bits(n_out=n_out)
        assert np.array_equal(dy, sw.dy_bits(n_out=n_out))  # seeded
        mag = np.abs(dy.view(np.float16).astype(np.float64))
        assert np.all(mag[:, :n_out] >= 2.0 ** -10) and np.all(mag[:, :n_out] < 2.0 ** 4) and not np.any(dy[:, n_out:])
        assert np.any(dy[:, :n_out] & 0x8000) and np.any(~dy[:, :n_out] & 0x8000)
        exps = np.unique(np.floor(np.log2(mag[:, :n_out])))
        assert exps.min() == -10 and exps.max() == 3 and exps.size == 14


@pytest.mark.parametrize("hidden,case", ALL_CASES, ids=[f"{h}-{sw.case_id(c)}" for h, c in ALL_CASES])
def test_oracle_network_is_the_elementwise_oracle(oracle, hidden, case):
    """on the rows whose results are all finite the oracle network's output is orc_activation(x) and its dL/dinput is
    orc_activation_backward(dL/dy, output), element by element, up to the sign of zero (the matrix product drops it); and at most 21 % of the
    rows leave that comparison for Exponential and Softplus, none for the others: the cap that keeps the GPU tests from comparing nothing"""
    ref = sw.reference(oracle, hidden, case)
    a, x, dy = sw.curved(case), sw.sweep_bits(), sw.dy_bits()
    fw = sw.elementwise_forward(oracle, a, x)
    if hidden == 2 and case[0] != "None":
        fw = sw.elementwise_forward(oracle, a, fw)
    rows_f = sw.finite_rows(ref["out"])
    rows = sw.finite_rows(ref["out"], ref["dx"])
    for r in (rows_f, rows):
        assert 1.0 - float(np.mean(r)) <= sw.MAX_SHARE_OUTSIDE.get(a, 0.0), (a, int(r.sum()))
    if a in ("Exponential", "Softplus") and hidden == 1:
        assert int(rows_f.sum()) == {"Exponential": 3288, "Softplus": 3271}[a]
    assert np.array_equal(sw.ordered(ref["out"][rows_f]), sw.ordered(fw[rows_f]))
    bw = sw.elementwise_backward(oracle, a, dy, ref["out"])
    if hidden == 2 and case[0] != "None":
        bw = sw.elementwise_backward(oracle, a, bw, sw.elementwise_forward(oracle, a, x))
    assert np.array_equal(sw.ordered(ref["dx"][rows]), sw.ordered(bw[rows]))
    assert np.any(ref["dx"][rows] & 0x7FFF)


@pytest.mark.parametrize("width,hidden,case", [(64, 1, ("Exponential", "None")), (128, 1, ("None", "Softplus")), (48, 1, ("Sine", "None")), (512, 1, ("Squareplus", "None")),
                                               (64, 2, ("LeakyReLU", "None")), (64, 2, ("None", "Exponential")), (256, 1, ("Softplus", "None"))],
                         ids=lambda v: sw.case_id(v) if isinstance(v, tuple) else str(v))
def test_the_reference_does_not_depend_on_the_width(oracle, width, hidden, case):
    """the GPU tests share one oracle step per case, computed at width 16: at any width the oracle returns the same bits, NaN rows included"""
    wide, ref = sw.oracle_step(oracle, width, hidden, case), sw.reference(oracle, hidden, case)
    assert np.array_equal(wide["out"], ref["out"]) and np.array_equal(wide["dx"], ref["dx"])


def test_identity_weights_put_a_neuron_in_every_tile(oracle):
    for width, hidden in [(16, 1), (48, 1), (64, 2), (128, 1), (256, 1), (512, 1)]:
        net = oracle.Mlp({"otype": "CutlassMLP", "n_input_dims": 16, "n_output_dims": 16, "n_neurons": width, "n_hidden_layers": hidden})
        slices = layer_slices(net)
        w = sw.identity_weights(slices, width)
        assert w.size == net.n_params and int(np.count_nonzero(w)) == 16 * len(slices) and set(np.unique(w)) == {0.0, 1.0}
        neurons = [sw.neuron_of(c, width) for c in range(16)]
        assert len(set(neurons)) == 16 and max(neurons) < width
        if width <= 256:
            assert {n // 16 for n in neurons} == set(range(width // 16))
        prod = np.eye(16)
        for off, rows, cols in slices:
            prod = w[off:off + rows * cols].reshape(rows, cols) @ prod
        assert np.array_equal(prod, np.eye(16))


def test_sine_backward_yardstick():
    """hmul(dL/dy, half(cosf(z))) against float64: the factor is cos(z) rounded once to half (within half a step of it, or one float32 ulp of
    cosf beyond), the product one more rounding"""
    z, dy = sw.sweep_bits(), sw.dy_bits()
    got = sw.sine_backward_from_preactivation(dy, z).view(np.float16).astype(np.float64)
    c64 = np.cos(z.view(np.float16).astype(np.float64))
    g64 = dy.view(np.float16).astype(np.float64)
    assert np.all(np.isfinite(got))
    spacing = lambda v: np.maximum(np.spacing(np.abs(v).astype(np.float16)).astype(np.float64), 2.0 ** -24)
    bound = np.abs(g64) * (0.5 * spacing(c64) + 2.0 ** -23) + 0.5 * spacing(g64 * c64) + 2.0 ** -24
    assert np.all(np.abs(got - g64 * c64) <= bound)
    assert np.any(got != g64)  # not the oracle's "gradient itself"


# ---------------------------------------------------------------------------------------------------- GPU: one step per path and case
def _trainer(tcnn, oracle, width, hidden, case):
    from test_gpu_parity import _t

    cfg = sw.trainer_config(width, hidden, case)
    net = oracle.Mlp({**cfg["network"], "n_input_dims": 16, "n_output_dims": 16})
    tr = tcnn.Trainer(16, 16, cfg, seed=1337)
    assert tr.n_params == net.n_params
    tr.set_params(_t(sw.identity_weights(layer_slices(net), width).astype(np.float16)))
    return tr


def _gpu_step(tcnn, oracle, monkeypatch, path, case):
    """two training steps of one trainer and an inference call: [(kernel, output bits, dL/dinput bits)] * 2, inference bits"""
    import torch

    from test_gpu_parity import _bits, _t

    _, width, hidden, env, _, _ = path
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        tr = _trainer(tcnn, oracle, width, hidden, case)
        x, dy = _t(sw.sweep_x()), _t(sw.dy_bits().view(np.float16))
        runs = []
        for _ in range(2):
            dx = torch.full((sw.N_ROWS, sw.N_COLS), 7.0, dtype=torch.float32, device="cuda")
            ctx = tr.training_step(x, None, run_optimizer=False, dL_dinput=dx, external_dL_dy=dy)
            runs.append((tr.last_step_kernel(), _bits(ctx.output()).copy(), sw.float_to_half_bits(dx.cpu().numpy())))
        inference = _bits(tr.inference_half(x)).copy()
    return runs, inference


@gpu
@pytest.mark.parametrize("path,case", RUNS, ids=[f"{p[0]}-{sw.case_id(c)}" for p, c in RUNS])
def test_activation_sweep_in_a_training_step(tcnn, oracle, monkeypatch, path, case):
    ref = sw.reference(oracle, path[2], case)
    runs, inference = _gpu_step(tcnn, oracle, monkeypatch, path, case)
    name, out, dx = runs[0]
    assert name == _kernel_name(path, case)
    what = f"sweep {path[0]} {sw.case_id(case)}"
    sw.compare(out, ref["out"], sw.finite_rows(ref["out"]), ref["out"], _forward_is_exact(case), what + " forward")
    name2, out2, dx2 = runs[1]
    assert name2 == name and np.array_equal(out, out2) and np.array_equal(dx, dx2), f"{what}: two runs differ"
    assert np.array_equal(inference, out), f"{what}: inference_half is not the training forward"
    rows = sw.finite_rows(ref["out"], ref["dx"])
    sw.compare(dx, _backward_yardstick(oracle, path, case, out), rows, ref["dx"], _backward_is_exact(path, case), what + " backward")


NETWORK_RUNS = [(w, c) for w, cs in ((64, FUSED_CASES), (48, LAYER_CASES)) for c in cs]


@gpu
@pytest.mark.parametrize("width,case", NETWORK_RUNS, ids=[f"{w}-{sw.case_id(c)}" for w, c in NETWORK_RUNS])
def test_activation_sweep_in_network_inference(tcnn, oracle, width, case):
    """tcnn.Network without gradients (the inference kernels of k_mlp.hip at 64, of k_mlp_layers.hip at 48) returns what its training forward
    returns, bit for bit on all rows, and that meets the forward bar against the oracle network"""
    import torch

    from test_gpu_parity import _bits, _t

    ref = sw.reference(oracle, 1, case)
    cfg = sw.network_config(width, 1, case)
    net = tcnn.Network(16, 16, cfg)
    native = net.native_tcnn_module
    slices = layer_slices(oracle.Mlp({**cfg, "n_input_dims": 16, "n_output_dims": 16}))
    params = _t(sw.identity_weights(slices, width).astype(np.float16))
    x = _t(sw.sweep_x())
    no_ctx, inferred = native.fwd(x, params)
    ctx, trained = native.fwd(x.clone().requires_grad_(True), params)
    assert no_ctx is None and ctx is not None
    torch.cuda.synchronize()
    what = f"sweep network{width} {sw.case_id(case)}"
    sw.compare(_bits(trained), ref["out"], sw.finite_rows(ref["out"]), ref["out"], _forward_is_exact(case), what + " forward")
    assert np.array_equal(_bits(inferred), _bits(trained)), f"{what}: inference is not the training forward"


# ---------------------------------------------------------------------------------------------------- GPU: second order
SECOND_ORDER_ACTIVATIONS = ["Exponential", "Sine", "Sigmoid", "Squareplus", "Softplus", "Tanh"]


def _second_order_tensors(oracle, act, width=48):
    """(network config, half weights, torch Ws / x / dL/dy / v as halves) of the second-order case"""
    import torch

    cfg = sw.network_config(width, 1, (act, "None"))
    slices = layer_slices(oracle.Mlp({**cfg, "n_input_dims": 16, "n_output_dims": 16}))
    w = sw.identity_weights(slices, width).astype(np.float16)
    Ws = [torch.from_numpy(w[o:o + r * c].reshape(r, c).copy()) for o, r, c in slices]
    x, dy, v = (torch.from_numpy(b.view(np.float16).copy()) for b in (sw.sweep_bits(), sw.dy_bits(), sw.dy_bits(seed=11)))
    return cfg, w, Ws, x, dy, v


@pytest.mark.parametrize("act", SECOND_ORDER_ACTIVATIONS)
def test_second_order_restatement_is_the_recipe(oracle, act):
    """activation_sweep.second_order_restatement against test_network_second_order._restate on the same tensors: the same classes everywhere,
    and on the rows finite in all of them as close to the float64 recipe as the torch restatement in half is, up to the factor 2 that
    test_network_second_order allows two realisations of the same roundings; no more than 21 % of the rows leave the comparison for
    Exponential, none for the others"""
    import torch

    from test_network_second_order import _restate

    _, _, Ws, x, dy, v = _second_order_tensors(oracle, act)
    rh = _restate(Ws, [act, "None"], x, dy, v, half=True)
    r64 = _restate(Ws, [act, "None"], x, dy, v, half=False)
    ours = sw.second_order_restatement(act, sw.sweep_bits(), sw.dy_bits(), sw.dy_bits(seed=11))
    for name, mine, h, ref in (("dL_ddLdoutput", ours[0], rh[0], r64[0]), ("dL_dinput", ours[1], rh[2], r64[2])):
        h_bits = sw.float_to_half_bits(h.numpy())
        assert np.array_equal(sw.classes(mine), sw.classes(h_bits)), name
        rows = sw.finite_rows(mine) & np.all(np.isfinite(ref.numpy()), axis=1)
        assert 1.0 - float(np.mean(rows)) <= sw.MAX_SHARE_OUTSIDE.get(act, 0.0), (name, int(rows.sum()))
        ref_rows = ref.numpy()[rows]
        e_mine = float(np.linalg.norm(mine[rows].view(np.float16).astype(np.float64) - ref_rows))
        e_h = float(np.linalg.norm(h.numpy()[rows].astype(np.float64) - ref_rows))
        assert e_mine <= 2 * e_h and np.any(mine[rows] & 0x7FFF), (name, e_mine, e_h)


@gpu
@pytest.mark.parametrize("act", SECOND_ORDER_ACTIVATIONS)
def test_activation_sweep_second_order(tcnn, oracle, act):
    """backward_backward_input on a CutlassMLP 48 wide (the only kernels with act_d1 / act_d2): dL/d(dL/doutput) = v a'(x) and the second-order
    dL/dinput = v dL/dy a''(x) against the recipe of test_network_second_order._restate(half=True) on the same tensors, restated op by op in
    float32 numpy (activation_sweep.second_order_restatement) -- at least 99.9 % of the halves identical and the others adjacent on the rows
    that are finite in the restatement, the same classes elsewhere; two runs agree."""
    import torch

    from test_gpu_parity import _t

    cfg, w, _, x, dy, v = _second_order_tensors(oracle, act)
    want_ddy, want_dx = sw.second_order_restatement(act, sw.sweep_bits(), sw.dy_bits(), sw.dy_bits(seed=11))
    net = tcnn.Network(16, 16, cfg)
    native = net.native_tcnn_module
    xt, pt, dyt = x.float().cuda().requires_grad_(True), _t(w), dy.cuda().requires_grad_(True)
    ctx, _ = native.fwd(xt, pt)
    results = [native.bwd_bwd_input(ctx, xt, pt, v.float().cuda(), dyt) for _ in range(2)]
    ddy, dparams, dx = results[0]
    assert dparams is None
    assert torch.equal(results[1][0].view(torch.int16), ddy.view(torch.int16)) and torch.equal(results[1][2].view(torch.int32), dx.view(torch.int32))
    for name, got, want in (("dL_ddLdoutput", ddy, want_ddy), ("dL_dinput", dx, want_dx)):
        got_bits = sw.float_to_half_bits(got.float().cpu().numpy())
        sw.compare(got_bits, want, sw.finite_rows(want), want, False, f"sweep second_order48 {act.lower()}-none {name}")
