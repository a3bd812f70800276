"""Every fused training kernel and every option of Trainer::training_step against the CPU oracle.

Trainer::training_step picks one of about twenty MLP training kernels (k_train.hip pick_config / dispatch_train, k_train_regs.hip,
k_train_r32*.hip) or the unfused sequence k_mlp_fwd -> k_loss -> k_mlp_bwd -> k_wgrad*.  Each case here first asserts which kernel ran
(Trainer.last_step_kernel), then compares the step with oracle.Trainer.training_step with the bars of test_training_step_matches_oracle,
and with the same step under TCNN_AMD_FUSED_STEP=0 with the bars of test_r32_kernels_other_output_counts_losses_and_batches.
Beyond the kernel forms: data_pdf, dL_dinput (AoS and SoA), the grid's first-order dL/dx through tcnn.Encoding, SoA input in a training
step and use_inference_params with EMA weights.
"""
import numpy as np
import pytest

from conftest import CONFIG_C2, CONFIG_C3A, CONFIG_C3B, CONFIG_C5_SMALL
from grad_checks import assert_structural_zeros, assert_weight_grads_close, layer_slices, subnormal_share
from grid_reference import edge_x
from test_gpu_parity import _bits, _exact_external_dy, _f32, _linear_net_params, _t, elem_close, rel_err
from test_losses import _assert_fused_loss_close

pytestmark = pytest.mark.gpu

ADAM = CONFIG_C3B["optimizer"]
GRID16 = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 16, "per_level_scale": 1.5}  # 2-D -> 16 inputs
GRID32 = {**GRID16, "n_levels": 16}  # 2-D -> 32 inputs


def _cfg(enc, width, hidden, act="ReLU", out_act="None", loss="L2"):
    otype = "CutlassMLP" if width > 128 else "FullyFusedMLP"  # wider than FullyFusedMLP allows
    return {"loss": {"otype": loss}, "optimizer": ADAM, "encoding": enc,
            "network": {"otype": otype, "activation": act, "output_activation": out_act, "n_neurons": width, "n_hidden_layers": hidden}}


def _targets(out_act, n, n_out, seed):
    """L2 targets inside the output activation's range"""
    t = np.random.RandomState(seed).uniform(0.05, 0.95, (n, n_out)).astype(np.float32)
    if out_act == "Tanh":
        t = t * 1.6 - 0.8
    elif out_act == "Exponential":
        t = t + 0.5
    return np.ascontiguousarray(t)


def _run(tcnn, monkeypatch, n_in, n_out, cfg, env, x, t, layout=None, params_half=None, **kw):
    """one training_step of a fresh trainer under `env`: (kernel name, output, L, dL_doutput, gradients, loss); params_half (uint16 bits of
    every parameter) replaces the initial parameters"""
    from tinycudann.native import LAYOUT_AOS, LAYOUT_SOA

    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        tr = tcnn.Trainer(n_in, n_out, cfg, seed=1337)
        if params_half is not None:
            tr.set_params(_t(params_half.view(np.float16)))
        xin = _t(x) if layout != "soa" else _t(np.ascontiguousarray(x.T))
        ctx = tr.training_step(xin, None if t is None else _t(t), run_optimizer=False, input_layout=LAYOUT_SOA if layout == "soa" else LAYOUT_AOS, **kw)
        res = {"kernel": tr.last_step_kernel(), "out": _bits(ctx.output()), "L": ctx.L().cpu().numpy(), "dy": _bits(ctx.dL_doutput()),
               "g": _bits(tr.param_gradients()), "loss": tr.loss(ctx)}
    return res


PER_LAYER_BAR_NOT_AT_INIT = {"v64_2_4_16_act"}


def _check_against_oracle(ref, want, grads32, got, n, n_out, what="", untouched=None, per_layer=True):
    """`untouched`: boolean mask over the encoding's parameters that no sample reaches; without it, the entries whose fp32 gradient is zero in
    the oracle stand for them (true while no touched entry's gradient rounds to zero)"""
    out, w_out = _f32(got["out"]).reshape(n, -1), _f32(want["output"])
    assert elem_close(out[:, :n_out], w_out[:, :n_out]) <= 1.0
    assert abs(got["loss"] - want["loss"]) <= 3e-2 * abs(want["loss"])
    assert rel_err(got["L"], want["L"]) < 3e-2
    dy, w_dy = _f32(got["dy"]).reshape(n, -1), _f32(want["dL_doutput"]).reshape(n, -1)
    assert elem_close(dy[:, :n_out], w_dy[:, :n_out], rtol=3e-2) <= 1.0
    assert np.all(got["L"][:, n_out:] == 0) and np.all(dy[:, n_out:] == 0) and np.any(dy[:, :n_out] != 0)
    g = _f32(got["g"])
    n_net = ref.model.network.n_params
    assert rel_err(g[:n_net], grads32[:n_net]) < 3e-2
    # the same 3e-2 with the maximum taken per layer and every element bounded by its own size (grad_checks.weight_grad_ratios); whole
    # rows / columns the oracle leaves zero -- padded outputs, zero-padded inputs -- are zero bit for bit
    what = f"{what} [{got.get('kernel', '?')}]"
    slices = layer_slices(ref.model.network)
    if per_layer:
        assert_weight_grads_close(g[:n_net], grads32[:n_net], slices, 3e-2, True, what)
    assert_structural_zeros(got["g"][:n_net], grads32[:n_net], slices, what)
    if ref.model.encoding.n_params > 0:
        ge, we = g[n_net:], grads32[n_net:]
        assert float(np.linalg.norm(ge - we)) <= 5e-2 * float(np.linalg.norm(we)) and np.all(ge[we == 0 if untouched is None else untouched] == 0)


def _check_against_unfused(got, unf):
    assert unf["kernel"] == "unfused"
    out, out0 = _f32(got["out"]), _f32(unf["out"])
    assert float(np.max(np.abs(out - out0))) <= 4e-3 * max(1.0, float(np.max(np.abs(out0))))
    assert abs(got["loss"] - unf["loss"]) <= 1e-4 * abs(unf["loss"])
    g, g0 = _f32(got["g"]), _f32(unf["g"])
    assert float(np.linalg.norm(g - g0)) <= 5e-3 * float(np.linalg.norm(g0))


# ---------------------------------------------------------------------------------------------------- c.1 the kernel forms
R0 = {"TCNN_AMD_MLP_REGS": "0", "TCNN_AMD_MLP_REGW": "0"}


def _v(nb, nw, maxt):
    return {**R0, "TCNN_AMD_MLP_VARIANT": f"{nb},{nw},{maxt}"}


# (id, encoding, n_in, width, n_hidden, activation, output activation, n_out, n, env, expected kernel).  The forced variants' shapes follow
# pick_config: a variant is taken when its activation images fit in LDS and the network's tiles fit `maxt` per wave.
FORM_CASES = [
    ("v64_1_8_8_relu", GRID16, 2, 64, 4, "ReLU", "None", 3, 256 * 9, _v(1, 8, 8), "train<64,1,8,8>/relu"),
    ("v64_1_8_8_act", GRID16, 2, 64, 1, "Tanh", "Sigmoid", 24, 256 * 5, _v(1, 8, 8), "train<64,1,8,8>/act"),
    ("v64_2_4_8_relu", GRID16, 2, 64, 2, "ReLU", "None", 17, 256 * 7, _v(2, 4, 8), "train<64,2,4,8>/relu"),
    ("v64_2_4_8_act", GRID16, 2, 64, 2, "Sigmoid", "None", 5, 256 * 9, _v(2, 4, 8), "train<64,2,4,8>/act"),
    ("v64_2_4_16_relu", GRID16, 2, 64, 3, "ReLU", "None", 32, 256 * 5, _v(2, 4, 16), "train<64,2,4,16>/relu"),
    ("v64_2_4_16_act", GRID16, 2, 64, 4, "LeakyReLU", "ReLU", 8, 256 * 11, _v(2, 4, 16), "train<64,2,4,16>/act"),
    # (with the grid at its initial values the negative side of a fourth LeakyReLU layer holds fp16 subnormals of 1-4 bits, and the order of
    # the fp32 sums alone moves the first layers' gradients by 0.6 of the per-layer bar -- tests/test_grad_checks.py asserts it: the 4-layer case
    # keeps every other bar there, PER_LAYER_BAR_NOT_AT_INIT, and meets the per-layer one with a U(-1, 1) grid; 3 layers meet it at init too)
    ("v64_2_4_16_act_3_hidden", GRID16, 2, 64, 3, "LeakyReLU", "ReLU", 8, 256 * 11, _v(2, 4, 16), "train<64,2,4,16>/act"),
    ("v64_1_4_16_relu", GRID16, 2, 64, 1, "ReLU", "None", 1, 256 * 13, _v(1, 4, 16), "train<64,1,4,16>/relu"),
    ("v64_1_4_16_act", GRID16, 2, 64, 4, "Squareplus", "Tanh", 24, 256 * 5, _v(1, 4, 16), "train<64,1,4,16>/act"),
    ("v64_1_4_32_relu", GRID16, 2, 64, 8, "ReLU", "None", 3, 256 * 9, _v(1, 4, 32), "train<64,1,4,32>/relu"),
    # (3 hidden layers: behind 6 Softplus layers dL/d(encoding) reaches fp16 subnormals, where "zero in the oracle" stops meaning "untouched")
    ("v64_1_4_32_act", GRID16, 2, 64, 3, "Softplus", "Exponential", 32, 256 * 7, _v(1, 4, 32), "train<64,1,4,32>/act"),
    ("v128_1_8_16_relu", GRID16, 2, 128, 2, "ReLU", "None", 3, 256 * 9, _v(1, 8, 16), "train<128,1,8,16>/relu"),
    ("v128_1_8_16_act", GRID16, 2, 128, 1, "Exponential", "None", 17, 256 * 5, _v(1, 8, 16), "train<128,1,8,16>/act"),
    ("v128_1_8_32_relu", GRID16, 2, 128, 1, "ReLU", "None", 24, 256 * 7, _v(1, 8, 32), "train<128,1,8,32>/relu"),
    ("v128_1_8_32_act", GRID16, 2, 128, 2, "None", "None", 8, 256 * 5, _v(1, 8, 32), "train<128,1,8,32>/act"),
    ("v128_1_4_32_relu", GRID16, 2, 128, 2, "ReLU", "None", 32, 256 * 5, _v(1, 4, 32), "train<128,1,4,32>/relu"),
    ("v128_1_4_32_act", GRID16, 2, 128, 2, "Tanh", "Sigmoid", 5, 256 * 9, _v(1, 4, 32), "train<128,1,4,32>/act"),
    # all weight fragments in registers: 64 x 2 with <= 32 inputs and 16 padded outputs; REGW=0 sends the same network to the table
    ("regw_relu", GRID32, 2, 64, 2, "ReLU", "None", 16, 256 * 5, {"TCNN_AMD_MLP_REGS": "0"}, "train_regw/relu"),
    ("regw_act", GRID32, 2, 64, 2, "Tanh", "None", 5, 256 * 7, {}, "train_regw/act"),
    ("regw_off", GRID32, 2, 64, 2, "Tanh", "None", 5, 256 * 7, {"TCNN_AMD_MLP_REGW": "0"}, "train<64,1,8,8>/act"),
    # OneBlob evaluated inside k_mlp_train (32 bins: not k_mlp_train_r32ob's shape)
    ("oneblob_relu", {"otype": "OneBlob", "n_bins": 32}, 2, 64, 2, "ReLU", "None", 3, 256 * 9, {}, "train_ob/relu"),
    ("oneblob_act", {"otype": "OneBlob", "n_bins": 32}, 2, 64, 2, "Tanh", "None", 3, 256 * 9, {}, "train_ob/act"),
    # register-resident kernels: FAST (compile-time formats) and the general form (5..16 outputs, activation None, FAST=0)
    ("regs_fast", GRID32, 2, 64, 2, "ReLU", "None", 3, 256 * 9, {"TCNN_AMD_MLP_R32": "0"}, "regs_fast"),
    ("regs_5", GRID32, 2, 64, 2, "ReLU", "None", 5, 256 * 9, {"TCNN_AMD_MLP_R32": "0"}, "regs"),
    ("regs_8_none", GRID32, 2, 64, 1, "None", "None", 8, 256 * 5, {}, "regs"),
    ("regs_16", GRID16, 2, 64, 2, "ReLU", "None", 16, 256 * 7, {}, "regs"),
    ("regs_fast_off", GRID32, 2, 64, 2, "ReLU", "None", 3, 256 * 5, {"TCNN_AMD_MLP_R32": "0", "TCNN_AMD_MLP_FAST": "0"}, "regs"),
    # the 32x32x16 kernels, for the record of forms
    ("r32a", CONFIG_C3B["encoding"], 2, 64, 2, "ReLU", "None", 3, 256 * 9, {}, "r32a"),
    ("r32", CONFIG_C3B["encoding"], 2, 64, 2, "ReLU", "None", 3, 256 * 9, {"TCNN_AMD_MLP_R32A": "0"}, "r32"),
    ("r32ob", CONFIG_C2["encoding"], 2, 64, 2, "ReLU", "None", 3, 256 * 9, {}, "r32ob"),
    ("r32w", CONFIG_C5_SMALL["encoding"], 3, 128, 2, "ReLU", "None", 3, 256 * 9, {}, "r32w"),
    # no fused kernel: widths 16, 32, 256 and more than 32 outputs
    ("unfused_w16", GRID16, 2, 16, 2, "Tanh", "None", 3, 256 * 5, {}, "unfused"),
    ("unfused_w32", GRID16, 2, 32, 1, "ReLU", "Sigmoid", 5, 256 * 5, {}, "unfused"),
    ("unfused_w256", GRID16, 2, 256, 1, "Squareplus", "None", 3, 256 * 5, {}, "unfused"),
    ("unfused_out40", GRID16, 2, 64, 2, "ReLU", "None", 40, 256 * 5, {}, "unfused"),
]


@pytest.mark.parametrize("case", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_training_kernel_forms_match_oracle(tcnn, oracle, monkeypatch, case):
    _, enc, n_in, width, hidden, act, out_act, n_out, n, env, kernel = case
    cfg = _cfg(enc, width, hidden, act, out_act)
    x = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in)
    t = _targets(out_act, n, n_out, 17)
    ref = oracle.Trainer(n_in, n_out, cfg, seed=1337)
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    want = ref.training_step(x, t, run_optimizer=False, grads_f32=grads32)
    got = _run(tcnn, monkeypatch, n_in, n_out, cfg, env, x, t)
    assert got["kernel"] == kernel
    per_layer = case[0] not in PER_LAYER_BAR_NOT_AT_INIT
    _check_against_oracle(ref, want, grads32, got, n, n_out, case[0], per_layer=per_layer)
    if kernel != "unfused":
        unf = _run(tcnn, monkeypatch, n_in, n_out, cfg, {**env, "TCNN_AMD_FUSED_STEP": "0"}, x, t)
        _check_against_unfused(got, unf)
        _check_against_oracle(ref, want, grads32, unf, n, n_out, case[0] + " with TCNN_AMD_FUSED_STEP=0", per_layer=per_layer)


# ---------------------------------------------------------------------------------------------------- c.2 data_pdf
def _pdf(n, n_out, seed):
    pdf = np.random.RandomState(seed).uniform(0.25, 4.0, (n, n_out)).astype(np.float32)
    pdf[np.log2(pdf) == np.round(np.log2(pdf))] *= np.float32(1.1)  # no powers of two: a dropped or inverted pdf cannot hide
    return np.ascontiguousarray(pdf)


PDF_CASES = [  # (id, config, n_in, n_out, n, env, kernel)
    ("regs", CONFIG_C3A, 2, 3, 1 << 18, {}, "regs"),  # r32 and regs_fast take no pdf
    ("train_3", CONFIG_C3B, 2, 3, 256 * 9, {"TCNN_AMD_MLP_REGS": "0"}, "train_regw/relu"),
    ("train_24", CONFIG_C3B, 2, 24, 256 * 9, {"TCNN_AMD_MLP_REGS": "0"}, "train<64,1,8,8>/relu"),
    ("oneblob", CONFIG_C2, 2, 3, 256 * 9, {}, "train_ob/relu"),  # r32ob takes no pdf
    ("unfused", CONFIG_C3B, 2, 3, 256 * 9, {"TCNN_AMD_FUSED_STEP": "0"}, "unfused"),
]


@pytest.mark.parametrize("loss", ["L2", "RelativeL2"])
@pytest.mark.parametrize("case", PDF_CASES, ids=[c[0] for c in PDF_CASES])
def test_data_pdf_in_each_training_kernel(tcnn, oracle, monkeypatch, case, loss):
    """data_pdf divides the loss and its gradient (loss_l2_fused's pdf branch, k_mlp_train_regs' and k_mlp_train's pdf loads, k_loss):
    the loss on the kernel's own predictions against oracle.loss_evaluate(data_pdf=...), then the whole step against the oracle."""
    _, base, n_in, n_out, n, env, kernel = case
    cfg = {**base, "loss": {"otype": loss}}
    x, t = oracle.synthetic_batch(n, n_in, n_out, seed=42)
    pdf = _pdf(n, n_out, 3)
    got = _run(tcnn, monkeypatch, n_in, n_out, cfg, env, x, t, data_pdf=_t(pdf))
    assert got["kernel"] == kernel
    want_v, want_g = oracle.loss_evaluate(loss, got["out"].reshape(n, -1), t, loss_scale=128.0, data_pdf=pdf)
    if kernel == "unfused":
        assert np.array_equal(got["L"].view(np.uint32), want_v.view(np.uint32)) and np.array_equal(got["dy"].reshape(n, -1), want_g)
    else:
        # loss_l2_fused divides by the pdf once more after its one reciprocal (dr / pdf): one rounding beyond the pdf-free bar of 4 ulp
        _assert_fused_loss_close(got["L"], want_v, got["dy"].reshape(n, -1), want_g, max_ulp=5)
    if n > 8192:
        return
    ref = oracle.Trainer(n_in, n_out, cfg, seed=1337)
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    want = ref.training_step(x, t, run_optimizer=False, grads_f32=grads32, data_pdf=pdf)
    _check_against_oracle(ref, want, grads32, got, n, n_out, f"pdf_{case[0]}/{loss}")


# ---------------------------------------------------------------------------------------------------- c.2b the same kernels, gradients in fp16's normal range
def o1_grid_params(oracle, ref):
    """the oracle trainer's parameters with the encoding's drawn from U(-1, 1) (as the encoding tests do) instead of the initial U(+-1e-4)"""
    n_net = ref.model.network.n_params
    p = ref.params.copy()
    p[n_net:] = oracle.half_bits(oracle.Pcg32(3).uniform_strided(ref.model.encoding.n_params, -1.0, 1.0))
    return p


MAX_SUBNORMAL_SHARE = 0.15  # a cap on the oracle's own half gradients (measured: <= 10 %)

# (id, config, n_in, n_out, n, env, kernel, output activation of the targets, pdf seed): every kernel form and every pdf case (a OneBlob
# encoding has no parameters to set: its cases run as above, their gradients are normal numbers already)
NORMAL_RANGE_CASES = [(c[0], _cfg(c[1], c[3], c[4], c[5], c[6]), c[2], c[7], c[8], c[9], c[10], c[6], None) for c in FORM_CASES] + \
                     [(f"pdf_{c[0]}_{loss}", {**c[1], "loss": {"otype": loss}}, c[2], c[3], c[4], c[5], c[6], None, 3) for c in PDF_CASES for loss in ("L2", "RelativeL2")]


def untouched_grid_entries(oracle, ref, x):
    """mask over the encoding's parameters: True where no sample of x lands with a non-zero interpolation weight (the gradient of an all-ones
    dL/dy is zero there).  With O(1) grid entries some touched entries' gradients are fp16 subnormals that round to zero on one side and to
    2^-24 on the other: "zero in the oracle" no longer means "untouched"."""
    enc = ref.model.encoding
    if enc.n_params == 0:
        return np.zeros(0, dtype=bool)
    _, ctx = enc.forward(x, np.ascontiguousarray(ref.params[ref.model.network.n_params:]))
    ones = oracle.half_bits(np.ones((x.shape[0], enc.padded_output_width), dtype=np.float32))
    touched = np.zeros(enc.n_params, dtype=np.float32)
    enc.backward(x, ctx, ones, grad_f32=touched)
    return touched == 0


def normal_range_inputs(oracle, case):
    """(x, targets, data_pdf) of a NORMAL_RANGE_CASES entry: those of the first regime's test of the same case"""
    _, cfg, n_in, n_out, n, _, _, out_act, pdf_seed = case
    if pdf_seed is None:
        return oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in), _targets(out_act, n, n_out, 17), None
    x, t = oracle.synthetic_batch(n, n_in, n_out, seed=42)
    return x, t, _pdf(n, n_out, pdf_seed)


@pytest.mark.parametrize("case", NORMAL_RANGE_CASES, ids=[c[0] for c in NORMAL_RANGE_CASES])
def test_training_kernels_match_oracle_with_gradients_in_the_normal_range(tcnn, oracle, monkeypatch, case):
    """With the L2 loss and the grid at its initial U(+-1e-4) values -- the setting of the tests above -- 90-100 % of the half gradients of
    every layer but the last are fp16 subnormals: the kernels' half stores are exercised where a half holds 1-9 significant bits.  Here the
    same kernels (asserted first) run with the grid's entries drawn from U(-1, 1): at most 15 % of any layer's gradients are subnormal (asserted
    on the oracle's values), and every bar of _check_against_oracle holds -- the per-layer, per-element one on gradients that are normal
    numbers."""
    name, cfg, n_in, n_out, n, env, kernel, _, _ = case
    x, t, pdf = normal_range_inputs(oracle, case)
    ref = oracle.Trainer(n_in, n_out, cfg, seed=1337)
    ref.params = o1_grid_params(oracle, ref)
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    want = ref.training_step(x, t, run_optimizer=False, grads_f32=grads32, data_pdf=pdf)
    share = subnormal_share(ref.grads[:ref.model.network.n_params], layer_slices(ref.model.network))
    assert max(share) <= MAX_SUBNORMAL_SHARE, share
    kw = {} if pdf is None else {"data_pdf": _t(pdf)}
    untouched = untouched_grid_entries(oracle, ref, x)
    got = _run(tcnn, monkeypatch, n_in, n_out, cfg, env, x, t, params_half=ref.params, **kw)
    assert got["kernel"] == kernel
    _check_against_oracle(ref, want, grads32, got, n, n_out, name + " (grid U(-1, 1))", untouched)
    if kernel != "unfused":
        unf = _run(tcnn, monkeypatch, n_in, n_out, cfg, {**env, "TCNN_AMD_FUSED_STEP": "0"}, x, t, params_half=ref.params, **kw)
        _check_against_unfused(got, unf)
        _check_against_oracle(ref, want, grads32, unf, n, n_out, name + " (grid U(-1, 1)) with TCNN_AMD_FUSED_STEP=0", untouched)


@pytest.mark.parametrize("name", ["RelativeL2Luminance", "L1", "RelativeL1", "Mape", "Smape", "CrossEntropy", "Variance"])
def test_data_pdf_in_k_loss(tcnn, oracle, monkeypatch, name):
    """the seven losses k_loss evaluates, with a per-element pdf: bit for bit against the oracle on the step's own predictions"""
    cfg = {**CONFIG_C3B, "loss": {"otype": name}}
    if name in ("CrossEntropy", "Variance"):
        cfg["network"] = {**CONFIG_C3B["network"], "output_activation": "Exponential"}
    n = 1024
    x, t = oracle.synthetic_batch(n, 2, 3, seed=42)
    t = np.ascontiguousarray(t * 0.9 + 0.05)
    pdf = _pdf(n, 3, 4)
    got = _run(tcnn, monkeypatch, 2, 3, cfg, {}, x, t, data_pdf=_t(pdf))
    assert got["kernel"] == "unfused"
    want_v, want_g = oracle.loss_evaluate(name, got["out"].reshape(n, -1), t, loss_scale=128.0, data_pdf=pdf)
    if name == "CrossEntropy":  # logf: device vs libm
        assert np.allclose(got["L"], want_v, rtol=1e-5, atol=1e-10)
    else:
        assert np.array_equal(got["L"].view(np.uint32), want_v.view(np.uint32))
    assert np.array_equal(got["dy"].reshape(n, -1), want_g)


# ---------------------------------------------------------------------------------------------------- c.3 dL_dinput
DX_MODELS = [  # (id, encoding, n_in)
    ("identity3", {"otype": "Identity"}, 3),
    ("identity32", {"otype": "Identity"}, 32),
    ("oneblob", {"otype": "OneBlob", "n_bins": 32}, 2),
    ("hash2d", GRID16, 2),
    ("hash3d", {**GRID16, "log2_hashmap_size": 14}, 3),
    ("dense", {"otype": "DenseGrid", "n_levels": 4, "n_features_per_level": 2, "base_resolution": 8, "per_level_scale": 2.0}, 2),
    ("smoothstep", {**GRID16, "interpolation": "Smoothstep"}, 2),
    ("composite", {"otype": "Composite", "nested": [{**GRID16, "n_dims_to_encode": 3, "log2_hashmap_size": 14}, {"otype": "SphericalHarmonics", "n_dims_to_encode": 3, "degree": 4}]}, 6),
]


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("model", DX_MODELS, ids=[m[0] for m in DX_MODELS])
def test_dL_dinput_is_bit_identical(tcnn, oracle, monkeypatch, model, fused, layout):
    """training_step(dL_dinput=...) in the exact setting of _linear_net_params / _exact_external_dy (every sum of the network's backward
    pass exact): dL/dinput -- in loss-scaled units, AoS [n][n_in] or SoA [n_in][n] like the input -- has the oracle's bits."""
    import torch

    _, enc, n_in = model
    cfg = _cfg(enc, 64, 2, act="None")
    n = 256 * 5
    ref = oracle.Trainer(n_in, 3, cfg, seed=1337)
    params_h, rs = _linear_net_params(oracle, ref.model, 5)
    ref.params = params_h.copy()
    x = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in)
    dy = oracle.half_bits(_exact_external_dy(rs, n, ref.model.padded_output_width))
    want = ref.training_step(x, None, run_optimizer=False, want_dL_dx=True, external_dL_dy=dy)
    from tinycudann.native import LAYOUT_AOS, LAYOUT_SOA

    with monkeypatch.context() as m:
        if not fused:
            m.setenv("TCNN_AMD_FUSED_STEP", "0")
        tr = tcnn.Trainer(n_in, 3, cfg, seed=1337)
        tr.set_params(_t(params_h.view(np.float16)))
        soa = layout == "soa"
        dx = torch.zeros((n_in, n) if soa else (n, n_in), dtype=torch.float32, device="cuda")
        tr.training_step(_t(np.ascontiguousarray(x.T)) if soa else _t(x), None, run_optimizer=False, dL_dinput=dx, external_dL_dy=_t(dy.view(np.float16)),
                         input_layout=LAYOUT_SOA if soa else LAYOUT_AOS)
        assert (tr.last_step_kernel() == "unfused") == (not fused)
        got = dx.cpu().numpy()
    got = got.T if soa else got
    assert np.any(want["dL_dinput"] != 0)
    assert np.array_equal(got.view(np.uint32), want["dL_dinput"].view(np.uint32)), float(np.max(np.abs(got - want["dL_dinput"])))
    if model[0].startswith("identity") or model[0] == "oneblob" or not fused:
        return
    # the grid's parameter gradients do not depend on whether dL/dinput was asked for (exact scatter sums, TCNN_AMD_MLP_R32=0 both sides)
    with monkeypatch.context() as m:
        m.setenv("TCNN_AMD_MLP_R32", "0")
        runs = []
        for with_dx in (False, True):
            tr = tcnn.Trainer(n_in, 3, cfg, seed=1337)
            tr.set_params(_t(params_h.view(np.float16)))
            d = torch.zeros((n, n_in), dtype=torch.float32, device="cuda") if with_dx else None
            tr.training_step(_t(x), None, run_optimizer=False, dL_dinput=d, external_dL_dy=_t(dy.view(np.float16)))
            runs.append(_bits(tr.param_gradients())[ref.model.network.n_params:])
    assert np.any(runs[0] != 0) and np.array_equal(runs[0], runs[1])


# ---------------------------------------------------------------------------------------------------- c.4 grid dL/dx through tcnn.Encoding
ENC_DX_CASES = [  # (n_in, encoding)
    (2, {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 16, "per_level_scale": 1.5}),
    (3, {"otype": "HashGrid", "n_levels": 6, "n_features_per_level": 4, "log2_hashmap_size": 14, "base_resolution": 8, "per_level_scale": 2.0}),
    (4, {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 1, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}),
    (2, {"otype": "DenseGrid", "n_levels": 3, "n_features_per_level": 8, "base_resolution": 8, "per_level_scale": 2.0}),
    (3, {"otype": "TiledGrid", "n_levels": 4, "n_features_per_level": 2, "base_resolution": 8, "per_level_scale": 1.5}),
    (2, {"otype": "HashGrid", "n_levels": 5, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 8, "per_level_scale": 1.5, "interpolation": "Smoothstep"}),
    (3, {"otype": "DenseGrid", "n_levels": 3, "n_features_per_level": 1, "base_resolution": 4, "per_level_scale": 2.0, "interpolation": "Smoothstep"}),
    (2, {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 8, "per_level_scale": 2.0, "interpolation": "Nearest"}),
    (4, {"otype": "TiledGrid", "n_levels": 2, "n_features_per_level": 4, "base_resolution": 4, "per_level_scale": 2.0, "interpolation": "Smoothstep"}),
]


@pytest.mark.parametrize("dtype", ["half", "float"])
@pytest.mark.parametrize("n_in,enc_cfg", ENC_DX_CASES)
def test_grid_input_gradient_through_encoding(tcnn, oracle, n_in, enc_cfg, dtype):
    """x.grad of tcnn.Encoding (k_grid_fwd's dy_dx, then k_grid_bwd_input) against orc_grid_forward(dy_dx) -> orc_grid_backward_input, with
    random and edge inputs: bit-identical for fp16 grids, within test_grid_encoding_fp32's tolerance for fp32 ones; the parameter gradients
    of a pass with x.requires_grad are those of a pass without it, bit for bit."""
    import torch

    fp16 = dtype == "half"
    enc = tcnn.Encoding(n_in, enc_cfg, dtype=torch.half if fp16 else torch.float32)
    ref = oracle.create_encoding(n_in, enc_cfg, alignment=0)
    params_h = oracle.half_bits(oracle.Pcg32(3).uniform_strided(ref.n_params, -1.0, 1.0))
    n = 1024
    x = np.concatenate([oracle.Pcg32(42).uniform_strided((n - 256) * n_in).reshape(n - 256, n_in), edge_x(256, n_in)]).astype(np.float32)
    width = enc.n_output_dims
    dy = oracle.half_bits(oracle.Pcg32(9).uniform_strided(n * width, -2.0, 2.0).reshape(n, width))
    _, ctx = ref.forward(x, params_h, want_dy_dx=True)
    want = ref.backward(x, ctx, dy, want_dL_dx=True)
    with torch.no_grad():
        enc.params.copy_(_t(params_h.view(np.float16).astype(np.float32)))
    grads = []
    for with_x in (True, False):
        enc.params.grad = None
        xt = _t(x).requires_grad_(with_x)
        out = enc(xt)
        out.backward(_t(dy.view(np.float16)).to(out.dtype))
        grads.append(enc.params.grad.detach().clone())
        if with_x:
            got = xt.grad.detach().cpu().numpy()
    if fp16 and enc_cfg["n_features_per_level"] > 1:
        assert torch.equal(grads[0], grads[1])
    else:
        # an fp32 grid's gradient, and an F = 1 grid's fp32 scratch (grid.h:660, 850-886), are summed with float atomics in arbitrary order
        # (k_grid_bwd): not even two runs of the same pass agree bit for bit; the F = 1 half gradient is that sum rounded once
        tol = 1e-5 if not fp16 else 1e-3
        assert float(torch.linalg.norm(grads[0] - grads[1])) <= tol * float(torch.linalg.norm(grads[1]))
    if enc_cfg.get("interpolation") == "Nearest":
        assert not np.any(got) and not np.any(want)
        return
    assert np.any(want != 0)
    if fp16:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.max(np.abs(got - want)))
    else:
        assert rel_err(got, want) < 2e-3  # fp32 grid: interpolation weights and values not rounded to fp16 as the oracle's


# ---------------------------------------------------------------------------------------------------- c.5 SoA input in a training step
@pytest.mark.parametrize("cfg,n_in,n", [(CONFIG_C3A, 2, 1 << 18), (CONFIG_C5_SMALL, 3, 256 * 9), (CONFIG_C2, 2, 256 * 9)], ids=["c3a", "c5_small", "c2"])
def test_soa_training_step_is_bit_identical(tcnn, oracle, monkeypatch, cfg, n_in, n):
    """input_layout=SoA ([n_in][n]) switches off the scatter records and the wide coordinate loads (C3A), and k_mlp_train_r32ob reads x
    through its strides (C2): everything the step returns equals the AoS step's, bit for bit."""
    x, t = oracle.synthetic_batch(n, n_in, 3, seed=42)
    a = _run(tcnn, monkeypatch, n_in, 3, cfg, {}, x, t)
    s = _run(tcnn, monkeypatch, n_in, 3, cfg, {}, x, t, layout="soa")
    assert a["kernel"] != "unfused" and s["kernel"] != "unfused"
    for k in ("out", "dy", "g"):
        assert np.array_equal(a[k], s[k]), k
    assert np.array_equal(a["L"].view(np.uint32), s["L"].view(np.uint32)) and a["loss"] == s["loss"]


# ---------------------------------------------------------------------------------------------------- c.6 use_inference_params
def test_use_inference_params_with_ema(tcnn, oracle):
    """Ema -> Adam for a few steps, then training_step(use_inference_params=True, run_optimizer=False): the unfused path at the EMA weights
    against the oracle at the same weights; the training weights do not move."""
    cfg = {**CONFIG_C3B, "optimizer": {"otype": "Ema", "decay": 0.9, "nested": CONFIG_C3B["optimizer"]}}
    n = 256 * 9
    tr = tcnn.Trainer(2, 3, cfg, seed=1337)
    for s in range(3):
        x, t = oracle.synthetic_batch(n, 2, 3, seed=100 + s)
        tr.training_step(_t(x), _t(t))
    ema = _bits(tr.params_inference())
    p_before, fp_before = _bits(tr.params()), tr.params_full_precision().cpu().numpy()
    assert not np.array_equal(ema, p_before)
    x, t = oracle.synthetic_batch(n, 2, 3, seed=7)
    ctx = tr.training_step(_t(x), _t(t), run_optimizer=False, use_inference_params=True)
    assert tr.last_step_kernel() == "unfused"
    assert np.array_equal(_bits(tr.params()), p_before) and np.array_equal(tr.params_full_precision().cpu().numpy(), fp_before)
    assert np.array_equal(_bits(tr.params_inference()), ema)
    ref = oracle.Trainer(2, 3, cfg, seed=1337)
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    ref.params = p_before.copy()
    ref.optimizer.weights_ema[:] = ema
    want = ref.training_step(x, t, run_optimizer=False, grads_f32=grads32, use_inference_params=True)
    got = {"out": _bits(ctx.output()), "L": ctx.L().cpu().numpy(), "dy": _bits(ctx.dL_doutput()), "g": _bits(tr.param_gradients()), "loss": tr.loss(ctx)}
    _check_against_oracle(ref, want, grads32, got, n, 3)
    # and not at the training weights
    out_train, _ = ref.model.forward(x, p_before)
    assert not np.array_equal(out_train, want["output"])
