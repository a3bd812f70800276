"""CPU tests of tests/grad_checks.py, the per-layer bar on the MLP's weight gradients: with the oracle alone (no GPU),

  1. the bar can be met: two evaluations of the reference's arithmetic that differ only in summation order stay below half of it in every
     case the GPU tests use with a piecewise-linear activation;
  2. the bar bites: six ways a weight-gradient kernel goes wrong are rejected, and what the norm-wise bar made of them is on record;
  3. the exact setting is exact: the conditions under which test_weight_gradients_exact.py asks for the oracle's bits hold for each of its cases.
"""
import numpy as np
import pytest

import grad_checks as gc
from test_gpu_parity import rel_err
from test_training_step_matrix import FORM_CASES, NORMAL_RANGE_CASES, PDF_CASES, PER_LAYER_BAR_NOT_AT_INIT, _cfg, _targets, normal_range_inputs, o1_grid_params
from test_weight_gradients_exact import EXACT_CASES

PIECEWISE_LINEAR = ("ReLU", "LeakyReLU", "None")
YARDSTICK_CAP = 0.5
MIN_NONZERO_SHARE = 0.15  # of every layer's live gradients in an exact case: the comparison is of numbers, not of zeros


def _yardstick(oracle, ref, cfg, x, t, n_out, pdf, rtol=3e-2):
    """weight_grad_ratios(float64_step, oracle fp32, q = 0) per layer, at the oracle trainer's parameters"""
    net = ref.model.network
    n_net, slices = net.n_params, gc.layer_slices(net)
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    ref.training_step(x, t, run_optimizer=False, grads_f32=grads32, data_pdf=pdf)
    enc_out, _ = ref.model.encoding.forward(x, np.ascontiguousarray(ref.params[n_net:]))
    st = gc.float64_step(oracle.half_to_f32(enc_out), oracle.half_to_f32(ref.params[:n_net]), slices, cfg["network"]["activation"], cfg["network"]["output_activation"],
                         loss=cfg["loss"]["otype"], target=t, n_out=n_out, data_pdf=pdf)
    return gc.weight_grad_ratios(st["grads"], grads32[:n_net], slices, rtol, False)


# ---------------------------------------------------------------------------------------------------- 1. the bar can be met
FIRST_REGIME = [(c[0], _cfg(c[1], c[3], c[4], c[5], c[6]), c[2], c[7], c[8], c[9], c[10], c[6], None) for c in FORM_CASES] + \
               [(f"pdf_{c[0]}_{loss}", {**c[1], "loss": {"otype": loss}}, c[2], c[3], c[4], c[5], c[6], None, 3) for c in PDF_CASES for loss in ("L2", "RelativeL2")]
YARDSTICK_CASES = [("init", c) for c in FIRST_REGIME if c[1]["network"]["activation"] in PIECEWISE_LINEAR and c[0] not in PER_LAYER_BAR_NOT_AT_INIT] + \
                  [("o1", c) for c in NORMAL_RANGE_CASES if c[1]["network"]["activation"] in PIECEWISE_LINEAR]


@pytest.mark.parametrize("regime,case", YARDSTICK_CASES, ids=[f"{r}-{c[0]}" for r, c in YARDSTICK_CASES])
def test_the_bar_can_be_met(oracle, regime, case):
    """float64 sums against the oracle's sequential fp32 fmaf, same roundings to half: <= 0.5 of the bar in every layer, with the grid as
    initialised ("init", test_training_kernel_forms_match_oracle / test_data_pdf_in_each_training_kernel) and drawn from U(-1, 1) ("o1")"""
    _, cfg, n_in, n_out, n, _, _, _, _ = case
    x, t, pdf = normal_range_inputs(oracle, case)
    ref = oracle.Trainer(n_in, n_out, cfg, seed=1337)
    if regime == "o1":
        ref.params = o1_grid_params(oracle, ref)
    ratios = _yardstick(oracle, ref, cfg, x, t, n_out, pdf)
    assert max(ratios) <= YARDSTICK_CAP, ratios


def test_where_the_bar_cannot_be_met_at_init(oracle):
    """the cases test_training_kernel_forms_match_oracle keeps under its other bars only (PER_LAYER_BAR_NOT_AT_INIT): summation order alone
    exceeds the cap with the grid as initialised (4 LeakyReLU layers: 0.6), and stays below it with the U(-1, 1) grid ("o1" above)"""
    for case in FIRST_REGIME:
        if case[0] not in PER_LAYER_BAR_NOT_AT_INIT:
            continue
        _, cfg, n_in, n_out, n, _, _, _, _ = case
        x, t, pdf = normal_range_inputs(oracle, case)
        ratios = _yardstick(oracle, oracle.Trainer(n_in, n_out, cfg, seed=1337), cfg, x, t, n_out, pdf)
        assert max(ratios) > YARDSTICK_CAP, (case[0], ratios)


def _parity_cases():
    """the cases of test_gpu_parity.py that ask for the per-layer bar on a training step: (id, config, n_in, n_out, n, batch seed)"""
    import test_gpu_parity as P
    from conftest import CONFIG_C2, CONFIG_C5_SMALL

    out = [(f"training_step_{i}", cfg, n_in, 3, n, 42) for i, (cfg, n_in, n) in enumerate(P.TRAINING_STEP_CASES)]
    out += [(f"r32_{i}", {**base, "loss": {"otype": loss}}, 3 if base is CONFIG_C5_SMALL else 2, n_out, n, 17) for i, (base, n_out, loss, n) in enumerate(P.R32_CASES)]
    out += [(f"wgrad_{w}x{h}_{b}", dict(CONFIG_C2, encoding={"otype": "OneBlob", "n_bins": b},
                                        network={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": w, "n_hidden_layers": h}), 2, 3, 8192,
             P.WGRAD_AGREE_BATCH_SEED) for w, h, b in P.WGRAD_AGREE_CASES]
    out.append(("c2_full_batch", CONFIG_C2, 2, 3, 65536, 70))
    return out


PARITY_CASES = _parity_cases()


@pytest.mark.parametrize("case", PARITY_CASES, ids=[c[0] for c in PARITY_CASES])
def test_the_bar_can_be_met_in_the_parity_tests(oracle, case):
    """test_gpu_parity's training steps (test_training_step_matches_oracle, test_r32_kernels_other_output_counts_losses_and_batches,
    test_weight_gradient_kernels_agree, test_c2_full_batch_two_trips_per_wave), up to 164 096 samples"""
    _, cfg, n_in, n_out, n, seed = case
    x, t = oracle.synthetic_batch(n, n_in, n_out, seed=seed)
    ref = oracle.Trainer(n_in, n_out, cfg, seed=1337)
    ratios = _yardstick(oracle, ref, cfg, x, t, n_out, None)
    assert max(ratios) <= YARDSTICK_CAP, ratios


def _network_yardstick(oracle, source, n_in, n_out, net_cfg, n, enc={"otype": "Identity"}):
    """tcnn.Network / tcnn.NetworkWithInputEncoding cases: random upstream gradient scaled by 128, rtol 2e-2"""
    ref = oracle.NetworkWithInputEncoding(n_in, n_out, enc, net_cfg)
    params_h = oracle.half_bits(ref.initialize_params(oracle.Pcg32(1337)))
    x = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in)
    out, ctx = ref.forward(x, params_h)
    dy = np.zeros((n, ref.padded_output_width), dtype=np.float32)
    if source == "parity":
        dy[:, :n_out] = oracle.Pcg32(5).uniform_strided(n * n_out, -1.0, 1.0).reshape(n, n_out)
    else:  # test_layerwise_mlp._fwd_bwd
        dy[:, :n_out] = np.random.RandomState(5).uniform(-1.0, 1.0, (n, n_out))
    dy_h = oracle.half_bits(dy.astype(np.float16).astype(np.float32) * 128.0)
    grads32 = np.zeros(ref.n_params, dtype=np.float32)
    ref.backward(x, params_h, ctx, out, dy_h, grads_f32=grads32)
    slices = gc.layer_slices(ref.network)
    st = gc.float64_step(oracle.half_to_f32(ctx["network_input"]), oracle.half_to_f32(params_h), slices, net_cfg["activation"], net_cfg["output_activation"],
                         external_dL_dy=oracle.half_to_f32(dy_h))
    return gc.weight_grad_ratios(st["grads"], grads32[:ref.network.n_params], slices, 2e-2, False)


def _network_cases():
    from test_gpu_parity import MLP_CASES
    from test_layerwise_mlp import FLIPS_EXCEED_THE_BAR_AT_2_16, ORACLE_CASES

    ok = lambda c: c[2]["activation"] in PIECEWISE_LINEAR and c[2]["output_activation"] in ("None", "ReLU", "Sigmoid")  # noqa: E731
    met = [("parity", c, 512) for c in MLP_CASES if ok(c)] + [("layerwise", c, 512) for c in ORACLE_CASES if ok(c)] + \
          [("layerwise", c, (1 << 16) + 256) for c in ORACLE_CASES if ok(c) and c[2]["n_neurons"] not in FLIPS_EXCEED_THE_BAR_AT_2_16]
    not_met = [("layerwise", c, (1 << 16) + 256) for c in ORACLE_CASES if ok(c) and c[2]["n_neurons"] in FLIPS_EXCEED_THE_BAR_AT_2_16]
    return met, not_met


NETWORK_MET, NETWORK_NOT_MET = _network_cases()
_net_id = lambda c: f"{c[0]}-{c[1][0]}x{c[1][2]['n_neurons']}x{c[1][2]['n_hidden_layers']}_{c[1][2]['activation']}_{c[1][2]['output_activation']}_o{c[1][1]}-n{c[2]}"  # noqa: E731


@pytest.mark.parametrize("case", NETWORK_MET, ids=[_net_id(c) for c in NETWORK_MET])
def test_the_bar_can_be_met_through_tcnn_network(oracle, case):
    """the cases of test_gpu_parity.test_network_forward_backward (512 rows) and of test_layerwise_mlp.test_layerwise_network_matches_oracle (512 and
    65 792 rows) with a piecewise-linear activation, wherever they ask for the bar"""
    source, (n_in, n_out, net_cfg), n = case
    ratios = _network_yardstick(oracle, source, n_in, n_out, net_cfg, n)
    assert max(ratios) <= YARDSTICK_CAP, ratios


@pytest.mark.parametrize("case", NETWORK_NOT_MET, ids=[_net_id(c) for c in NETWORK_NOT_MET])
def test_relu_flips_exceed_the_bar_over_2_16_rows(oracle, case):
    """test_layerwise_mlp.FLIPS_EXCEED_THE_BAR_AT_2_16: in the 192- and 512-wide two-hidden-layer ReLU networks at 65 792 rows summation order alone
    exceeds the cap (measured 2.36 and 2.40 in the second layer; 1.2-1.9 with other input seeds): no implementation can be held to the bar there"""
    source, (n_in, n_out, net_cfg), n = case
    ratios = _network_yardstick(oracle, source, n_in, n_out, net_cfg, n)
    assert max(ratios) > YARDSTICK_CAP, ratios


def test_the_bar_can_be_met_through_network_with_input_encoding(oracle):
    """the two cases of test_layerwise_mlp.test_network_with_input_encoding (2048 rows)"""
    from test_layerwise_mlp import _net

    for enc, n_in, width in (({"otype": "OneBlob", "n_bins": 32}, 2, 96),
                             ({"otype": "Composite", "nested": [{"n_dims_to_encode": 1, "otype": "OneBlob", "n_bins": 16}, {"otype": "Identity"}]}, 3, 48)):
        ratios = _network_yardstick(oracle, "layerwise", n_in, 3, _net(width, 2, "ReLU"), 2048, enc)
        assert max(ratios) <= YARDSTICK_CAP, (enc, ratios)


def test_the_bar_can_be_met_at_c5_full_size(oracle):
    """test_gpu_parity.test_c5_full_size_training_step (i): 4096 samples, 210.9 M parameters (the network's part of the step only)"""
    from conftest import CONFIG_C5

    ref = oracle.Trainer(3, 3, CONFIG_C5, seed=1337)
    x, t = oracle.synthetic_batch(4096, 3, 3, seed=42)
    net = ref.model.network
    n_net, slices = net.n_params, gc.layer_slices(net)
    net_p = np.ascontiguousarray(ref.params[:n_net])
    enc_out, _ = ref.model.encoding.forward(x, np.ascontiguousarray(ref.params[n_net:]))
    out, hidden = net.forward(enc_out, net_p)
    _, dL_dout = oracle.loss_evaluate("RelativeL2", out, t)
    grads32 = np.zeros(n_net, dtype=np.float32)
    net.backward(enc_out, net_p, hidden, out, dL_dout, False, None, grads32)
    st = gc.float64_step(oracle.half_to_f32(enc_out), oracle.half_to_f32(net_p), slices, "ReLU", "None", loss="RelativeL2", target=t, n_out=3)
    ratios = gc.weight_grad_ratios(st["grads"], grads32, slices, 3e-2, False)
    assert max(ratios) <= YARDSTICK_CAP, ratios


def test_the_oracles_own_half_gradients_pass(oracle):
    """with q = 2^-24 the oracle's half gradient against its fp32 one is below 0.5 by construction, subnormals or not"""
    for name in ("v64_1_4_32_act", "v64_1_4_32_relu", "r32a"):
        c = next(c for c in FORM_CASES if c[0] == name)
        cfg = _cfg(c[1], c[3], c[4], c[5], c[6])
        n_in, n_out, n = c[2], c[7], c[8]
        ref = oracle.Trainer(n_in, n_out, cfg, seed=1337)
        grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
        ref.training_step(oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in), _targets(c[6], n, n_out, 17), run_optimizer=False, grads_f32=grads32)
        n_net, slices = ref.model.network.n_params, gc.layer_slices(ref.model.network)
        assert max(gc.weight_grad_ratios(oracle.half_to_f32(ref.grads[:n_net]), grads32[:n_net], slices, 3e-2, True)) <= 0.5
        gc.assert_structural_zeros(ref.grads[:n_net], grads32[:n_net], slices, name)


# ---------------------------------------------------------------------------------------------------- 2. the bar bites
BITE_CONFIGS = ["v64_1_4_32_act", "v64_1_8_8_relu", "v64_1_4_32_relu", "r32a", "oneblob_relu"]
CORRUPTIONS = ["layer0_scaled", "layer0_tile_zeroed", "hidden_tile_transposed", "hidden_rows_swapped", "hidden_layer_short_batch", "padded_row_written"]
# what rel_err < 3e-2 over all layers at once -- the only bar until now -- makes of each corruption: "accepts", "rejects", or per configuration
_SOFTPLUS_ONLY = {"v64_1_4_32_act": "accepts", "v64_1_8_8_relu": "rejects", "v64_1_4_32_relu": "rejects", "r32a": "rejects", "oneblob_relu": "rejects"}
OLD_BAR = {"layer0_scaled": "accepts", "padded_row_written": "accepts", "hidden_tile_transposed": "rejects", "hidden_rows_swapped": _SOFTPLUS_ONLY,
           "layer0_tile_zeroed": _SOFTPLUS_ONLY,
           "hidden_layer_short_batch": {"v64_1_4_32_act": "accepts", "v64_1_8_8_relu": "accepts", "v64_1_4_32_relu": "accepts", "r32a": "rejects", "oneblob_relu": "rejects"}}
# (v64_1_4_32_act pads no output row: 32 outputs)
BITE_CASES = [(n, c) for n in BITE_CONFIGS for c in CORRUPTIONS if not (c == "padded_row_written" and n == "v64_1_4_32_act")]


def _short_batch_layer(oracle, ref, x, t, layer, n_keep):
    """fp32 gradient of one layer summed over the first n_keep samples only (dL/doutput still that of the whole batch)"""
    net = ref.model.network
    n_net = net.n_params
    out, ctx = ref.model.forward(x, ref.params)
    _, dL_dout = oracle.loss_evaluate(ref.loss_type, out, t)
    g = np.zeros(n_net, dtype=np.float32)
    net.backward(np.ascontiguousarray(ctx["network_input"][:n_keep]), np.ascontiguousarray(ref.params[:n_net]), np.ascontiguousarray(ctx["hidden"][:, :n_keep]),
                 np.ascontiguousarray(out[:n_keep]), np.ascontiguousarray(dL_dout[:n_keep]), False, None, g)
    o, r, c = gc.layer_slices(net)[layer]
    return g[o:o + r * c]


@pytest.mark.parametrize("name,corruption", BITE_CASES, ids=[f"{n}-{c}" for n, c in BITE_CASES])
def test_the_bar_bites(oracle, name, corruption):
    """The oracle's own half gradients, corrupted one way at a time: the per-layer checks reject every one.  Today's rel_err < 3e-2 is evaluated
    on each as well and what it does is asserted, so that this file records what was invisible."""
    c = next(c for c in FORM_CASES if c[0] == name)
    cfg = _cfg(c[1], c[3], c[4], c[5], c[6])
    n_in, n_out, n = c[2], c[7], c[8]
    x, t = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in), _targets(c[6], n, n_out, 17)
    ref = oracle.Trainer(n_in, n_out, cfg, seed=1337)
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    ref.training_step(x, t, run_optimizer=False, grads_f32=grads32)
    n_net, slices = ref.model.network.n_params, gc.layer_slices(ref.model.network)
    want = grads32[:n_net]
    g = oracle.half_to_f32(ref.grads[:n_net]).copy()
    assert max(gc.weight_grad_ratios(g, want, slices, 3e-2, True)) <= 0.5
    assert rel_err(g, want) < 3e-2

    def layer(l):
        o, r, c_ = slices[l]
        return g[o:o + r * c_].reshape(r, c_)  # a view

    hidden = 1  # the first hidden-to-hidden matrix (every configuration here has at least two hidden layers)
    assert slices[hidden][1] == slices[hidden][2]
    if corruption == "layer0_scaled":
        layer(0)[:] = oracle.half_to_f32(oracle.half_bits(layer(0) * np.float32(1.25)))
    elif corruption == "layer0_tile_zeroed":
        layer(0)[16:32, 0:16] = 0  # a fixed tile, as below
    elif corruption == "hidden_tile_transposed":
        layer(hidden)[16:32, 32:48] = layer(hidden)[16:32, 32:48].T.copy()
    elif corruption == "hidden_rows_swapped":
        rows = np.argsort(-np.max(np.abs(layer(hidden)), axis=1))[:2]  # the two rows with the largest gradients
        layer(hidden)[rows] = layer(hidden)[rows[::-1]].copy()
    elif corruption == "hidden_layer_short_batch":
        layer(hidden)[:] = oracle.half_to_f32(oracle.half_bits(_short_batch_layer(oracle, ref, x, t, hidden, n - 256))).reshape(layer(hidden).shape)
    else:
        last = layer(len(slices) - 1)
        assert n_out < last.shape[0] and not np.any(want[slices[-1][0]:].reshape(last.shape)[n_out:])
        last[n_out, :] = oracle.half_to_f32(oracle.half_bits(np.float32(1e-2 * np.max(np.abs(want)))))

    ratios = gc.weight_grad_ratios(g, want, slices, 3e-2, True)
    print(f"{name} {corruption}: worst per-layer ratio {max(ratios):.3g}, rel_err over all layers {rel_err(g, want):.3g}")
    assert max(ratios) > 1.0, (ratios, "the per-layer bar accepts this corruption")
    if corruption == "padded_row_written":
        with pytest.raises(AssertionError):
            gc.assert_structural_zeros(oracle.half_bits(g), want, slices, name)
    old = OLD_BAR[corruption]
    old = old[name] if isinstance(old, dict) else old
    assert (rel_err(g, want) < 3e-2) == (old == "accepts"), (rel_err(g, want), old)


# ---------------------------------------------------------------------------------------------------- 3. the exact setting is exact
@pytest.mark.parametrize("case", EXACT_CASES, ids=[gc.exact_case_id(c) for c in EXACT_CASES])
def test_the_exact_setting_is_exact(oracle, case):
    """From unrounded float64 values: every activation and every dL/dhidden is an fp16 number, sum_i |dO_i| |In_i| / quantum < 2^24 for every
    weight (and for every matrix-vector sum of the forward and backward passes), max |dW| < 65504 -- so every fp32 sum is exact in any order,
    no ReLU can flip and the rounding to half is the only one -- and the oracle's grads_f32 equals the unrounded float64 product exactly."""
    cfg = gc.exact_case_config(case)
    ref = oracle.Trainer(case["n_in"], case["n_out"], cfg, seed=1337)
    net = ref.model.network
    slices = gc.layer_slices(net)
    w, x, dy = gc.exact_case_inputs(case, net.n_params, net.padded_output_width)
    ref.params = oracle.half_bits(w)
    assert np.array_equal(oracle.half_to_f32(ref.params), w)
    rep = gc.exactness_report(case, w, x, dy, slices)
    print(f"{gc.exact_case_id(case)}: log2(sum of terms / quantum) <= {rep['max_log2_terms']:.1f}, max|dW| {rep['max_abs_grad']:.0f}")
    assert rep["representable"]
    assert rep["max_log2_terms"] < 24
    assert rep["max_abs_grad"] < 65504
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    ref.training_step(x, None, run_optimizer=False, grads_f32=grads32, external_dL_dy=oracle.half_bits(dy))
    assert np.array_equal(grads32.astype(np.float64), rep["grads"])
    assert np.array_equal(ref.grads, rep["grads"].astype(np.float16).view(np.uint16))  # and its half gradient is that product rounded once
    # the case says something: most of every layer's live gradients are non-zero, and some are not half-representable before the rounding
    live_rows, shares = case["n_out"], []
    for l, (o, r, c) in enumerate(slices):
        g = rep["grads"][o:o + r * c].reshape(r, c)
        if l == len(slices) - 1:
            assert not np.any(g[live_rows:])
            g = g[:live_rows]
        shares.append(np.count_nonzero(g) / g.size)
    print("non-zero share per layer", [f"{v:.2f}" for v in shares])
    assert min(shares) >= MIN_NONZERO_SHARE, shares
