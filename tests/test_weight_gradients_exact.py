"""The MLP's weight gradients bit for bit against the oracle, kernel by kernel.

In the exact setting of grad_checks.exact_case -- Identity-encoded inputs in quarters, weights in {-1, 0, 1}, an external dL/dy in eighths --
every activation and every dL/dhidden is an fp16 number and every fp32 partial sum of every product is exact whatever its order
(tests/test_grad_checks.py::test_the_exact_setting_is_exact proves it for each case below, on the CPU).  ReLU cannot flip, the one rounding
to half is determined: the network's half gradients must equal oracle.Trainer(...).grads bit for bit, and two runs must agree.  A kernel
that dropped a batch block, mis-addressed a tile, summed a slab twice or held a partial sum in less than fp32 fails here by at least one
bit of one element.

Covered, each asserted by Trainer.last_step_kernel: every train<W,NB,NW,MAXT> instance of k_train.hip (/relu and /act),
train_regw, regs (the general form: an external dL/dy is its loss 0), the unfused sequence k_mlp_fwd -> k_mlp_bwd -> k_wgrad / k_wgrad_rows /
k_wgrad_cols (widths 16, 32, 64, 128, 256 and 40 outputs, TCNN_AMD_WGRAD_ROWS=0 and 1), the layer-by-layer path of k_mlp_layers.hip (48, 96,
512 wide and zero hidden layers), with ReLU and with None, at 256 x 5, 256 x 9 and 2^16 samples, the slab reduction as a launch of its own
(run_optimizer=False), inside the optimizer's launch (k_wgrad_reduce_adam) and in front of it (TCNN_AMD_ADAM_IN_REDUCE=0), and
tcnn.Network(...).backward.

NOT reachable in this setting: regs_fast, r32, r32a, r32w (they take a loss, not an external dL/dy, and their first-layer input is an
interpolated grid value), r32ob and train_ob (a OneBlob value), and the slab reduction that rides on the grid scatter's finalize launch or the
optimizer's prologue (it needs a grid encoding).  Those rest on the per-layer bar of test_training_step_matrix.py, in both of its regimes, and on
test_finalize_pass_inside_the_optimizer_launch_is_bit_identical.
"""
import numpy as np
import pytest

import grad_checks as gc
from grad_checks import exact_case as E
from test_gpu_parity import _bits, _t

pytestmark = pytest.mark.gpu

R0 = {"TCNN_AMD_MLP_REGS": "0", "TCNN_AMD_MLP_REGW": "0"}
BIG = {"x_levels": 2, "dy_den": 4}  # 2^16 samples: x in {0, 1/2}, dL/dy in quarters
DEEP = {"x_levels": 2, "dy_den": 4, "nonzero": 1 / 16}  # 8 hidden layers (ReLU only: without an activation the hidden sums leave fp16)
N5, N9, N16 = 256 * 5, 256 * 9, 1 << 16


def _v(nb, nw, maxt):
    return {**R0, "TCNN_AMD_MLP_VARIANT": f"{nb},{nw},{maxt}"}


def _both(case_relu, case_none, env, kernel_relu, kernel_none):
    return [(case_relu, env, kernel_relu), (case_none, env, kernel_none)]


# (exact case, environment, expected kernel).  The forced variants' shapes are those of test_training_step_matrix.FORM_CASES (16 inputs).
RUNS = (
    _both(E(16, 64, 4, "ReLU", 3, N16, **BIG), E(16, 64, 1, "None", 24, N5), _v(1, 8, 8), "train<64,1,8,8>/relu", "train<64,1,8,8>/act")
    + _both(E(16, 64, 2, "ReLU", 24, N9), E(16, 64, 2, "None", 3, N5), _v(2, 4, 8), "train<64,2,4,8>/relu", "train<64,2,4,8>/act")
    + _both(E(16, 64, 3, "ReLU", 24, N5), E(16, 64, 4, "None", 3, N9), _v(2, 4, 16), "train<64,2,4,16>/relu", "train<64,2,4,16>/act")
    + _both(E(16, 64, 1, "ReLU", 3, N9), E(16, 64, 4, "None", 24, N5, out_nonzero=1 / 8), _v(1, 4, 16), "train<64,1,4,16>/relu", "train<64,1,4,16>/act")
    + _both(E(16, 64, 8, "ReLU", 3, N9, **DEEP), E(16, 64, 3, "None", 24, N16, **BIG), _v(1, 4, 32), "train<64,1,4,32>/relu", "train<64,1,4,32>/act")
    + _both(E(16, 128, 2, "ReLU", 3, N9), E(16, 128, 1, "None", 24, N5), _v(1, 8, 16), "train<128,1,8,16>/relu", "train<128,1,8,16>/act")
    + _both(E(16, 128, 1, "ReLU", 24, N5), E(16, 128, 2, "None", 3, N16, **BIG), _v(1, 8, 32), "train<128,1,8,32>/relu", "train<128,1,8,32>/act")
    + _both(E(16, 128, 2, "ReLU", 24, N5), E(16, 128, 2, "None", 3, N9), _v(1, 4, 32), "train<128,1,4,32>/relu", "train<128,1,4,32>/act")
    # all weight fragments in registers
    + _both(E(32, 64, 2, "ReLU", 16, N16, **BIG), E(16, 64, 2, "None", 3, N9), {"TCNN_AMD_MLP_REGS": "0"}, "train_regw/relu", "train_regw/act")
    # register-resident kernels, general form (an external dL/dy is not one of regs_fast's compile-time formats)
    + _both(E(32, 64, 2, "ReLU", 3, N9), E(32, 64, 2, "None", 16, N16, **BIG), {}, "regs", "regs")
    + _both(E(16, 64, 1, "ReLU", 16, N5), E(16, 64, 1, "None", 3, N9), {}, "regs", "regs")
    + _both(E(16, 64, 2, "ReLU", 3, N5), E(32, 64, 1, "None", 16, N5), {}, "regs", "regs")
)
# the unfused sequence, with both weight-gradient kernels: shapes with a fused kernel of their own (TCNN_AMD_FUSED_STEP=0) and shapes without
for rows in ("0", "1"):
    unf = {"TCNN_AMD_WGRAD_ROWS": rows}
    RUNS += (
        _both(E(32, 64, 2, "ReLU", 3, N9), E(16, 128, 2, "None", 3, N16, **BIG), {**unf, "TCNN_AMD_FUSED_STEP": "0"}, "unfused", "unfused")
        + _both(E(16, 16, 2, "ReLU", 3, N5), E(16, 16, 3, "None", 16, N9), unf, "unfused", "unfused")
        + _both(E(32, 32, 1, "ReLU", 24, N16, **BIG), E(16, 32, 2, "None", 3, N5), unf, "unfused", "unfused")
        + _both(E(16, 256, 1, "ReLU", 3, N5), E(32, 256, 1, "None", 16, N9), unf, "unfused", "unfused")
        + _both(E(16, 64, 2, "ReLU", 40, N5), E(32, 64, 2, "None", 40, N9), unf, "unfused", "unfused")
    )
# the layer-by-layer path (CutlassMLP widths without a kernel of their own, zero hidden layers)
RUNS += (
    _both(E(32, 48, 2, "ReLU", 3, N5), E(16, 48, 2, "None", 16, N9), {}, "unfused", "unfused")
    + _both(E(16, 96, 3, "ReLU", 24, N9), E(32, 96, 1, "None", 3, N16, **BIG), {}, "unfused", "unfused")
    + _both(E(32, 512, 1, "ReLU", 3, N5, out_nonzero=1 / 8), E(32, 512, 1, "None", 24, N5, out_nonzero=1 / 8), {}, "unfused", "unfused")
    + _both(E(32, 64, 0, "ReLU", 24, N16, **BIG), E(16, 64, 0, "None", 3, N5), {}, "unfused", "unfused")
)


def _run_id(run):
    case, env, kernel = run
    tag = ",".join(f"{k.replace('TCNN_AMD_', '').lower()}={v}" for k, v in sorted(env.items()) if k in ("TCNN_AMD_WGRAD_ROWS", "TCNN_AMD_FUSED_STEP"))
    return f"{kernel}-{gc.exact_case_id(case)}" + (f"-{tag}" if tag else "")


# the distinct exact cases (tests/test_grad_checks.py checks the setting's conditions for each of them on the CPU)
NETWORK_CASES = [E(32, 64, 2, "ReLU", 3, N5), E(16, 128, 2, "None", 16, N9), E(32, 48, 2, "ReLU", 24, N5), E(16, 64, 0, "None", 3, N9), E(16, 256, 1, "ReLU", 3, N5)]
# exact cases that no run above uses any more (they were the cases of a kernel form that has been removed): tests/test_grad_checks.py keeps
# proving on the CPU that the exact setting holds for these shapes too -- 16 and 32 inputs into 64 x 1 and 64 x 2 with 3, 16 and 24 outputs
EXACT_ONLY = [E(16, 64, 2, "ReLU", 16, N5), E(32, 64, 1, "None", 3, N9), E(32, 64, 2, "ReLU", 24, N9), E(16, 64, 2, "None", 24, N5)]
EXACT_CASES = list({gc.exact_case_id(c): c for c in [r[0] for r in RUNS] + EXACT_ONLY + NETWORK_CASES}.values())


def _oracle_step(oracle, case):
    cfg = gc.exact_case_config(case)
    ref = oracle.Trainer(case["n_in"], case["n_out"], cfg, seed=1337)
    net = ref.model.network
    w, x, dy = gc.exact_case_inputs(case, net.n_params, net.padded_output_width)
    ref.params = oracle.half_bits(w)
    grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
    ref.training_step(x, None, run_optimizer=False, grads_f32=grads32, external_dL_dy=oracle.half_bits(dy))
    return cfg, gc.layer_slices(net), w, x, dy, ref.grads.copy(), grads32


def _gpu_step(tcnn, monkeypatch, case, cfg, env, w, x, dy, run_optimizer=False, info=None):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        tr = tcnn.Trainer(case["n_in"], case["n_out"], cfg, seed=1337)
        tr.set_params(_t(w.astype(np.float16)))
        tr.training_step(_t(x), None, run_optimizer=run_optimizer, external_dL_dy=_t(dy.astype(np.float16)))
        if info is not None:
            info["params_updated_in_flush"] = tr.params_updated_in_flush()
        return tr.last_step_kernel(), _bits(tr.param_gradients()).copy()


def _assert_same_bits(got, want, slices, what):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    l = max(k for k, (o, _, _) in enumerate(slices) if o <= i)
    o, _, c = slices[l]
    per_layer = [int(np.count_nonzero((bad >= o_) & (bad < o_ + r_ * c_))) for o_, r_, c_ in slices]
    raise AssertionError(f"{what}: {bad.size} of {got.size} half gradients differ from the oracle's (per layer {per_layer}); first: layer {l}, row {(i - o) // c}, "
                         f"column {(i - o) % c}: got {float(got[i:i + 1].view(np.float16)[0])!r} (0x{int(got[i]):04x}), want {float(want[i:i + 1].view(np.float16)[0])!r} (0x{int(want[i]):04x})")


@pytest.mark.parametrize("run", RUNS, ids=[_run_id(r) for r in RUNS])
def test_weight_gradients_are_bit_identical(tcnn, oracle, monkeypatch, run):
    case, env, kernel = run
    cfg, slices, w, x, dy, want, grads32 = _oracle_step(oracle, case)
    assert np.any(want != 0)
    name, got = _gpu_step(tcnn, monkeypatch, case, cfg, env, w, x, dy)
    assert name == kernel
    what = f"{gc.exact_case_id(case)} [{name}]"
    _assert_same_bits(got, want, slices, what)
    gc.assert_structural_zeros(got, grads32, slices, what)
    name2, again = _gpu_step(tcnn, monkeypatch, case, cfg, env, w, x, dy)
    assert name2 == kernel and np.array_equal(got, again), f"{what}: two runs differ"


@pytest.mark.parametrize("in_reduce", [True, False], ids=["k_wgrad_reduce_adam", "adam_in_reduce_0"])
@pytest.mark.parametrize("run", [next(r for r in RUNS if r[2] == k) for k in ("train<64,1,8,8>/relu", "train_regw/act", "regs")], ids=["train<64,1,8,8>", "train_regw", "regs"])
def test_weight_gradients_are_bit_identical_with_the_optimizer_in_the_step(tcnn, oracle, monkeypatch, run, in_reduce):
    """run_optimizer=True: the 256-slab reduction of a model without encoding parameters runs inside the optimizer's launch (k_wgrad_reduce_adam
    applies the update to every parameter itself) or, with TCNN_AMD_ADAM_IN_REDUCE=0, as a launch of its own in front of k_adam; which of the
    two ran is asserted (Trainer.params_updated_in_flush), and the gradients it leaves are the oracle's either way"""
    case, kernel_env, kernel = run
    cfg, slices, w, x, dy, want, _ = _oracle_step(oracle, case)
    info = {}
    name, got = _gpu_step(tcnn, monkeypatch, case, cfg, {**kernel_env, **({} if in_reduce else {"TCNN_AMD_ADAM_IN_REDUCE": "0"})}, w, x, dy, run_optimizer=True, info=info)
    assert name == kernel
    assert info["params_updated_in_flush"] == (want.size if in_reduce else 0), "which launch summed the slabs is not what this run asked for"
    _assert_same_bits(got, want, slices, f"{gc.exact_case_id(case)} [{name}] with the optimizer, reduction {'inside' if in_reduce else 'in front of'} its launch")


@pytest.mark.parametrize("case", NETWORK_CASES, ids=[gc.exact_case_id(c) for c in NETWORK_CASES])
def test_network_module_weight_gradients_are_bit_identical(tcnn, oracle, case):
    """tcnn.Network(...).backward (k_mlp_bwd + k_wgrad*, k_mlp_layers.hip for the widths without a kernel of their own): the module scales the
    upstream gradient by 128 and divides the parameter gradient by it -- with dL/dy / 128 upstream, params.grad * 128 is the oracle's half
    gradient exactly"""
    import torch

    cfg, slices, w, x, dy, want, grads32 = _oracle_step(oracle, case)
    net = tcnn.Network(case["n_in"], case["n_out"], cfg["network"], seed=1337)
    with torch.no_grad():
        net.params.copy_(_t(w))
    runs = []
    for _ in range(2):
        net.params.grad = None
        out = net(_t(x))
        up = (dy[:, :case["n_out"]] / np.float32(128.0)).astype(np.float16)
        assert np.array_equal(up.astype(np.float32) * np.float32(128.0), dy[:, :case["n_out"]])
        out.backward(_t(up).to(out.dtype))
        g = net.params.grad.detach().float().cpu().numpy() * np.float32(128.0)
        assert np.array_equal(g.astype(np.float16).astype(np.float32), g)  # a half value, exactly
        runs.append(g.astype(np.float16).view(np.uint16))
    what = f"tcnn.Network {gc.exact_case_id(case)}"
    _assert_same_bits(runs[0], want, slices, what)
    gc.assert_structural_zeros(runs[0], grads32, slices, what)
    assert np.array_equal(runs[0], runs[1]), f"{what}: two runs differ"
