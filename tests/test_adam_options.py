"""Adam per element, option by option, on every stand-alone route (tests/adam_reference.py holds the inputs, the option sets and the comparator).

Without a GPU: the oracle's Adam against the numpy restatement of tests/train_f32_reference.py under every option set, and the comparator
against nine restatements with one thing wrong each.  On the GPU: k_adam (quad-uniform and not, with its ragged tail) and k_adam_scalar
through tcnn.optimizers.NativeOptimizer against the oracle -- moments and step counts bit for bit, weights within the per-element bound."""
import ctypes as C

import numpy as np
import pytest

import adam_reference as ar

LOSS_SCALES = (128.0, 100.0)  # a power of two inside the exact window (the reciprocal multiply), and one that takes g / loss_scale


def _libm_powf(oracle):
    """the C library's powf, which orc_adam_step calls, through the oracle's own handle"""
    fn = oracle.lib().powf
    fn.restype, fn.argtypes = C.c_float, [C.c_float, C.c_float]
    return fn


@pytest.fixture(scope="module")
def k_host(oracle):
    k = ar.k_host(_libm_powf(oracle))
    print(f"K_HOST = {k}")
    return k


# ---------------------------------------------------------------------------------------------------------------- without a GPU
def test_inputs_reach_what_they_are_meant_to():
    n, layers = ar.STANDARD
    n_matrix = ar.n_matrix_of(layers)
    w = ar.initial_weights(n)
    assert np.abs(w).max() <= 0.5
    for part in (w[:n_matrix], w[n_matrix:]):
        assert np.any((part == 0) & np.signbit(part)) and np.any((part == 0) & ~np.signbit(part))
    first = n_matrix // 4
    for step in range(ar.N_STEPS):
        bits = ar.gradient_bits(n, n_matrix, step)
        g = ar.half_to_float(bits)
        assert np.all(np.isfinite(g)) and np.all(g[:first * 4] != 0)
        mags = np.abs(g[g != 0])
        assert mags.min() <= 2.0 ** -23 and mags.max() >= 2.0 ** 14 and np.any(g < 0) and np.any(g > 0)
        quads = g[first * 4:(n // 4) * 4].reshape(-1, 4)
        zeros = (quads == 0).sum(axis=1)
        kind = (np.arange(first, n // 4) + step) % 3
        assert np.all(zeros[kind == 0] == 4) and np.all(zeros[kind == 1] == 1) and np.all(zeros[kind == 2] == 0)
        zero_bits = bits[first * 4:][g[first * 4:] == 0]
        assert np.any(zero_bits == 0x8000) and np.any(zero_bits == 0)
        lanes = np.argmax(quads[kind == 1] == 0, axis=1)
        assert set(lanes) == {0, 1, 2, 3}


@pytest.mark.parametrize("loss_scale", LOSS_SCALES)
@pytest.mark.parametrize("name", list(ar.OPTION_SETS))
def test_oracle_against_the_restatement(oracle, k_host, name, loss_scale):
    """Both sides are host arithmetic: K_POWF := K_HOST."""
    n, layers = ar.STANDARD
    cfg = ar.OPTION_SETS[name]
    worst, ex = ar.run(ar.one_slice(cfg, n, layers), n, ar.RestatementSide(cfg, n, layers), ar.OracleSide(oracle, cfg, n, layers), k_host, k_host,
                       loss_scale=loss_scale, what=name)
    print(f"{name} @ {loss_scale}: worst error / bound {worst:.3f}; clipped {ex.clipped}, at the lower bound {ex.at_lower}, at the upper {ex.at_upper} of {ex.updated}")


@pytest.mark.parametrize("loss_scale", LOSS_SCALES)
@pytest.mark.parametrize("name", ["full", "frozen_matrix", "frozen_grid"])
def test_comparator_accepts_the_unmutated_restatement(oracle, k_host, name, loss_scale):
    n, layers = ar.STANDARD
    cfg = ar.OPTION_SETS[name]
    ar.run(ar.one_slice(cfg, n, layers), n, ar.OracleSide(oracle, cfg, n, layers), ar.AdamVariant(cfg, n, ar.n_matrix_of(layers)), k_host, k_host,
           loss_scale=loss_scale, what=name)


MUTANT_SETS = {m: "full" for m in ar.MUTANTS}
MUTANT_SETS["frozen_class_moves_moments"] = "frozen_grid"


@pytest.mark.parametrize("loss_scale", LOSS_SCALES)
@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_comparator_rejects_every_mutant(oracle, k_host, mutant, loss_scale):
    n, layers = ar.STANDARD
    cfg = ar.OPTION_SETS[MUTANT_SETS[mutant]]
    with pytest.raises(AssertionError) as caught:
        ar.run(ar.one_slice(cfg, n, layers), n, ar.OracleSide(oracle, cfg, n, layers), ar.AdamVariant(cfg, n, ar.n_matrix_of(layers), mutant=mutant), k_host, k_host,
               loss_scale=loss_scale, what=mutant)
    print(f"{mutant}: {str(caught.value)[:200]}")
    assert f"{mutant} [0, {n}) step" in str(caught.value), "rejected by something other than the comparator"


def test_frozen_matrix_mutant_is_rejected_too(oracle, k_host):
    n, layers = ar.STANDARD
    cfg = ar.OPTION_SETS["frozen_matrix"]
    with pytest.raises(AssertionError, match="m1 differs"):
        ar.run(ar.one_slice(cfg, n, layers), n, ar.OracleSide(oracle, cfg, n, layers), ar.AdamVariant(cfg, n, ar.n_matrix_of(layers), mutant="frozen_class_moves_moments"),
               k_host, k_host, what="frozen")


# ------------------------------------------------------------------------------------------------------------------- on the GPU
SHAPES = {
    "ragged": ar.STANDARD,               # n_matrix = 775: k_adam<false>, the last 3 parameters are the ragged tail
    "uniform": (8192, [(16, 32), (32, 8)]),  # n_matrix = 768: k_adam<true>
}
# A Composite of three Adams on 8195 parameters, the last 5 of them nobody's: [0, 465) is the first matrix (k_adam, with a tail of its own);
# [465, 1077) starts at an odd offset with the second matrix in front of 333 grid entries, [1077, 8190) is grid entries only: k_adam_scalar
COMPOSITE_N, COMPOSITE_LAYERS = 8195, [(15, 31), (31, 9)]
COMPOSITE_SLICES = [(0, 465, {}, 465), (465, 612, {}, 279), (1077, 7113, {"learning_rate": 5e-3}, 0)]


class DeviceSide:
    """a NativeOptimizer behind the interface of adam_reference.AdamVariant: the weights are the caller's tensors, the moments and counts
    are read from its snapshot"""

    def __init__(self, tcnn, cfg, n, layers):
        self.opt = tcnn.optimizers.NativeOptimizer(cfg, n, layers)
        self.n = n

    def update(self, delta):
        self.opt.update_hyperparams(delta)

    def step(self, loss_scale, w_fp, w_half, g):
        import msgpack
        import torch

        w_fp_t, w_half_t = torch.from_numpy(w_fp.copy()).cuda(), torch.from_numpy(w_half.view(np.float16).copy()).cuda()
        g_t = torch.from_numpy(g.view(np.float16).copy() if g.dtype == np.uint16 else g).cuda()
        self.opt.step(w_fp_t, w_half_t, g_t, loss_scale)
        torch.cuda.synchronize()
        state = msgpack.unpackb(self.opt.serialize(), raw=False)
        adams = state["nested"] if "nested" in state else [state]
        gather = lambda key, dtype: np.concatenate([np.frombuffer(a[key], dtype=dtype) for a in adams])
        out = {"m1": gather("first_moments_binary", np.float32), "m2": gather("second_moments_binary", np.float32), "steps": gather("param_steps_binary", np.uint32)}
        out = {k: np.concatenate([v, np.zeros(self.n - v.size, dtype=v.dtype)]) for k, v in out.items()}
        return {"w_fp": w_fp_t.cpu().numpy(), "w_half": w_half_t.cpu().numpy().view(np.uint16), **out}


def _device_run(tcnn, oracle, k_host, shape, cfg, what, **kw):
    if shape == "composite":
        n, layers = COMPOSITE_N, COMPOSITE_LAYERS
        slices = [(a, c, {**cfg, **extra}, nm) for a, c, extra, nm in COMPOSITE_SLICES]
        full = {"otype": "Composite", "nested": [{**c_, "n_params_to_optimize": c} for _, c, c_, _ in slices]}
    else:
        n, layers = SHAPES[shape]
        slices, full = ar.one_slice(cfg, n, layers), cfg
    worst, ex = ar.run(slices, n, ar.OracleSide(oracle, full, n, layers), DeviceSide(tcnn, full, n, layers), ar.K_POWF, k_host, what=what, **kw)
    print(f"RATIO {what}: worst error / bound {worst:.4f}")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "uniform", "composite"])
@pytest.mark.parametrize("name", list(ar.OPTION_SETS))
def test_device_against_the_oracle(tcnn, oracle, k_host, name, shape):
    """Every option set on k_adam<false> with its ragged tail, k_adam<true> and k_adam_scalar: half gradients, loss scale 128."""
    _device_run(tcnn, oracle, k_host, shape, ar.OPTION_SETS[name], f"{name}/{shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "uniform"])
def test_device_on_fp32_gradients(tcnn, oracle, k_host, shape):
    """The caller's own fp32 gradients (16-byte quads): the same values, float(g_half), against the oracle's half gradients."""
    _device_run(tcnn, oracle, k_host, shape, ar.FULL, f"full/{shape}/fp32", gradients=ar.half_to_float)


@pytest.mark.gpu
@pytest.mark.parametrize("loss_scale", [100.0, 2.0 ** 17, 2.0 ** -3])
def test_device_at_other_loss_scales(tcnn, oracle, k_host, loss_scale):
    """No power of two, and a power of two beyond the window of the exact reciprocal: g / loss_scale; 2^-3: the reciprocal, above one.
    (What the inputs reach is asserted at the loss scales they were made for, 128 and 100: under 2^17 the unscaled gradients are so small
    that no effective rate comes down to adabound's lower bound.)"""
    _device_run(tcnn, oracle, k_host, "ragged", ar.FULL, f"full/ragged/{loss_scale}", loss_scale=loss_scale, check_exercise=loss_scale == 100.0)


@pytest.mark.gpu
def test_device_with_wide_step_counts(tcnn, oracle, k_host, monkeypatch):
    monkeypatch.setenv("TCNN_AMD_ADAM_STEPS32", "1")
    _device_run(tcnn, oracle, k_host, "ragged", ar.FULL, "full/ragged/steps32")


@pytest.mark.gpu
def test_device_across_a_change_of_the_betas(tcnn, oracle, k_host):
    """update_hyperparams after step 2, on both sides: the debias table is refilled (a stale one is wrong by far more than eps_t: at count 3
    the factor is 0.637 under (0.9, 0.99) and 0.774 under (0.8, 0.95))."""
    _device_run(tcnn, oracle, k_host, "ragged", ar.FULL, "full/ragged/betas", changes={2: ar.MID_RUN_CHANGE})
