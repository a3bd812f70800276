"""Full-precision (fp32) training: Trainer(dtype=torch.float32), the loss on float predictions and the optimizers with fp32 weights.

The chain that holds the numbers: oracle.py <-> tests/train_f32_reference.py on the CPU (bit for bit where the existing tests compare the
optimizers bit for bit), train_f32_reference.py <-> the kernels on the GPU.  A trainer's step is the composition of passes that are pinned
elsewhere: the fp32 module's forward and backward (test_fp32_network.py, test_grid_reference_kernels.py), the loss and the optimizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import train_f32_reference as R
from conftest import ROOT
from grid_reference import U32, check_sum_per_level, gamma
from test_fp32_network import HASHGRID, _create, _net

FP32, FP16 = 0, 1
NEW_SYMBOLS = {
    "tcnn_create_from_config_precision": (C.c_int, [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "tcnn_trainer_precision": (C.c_int, [C.c_void_p]),
    "tcnn_optimizer_create_precision": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "tcnn_optimizer_weight_precision": (C.c_int, [C.c_void_p]),
}

ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}
ADAM_FULL = {**ADAM, "l2_reg": 1e-4, "relative_decay": 0.01, "absolute_decay": 1e-4, "clipping_magnitude": 0.3, "adabound": True}
SGD = {"otype": "SGD", "learning_rate": 1e-2, "l2_reg": 1e-4}
NOVOGRAD = {"otype": "Novograd", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8, "relative_decay": 0.01, "absolute_decay": 1e-4}
NESTED = {"otype": "Ema", "decay": 0.9, "nested": {"otype": "ExponentialDecay", "decay_start": 2, "decay_interval": 1, "decay_base": 0.5, "nested": ADAM}}

# configuration A: no atomics anywhere, so everything is bitwise.  B: the hash grid of test_fp32_network.py in front.
CONFIG_A = {"loss": {"otype": "L2"}, "optimizer": {**ADAM, "epsilon": 1e-8}, "encoding": {"otype": "Frequency", "n_frequencies": 4}, "network": _net(48, 2, "Tanh")}
CONFIG_B = {"loss": {"otype": "RelativeL2"}, "optimizer": ADAM, "encoding": HASHGRID, "network": _net(32, 1, "ReLU")}


# ================================================================================================================== without a GPU
def test_new_c_symbols_are_declared_exported_and_bound(tcnn):
    from tinycudann import _C

    header = open(os.path.join(ROOT, "include", "tcnn_amd.h")).read()
    for name, (restype, argtypes) in NEW_SYMBOLS.items():
        fn = getattr(_C.lib, name)  # AttributeError: the library does not export it
        assert name in _C._SIGNATURES and fn.restype == restype and list(fn.argtypes) == argtypes, name
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert decl is not None and len(decl.group(1).split(",")) == len(argtypes), name
    assert _C.default_loss_scale(FP32) == 1.0 and _C.preferred_precision() == FP16


def test_python_keywords_are_checked_before_any_device_use(tcnn):
    """(where there is no GPU the next thing either constructor does is fail for want of one: the ValueError comes first)"""
    import torch

    for make in (lambda: tcnn.native.Trainer(3, 3, CONFIG_A, dtype=torch.bfloat16), lambda: tcnn.native.create_from_config(3, 3, CONFIG_A, dtype=torch.float64),
                 lambda: tcnn.optimizers.NativeOptimizer(ADAM, 64, [(4, 4)], weight_dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="only supports fp32 or fp16 precision"):
            make()


def test_configuration_errors_need_no_device(tcnn):
    from tinycudann import _C

    def trainer(cfg, precision):
        h = C.c_void_p()
        assert _C.lib.tcnn_create_from_config_precision(3, 3, _C.to_json_bytes(cfg), 1337, precision, C.byref(h)) == 1 and not h.value
        return _C.lib.tcnn_last_error().decode()

    def optimizer(cfg, precision):
        h = C.c_void_p()
        sizes = (C.c_uint32 * 2)(4, 4)
        assert _C.lib.tcnn_optimizer_create_precision(_C.to_json_bytes(cfg), 64, sizes, 1, precision, C.byref(h)) == 1 and not h.value
        return _C.lib.tcnn_last_error().decode()

    assert "FullyFusedMLP can only be used if the network precision is set to __half." in trainer({**CONFIG_A, "network": _net(64, 2, otype="FullyFusedMLP")}, FP32)
    assert "Unknown precision" in trainer(CONFIG_A, 7)
    assert "Invalid optimizer type: Shampoo" in optimizer({"otype": "Shampoo"}, FP32)
    assert "Unknown precision" in optimizer(ADAM, 7)


def _hip_libdir():
    for d in ("/opt/rocm/lib",):
        if os.path.exists(os.path.join(d, "libamdhip64.so")):
            return d
    import torch

    return os.path.join(os.path.dirname(torch.__file__), "lib")


def _compile(tmp_dir, name):
    """the recipe of test_cpp_api.py: plain g++, C++14, against include/, linked with the library"""
    out = str(tmp_dir / name)
    libdir, hip = os.path.join(ROOT, "tiny-cuda-nn_amd"), _hip_libdir()
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-O1", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), f"-L{libdir}",
                           "-ltcnn_amd", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{hip}", f"-Wl,-rpath-link,{hip}", "-o", out])
    return out


@pytest.fixture(scope="module")
def trainer_f32_binary(tcnn, tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("cpp_f32"), "trainer_f32_api")


def test_cpp_header_api_compiles_with_the_fp32_surfaces(tcnn, trainer_f32_binary, tmp_path):
    r = subprocess.run([trainer_f32_binary, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host checks ok" in r.stdout, r.stdout + r.stderr
    _compile(tmp_path, "header_api")  # the unchanged caller of the half surface still compiles, warnings as errors


def test_cpp_mixed_trainer_parameters_do_not_compile(tcnn, tmp_path):
    src = tmp_path / "mixed.cpp"
    src.write_text("#include <tiny-cuda-nn/config.h>\nint main() { return sizeof(tcnn::Trainer<float, tcnn::half, float>) > 0 ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "both half or both float" in r.stderr


# ---- the yardstick against the oracle
N_OPT, N_MATRIX, LAYERS = 4099, 2048, [(32, 64)]  # not a multiple of 4: a ragged last quad


def _gradients(oracle, step, half):
    """pcg32 gradients, every third non-matrix one exactly zero; half: rounded to half (what the oracle's optimizers take)"""
    g = oracle.Pcg32(11 + step).uniform_strided(N_OPT, -4.0, 4.0).astype(np.float32)
    g[N_MATRIX + step::3] = 0.0
    return oracle.half_to_f32(oracle.half_bits(g)) if half else g


def _start_weights(oracle):
    return oracle.Pcg32(5).uniform_strided(N_OPT, -0.5, 0.5).astype(np.float32)


def _composite_unaligned(inner):
    """slice offsets that are no multiples of 4 (2048 + 333; the last 5 parameters belong to nobody)"""
    return {"otype": "Composite", "nested": [{**SGD, "n_params_to_optimize": N_MATRIX}, {**inner, "n_params_to_optimize": 333},
                                             {"otype": "Ema", "decay": 0.9, "nested": inner, "n_params_to_optimize": N_OPT - N_MATRIX - 333 - 5}]}


WRAPPED_SGD = {"average": {"otype": "Average", "n_samples": 3, "nested": SGD}, "batched": {"otype": "Batched", "batch_size_multiplier": 2, "nested": SGD},
               "lookahead": {"otype": "Lookahead", "alpha": 0.25, "n_steps": 2, "nested": SGD},
               "ema_sgd": {"otype": "Ema", "decay": 0.9, "nested": SGD}, "composite_sgd": _composite_unaligned(SGD)}
# the optimizers whose comparison with the oracle is bitwise in tests/test_optimizers.py (SGD and the wrappers around it), and the ones held
# under that file's bar, max|got - ref| <= 1e-5 max|update| + 1e-9 (Adam: powf; Novograd: a sum whose order is not specified)
BITWISE = {"sgd": SGD, **WRAPPED_SGD}
BARRED = {"adam": ADAM, "adam_full": ADAM_FULL, "novograd": NOVOGRAD, "nested": NESTED, "composite": _composite_unaligned(ADAM)}


def _run_restatement(oracle, cfg, wdtype, gdtype, steps=4, half_gradients=False):
    opt = R.create_optimizer(cfg, wdtype, gdtype)
    opt.allocate(N_OPT, LAYERS)
    w_fp = _start_weights(oracle)
    w = w_fp.astype(np.float16) if wdtype == np.float16 else None
    for step in range(steps):
        opt.step(128.0 if half_gradients else 1.0, w_fp, w, _gradients(oracle, step, half_gradients))
    return opt, w_fp, w


@pytest.mark.parametrize("name", list(BITWISE) + list(BARRED))
def test_restatement_reproduces_the_oracles_optimizers(oracle, name):
    """weight dtype half, half gradients at loss scale 128, 4 steps: master weights, half weights and custom weights"""
    cfg = {**BITWISE, **BARRED}[name]
    ref = oracle.create_optimizer(cfg)
    ref.allocate(N_OPT, LAYERS)
    w_fp0 = _start_weights(oracle)
    w_fp, w_h = w_fp0.copy(), oracle.half_bits(w_fp0)
    for step in range(4):
        ref.step(128.0, w_fp, w_h, oracle.half_bits(_gradients(oracle, step, True)))
    opt, got_fp, got_h = _run_restatement(oracle, cfg, np.float16, np.float16, half_gradients=True)
    assert not np.array_equal(w_fp, w_fp0)
    if name in BITWISE:
        assert np.array_equal(got_fp.view(np.uint32), w_fp.view(np.uint32)) and np.array_equal(got_h.view(np.uint16), w_h)
        if ref.custom_weights() is not None:
            assert np.array_equal(opt.custom_weights().view(np.uint16), ref.custom_weights())
    else:
        upd = float(np.max(np.abs(w_fp - w_fp0)))
        err = float(np.max(np.abs(got_fp - w_fp)))
        print(f"restatement vs oracle {name}: max|diff| {err:.3g}, max|update| {upd:.3g}, bitwise {np.array_equal(got_fp.view(np.uint32), w_fp.view(np.uint32))}")
        assert upd > 0 and err <= 1e-5 * upd + 1e-9


def _loss_inputs(oracle, loss, n=256, dims=3, stride=16):
    """predictions that are exactly half-representable (positive where the loss takes a logarithm or divides by them), targets, a pdf"""
    pred = oracle.Pcg32(21).uniform_strided(n * stride, 0.05 if loss in ("CrossEntropy", "Variance") else -2.0, 2.0).reshape(n, stride)
    pred = oracle.half_to_f32(oracle.half_bits(pred))
    target = oracle.Pcg32(22).uniform_strided(n * dims, 0.05 if loss in ("CrossEntropy", "Variance") else -2.0, 2.0).reshape(n, dims).astype(np.float32)
    pdf = oracle.Pcg32(23).uniform_strided(n * dims, 0.25, 2.0).reshape(n, dims).astype(np.float32)
    return pred, target, pdf


@pytest.mark.parametrize("loss", R.LOSSES)
def test_restatement_reproduces_the_oracles_loss(oracle, loss):
    """the float loss on half-representable predictions: the oracle's values, and gradients whose rounding to half gives the oracle's bits --
    at loss scales 128 and 1, with and without data_pdf, and RelativeL2Luminance's dims >= 6 branch"""
    for dims in (3, 6) if loss == "RelativeL2Luminance" else (3,):
        pred, target, pdf = _loss_inputs(oracle, loss, dims=dims)
        for loss_scale in (128.0, 1.0):
            for data_pdf in (None, pdf):
                want_v, want_g = oracle.loss_evaluate(loss, oracle.half_bits(pred), target, loss_scale, data_pdf)
                got_v, got_g = R.loss(loss, pred, target, loss_scale, data_pdf)
                what = f"{loss} dims {dims} loss scale {loss_scale} pdf {data_pdf is not None}"
                if loss == "CrossEntropy":  # logf is not correctly rounded: both within the device allowance of the float64 value
                    v64 = R.loss_float64(loss, pred, target, data_pdf)
                    for v in (want_v, got_v):
                        assert np.all(np.abs(v[:, :dims].astype(np.float64) - v64) <= 4 * 2.0 ** -24 * np.abs(v64)), what
                        assert not np.any(v[:, dims:])
                else:
                    assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), what
                with np.errstate(over="ignore"):
                    assert np.array_equal(got_g.astype(np.float16).view(np.uint16), want_g), what
                assert np.any(got_g != 0) and not np.any(got_g[:, dims:])


# ======================================================================================================================= on the GPU
def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert got.shape == want.shape and not np.any(differ), (
        f"{what}: {int(np.count_nonzero(differ))} of {differ.size} values differ, first at {tuple(np.argwhere(differ)[0])}: got {got[differ][0]!r}, want {want[differ][0]!r}")


def _batch(oracle, n, n_in, n_out, seed=42, positive=False):
    x = oracle.Pcg32(seed).uniform_strided(n * n_in).reshape(n, n_in).astype(np.float32)
    t = oracle.Pcg32(seed + 1).uniform_strided(n * n_out, 0.05 if positive else -1.0, 1.0).reshape(n, n_out).astype(np.float32)
    pdf = oracle.Pcg32(seed + 2).uniform_strided(n * n_out, 0.25, 2.0).reshape(n, n_out).astype(np.float32)
    return x, t, pdf


# ---------------------------------------------------------------------------------------------------------------- 1. the loss
LOSS_CASES = [(l, 3) for l in R.LOSSES] + [("RelativeL2Luminance", 6)]


@pytest.mark.gpu
@pytest.mark.parametrize("loss,dims", LOSS_CASES, ids=[f"{l}-{d}" for l, d in LOSS_CASES])
def test_loss_on_float_predictions(tcnn, oracle, loss, dims):
    """Identity(3) -> CutlassMLP 32 x 1 -> dims outputs, n = 512, through Trainer.forward with data_pdf, at loss scales 1 and 128: ctx.L and
    ctx.dL_doutput are the restatement applied to the GPU's own ctx.output, bit for bit; padded columns exactly zero; CrossEntropy's value
    within 4 * 2^-24 of the float64 value; Trainer.loss within gamma(n) * sum |L| of the exact sum.
    (Every network pads its output to a multiple of 16, so the four-elements-per-thread kernel runs here; the one-element form k_loss<float>
    takes strides that are no multiple of 4, which no network produces: no case of this test can reach it.)"""
    import torch

    positive = loss in ("CrossEntropy", "Variance")
    cfg = {"loss": {"otype": loss}, "optimizer": ADAM, "encoding": {"otype": "Identity"}, "network": _net(32, 1, "ReLU", "Exponential" if positive else "None")}
    n = 512
    tr = tcnn.native.Trainer(3, dims, cfg, seed=1337, dtype=torch.float32)
    x, t, pdf = _batch(oracle, n, 3, dims, positive=positive)
    for loss_scale in (1.0, 128.0):
        ctx = tr.forward(_t(x), _t(t), loss_scale=loss_scale, data_pdf=_t(pdf))
        out, L, dy = ctx.output(), ctx.L(), ctx.dL_doutput()
        assert out.dtype == dy.dtype == L.dtype == torch.float32 and tuple(out.shape) == (n, 16)
        out, L, dy = out.cpu().numpy(), L.cpu().numpy(), dy.cpu().numpy()
        want_L, want_dy = R.loss(loss, out, t, loss_scale, pdf)
        what = f"{loss} dims {dims} loss scale {loss_scale}"
        if loss == "CrossEntropy":
            v64 = R.loss_float64(loss, out, t, pdf)
            worst = float(np.max(np.abs(L[:, :dims].astype(np.float64) - v64) / np.abs(v64)))
            print(f"{what}: worst |L - v64| / |v64| = {worst / 2.0 ** -24:.3f} u")
            assert worst <= 4 * 2.0 ** -24
        else:
            _same_bits(L, want_L, what + " L")
        _same_bits(dy, want_dy, what + " dL_doutput")
        assert not np.any(L[:, dims:].view(np.uint32)) and not np.any(dy[:, dims:].view(np.uint32)) and np.any(dy[:, :dims] != 0)
        S, A = float(np.sum(L.astype(np.float64))), float(np.sum(np.abs(L.astype(np.float64))))
        got = tr.loss(ctx)
        assert abs(got - S) <= float(gamma(L.size, U32)) * A, (what, got, S)


# ---------------------------------------------------------------------------------------------------------------- 2. optimizers
OPT_CASES = {"adam": ADAM, "adam_full": ADAM_FULL, "sgd": SGD, "novograd": NOVOGRAD, "nested": NESTED, "average": WRAPPED_SGD["average"], "batched": WRAPPED_SGD["batched"],
             "lookahead": WRAPPED_SGD["lookahead"], "composite": _composite_unaligned(ADAM), "composite_sgd": WRAPPED_SGD["composite_sgd"]}
# (Batched's half pool exists only beside half weights)
WEIGHT_TYPED_BLOBS = ("weights_ema_binary", "weights_samples_binary", "weights_average_binary", "weights_lookahead_binary", "averaged_gradients_half_binary")


def _state(opt):
    import msgpack

    return msgpack.unpackb(opt.serialize(), raw=False)


def _same_state(a, b, path="state"):
    """snapshot objects equal everywhere but in the blobs that hold weights of the optimizer's own precision"""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert set(a) - set(WEIGHT_TYPED_BLOBS) == set(b) - set(WEIGHT_TYPED_BLOBS), path
        for k in set(a) - set(WEIGHT_TYPED_BLOBS):
            _same_state(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _same_state(u, v, f"{path}[{i}]")
    else:
        assert a == b, path


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OPT_CASES))
def test_fp32_weight_optimizers(tcnn, oracle, name):
    import torch

    cfg = OPT_CASES[name]
    NO = tcnn.optimizers.NativeOptimizer
    full, half = NO(cfg, N_OPT, LAYERS, weight_dtype=torch.float32), NO(cfg, N_OPT, LAYERS)
    from tinycudann import _C

    assert _C.lib.tcnn_optimizer_weight_precision(full._h) == FP32 and _C.lib.tcnn_optimizer_weight_precision(half._h) == FP16
    w0 = _start_weights(oracle)
    w32, w16_fp, w16 = _t(w0), _t(w0), _t(w0).half()
    for step in range(4):
        g = _t(_gradients(oracle, step, False))
        full.step(w32, None if step % 2 else w32, g, 1.0)  # weights: null, or the master vector itself
        half.step(w16_fp, w16, g, 1.0)
    torch.cuda.synchronize()
    assert full.step_count() == half.step_count() and not np.array_equal(_u32(w32), w0.view(np.uint32))
    # (a) the master-weight arithmetic is the existing one: bit-identical to the half-weight optimizer fed the same fp32 gradients
    # (Lookahead pulls the master weights towards slow weights it keeps in its own precision: not comparable)
    if name != "lookahead":
        _same_bits(w32.cpu().numpy(), w16_fp.cpu().numpy(), f"{name}: master weights, fp32-weight against half-weight optimizer")
        _same_state(_state(full), _state(half))  # moments, step counts, pools, learning rates
    # (b) against the restatement
    ref, want, _ = _run_restatement(oracle, cfg, np.float32, np.float32)
    got = w32.cpu().numpy()
    custom, want_custom = full.custom_weights(), ref.custom_weights()
    assert (custom is None) == (want_custom is None) and (custom is None or custom.dtype == torch.float32)
    if name in BITWISE:
        _same_bits(got, want, f"{name}: weights against the restatement")
        if custom is not None:
            _same_bits(custom.cpu().numpy(), want_custom, f"{name}: custom weights against the restatement")
    else:
        upd = float(np.max(np.abs(want - w0)))
        err = float(np.max(np.abs(got - want)))
        print(f"{name}: max|got - ref| {err:.3g}, bar {1e-5 * upd + 1e-9:.3g}")
        assert upd > 0 and err <= 1e-5 * upd + 1e-9
        if name.startswith("composite"):
            _same_bits(got[:N_MATRIX], want[:N_MATRIX], f"{name}: the SGD slice")
            _same_bits(got[-5:], w0[-5:], f"{name}: the parameters behind the last slice")
        if custom is not None:
            # the same bar: the EMA is a debiased convex combination of the weights seen, evaluated with the same IEEE operations on both sides
            err_custom = float(np.max(np.abs(custom.cpu().numpy() - want_custom)))
            print(f"{name}: custom weights max|got - ref| {err_custom:.3g}, bar {1e-5 * upd + 1e-9:.3g}")
            assert err_custom <= 1e-5 * upd + 1e-9
    # (c) serialize -> a fresh fp32 optimizer -> the same next step
    resumed = NO(cfg, N_OPT, LAYERS, weight_dtype=torch.float32)
    resumed.deserialize(full.serialize())
    w_resumed = w32.clone()
    resumed.weights_restored(w_resumed)
    g = _t(_gradients(oracle, 4, False))
    full.step(w32, None, g, 1.0)
    resumed.step(w_resumed, None, g, 1.0)
    torch.cuda.synchronize()
    _same_bits(w_resumed.cpu().numpy(), w32.cpu().numpy(), f"{name}: the step after a snapshot round trip")
    if custom is not None:
        _same_bits(resumed.custom_weights().cpu().numpy(), full.custom_weights().cpu().numpy(), f"{name}: custom weights after a snapshot round trip")


@pytest.mark.gpu
def test_fp32_weight_optimizer_refusals(tcnn, oracle):
    import torch

    NO = tcnn.optimizers.NativeOptimizer
    full, half = NO(NESTED, N_OPT, LAYERS, weight_dtype=torch.float32), NO(NESTED, N_OPT, LAYERS)
    w = _t(_start_weights(oracle))
    g = _t(_gradients(oracle, 0, False))
    half.step(w.clone(), w.half(), g, 1.0)
    with pytest.raises(RuntimeError, match="wrong size"):  # half EMA weights are never reinterpreted as floats
        full.deserialize(half.serialize())
    with pytest.raises(RuntimeError, match="gradients must be fp32"):
        full.step(w, None, g.half(), 1.0)
    with pytest.raises(RuntimeError, match="one weight vector"):
        full.step(w, w.half(), g, 1.0)
    with pytest.raises(RuntimeError, match="one weight vector"):
        full.step_unchecked(w, w.clone(), g, 1.0)
    assert full.step_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 3. the trainer
def _module_passes(tcnn, n_in, n_out, cfg, x, params, dy, max_level=None):
    """forward (with input gradients) and backward of the fp32 C-ABI module on the given parameters"""
    native = _create(tcnn, n_in, n_out, cfg["network"], FP32, cfg["encoding"])
    if max_level is not None:
        native.set_max_level(max_level)
    xt, pt = _t(x).requires_grad_(True), params.clone().requires_grad_(True)
    ctx, out = native.fwd(xt, pt)
    if dy is None:
        return out.detach().cpu().numpy(), None, None
    dx, dp = native.bwd(ctx, xt, pt, out, dy)
    return out.detach().cpu().numpy(), dx.detach().cpu().numpy(), dp.detach().cpu().numpy()


@pytest.mark.gpu
def test_trainer_composition_without_atomics(tcnn, oracle):
    """configuration A at n = 512: everything bit for bit"""
    import torch

    T = tcnn.native
    n = 512
    x, t, _ = _batch(oracle, n, 3, 3)
    xt, tt = _t(x), _t(t)
    tr = T.Trainer(3, 3, CONFIG_A, seed=1337, dtype=torch.float32)
    assert tr.dtype == torch.float32 and tr.params().dtype == torch.float32
    from tinycudann import _C

    assert _C.lib.tcnn_trainer_precision(tr._h) == FP32 and _C.lib.tcnn_trainer_params(tr._h) == _C.lib.tcnn_trainer_params_full_precision(tr._h)
    _same_bits(tr.params_full_precision().cpu().numpy(), T.Trainer(3, 3, CONFIG_A, seed=1337).params_full_precision().cpu().numpy(), "initial parameters, fp32 against half trainer")
    with pytest.raises(TypeError, match="inference"):
        tr.inference_half(xt)
    # forward and backward are the module's
    ctx = tr.forward(xt, tt, prepare_input_gradients=True)
    dx = torch.zeros(n, 3, device="cuda")
    tr.backward(ctx, xt, dL_dinput=dx)
    g = tr.param_gradients()
    assert g.dtype == torch.float32
    out_m, dx_m, dp_m = _module_passes(tcnn, 3, 3, CONFIG_A, x, tr.params(), ctx.dL_doutput())
    _same_bits(ctx.output().cpu().numpy(), out_m, "ctx.output against the module's forward")
    _same_bits(g.cpu().numpy(), dp_m, "parameter gradients against the module's backward")
    _same_bits(dx.cpu().numpy(), dx_m, "dL_dinput against the module's backward")
    assert np.any(dp_m != 0) and np.any(dx_m != 0)
    # Accumulate after Overwrite: exactly twice
    tr.backward(ctx, xt, gradient_mode=T.GRADIENT_ACCUMULATE)
    _same_bits(tr.param_gradients().cpu().numpy(), 2 * g.cpu().numpy(), "Accumulate after Overwrite")
    # a float external_dL_dy reproduces the loss-driven gradients
    ctx2 = tr.forward(xt, None, external_dL_dy=ctx.dL_doutput())
    tr.backward(ctx2, xt)
    _same_bits(tr.param_gradients().cpu().numpy(), g.cpu().numpy(), "gradients from external_dL_dy")
    with pytest.raises(TypeError, match="external_dL_dy"):
        tr.forward(xt, None, external_dL_dy=ctx.dL_doutput().half())
    # Ignore leaves the gradients alone
    tr.backward(ctx, xt, gradient_mode=T.GRADIENT_IGNORE)
    _same_bits(tr.param_gradients().cpu().numpy(), g.cpu().numpy(), "gradients after an Ignore pass")
    # training_step is forward + backward + optimizer_step at loss scale 1
    a, b = T.Trainer(3, 3, CONFIG_A, seed=7, dtype=torch.float32), T.Trainer(3, 3, CONFIG_A, seed=7, dtype=torch.float32)
    for _ in range(2):
        ctx_a = a.training_step(xt, tt)
        ctx_b = b.forward(xt, tt)
        b.backward(ctx_b, xt)
        b.optimizer_step(1.0)
    assert a.last_step_kernel() == "unfused" and a.optimizer_step_count() == b.optimizer_step_count() == 2
    assert a.params_updated_in_flush() == 0 and a.optimizer_prologue_steps() == 0
    _same_bits(a.params().cpu().numpy(), b.params().cpu().numpy(), "training_step against its pieces")
    _same_bits(ctx_a.L().cpu().numpy(), ctx_b.L().cpu().numpy(), "L of the second step")
    assert a.loss(ctx_a) == b.loss(ctx_b)
    # inference is the module's forward, trimmed; set_params takes floats
    y = a.inference(xt)
    out_m, _, _ = _module_passes(tcnn, 3, 3, CONFIG_A, x, a.params(), None)
    _same_bits(y.cpu().numpy(), out_m[:, :3], "inference against the module's forward")
    c = T.Trainer(3, 3, CONFIG_A, seed=99, dtype=torch.float32)
    c.set_params(a.params())
    assert torch.equal(c.inference(xt), y) and torch.equal(c.params_full_precision(), a.params())
    _C.check(_C.lib.tcnn_trainer_initialize_params(c._h))  # (re-initialise: continues the rng stream)
    assert not torch.equal(c.params(), a.params())
    c.update_hyperparams({"optimizer": {"learning_rate": 0.5}})
    assert c.hyperparams()["optimizer"]["learning_rate"] == 0.5


@pytest.mark.gpu
def test_trainer_inference_parameters_are_the_ema_floats(tcnn, oracle):
    import torch

    T = tcnn.native
    x, t, _ = _batch(oracle, 512, 3, 3)
    xt, tt = _t(x), _t(t)
    for opt in ({"otype": "Ema", "decay": 0.9, "nested": CONFIG_A["optimizer"]}, {"otype": "Average", "n_samples": 2, "nested": SGD}, {"otype": "Lookahead", "alpha": 0.5, "n_steps": 2, "nested": SGD}):
        tr = T.Trainer(3, 3, {**CONFIG_A, "optimizer": opt}, seed=1337, dtype=torch.float32)
        for _ in range(3):
            tr.training_step(xt, tt)
        ema = tr.params_inference()
        assert ema.dtype == torch.float32 and not torch.equal(ema, tr.params())
        y = tr.inference(xt)  # (use_inference_params)
        other = T.Trainer(3, 3, CONFIG_A, seed=1, dtype=torch.float32)
        other.set_params(ema)
        assert torch.equal(other.inference(xt), y), opt["otype"]
        other.set_params(tr.params())
        assert not torch.equal(other.inference(xt), y)
        # a training step with use_inference_params evaluates them too
        ctx = tr.training_step(xt, tt, run_optimizer=False, use_inference_params=True)
        assert torch.equal(ctx.output()[:, :3], y)


@pytest.mark.gpu
def test_trainer_composition_with_a_hash_grid(tcnn, oracle):
    """configuration B at n = 512: output, the network's gradients and dL_dinput bit for bit against the module; the grid's gradients -- float
    atomics, an order that is not defined -- per parameter within gamma(k - 1) * sum |term| of the exact sum of the oracle's terms"""
    import torch

    import oracle as orc

    T = tcnn.native
    n = 512
    x, t, _ = _batch(oracle, n, 3, 1)
    xt, tt = _t(x), _t(t)
    tr = T.Trainer(3, 1, CONFIG_B, seed=1337, dtype=torch.float32)
    _same_bits(tr.params_full_precision().cpu().numpy(), T.Trainer(3, 1, CONFIG_B, seed=1337).params_full_precision().cpu().numpy(), "initial parameters, fp32 against half trainer")
    with torch.no_grad():  # grid entries start at +-1e-4: give the gradients something to see
        p = tr.params().clone()
        n_net = 32 * 16 + 16 * 32
        p[n_net:] = _t(oracle.Pcg32(3).uniform_strided(p.numel() - n_net, -1.0, 1.0).astype(np.float32))
        tr.set_params(p)
    ctx = tr.forward(xt, tt, prepare_input_gradients=True)
    dx = torch.zeros(n, 3, device="cuda")
    tr.backward(ctx, xt, dL_dinput=dx)
    g = tr.param_gradients().cpu().numpy()
    out_m, dx_m, dp_m = _module_passes(tcnn, 3, 1, CONFIG_B, x, tr.params(), ctx.dL_doutput())
    _same_bits(ctx.output().cpu().numpy(), out_m, "ctx.output against the module's forward")
    _same_bits(g[:n_net], dp_m[:n_net], "the network's gradients against the module's backward")
    _same_bits(dx.cpu().numpy(), dx_m, "dL_dinput against the module's backward")
    # the grid part: dL/d(encoded batch) from the network alone, on the oracle's encoded batch (the same bits, padding included: the output
    # it gives must be the trainer's), then the oracle's terms
    ref = orc.create_encoding(3, HASHGRID, alignment=0)
    ref.n_to_pad = 16 - ref.n_output_dims
    params = tr.params().cpu().numpy()
    encoded, _ = ref.forward_f32(x, params[n_net:])
    net = _create(tcnn, 16, 1, CONFIG_B["network"], FP32)
    et, pt = _t(encoded).requires_grad_(True), _t(params[:n_net]).requires_grad_(True)
    nctx, nout = net.fwd(et, pt)
    _same_bits(nout.detach().cpu().numpy(), out_m, "the network on the oracle's encoded batch")
    dE, _ = net.bwd(nctx, et, pt, nout, ctx.dL_doutput())
    terms = ref.backward_terms(x, dE.detach().cpu().numpy(), orc.PRODUCT_FP32)
    for what, grid in (("trainer", g[n_net:]), ("module", dp_m[n_net:])):
        records = check_sum_per_level(ref, (grid.astype(np.float64), grid.view(np.uint32)), terms, U32, label=f"configuration B grid gradients ({what})")
        assert len(records) == 4 and np.any(grid != 0)
    # a scalar max_level zeroes what it zeroes on the module
    tr.set_max_level(0.5)
    ctx_half = tr.forward(xt, tt)
    out_half, _, _ = _module_passes(tcnn, 3, 1, CONFIG_B, x, tr.params(), None, max_level=0.5)
    _same_bits(ctx_half.output().cpu().numpy(), out_half, "ctx.output under max_level 0.5")
    assert tr.max_level == 0.5 and not np.array_equal(out_half, out_m)
    tr.backward(ctx_half, xt)
    g_half = tr.param_gradients().cpu().numpy()[n_net:]
    off = ref.offsets.astype(np.int64) * 2
    assert np.any(g_half[: off[2]] != 0) and not np.any(g_half[off[3]:].view(np.uint32))  # levels 0, 1 live; level 3 receives nothing
    # per sample: rows alternate between every level and none
    per_sample = torch.where(torch.arange(n, device="cuda") % 2 == 0, 1000.0, 0.0).float().contiguous()
    tr.set_max_level_gpu(per_sample)
    mixed = tr.forward(xt, tt).output().cpu().numpy()
    tr.set_max_level_gpu(None)
    tr.set_max_level(1000.0)
    _same_bits(mixed[::2], out_m[::2], "rows with every level under a per-sample max_level")
    assert not np.array_equal(mixed[1::2], out_m[1::2])
    with pytest.raises(RuntimeError, match="holds 512 values"):
        tr.set_max_level_gpu(per_sample)
        tr.forward(_t(np.concatenate([x, x])), _t(np.concatenate([t, t])))
    tr.set_max_level_gpu(None)


# ---------------------------------------------------------------------------------------------------------------- 4. snapshots
@pytest.mark.gpu
def test_snapshots(tcnn, oracle):
    import msgpack
    import torch

    T = tcnn.native
    x, t, _ = _batch(oracle, 512, 3, 3)
    xt, tt = _t(x), _t(t)
    cfg = {**CONFIG_A, "optimizer": {"otype": "Ema", "decay": 0.9, "nested": CONFIG_A["optimizer"]}}
    tr = T.Trainer(3, 3, cfg, seed=1337, dtype=torch.float32)
    for _ in range(2):
        tr.training_step(xt, tt)
    blob = tr.serialize(True)
    snap = msgpack.unpackb(blob, raw=False)
    n = tr.n_params
    assert snap["params_type"] == "float" and snap["n_params"] == n and len(snap["params_binary"]) == 4 * n
    _same_bits(np.frombuffer(snap["params_binary"], dtype=np.float32), tr.params_inference().cpu().numpy(), "params_binary: the inference parameters")  # trainer.h:281
    assert len(snap["optimizer"]["weights_ema_binary"]) == 4 * n and snap["optimizer"]["nested"]["current_step"] == 2
    # A snapshot carries the inference parameters (the EMA floats) as its parameters, so a restored trainer trains on from those.  The
    # yardstick is therefore the original, never restored, with its parameters set to its EMA by set_params: its optimizer state
    # (moments, step counts, EMA) is what the two steps left, and a restore that lost any of it would take another third step.
    fresh = T.Trainer(3, 3, cfg, seed=5, dtype=torch.float32)
    fresh.deserialize(blob)
    tr.set_params(tr.params_inference())
    _same_bits(fresh.params().cpu().numpy(), np.frombuffer(snap["params_binary"], dtype=np.float32), "parameters after deserialize")
    assert torch.equal(fresh.params_inference(), tr.params_inference()) and fresh.optimizer_step_count() == 2
    for trainer in (tr, fresh):
        trainer.training_step(xt, tt)
    _same_bits(fresh.params().cpu().numpy(), tr.params().cpu().numpy(), "the third step after a restore")
    _same_bits(fresh.params_inference().cpu().numpy(), tr.params_inference().cpu().numpy(), "the EMA after the third step")
    # across precisions: the parameters alone (optimizer state holds weights of its own precision and is never reinterpreted)
    floats = tr.serialize(False)
    half = T.Trainer(3, 3, cfg, seed=6)
    half.deserialize(floats)
    _same_bits(half.params_full_precision().cpu().numpy(), tr.params_inference().cpu().numpy(), "an fp32 snapshot in a half trainer")
    assert torch.equal(half.params(), tr.params_inference().half())
    halves = half.serialize(False)
    assert msgpack.unpackb(halves, raw=False)["params_type"] == "__half"
    back = T.Trainer(3, 3, cfg, seed=8, dtype=torch.float32)
    back.deserialize(halves)
    assert torch.equal(back.params(), half.params().float()) and torch.equal(back.params_inference(), half.params().float())
    with pytest.raises(RuntimeError, match="wrong size"):
        back.deserialize(half.serialize(True))
    with pytest.raises(RuntimeError, match="wrong size"):
        half.deserialize(blob)


# ---------------------------------------------------------------------------------------------------------------- 5. learning
@pytest.mark.gpu
def test_fp32_trainer_learns(tcnn, oracle):
    """configuration B on sin(2 pi x) cos(2 pi y) z, n = 4096, 100 steps: every loss finite, the last below the first; the half trainer runs the
    same data and both curves go to profiles/fp32_training_curves.json when TCNN_WRITE_PROFILES=1 (no ratio between them is asserted)"""
    import json

    import torch

    n = 4096
    x = oracle.Pcg32(77).uniform_strided(n * 3).reshape(n, 3).astype(np.float32)
    t = (np.sin(2 * np.pi * x[:, 0]) * np.cos(2 * np.pi * x[:, 1]) * x[:, 2]).astype(np.float32).reshape(n, 1)
    xt, tt = _t(x), _t(t)
    curves = {}
    for name, dtype in (("fp32", torch.float32), ("half", None)):
        tr = tcnn.native.Trainer(3, 1, CONFIG_B, seed=1337, dtype=dtype)
        contexts = [tr.training_step(xt, tt) for _ in range(100)]
        curves[name] = [tr.loss(c) for c in contexts[::3] + [contexts[-1]]]
    print("fp32 training curve:", " ".join(f"{v:.4g}" for v in curves["fp32"]))
    print("half training curve:", " ".join(f"{v:.4g}" for v in curves["half"]))
    assert all(np.isfinite(v) for v in curves["fp32"]) and curves["fp32"][-1] < curves["fp32"][0]
    assert all(np.isfinite(v) for v in curves["half"])
    if os.environ.get("TCNN_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "fp32_training_curves.json"), "w") as f:
            json.dump({"config": CONFIG_B, "n": n, "steps": 100, "loss_every_third_step_and_last": curves}, f, indent=1)


# ---------------------------------------------------------------------------------------------------------------- 6. the half path
@pytest.mark.gpu
def test_half_trainer_is_untouched_by_an_fp32_one(tcnn, oracle):
    import torch

    from test_gpu_parity import CONFIG_C3B

    def three_steps():
        tr = tcnn.native.Trainer(2, 3, CONFIG_C3B, seed=1337)
        for s in range(3):
            x, t = oracle.synthetic_batch(1024, 2, 3, seed=100 + s)
            tr.training_step(_t(x), _t(t))
        return tr.params().cpu().numpy().view(np.uint16), tr.params_full_precision().cpu().numpy().view(np.uint32), tr.last_step_kernel()

    before = three_steps()
    f = tcnn.native.Trainer(3, 1, CONFIG_B, seed=1, dtype=torch.float32)
    x, t, _ = _batch(oracle, 512, 3, 1)
    f.training_step(_t(x), _t(t))
    assert f.last_step_kernel() == "unfused"
    after = three_steps()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2] != "unfused"


# ---------------------------------------------------------------------------------------------------------------- 7. C++
@pytest.mark.gpu
def test_cpp_fp32_trainer_trains(trainer_f32_binary):
    r = subprocess.run([trainer_f32_binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gpu checks ok" in r.stdout, r.stdout + r.stderr
