"""The standalone optimizer handle of the C ABI (tcnn_optimizer_*, include/tcnn_amd.h): the optimizers a Trainer runs, stepped by a
caller on its own parameter and gradient vectors, with half gradients (scaled by the loss scale) or fp32 ones.

Scheme of test_optimizers.py::_drive: pcg32 gradients on the C3B parameter vector, every third grid gradient zero.  The fp32 form
gets float(g_half) / 128 with loss scale 1 -- a half times 2^-7 is exact in fp32 -- so both forms and the Trainer see the same
unscaled gradient and run the same adam_one / k_sgd / k_novo_* arithmetic: everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

from test_optimizers import NESTED, _composite

ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}
SGD = {"otype": "SGD", "learning_rate": 1e-2, "l2_reg": 1e-4}
NOVOGRAD = {"otype": "Novograd", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8, "relative_decay": 0.01, "absolute_decay": 1e-4}
LOSS_SCALE = 128.0

NEW_SYMBOLS = {
    "tcnn_module_layer_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "tcnn_optimizer_create": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_void_p)]),
    "tcnn_optimizer_destroy": (None, [C.c_void_p]),
    "tcnn_optimizer_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "tcnn_optimizer_step_count": (C.c_uint32, [C.c_void_p]),
    "tcnn_optimizer_n_params": (C.c_size_t, [C.c_void_p]),
    "tcnn_optimizer_learning_rate": (C.c_float, [C.c_void_p]),
    "tcnn_optimizer_set_learning_rate": (C.c_int, [C.c_void_p, C.c_float]),
    "tcnn_optimizer_update_hyperparams": (C.c_int, [C.c_void_p, C.c_char_p]),
    "tcnn_optimizer_hyperparams": (C.c_char_p, [C.c_void_p]),
    "tcnn_optimizer_custom_weights": (C.c_void_p, [C.c_void_p]),
    "tcnn_optimizer_weights_restored": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tcnn_optimizer_serialize": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "tcnn_optimizer_deserialize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
}


# ---------------------------------------------------------------------------------------------------------------- without a GPU
def test_c_abi_exports_the_optimizer_entry_points(tcnn):
    import os
    import re

    from conftest import ROOT
    from tinycudann import _C

    header = open(os.path.join(ROOT, "include", "tcnn_amd.h")).read()
    for name, (restype, argtypes) in NEW_SYMBOLS.items():
        fn = getattr(_C.lib, name)  # AttributeError: the library does not export it
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert decl is not None, f"{name} is not declared in tcnn_amd.h"
        assert len(decl.group(1).split(",")) == len(argtypes), name
    assert "typedef struct tcnn_optimizer_s* tcnn_optimizer_t;" in header


def test_create_reports_a_bad_configuration_without_a_device(tcnn):
    from tinycudann import _C

    sizes = (C.c_uint32 * 2)(4, 4)
    for cfg, message in (({"otype": "Shampoo"}, "Invalid optimizer type: Shampoo"),
                         ({"otype": "Composite", "nested": {"otype": "Adam"}}, "Must provide an array of nested"),
                         ({"otype": "Ema", "nested": {"otype": "Shampoo"}}, "Invalid optimizer type: Shampoo")):
        h = C.c_void_p()
        assert _C.lib.tcnn_optimizer_create(_C.to_json_bytes(cfg), 64, sizes, 1, C.byref(h)) == 1  # TCNN_ERROR
        assert message in _C.lib.tcnn_last_error().decode() and not h.value
    with pytest.raises(RuntimeError, match="Invalid optimizer type: Shampoo"):
        tcnn.optimizers.NativeOptimizer({"otype": "Shampoo"}, 64, [(4, 4)])


def test_package_exports_optimizers(tcnn):
    import torch

    assert issubclass(tcnn.optimizers.Optimizer, torch.optim.Optimizer)
    assert callable(tcnn.optimizers.NativeOptimizer) and callable(tcnn.optimizers.module_layer_sizes)


# ------------------------------------------------------------------------------------------------------------------- on the GPU
_SHAPES, _RUNS = {}, {}


def _shapes(oracle):
    """(n, n_net, layer_sizes) of the C3B parameter vector"""
    if not _SHAPES:
        from test_gpu_parity import CONFIG_C3B

        model = oracle.Trainer(2, 3, CONFIG_C3B, seed=1337).model
        _SHAPES["v"] = (model.n_params, model.network.n_params, [tuple(ls) for ls in model.network.layer_sizes()])
    return _SHAPES["v"]


def _gradient_bits(oracle, step):
    """half bits of the gradients of one step (test_optimizers.py::_drive)"""
    n, n_net, _ = _shapes(oracle)
    g = oracle.Pcg32(11 + step).uniform_strided(n, -4.0, 4.0)
    g[n_net + step::3] = 0.0
    return oracle.half_bits(g)


def _configs(oracle):
    n, n_net, _ = _shapes(oracle)
    adam = ADAM
    unaligned = {"otype": "Composite", "nested": [  # test_optimizers.py::test_composite_optimizer_with_unaligned_slices: the element-wise Adam kernel
        {**SGD, "n_params_to_optimize": n_net},
        {**adam, "n_params_to_optimize": 333},
        {**adam, "learning_rate": 5e-3, "n_params_to_optimize": n - n_net - 333 - 5},
    ]}
    import adam_reference as ar

    # (the options of tests/test_adam_options.py, which holds the stand-alone kernels to the oracle per element: here the trainer's launch to them)
    return {"adam": (ADAM, 4), "adam_full": (ar.FULL, 4), "adam_frozen_grid": (ar.OPTION_SETS["frozen_grid"], 4), "sgd": (SGD, 4), "nested": (NESTED, 5), "composite": (_composite(n_net, n - n_net), 4), "unaligned": (unaligned, 3), "novograd": (NOVOGRAD, 4)}


class _State:
    """master weights, half weights and a native optimizer on them"""

    def __init__(self, tcnn, oracle, cfg, w_fp, w_h):
        n, _, layers = _shapes(oracle)
        self.opt = tcnn.optimizers.NativeOptimizer(cfg, n, layers)
        self.w_fp, self.w_h = w_fp.clone(), w_h.clone()

    def step(self, oracle, step, fp32):
        import torch

        g_h = torch.from_numpy(_gradient_bits(oracle, step).view(np.float16)).cuda()
        if fp32:
            self.opt.step(self.w_fp, self.w_h, g_h.float() / LOSS_SCALE, 1.0)
        else:
            self.opt.step(self.w_fp, self.w_h, g_h, LOSS_SCALE)

    def bits(self):
        return self.w_fp.cpu().numpy().view(np.uint32), self.w_h.cpu().numpy().view(np.uint16)


def _run(tcnn, oracle, name):
    """One configuration driven three ways from the same start: a Trainer, a standalone handle on half gradients, one on fp32 gradients."""
    if name in _RUNS:
        return _RUNS[name]
    import torch
    from tinycudann import _C

    from test_gpu_parity import CONFIG_C3B

    cfg, steps = _configs(oracle)[name]
    n = _shapes(oracle)[0]
    tr = tcnn.Trainer(2, 3, {**CONFIG_C3B, "optimizer": cfg}, seed=1337)
    w_fp0, w_h0 = tr.params_full_precision(), tr.params()
    half, full = _State(tcnn, oracle, cfg, w_fp0, w_h0), _State(tcnn, oracle, cfg, w_fp0, w_h0)
    for step in range(steps):
        gt = torch.from_numpy(_gradient_bits(oracle, step).view(np.float16)).cuda()
        _C.memcpy_dtod(_C.lib.tcnn_trainer_param_gradients(tr._h), gt.data_ptr(), n * 2)
        tr.optimizer_step(LOSS_SCALE)
        half.step(oracle, step, fp32=False)
        full.step(oracle, step, fp32=True)
    torch.cuda.synchronize()
    _RUNS[name] = {"cfg": cfg, "steps": steps, "trainer": tr, "half": half, "fp32": full, "w_fp0": w_fp0.cpu().numpy(), "w_h0": w_h0.cpu().numpy().view(np.uint16)}
    return _RUNS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["adam", "adam_full", "adam_frozen_grid", "sgd", "nested", "composite", "unaligned", "novograd"])
def test_standalone_steps_equal_the_trainers_bitwise(tcnn, oracle, name):
    from test_gpu_parity import _bits

    run = _run(tcnn, oracle, name)
    tr = run["trainer"]
    want_fp, want_h = tr.params_full_precision().cpu().numpy().view(np.uint32), _bits(tr.params())
    assert not np.array_equal(want_fp, run["w_fp0"].view(np.uint32)), "the trainer did not move"
    for form in ("half", "fp32"):
        got_fp, got_h = run[form].bits()
        assert np.array_equal(got_fp, want_fp), f"{name}/{form}: fp32 master weights differ in {np.count_nonzero(got_fp != want_fp)} places"
        assert np.array_equal(got_h, want_h), f"{name}/{form}: half weights differ in {np.count_nonzero(got_h != want_h)} places"
        assert run[form].opt.step_count() == tr.optimizer_step_count() == run["steps"]
        custom = run[form].opt.custom_weights()
        if name in ("nested", "composite"):
            assert np.array_equal(_bits(custom), _bits(tr.params_inference())), f"{name}/{form}: inference weights"
            assert not np.array_equal(_bits(custom), got_h)
        else:
            assert custom is None
    assert run["half"].opt.hyperparams() == tr.hyperparams()["optimizer"]


@pytest.mark.gpu
def test_standalone_matches_the_oracle(tcnn, oracle):
    """The bars of test_optimizers.py: SGD bitwise, Adam within 1e-5 max|update| + 1e-9, EMA halves >= 99.9 % identical and within
    2^-9 max(1, max|w|)."""
    from test_gpu_parity import _bits, _f32

    n, _, layers = _shapes(oracle)

    def reference(name):
        run = _run(tcnn, oracle, name)
        ref = oracle.create_optimizer(run["cfg"])
        ref.allocate(n, layers)
        w_fp, w_h = run["w_fp0"].copy(), run["w_h0"].copy()
        for step in range(run["steps"]):
            ref.step(LOSS_SCALE, w_fp, w_h, _gradient_bits(oracle, step))
        return run, ref, w_fp, w_h

    run, ref, w_fp, w_h = reference("sgd")
    for form in ("half", "fp32"):
        got_fp, got_h = run[form].bits()
        assert np.array_equal(got_fp, w_fp.view(np.uint32)) and np.array_equal(got_h, w_h)
    run, ref, w_fp, w_h = reference("adam")
    upd = float(np.max(np.abs(w_fp - run["w_fp0"])))
    for form in ("half", "fp32"):
        got = run[form].w_fp.cpu().numpy()
        err = float(np.max(np.abs(got - w_fp)))
        print(f"adam/{form}: max error {err:.3e}, bar {1e-5 * upd + 1e-9:.3e}")
        assert upd > 0 and err <= 1e-5 * upd + 1e-9
    run, ref, w_fp, w_h = reference("nested")
    upd = float(np.max(np.abs(w_fp - run["w_fp0"])))
    for form in ("half", "fp32"):
        assert float(np.max(np.abs(run[form].w_fp.cpu().numpy() - w_fp))) <= 1e-5 * upd + 1e-9
        ema = _bits(run[form].opt.custom_weights())
        same = float(np.mean(ema == ref.weights_ema))
        err = float(np.max(np.abs(_f32(ema) - _f32(ref.weights_ema))))
        print(f"ema/{form}: {same:.6f} identical, max error {err:.3e}")
        assert same >= 0.999 and err <= 2.0 ** -9 * max(1.0, float(np.max(np.abs(_f32(ema)))))


@pytest.mark.gpu
def test_grid_entries_with_zero_gradient_are_left_alone(tcnn, oracle):
    """adam.h:76-84: a non-matrix parameter whose gradient is zero is skipped -- fp32 and half bits, moments and count stay; a
    matrix weight with a zero gradient still moves (l2_reg)."""
    import msgpack
    import torch

    n, n_net, layers = _shapes(oracle)
    w_fp0 = torch.from_numpy(oracle.Pcg32(3).uniform_strided(n, -0.5, 0.5).astype(np.float32)).cuda()
    # half weights that are NOT the rounding of the master weights where nothing may be written: a store there would show
    w_h0 = w_fp0.half()
    dead = np.zeros(n, dtype=bool)
    dead[n_net + 1::3] = True          # single entries: live quads with dead lanes
    dead[n_net + 4096:n_net + 8192] = True  # whole quads: the skip before anything else is read
    dead[n - 3:] = True
    dead_t = torch.from_numpy(dead).cuda()
    w_h0[dead_t] = 1.5
    zero_matrix = slice(64, 128)
    for fp32 in (False, True):
        opt = tcnn.optimizers.NativeOptimizer({**ADAM, "l2_reg": 1e-2}, n, layers)
        w_fp, w_h = w_fp0.clone(), w_h0.clone()
        for step in range(3):
            g = torch.from_numpy(oracle.Pcg32(40 + step).uniform_strided(n, 0.5, 4.0).astype(np.float32)).cuda().half()
            g[dead_t] = 0.0
            g[zero_matrix] = 0.0
            opt.step(w_fp, w_h, g.float() / LOSS_SCALE if fp32 else g, 1.0 if fp32 else LOSS_SCALE)
        state = msgpack.unpackb(opt.serialize(), raw=False)
        m1, m2 = (np.frombuffer(state[k], dtype=np.float32) for k in ("first_moments_binary", "second_moments_binary"))
        steps = np.frombuffer(state["param_steps_binary"], dtype=np.uint32)
        got_fp, got_h = w_fp.cpu().numpy(), w_h.cpu().numpy().view(np.uint16)
        assert np.array_equal(got_fp[dead].view(np.uint32), w_fp0.cpu().numpy()[dead].view(np.uint32))
        assert np.all(got_h[dead] == np.float16(1.5).view(np.uint16))
        assert not m1[dead].any() and not m2[dead].any() and not steps[dead].any()
        live = ~dead
        assert np.all(steps[live] == 3) and np.all(got_fp[live] != w_fp0.cpu().numpy()[live])
        assert np.all(got_fp[zero_matrix] != w_fp0.cpu().numpy()[zero_matrix]) and np.all(m1[zero_matrix] != 0)  # l2_reg alone moves them


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["adam", "nested", "composite"])
def test_snapshot_resumes_bitwise_and_is_the_trainers(tcnn, oracle, name):
    import msgpack
    import torch

    from test_gpu_parity import CONFIG_C3B, _bits

    run = _run(tcnn, oracle, name)
    n = _shapes(oracle)[0]
    cfg, tr, ours = run["cfg"], run["trainer"], run["fp32"]
    blob = ours.opt.serialize()
    # the same bytes a trainer's snapshot carries as its "optimizer" entry
    trainer_entry = msgpack.unpackb(tr.serialize(serialize_optimizer=True), raw=False)["optimizer"]
    assert msgpack.unpackb(blob, raw=False) == trainer_entry
    # -> a fresh handle, fed from the TRAINER's entry, continues like the uninterrupted one
    fresh = _State(tcnn, oracle, cfg, ours.w_fp, ours.w_h)
    fresh.opt.deserialize(msgpack.packb(trainer_entry, use_bin_type=True))
    fresh.opt.weights_restored(fresh.w_h)  # what Trainer::deserialize does: a Composite's inference weights are not part of a snapshot
    assert fresh.opt.step_count() == run["steps"] and fresh.opt.learning_rate() == ours.opt.learning_rate()
    if name != "adam":
        assert np.array_equal(_bits(fresh.opt.custom_weights()), _bits(ours.opt.custom_weights()))
    cont = _State(tcnn, oracle, cfg, ours.w_fp, ours.w_h)  # the uninterrupted run goes on from copies: `run` stays as it is for the other tests
    cont.opt.deserialize(blob)
    a = _State(tcnn, oracle, cfg, ours.w_fp, ours.w_h)
    a.opt.deserialize(blob)
    for s, fp32 in ((run["steps"], True), (run["steps"] + 1, False)):
        for st in (fresh, cont, a):
            st.step(oracle, s, fp32)
    assert all(np.array_equal(x, y) for x, y in zip(fresh.bits(), cont.bits()))
    assert all(np.array_equal(x, y) for x, y in zip(a.bits(), cont.bits())), "two runs from the same state differ"
    # the reverse: the standalone state restores a trainer, whose next step equals the standalone one's
    other = tcnn.Trainer(2, 3, {**CONFIG_C3B, "optimizer": cfg}, seed=5)
    other.deserialize(msgpack.packb({"params_type": "__half", "params_binary": ours.w_h.cpu().numpy().tobytes(), "optimizer": msgpack.unpackb(blob, raw=False)}, use_bin_type=True))
    assert other.optimizer_step_count() == run["steps"]
    twin = _State(tcnn, oracle, cfg, other.params_full_precision(), other.params())  # a snapshot carries half parameters: the master weights restart from them
    twin.opt.deserialize(blob)
    from tinycudann import _C

    gt = torch.from_numpy(_gradient_bits(oracle, run["steps"]).view(np.float16)).cuda()
    _C.memcpy_dtod(_C.lib.tcnn_trainer_param_gradients(other._h), gt.data_ptr(), n * 2)
    other.optimizer_step(LOSS_SCALE)
    twin.step(oracle, run["steps"], fp32=True)
    got_fp, got_h = twin.bits()
    assert np.array_equal(got_fp, other.params_full_precision().cpu().numpy().view(np.uint32)) and np.array_equal(got_h, _bits(other.params()))


@pytest.mark.gpu
def test_two_runs_give_the_same_bits(tcnn, oracle):
    run = _run(tcnn, oracle, "adam")
    again = _State(tcnn, oracle, run["cfg"], __import__("torch").from_numpy(run["w_fp0"]).cuda(), __import__("torch").from_numpy(run["w_h0"].view(np.float16)).cuda())
    for step in range(run["steps"]):
        again.step(oracle, step, fp32=True)
    assert all(np.array_equal(x, y) for x, y in zip(again.bits(), run["fp32"].bits()))
    assert again.opt.serialize() == run["fp32"].opt.serialize()


@pytest.mark.gpu
def test_hyperparameters_and_learning_rate(tcnn, oracle):
    opt = tcnn.optimizers.NativeOptimizer(NESTED, 64, [(8, 8)])
    assert abs(opt.learning_rate() - 1e-2) < 1e-9 and opt.step_count() == 0
    opt.set_learning_rate(5e-3)
    assert abs(opt.learning_rate() - 5e-3) < 1e-9
    opt.update_hyperparams({"decay": 0.5, "nested": {"nested": {"beta1": 0.5}}})
    hp = opt.hyperparams()
    assert hp["otype"] == "EMA" and hp["decay"] == 0.5 and hp["nested"]["nested"]["beta1"] == 0.5
    with pytest.raises(RuntimeError, match="more weights than n_params"):
        tcnn.optimizers.NativeOptimizer(ADAM, 63, [(8, 8)])


WRAPPED = {"otype": "Average", "n_samples": 2, "nested": {"otype": "Lookahead", "alpha": 0.5, "n_steps": 3, "nested": {"otype": "Batched", "batch_size_multiplier": 2, "nested": SGD}}}


@pytest.mark.gpu
def test_wrappers_pass_fp32_gradients_through(tcnn, oracle):
    """Average -> Lookahead -> Batched -> SGD on fp32 gradients.  Batched hands the nested optimizer its fp32 mean as it is where the
    half form rounds the mean to half first; with gradients k / 4 (|k| <= 64, scaled by 128) the mean of two, (k1 + k2) / 8, is exact
    in half, so here both forms must give the bits of a Trainer (whose wrappers test_optimizers.py pins to the oracle bit for bit)."""
    import torch
    from tinycudann import _C

    from test_gpu_parity import CONFIG_C3B, _bits

    n = _shapes(oracle)[0]
    tr = tcnn.Trainer(2, 3, {**CONFIG_C3B, "optimizer": WRAPPED}, seed=1337)
    w_fp0, w_h0 = tr.params_full_precision(), tr.params()
    half, full = _State(tcnn, oracle, WRAPPED, w_fp0, w_h0), _State(tcnn, oracle, WRAPPED, w_fp0, w_h0)
    for step in range(8):
        k = (np.arange(n, dtype=np.int64) * 7 + step * 13) % 129 - 64
        g_h = torch.from_numpy((k / 4.0).astype(np.float16)).cuda()
        _C.memcpy_dtod(_C.lib.tcnn_trainer_param_gradients(tr._h), g_h.data_ptr(), n * 2)
        tr.optimizer_step(LOSS_SCALE)
        half.opt.step(half.w_fp, half.w_h, g_h, LOSS_SCALE)
        full.opt.step(full.w_fp, full.w_h, g_h.float() / LOSS_SCALE, 1.0)
    want_fp, want_h, want_custom = tr.params_full_precision().cpu().numpy().view(np.uint32), _bits(tr.params()), _bits(tr.params_inference())
    assert not np.array_equal(want_fp, w_fp0.cpu().numpy().view(np.uint32))
    for state in (half, full):
        got_fp, got_h = state.bits()
        assert np.array_equal(got_fp, want_fp) and np.array_equal(got_h, want_h)
        assert np.array_equal(_bits(state.opt.custom_weights()), want_custom) and not np.array_equal(want_custom, want_h)
        assert state.opt.step_count() == tr.optimizer_step_count() == 8


def test_getters_report_a_null_handle(tcnn):
    from tinycudann import _C

    assert _C.lib.tcnn_optimizer_step_count(None) == 0 and "o && o->optimizer" in _C.lib.tcnn_last_error().decode()
    assert _C.lib.tcnn_optimizer_n_params(None) == 0 and _C.lib.tcnn_optimizer_hyperparams(None) is None and _C.lib.tcnn_optimizer_custom_weights(None) is None
    assert np.isnan(_C.lib.tcnn_optimizer_learning_rate(None))
