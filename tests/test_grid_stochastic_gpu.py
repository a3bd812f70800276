"""stochastic_interpolation of the grid encodings on the GPU (grid.h:284-298): the parameter gradients of every gradient route against the
numpy restatement (tests/grid_stochastic_reference.py), everything else against the same grid without the key.

  exact routes (half grids, two or more features per level: k_grid_scatter with and without its bit-plane filter, k_grid_bin): the exact sum
      of the selected dL/dy halves rounded once -- bit for bit, through tcnn.Encoding, NetworkWithInputEncoding.backward and the fused and
      unfused Trainer steps (those under GradientMode::Overwrite and then Accumulate; a module's backward pass has no Accumulate);
  atomic routes (fp32 grids, half grids with one feature per level, TCNN_AMD_GRID_SCATTER=atomic): per parameter the bounds of
      tests/test_grid_reference_kernels.py -- |got - S| <= gamma(k - 1) * A at u = 2^-24 (fp32), u = 2^-11 (packed fp16),
      [rn_half(S - e), rn_half(S + e)] for the fp32 scratch of F = 1; untouched parameters exactly +0.  No slack term: with weight 1 every
      contribution is dL/dy itself and sums of fp16 subnormals are exact.
Batches of 256 and 512 rows (the draw of row i on level l has index i + l * n: the two batches give every level but the first other draws);
tables of 16 to 256 entries per level, so that hundreds of samples meet in one entry.  dL/dy given to an encoding directly has subnormals, zeros of both signs
and 24 binades of magnitude; dL/dy that a network's backward pass produces (linear network, weights in {-1, 0, 1}: every fp32 sum exact in
any order, so the oracle's dL/d(encoded) has the kernels' bits) spans 9 binades and zero rows."""
import numpy as np
import pytest

import grid_stochastic_reference as gsr
from conftest import CONFIG_C3B
from grid_reference import U16, U32, check_rounded_sum_per_level, check_sum_per_level
from test_grid_stochastic import ATOMIC_CASES, BATCHES, EXACT_CASES, case_id, selection_of

pytestmark = pytest.mark.gpu

LISTS = {"TCNN_AMD_SCATTER_LISTS": "1"}
NET = {"otype": "FullyFusedMLP", "activation": "None", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
# the smallest table with a binned level (GridEncoding::facts().any_binned; tests/cpp/grid_route_stochastic.cpp checks both sides of the
# threshold): eight features per level cut a level into chunks of 2048 entries, and without scatter records more than 8 chunks are binned --
# 129^2 = 16641 entries are 9 chunks, 128^2 are 8.  One level is all that needs.
BINNED_CASE = (2, {"otype": "DenseGrid", "n_levels": 1, "n_features_per_level": 8, "base_resolution": 129, "per_level_scale": 2.0, "interpolation": "Linear", "stochastic_interpolation": True})


def _t(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared references are read-only)


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32)


def _plain(cfg):
    return {k: v for k, v in cfg.items() if k != "stochastic_interpolation"}


def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_same(got, want, what):
    differ = got != want
    assert not np.any(differ), f"{what}: {int(np.count_nonzero(differ))} of {differ.size} values differ, first at {int(np.argwhere(differ)[0][0])}: got {int(got[differ][0]):#x}, want {int(want[differ][0]):#x}"


def _native_gradient(native, x, params, dy):
    """forward (training form, parameter gradients prepared) and backward through a native module: dL/dparams"""
    xt, pt = _t(x), _t(params).requires_grad_(True)
    ctx, out = native.fwd(xt, pt)
    _, g = native.bwd(ctx, xt, pt, out, _t(dy))
    return g


# ---------------------------------------------------------------------------------------------------- exact routes: the encoding alone
@pytest.mark.parametrize("env", [{}, LISTS], ids=["default", "lists_asked_for"])
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("case", EXACT_CASES + [BINNED_CASE], ids=case_id)
def test_encoding_backward_is_exact(tcnn, oracle, monkeypatch, case, n, env):
    """tcnn.Encoding's native module: k_grid_scatter behind the bit planes of either forward kernel (k_grid_bin for the binned level), also
    where hit lists are asked for everywhere -- the route declines them"""
    n_in, cfg = case
    ref, x, sel = selection_of(oracle, case, n)
    _env(monkeypatch, env)
    native = tcnn.Encoding(n_in, cfg).native_tcnn_module
    assert native.n_params() == ref.n_params and native.n_output_dims() == ref.n_output_dims
    dy = gsr.stochastic_gradients(oracle, n, ref.n_output_dims)
    want = gsr.exact_half_gradient(oracle, ref, sel, dy)
    assert np.count_nonzero(want) > 0 and np.any((dy & 0x7C00) == 0) and np.any(dy == 0x8000)  # (subnormals and zeros of both signs go in)
    got = _bits(_native_gradient(native, x, np.zeros(ref.n_params, dtype=np.float16), dy.view(np.float16)))
    assert native.list_scatters() == 0
    _assert_same(got, want, case_id(case))
    # and it is not the n-linear gradient: the plain grid's differs
    plain = tcnn.Encoding(n_in, _plain(cfg)).native_tcnn_module
    assert not np.array_equal(_bits(_native_gradient(plain, x, np.zeros(ref.n_params, dtype=np.float16), dy.view(np.float16))), want)


# ---------------------------------------------------------------------------------------------------- exact routes: behind a network
def _linear_params(oracle, ref_model, seed=5):
    """weights in {-1, 0, 1}, sparse: every sum of the MLP's backward pass is exact in fp32 whatever its order"""
    rs = np.random.RandomState(seed)
    n_net = ref_model.network.n_params
    params = oracle.Pcg32(3).uniform_strided(ref_model.n_params, -1.0, 1.0).astype(np.float32)
    params[:n_net] = rs.choice([-1.0, 0.0, 1.0], size=n_net, p=[1 / 16, 7 / 8, 1 / 16])
    return oracle.half_bits(params), rs


def _network_dy(oracle, rs, n, width):
    """dL/d(output): multiples of 1/64 in [-2, 2] scaled per row by 2^0, 2^-3, 2^-6 or 2^-8 (all normal halves), every seventh row zero"""
    dy = (rs.randint(-128, 129, size=(n, width)) / 64.0) * (2.0 ** -np.array([0, 3, 6, 8]))[np.arange(n) % 4][:, None]
    dy[::7] = 0
    return oracle.half_bits(dy.astype(np.float32))


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("case", EXACT_CASES, ids=case_id)
def test_network_with_input_encoding_backward_is_exact(tcnn, oracle, case, n):
    n_in, cfg = case
    _, x, sel = selection_of(oracle, case, n)
    m = tcnn.NetworkWithInputEncoding(n_in, 16, cfg, NET)
    native = m.native_tcnn_module
    ref = oracle.NetworkWithInputEncoding(n_in, 16, cfg, NET)
    assert native.n_params() == ref.n_params
    params_h, rs = _linear_params(oracle, ref)
    dy = _network_dy(oracle, rs, n, ref.padded_output_width)
    out, ctx = ref.forward(x, params_h)
    _, dnet_in = ref.backward(x, params_h, ctx, out, dy)
    assert np.any(dnet_in != 0)
    want = gsr.exact_half_gradient(oracle, ref.encoding, sel, dnet_in)
    got = _bits(_native_gradient(native, x, params_h.view(np.float16), dy.view(np.float16)))[ref.network.n_params:]
    assert np.count_nonzero(want) > 0 and native.list_scatters() == 0
    _assert_same(got, want, case_id(case))


@pytest.mark.parametrize("step_env,n,env", [({}, 256, {}), ({}, 512, {}), ({}, 512, LISTS), ({"TCNN_AMD_FUSED_STEP": "0"}, 256, {}), ({"TCNN_AMD_FUSED_STEP": "0"}, 512, {})],
                         ids=["fused-256", "fused-512", "fused-512-lists_asked_for", "unfused-256", "unfused-512"])
@pytest.mark.parametrize("case", EXACT_CASES, ids=case_id)
def test_trainer_steps_are_exact(tcnn, oracle, monkeypatch, case, step_env, n, env):
    """training_step(external_dL_dy) under GradientMode::Overwrite, then Accumulate on top of it with another dL/dy"""
    from tinycudann.native import GRADIENT_ACCUMULATE, GRADIENT_OVERWRITE

    n_in, enc = case
    _, x, sel = selection_of(oracle, case, n)
    cfg = {**CONFIG_C3B, "encoding": enc, "network": NET}
    _env(monkeypatch, {**step_env, **env})
    tr = tcnn.Trainer(n_in, 3, cfg, seed=1337)
    ref = oracle.Trainer(n_in, 3, cfg, seed=1337)
    params_h, rs = _linear_params(oracle, ref.model)
    tr.set_params(_t(params_h.view(np.float16)))
    n_net = ref.model.network.n_params
    want = None
    for step, mode in enumerate((GRADIENT_OVERWRITE, GRADIENT_ACCUMULATE)):
        dy = _network_dy(oracle, rs, n, ref.model.padded_output_width)
        out, ctx = ref.model.forward(x, params_h)
        _, dnet_in = ref.model.backward(x, params_h, ctx, out, dy)
        want = gsr.exact_half_gradient(oracle, ref.model.encoding, sel, dnet_in, previous_bits=want)
        tr.training_step(_t(x), None, run_optimizer=False, gradient_mode=mode, external_dL_dy=_t(dy.view(np.float16)))
        kernel = tr.last_step_kernel()
        assert (kernel == "unfused") == bool(step_env) and kernel != "", kernel
        assert tr.list_scatters() == 0 and tr.list_gradient_tails() == 0
        got = _bits(tr.param_gradients())[n_net:]
        assert np.count_nonzero(want) > 0
        _assert_same(got, want, f"{case_id(case)} {kernel} pass {step}")


# ---------------------------------------------------------------------------------------------------- Nearest
@pytest.mark.parametrize("n_in,F", [(2, 2), (3, 4)])
def test_nearest_ignores_the_key(tcnn, oracle, n_in, F):
    cfg = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": F, "log2_hashmap_size": 6, "base_resolution": 3, "per_level_scale": 1.5, "interpolation": "Nearest"}
    ref = oracle.create_encoding(n_in, cfg, alignment=0)
    n = 512
    x = gsr.stochastic_rows(oracle, ref, n)
    dy = gsr.stochastic_gradients(oracle, n, ref.n_output_dims).view(np.float16)
    zeros = np.zeros(ref.n_params, dtype=np.float16)
    g_plain = _bits(_native_gradient(tcnn.Encoding(n_in, cfg).native_tcnn_module, x, zeros, dy))
    g_flag = _bits(_native_gradient(tcnn.Encoding(n_in, dict(cfg, stochastic_interpolation=True)).native_tcnn_module, x, zeros, dy))
    want = np.zeros(ref.n_params, dtype=np.uint16)
    ref.backward_exact(x, dy.view(np.uint16), want)
    assert np.count_nonzero(want) > 0
    _assert_same(g_plain, want, "plain Nearest")
    _assert_same(g_flag, g_plain, "Nearest with the key")


# ---------------------------------------------------------------------------------------------------- atomic routes
def _fp32_gradients(oracle, n, width):
    """float dL/dy: uniform in [-2, 2) over 24 binades (all normal floats), every seventh row zero"""
    v = oracle.Pcg32(9).uniform_strided(n * width, -2.0, 2.0).reshape(n, width).astype(np.float64)
    e = (np.arange(width)[None, :] + np.arange(n)[:, None]) % 24
    dy = (v * 2.0 ** -e).astype(np.float32)
    dy[::7] = 0
    return dy


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("case", ATOMIC_CASES, ids=case_id)
def test_fp32_grid_gradient_per_element(tcnn, oracle, case, n):
    """k_grid_bwd<float, float>: one float atomic per (sample, level, feature), the value dL/dy itself"""
    import torch

    n_in, cfg = case
    ref, x, sel = selection_of(oracle, case, n)
    native = tcnn.Encoding(n_in, cfg, dtype=torch.float32).native_tcnn_module
    dy = _fp32_gradients(oracle, n, ref.n_output_dims)
    terms = gsr.atomic_terms(oracle, ref, sel, dy)
    g = _native_gradient(native, x, np.zeros(ref.n_params, dtype=np.float32), dy).cpu().numpy()
    assert np.any(g != 0)
    check_sum_per_level(ref, (g.astype(np.float64), g.view(np.uint32)), terms, U32, label=f"{case_id(case)} fp32")


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("case", [c for c in ATOMIC_CASES if c[1]["n_features_per_level"] == 1], ids=case_id)
def test_scalar_feature_half_gradient_in_rounding_interval(tcnn, oracle, case, n):
    """k_grid_bwd<half, float> into the fp32 scratch, one cast"""
    n_in, cfg = case
    ref, x, sel = selection_of(oracle, case, n)
    native = tcnn.Encoding(n_in, cfg).native_tcnn_module
    dy = gsr.stochastic_gradients(oracle, n, ref.n_output_dims)
    terms = gsr.atomic_terms(oracle, ref, sel, dy)
    bits = _bits(_native_gradient(native, x, np.zeros(ref.n_params, dtype=np.float16), dy.view(np.float16)))
    assert np.any(bits != 0)
    check_rounded_sum_per_level(ref, bits, terms, label=f"{case_id(case)} scratch32")


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("case", [c for c in ATOMIC_CASES + EXACT_CASES[:2] if c[1]["n_features_per_level"] == 2], ids=case_id)
def test_packed_fp16_atomic_gradient_per_element(tcnn, oracle, monkeypatch, case, n):
    """k_grid_bwd<half, half> under TCNN_AMD_GRID_SCATTER=atomic: one packed-fp16 atomic per (sample, level, feature pair)"""
    n_in, cfg = case
    ref, x, sel = selection_of(oracle, case, n)
    monkeypatch.setenv("TCNN_AMD_GRID_SCATTER", "atomic")
    native = tcnn.Encoding(n_in, cfg).native_tcnn_module
    dy = gsr.stochastic_gradients(oracle, n, ref.n_output_dims)
    terms = gsr.atomic_terms(oracle, ref, sel, dy)
    bits = _bits(_native_gradient(native, x, np.zeros(ref.n_params, dtype=np.float16), dy.view(np.float16)))
    assert np.any(bits != 0)
    check_sum_per_level(ref, (bits.view(np.float16).astype(np.float64), bits), terms, U16, label=f"{case_id(case)} packed fp16")


# ---------------------------------------------------------------------------------------------------- max_level
def _off(ml, L, F):
    """the gradient rule in the reference's fp32 expressions (grid.h:237-245): level > (ml * (L * F)) / F + 1e-3f"""
    t = (np.asarray(ml, dtype=np.float32) * np.float32(L * F)) / np.float32(F) + np.float32(1e-3)
    return np.arange(L, dtype=np.float32) > t[..., None]


@pytest.mark.parametrize("fp32", [False, True], ids=["half", "fp32"])
def test_max_level_scalar_and_per_sample(tcnn, oracle, fp32):
    import torch

    case = EXACT_CASES[1] if not fp32 else ATOMIC_CASES[2]
    n_in, cfg = case
    n, L, F = 512, cfg["n_levels"], cfg["n_features_per_level"]
    ref, x, sel = selection_of(oracle, case, n)
    native = tcnn.Encoding(n_in, cfg, dtype=torch.float32 if fp32 else None).native_tcnn_module
    dy = _fp32_gradients(oracle, n, ref.n_output_dims) if fp32 else gsr.stochastic_gradients(oracle, n, ref.n_output_dims)
    per_sample = oracle.Pcg32(11).uniform_strided(n).astype(np.float32)
    per_sample[::5] = 1000.0
    per_sample[::9] = 0.0
    for setting, off in (("scalar", np.broadcast_to(_off(np.float32(0.5), L, F), (n, L))), ("per sample", _off(per_sample, L, F))):
        assert off.any() and not off.all()
        mlt = _t(per_sample)
        if setting == "scalar":
            native.set_max_level(0.5)
        else:
            native.set_max_level(1000.0)
            native.set_max_level_gpu(mlt)
        if fp32:
            g = _native_gradient(native, x, np.zeros(ref.n_params, dtype=np.float32), dy).cpu().numpy()
            check_sum_per_level(ref, (g.astype(np.float64), g.view(np.uint32)), gsr.atomic_terms(oracle, ref, sel, dy, off=off), U32, label=f"fp32 {setting}")
            assert np.any(g != 0)
        else:
            got = _bits(_native_gradient(native, x, np.zeros(ref.n_params, dtype=np.float16), dy.view(np.float16)))
            want = gsr.exact_half_gradient(oracle, ref, sel, dy, off=off)
            assert np.count_nonzero(want) > 0
            _assert_same(got, want, f"half {setting}")
        native.set_max_level_gpu(None)


# ---------------------------------------------------------------------------------------------------- what the key does not touch
@pytest.mark.parametrize("dtype,n_in,cfg", [
    (None, 3, {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 8, "base_resolution": 3, "per_level_scale": 1.5, "interpolation": "Smoothstep"}),
    ("float32", 2, {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 4, "log2_hashmap_size": 8, "base_resolution": 4, "per_level_scale": 2.0}),
], ids=["half-3d-smoothstep", "fp32-2d-linear"])
def test_everything_but_the_parameter_gradient_is_untouched(tcnn, oracle, dtype, n_in, cfg):
    """forward output (inference and training form), dL/dx (so dy_dx), and the second-order pass -- dL_ddLdy, its dL/dx and its parameter
    gradient (grid.h:360: kernel_grid_backward_input_backward_grid has the parameter commented out) -- bit for bit those of the plain grid.
    The second-order parameter gradient is a sum of float atomics in an order nobody fixes, so two runs of ONE grid need not agree in their
    bits; the fp32 case makes it independent of the order -- coordinates on multiples of 1/16, scales 3, 7, 15, 31, small integers for
    dL/dy and dL_ddLdx: every contribution a multiple of 2^-4 below 2^6, every sum of them exact in fp32 -- and is where it is compared.
    The half case (packed-fp16 atomics, Smoothstep weights) compares the other five."""
    import torch

    dt = getattr(torch, dtype) if dtype else torch.half
    n = 512
    rs = np.random.RandomState(3)
    ref = oracle.create_encoding(n_in, cfg, alignment=0)
    if dtype:
        x = (rs.randint(0, 16, size=(n, n_in)) / 16.0).astype(np.float32)
        dy = rs.randint(-2, 3, size=(n, ref.n_output_dims)).astype(np.float32)
        v = rs.randint(-1, 2, size=(n, n_in)).astype(np.float32)
        params = rs.randint(-4, 5, size=ref.n_params).astype(np.float32)
    else:
        x = gsr.stochastic_rows(oracle, ref, n)
        dy = gsr.stochastic_gradients(oracle, n, ref.n_output_dims).view(np.float16)
        v = (rs.rand(n, n_in) - 0.5).astype(np.float32)
        params = oracle.half_bits(oracle.Pcg32(3).uniform_strided(ref.n_params, -1.0, 1.0)).view(np.float16)
    results = []
    for c in (cfg, dict(cfg, stochastic_interpolation=True)):
        native = tcnn.Encoding(n_in, c, dtype=dt if dtype else None).native_tcnn_module
        with torch.no_grad():
            _, inference = native.fwd(_t(x), _t(params))
        xt, pt = _t(x).requires_grad_(True), _t(params).requires_grad_(True)
        ctx, out = native.fwd(xt, pt)
        dx, g = native.bwd(ctx, xt, pt, out, _t(dy))
        ddy, dp, dx2 = native.bwd_bwd_input(ctx, xt, pt, _t(v), _t(dy).requires_grad_(True))
        results.append((inference, out, dx, ddy, dx2, dp, g))
    names = ("inference output", "training output", "dL/dx", "dL_ddLdy", "second-order dL/dx", "second-order dL/dparams")
    for name, a, b in zip(names if dtype else names[:5], results[0], results[1]):
        assert a is not None and torch.any(a != 0), name
        _assert_same(_bits(b), _bits(a), name)
    if not dtype:  # (exact route: the first-order parameter gradient is the one thing that differs)
        assert not torch.equal(results[0][6], results[1][6])


# ---------------------------------------------------------------------------------------------------- the whole path
def test_stochastic_trainer_learns(tcnn):
    """the shipped hash-grid config with the key, 20 steps at batch 1024: finite, decreasing loss -- a smoke check, not a parity check"""
    import torch

    cfg = {**CONFIG_C3B, "encoding": dict(CONFIG_C3B["encoding"], stochastic_interpolation=True)}
    tr = tcnn.Trainer(2, 3, cfg, seed=7)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(256 * 4, 2, device="cuda", generator=g)
    y = torch.stack([torch.sin(6 * x[:, 0]) * 0.5 + 0.5, x[:, 1], x[:, 0] * x[:, 1]], dim=1).contiguous()
    losses = [tr.loss(tr.training_step(x, y)) for _ in range(20)]
    assert tr.last_step_kernel() not in ("", "unfused") and tr.list_scatters() == 0 and tr.list_gradient_tails() == 0
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses
