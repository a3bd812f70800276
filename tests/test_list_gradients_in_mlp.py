"""dL/dy in hit-list order as the tail of k_mlp_train_r32 (GridListTail, GridItemMap; TCNN_AMD_LISTGRAD_IN_MLP=0: k_grid_list_gradients as
a launch of its own).  Trainer.list_gradient_tails() counts the steps that took the tail; every case asserts the path it means to test.

Where the tail exists.  A work item of the grid's hit lists must be exactly what one workgroup of k_mlp_train_r32 produces.  The plan
(mlp_train_plan, k_train_r32.hip r32_plan) runs that kernel over grid = min(256, n / 256) workgroups of 8 waves, each wave 32 samples per
trip: a workgroup makes trips = n / (256 grid) trips of 256 samples, i.e. ONE trip for every n <= 65536 and 4 trips first at n = 2^18.  An
item is 1024 samples in 2-D and 512 in 3-D (grid_planes_spt), so the smallest batch that takes the tail is n = 2^18 in 2-D (256 workgroups
x 4 trips, 256 items per level) and n = 2^17 in 3-D (256 x 2 trips; the plan gives batches of <= 131072 samples to k_mlp_train_r32a,
which has no tail: TCNN_AMD_MLP_R32A=0 there).  Four times those sizes make 16 / 8 trips per workgroup, more than an item holds: they
fall back (covered below at the sizes that are quick).  No smaller shape reaches the code under test.

Exactness.  k_mlp_train_r32 takes ReLU networks with the loss evaluated in the kernel only, so the oracle's exact scatter
(orc_grid_backward_exact, grid.h:215-320) is fed the way test_hit_list_scatter_matches_oracle feeds it, by other means: network weights
in {-1, 0, 1} (every sum of the MLP exact in fp32 whatever its order: activations, ReLU masks and dL/d(encoded input) have the oracle's
bits), the L2 loss, and targets chosen from the oracle's own prediction so that the kernel's fp32 expressions for the loss gradient
round to a given half: dL/doutput is then the exact pattern _exact_external_dy gives (multiples of a power of two over 8 bits), scaled.
Both premises (output bits, dL/doutput bits) are asserted before the gradients are compared.
"""
import numpy as np
import pytest

from conftest import CONFIG_C3A
from test_gpu_parity import _bits, _f32, _linear_net_params, _t, elem_close, rel_err
from test_grid_max_level import F32, levels_on

pytestmark = pytest.mark.gpu

N_OUT = 4
LOSS_SCALE = 128.0  # training_step's (tcnn_default_loss_scale)
N_2D = 1 << 18     # smallest 2-D batch that takes the tail (module docstring)
N_3D = 1 << 17     # ... and 3-D, with k_mlp_train_r32 forced
ENC_3D = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 1.5}
CONFIG_3D = {**CONFIG_C3A, "encoding": ENC_3D}
R32 = {"TCNN_AMD_MLP_R32A": "0"}  # k_mlp_train_r32 at batches the plan gives to k_mlp_train_r32a


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _exact_steps(tcnn, oracle, cfg, n_in, n, modes, max_level=None):
    """training_step()s of a ReLU network with weights in {-1, 0, 1}, L2 loss, targets that make dL/doutput exact (module docstring): yields
    (trainer, grid gradient bits, the oracle's exact scatter of the same dL/d(encoded input)) after every step; every step a new batch."""
    cfg = {**cfg, "loss": {"otype": "L2"}}
    ref = oracle.Trainer(n_in, N_OUT, cfg, seed=1337)
    tr = tcnn.Trainer(n_in, N_OUT, cfg, seed=1337)
    params_h, rs = _linear_net_params(oracle, ref.model, 5)
    tr.set_params(_t(params_h.view(np.float16)))
    n_net = ref.model.network.n_params
    enc = cfg["encoding"]
    L, F = enc["n_levels"], enc["n_features_per_level"]
    starts = ref.model.encoding.offsets.astype(np.int64) * F
    on = cut = L
    params_ref = params_h
    if max_level is not None:  # grid.h:67-90, 237-245: levels >= on encode zeros, levels >= cut receive no gradient
        tr.set_max_level(max_level)
        on, cut = levels_on(F32(max_level), L, F, False), levels_on(F32(max_level), L, F, True)
        params_ref = params_h.copy()
        params_ref[n_net + int(starts[on]):] = 0
    want = np.zeros(ref.model.encoding.n_params, dtype=np.uint16)
    for step, mode in enumerate(modes):
        x = oracle.Pcg32(42 + step).uniform_strided(n * n_in).reshape(n, n_in)
        x[:8] = np.float32([[0.0] * n_in, [1.0] * n_in, [0.5] * n_in, [0.999999] * n_in, [1e-7] * n_in, [0.25] * n_in, [0.75] * n_in, [0.125] * n_in])  # cell corners and edges
        out, ctx = ref.model.forward(x, params_ref)
        pred = _f32(out)[:, :N_OUT]
        # the pattern dL/doutput shall be: multiples of 2^-18 up to 2^-11 (_exact_external_dy's, scaled by loss_scale 2 / 2^20), and a target
        # that gives it by the kernel's own fp32 expressions (mlp_device.h loss_l2_fused): d = prediction - target, (d + d) (loss_scale / n_total)
        want_dy = (rs.randint(-128, 129, size=(n, N_OUT)) / 64.0).astype(np.float32) * F32(2.0 ** -12)
        want_dy[::7] = 0
        c = F32(LOSS_SCALE) / F32(n * N_OUT)
        target = (pred.astype(np.float64) - want_dy.astype(np.float64) / (2.0 * float(c))).astype(np.float32)
        d = pred - target
        missed = oracle.half_bits((d + d) * c) != oracle.half_bits(want_dy)  # (a prediction far larger than the difference: no gradient from that output)
        target[missed] = pred[missed]
        want_dy[missed] = 0
        assert np.count_nonzero(want_dy) > n  # the pattern survives
        dy = np.zeros((n, ref.model.padded_output_width), dtype=np.float32)
        dy[:, :N_OUT] = want_dy
        dy_h = oracle.half_bits(dy)
        assert np.array_equal(_f32(dy_h), dy)
        _, dnet_in = ref.model.backward(x, params_ref, ctx, out, dy_h)
        ref.model.encoding.backward_exact(x, dnet_in, want, accumulate=step > 0)
        if cut < L:
            want[int(starts[cut]):] = 0
        got_ctx = tr.training_step(_t(x), _t(target), run_optimizer=False, gradient_mode=mode)
        assert np.array_equal(_bits(got_ctx.output())[:, :N_OUT], out[:, :N_OUT]), "premise: the forward pass has the oracle's bits"
        assert np.array_equal(_bits(got_ctx.dL_doutput()).reshape(n, -1)[:, :N_OUT], dy_h[:, :N_OUT]), "premise: dL/doutput has the oracle's bits"
        yield tr, _bits(tr.param_gradients())[n_net:], want


def _check_exact(tcnn, oracle, cfg, n_in, n, tails_per_step, max_level=None, accumulate=True):
    from tinycudann.native import GRADIENT_ACCUMULATE, GRADIENT_OVERWRITE

    modes = (GRADIENT_OVERWRITE, GRADIENT_ACCUMULATE) if accumulate else (GRADIENT_OVERWRITE,)
    passes = 0
    for tr, got, want in _exact_steps(tcnn, oracle, cfg, n_in, n, modes, max_level):
        passes += 1
        assert tr.last_step_kernel() == "r32"
        assert tr.list_scatters() == passes, "the list-fed gradient kernel did not run"
        assert tr.list_gradient_tails() == passes * tails_per_step, "dL/dy came into list order by the other path"
        assert np.count_nonzero(want) > 100_000
        assert np.array_equal(got, want), f"pass {passes}"


def test_tail_gradients_match_oracle_2d(tcnn, oracle):
    """BASELINE config 3a's grid (2-D, F = 2, L = 16, T = 2^19) at the smallest batch that takes the tail, default switches, Overwrite and then
    Accumulate: the grid's gradient bit for bit the oracle's exact scatter; 256 items on every level, 13 listed levels."""
    _check_exact(tcnn, oracle, CONFIG_C3A, 2, N_2D, 1)


def test_tail_gradients_match_oracle_3d(tcnn, oracle, monkeypatch):
    """3-D (items of 512 samples: two trips per workgroup, four cell rows per sample) at the smallest batch that takes the tail"""
    _setenv(monkeypatch, R32)
    _check_exact(tcnn, oracle, CONFIG_3D, 3, N_3D, 1)


FALLBACKS = [
    # (id, config, n_in, n, environment, max_level)
    ("two_trips_per_item_of_four", CONFIG_C3A, 2, 1 << 17, {**R32, "TCNN_AMD_SCATTER_LISTS": "1"}, None),  # trips x 256 = 512, the item 1024
    ("four_trips_per_item_of_two", CONFIG_3D, 3, 1 << 18, {}, None),                                      # trips x 256 = 1024, the item 512
    ("unequal_trips", CONFIG_C3A, 2, N_2D + 256, {}, None),  # not whole windows per workgroup (the batch granularity is the window: one window more)
    ("scalar_max_level", CONFIG_C3A, 2, N_2D, {}, 0.5),
    ("switched_off", CONFIG_C3A, 2, N_2D, {"TCNN_AMD_LISTGRAD_IN_MLP": "0"}, None),
]


@pytest.mark.parametrize("name,cfg,n_in,n,env,max_level", FALLBACKS, ids=[c[0] for c in FALLBACKS])
def test_fallbacks_keep_the_separate_pass(tcnn, oracle, monkeypatch, name, cfg, n_in, n, env, max_level):
    """Wherever a workgroup of the MLP kernel does not produce one whole item, under a max_level cut-off and with the switch off the tail
    is not taken (the counter stays 0), the list-fed kernel runs behind k_grid_list_gradients -- which reads the items through the same
    map -- and the gradient is the oracle's, bit for bit."""
    _setenv(monkeypatch, env)
    _check_exact(tcnn, oracle, cfg, n_in, n, 0, max_level, accumulate=max_level is None)


def test_whole_steps_on_the_tail_match_oracle(tcnn, oracle):
    """Two consecutive training_step()s with the optimizer, on different batches, both on the tail: output, loss, loss values, dL/doutput and
    the parameters after Adam against the oracle trainer, at the bars of test_training_step_matches_oracle (tests/test_gpu_parity.py:
    restated below, its literals cannot be imported).  dL/dinput is not asked for: a step that prepares input gradients encodes rows, not
    level planes, and writes no hit lists."""
    n, n_in, cfg = N_2D, 2, CONFIG_C3A
    ref = oracle.Trainer(n_in, 3, cfg, seed=1337)
    tr = tcnn.Trainer(n_in, 3, cfg, seed=1337)
    p0 = ref.params_fp.copy()
    for step in range(2):
        x, t = oracle.synthetic_batch(n, n_in, 3, seed=42 + step)
        if step > 0:
            # Adam's first update moves every touched parameter by about lr sign(g), two orders above the grid's initial values: where the two
            # gradients round to different signs the parameters part by 2 lr.  The second step is compared from the SAME parameters (the
            # oracle keeps its own optimizer state, which is within the gradients' tolerance of the other).
            ref.params_fp[:] = tr.params_full_precision().cpu().numpy()
            ref.params[:] = oracle.half_bits(ref.params_fp)
            assert np.array_equal(ref.params, _bits(tr.params()))
        grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
        before = ref.params_fp.copy()
        want = ref.training_step(x, t, run_optimizer=True, grads_f32=grads32)
        ctx = tr.training_step(_t(x), _t(t), run_optimizer=True)
        assert tr.list_gradient_tails() == step + 1 and tr.list_scatters() == step + 1 and tr.last_step_kernel() == "r32"
        got_out, want_out = _f32(_bits(ctx.output())), _f32(want["output"])
        assert rel_err(got_out[:, :3], want_out[:, :3]) < 1e-2
        assert elem_close(got_out[:, :3], want_out[:, :3]) <= 1.0
        assert abs(tr.loss(ctx) - want["loss"]) <= 2e-2 * abs(want["loss"])
        assert rel_err(ctx.L().cpu().numpy(), want["L"]) < 3e-2
        got_dy, want_dy = _f32(_bits(ctx.dL_doutput())).reshape(n, -1), _f32(want["dL_doutput"]).reshape(n, -1)
        assert elem_close(got_dy[:, :3], want_dy[:, :3], rtol=3e-2) <= 1.0
        n_net = ref.model.network.n_params
        g = _f32(_bits(tr.param_gradients()))
        assert rel_err(g[:n_net], grads32[:n_net]) < 3e-2
        ge, we = g[n_net:], grads32[n_net:]
        assert float(np.linalg.norm(ge - we)) <= 5e-2 * float(np.linalg.norm(we))
        # entries never touched stay exactly zero (adam.h:76-79 relies on it).  Untouched: no corner weight of any sample on the entry -- the
        # exact scatter of an all-ones dL/dy leaves it zero.  (Not "the oracle's fp32 sum is zero": among 2^18 samples x 64 corner rows one
        # touched entry's fp32 sum cancels to 0 where the exact sum rounds to 2^-24 -- measured on the second batch: 1 of 2 139 809.)
        ones = np.full((n, ref.model.encoding.padded_output_width), oracle.half_bits(np.float32([1.0]))[0], dtype=np.uint16)
        untouched = ref.model.encoding.backward_exact(x, ones, np.zeros(ref.model.encoding.n_params, dtype=np.uint16)) == 0
        assert np.count_nonzero(untouched) > 1_000_000 and np.all(we[untouched] == 0)
        assert np.all(ge[untouched] == 0)
        # Adam ran: where the gradient is clearly non-zero the updates' signs agree
        upd_got, upd_want = tr.params_full_precision().cpu().numpy() - before, ref.params_fp - before
        big = np.abs(grads32) > 1e-3 * np.max(np.abs(grads32))
        assert np.mean(np.sign(upd_got[big]) == np.sign(upd_want[big])) > 0.99
    assert tr.optimizer_step_count() == 2
    assert np.any(tr.params_full_precision().cpu().numpy() != p0)


def test_tail_is_deterministic_and_equals_the_separate_pass(tcnn, oracle, monkeypatch):
    """The same two steps from the same parameters, twice on the tail and once with TCNN_AMD_LISTGRAD_IN_MLP=0: identical bits for the
    gradients after the first step and for the parameters after the second -- the fixed-point sums do not depend on the order of the
    elements, and the MLP kernel's own results do not depend on its tail."""
    n, n_in, cfg = N_2D, 2, CONFIG_C3A
    batches = [oracle.synthetic_batch(n, n_in, 3, seed=7 + s) for s in range(2)]

    def run(env, tails):
        _setenv(monkeypatch, env)
        tr = tcnn.Trainer(n_in, 3, cfg, seed=1337)
        res = []
        for x, t in batches:
            ctx = tr.training_step(_t(x), _t(t), run_optimizer=True)
            res += [_bits(tr.param_gradients()).copy(), _bits(ctx.output()).copy()]
        res.append(tr.params_full_precision().cpu().numpy().view(np.uint32).copy())
        assert tr.list_gradient_tails() == tails and tr.list_scatters() == 2
        for k in env:
            monkeypatch.delenv(k)
        return res

    a, b, c = run({}, 2), run({}, 2), run({"TCNN_AMD_LISTGRAD_IN_MLP": "0"}, 0)
    assert np.any(a[0] != 0)
    for i, (u, v, w) in enumerate(zip(a, b, c)):
        assert np.array_equal(u, v), f"two runs on the tail differ in result {i}"
        assert np.array_equal(u, w), f"the tail and the separate pass differ in result {i}"
