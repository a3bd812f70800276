"""Adam on every route it takes -- k_adam (quads, matrix / grid boundary on and off a quad's edge), k_adam_scalar (an unaligned base),
k_adam_prologue and k_wgrad_reduce_adam (a trainer's fused step) -- from crafted state, bit for bit against tests/adam_reference.py.

What is crafted reaches both sides of every range test in adam_device.h and every lookup of the debiasing table:
  gradients       +-0, the smallest and largest half denormals, the smallest and largest normal halves, +-inf, NaN, among log-uniform ones,
                  with all-zero quads and quads with one zero lane behind the matrix weights (adam_reference.gradient_bits)
  second moments  0, fp32 denormals, the smallest normal, values on both sides of 2^-96 and 2^32 (the fast square root's bounds), up to 1e30
  weights         +-0 among ordinary ones
  step counts     lagging the optimizer's own by 0, 1, 300 (uint16 counts) and 70 000 (uint32 counts), or by up to 11 of 12
  epsilon         1e-15 and 1e-8; loss scales 100 (no power of two: g / loss_scale) and 128 (the exact reciprocal)

The debiasing factor sqrtf(1 - powf(beta2, t)) / (1 - powf(beta1, t)) is the one place where the two sides do not run the same IEEE
operations (powf).  So that bits can be compared all the same, the counts are chosen where any powf within a few float steps gives the same
factor: with (0.9, 0.99) every count is at least 2000, where both powers are below 2^-25 and the factor is 1.0f exactly; the factors that
differ from count to count are met with beta1 = beta2 = 0.5 at counts 1 .. 13, where the powers are powers of two.

NaN: a result that is NaN on both sides counts as equal whatever its payload (IEEE 754 leaves it open, numpy and the device differ).
Infinite and NaN gradients poison both moments together, so the clamps' different NaN conventions (fmaxf drops a NaN, np.maximum keeps
it) are never decisive: the product with the first moment is NaN either way."""
import numpy as np
import pytest

import adam_reference as ar
from conftest import CONFIG_C2, CONFIG_C3B

F = np.float32
N = 4096
SPECIAL_HALVES = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00], dtype=np.uint16)
SECOND_MOMENTS = np.array([0.0, 1e-45, 1e-40, 1.1754944e-38, 1e-30, 1.2e-29, 1.3e-29, 1e-20, 1e-10, 1e-4, 1.0, 4.2e9, 4.4e9, 1e20, 1e30], dtype=np.float64)

# name: (common step, lags, beta1, beta2, epsilon, loss scale)
STATES = {
    "u16": (2400, (0, 1, 300), 0.9, 0.99, 1e-15, 100.0),
    "u32": (72100, (0, 1, 300, 70000), 0.9, 0.99, 1e-8, 128.0),
    "index": (12, (0, 1, 3, 5, 11), 0.5, 0.5, 1e-15, 100.0),
}
# name: (layers, elements the tensors' base is shifted by, fp32 gradients)
ROUTES = {
    "quad_uniform": ([(16, 32), (32, 8)], 0, False),  # n_matrix = 768: k_adam<QUAD_UNIFORM>
    "quad_mixed": ([(16, 31), (31, 9)], 0, False),    # n_matrix = 775: the boundary inside a quad
    "quad_mixed_fp32": ([(16, 31), (31, 9)], 0, True),
    "scalar": ([(16, 31), (31, 9)], 1, False),        # no 16-byte alignment: k_adam_scalar
}
N_STEPS = 3


def crafted_state(n, common, lags, seed=11):
    rs = np.random.RandomState(seed)
    i = np.arange(n)
    m2 = (SECOND_MOMENTS[i % len(SECOND_MOMENTS)] * rs.uniform(1.0, 1.03, n)).astype(F)
    m1 = (rs.standard_normal(n) * 1e-3).astype(F)
    m1[5::17] = F(0.0)
    m1[6::17] = F(1e-41)
    steps = (common - np.asarray(lags, dtype=np.int64)[(i // 3) % len(lags)]).astype(np.uint32)
    return m1, m2, steps


def crafted_gradients(n, n_matrix, step):
    g = ar.gradient_bits(n, n_matrix, step).copy()
    at = np.flatnonzero(np.arange(n) % 8 == (3 + step) % 8)
    g[at] = SPECIAL_HALVES[(at // 8 + step) % len(SPECIAL_HALVES)]
    return g


def same_f32(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def same_f16(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.uint16), np.ascontiguousarray(b, dtype=np.uint16)
    return (a == b) | (np.isnan(a.view(np.float16)) & np.isnan(b.view(np.float16)))


def assert_same_state(got, want, what):
    for key, same in (("m1", same_f32), ("m2", same_f32), ("w_fp", same_f32), ("w_half", same_f16)):
        bad = np.flatnonzero(~same(got[key], want[key]))
        assert bad.size == 0, f"{what}: {key} differs in {bad.size} places, first at {bad[0]}: {got[key][bad[0]]!r} != {want[key][bad[0]]!r}"
    bad = np.flatnonzero(np.asarray(got["steps"], dtype=np.uint32) != want["steps"])
    assert bad.size == 0, f"{what}: step counts differ in {bad.size} places, first at {bad[0]}: {got['steps'][bad[0]]} != {want['steps'][bad[0]]}"


def reference(cfg, n, n_matrix, common, m1, m2, steps):
    ref = ar.AdamVariant(cfg, n, n_matrix)
    ref.m1, ref.m2, ref.steps, ref.current_step = m1.copy(), m2.copy(), steps.copy(), common
    return ref


def optimizer_state(blob):
    import msgpack

    s = msgpack.unpackb(blob, raw=False)
    return {"m1": np.frombuffer(s["first_moments_binary"], dtype=F), "m2": np.frombuffer(s["second_moments_binary"], dtype=F),
            "steps": np.frombuffer(s["param_steps_binary"], dtype=np.uint32)}


def with_state(snapshot, common, m1, m2, steps):
    snapshot = dict(snapshot)
    snapshot.update(current_step=int(common), first_moments_binary=m1.tobytes(), second_moments_binary=m2.tobytes(), param_steps_binary=steps.astype(np.uint32).tobytes())
    return snapshot


@pytest.mark.gpu
@pytest.mark.parametrize("state", list(STATES))
@pytest.mark.parametrize("route", list(ROUTES))
def test_standalone_optimizer_from_crafted_state(tcnn, route, state):
    import msgpack
    import torch

    common, lags, beta1, beta2, epsilon, loss_scale = STATES[state]
    layers, shift, fp32_gradients = ROUTES[route]
    n_matrix = ar.n_matrix_of(layers)
    cfg = {"otype": "Adam", "learning_rate": 1e-2, "beta1": beta1, "beta2": beta2, "epsilon": epsilon, "l2_reg": 1e-6}
    m1, m2, steps = crafted_state(N, common, lags)
    opt = tcnn.optimizers.NativeOptimizer(cfg, N, layers)
    opt.deserialize(msgpack.packb(with_state(msgpack.unpackb(opt.serialize(), raw=False), common, m1, m2, steps), use_bin_type=True))
    ref = reference(cfg, N, n_matrix, common, m1, m2, steps)

    def on_device(a):  # a tensor of a.size elements whose base lies `shift` elements behind an allocation's
        buf = torch.zeros(a.size + 8, dtype=torch.from_numpy(a[:1]).dtype, device="cuda")
        view = buf[shift:shift + a.size]
        view.copy_(torch.from_numpy(a))
        assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (shift == 0)
        return view

    w_fp = ar.initial_weights(N)
    lagging = False
    for s in range(N_STEPS):
        g = crafted_gradients(N, n_matrix, s)
        skipped = ar.skipped_mask(cfg, N, n_matrix, g, loss_scale)
        w_half = ar.half_with_sentinel(w_fp, skipped)
        want = ref.step(loss_scale, w_fp, w_half, g)
        w_fp_t, w_half_t = on_device(w_fp), on_device(w_half.view(np.float16))
        g_t = on_device(ar.half_to_float(g)) if fp32_gradients else on_device(g.view(np.float16))
        opt.step(w_fp_t, w_half_t, g_t, loss_scale)
        torch.cuda.synchronize()
        got = {"w_fp": w_fp_t.cpu().numpy(), "w_half": w_half_t.cpu().numpy().view(np.uint16), **optimizer_state(opt.serialize())}
        assert_same_state(got, want, f"{route}/{state} step {s + 1}")
        assert opt.step_count() == common + s + 1
        lagging |= bool(np.any(want["steps"][~skipped] < common + s + 1))
        assert np.any(skipped) and np.any(np.isnan(want["w_fp"])) and np.any(np.isfinite(want["w_fp"]) & ~skipped)
        w_fp = want["w_fp"]
    assert lagging, "no updated parameter had a count of its own"


TRAINERS = {
    "prologue": CONFIG_C3B,   # HashGrid + 64 x 2: k_adam_prologue steps everything
    "in_reduce": CONFIG_C2,   # OneBlob + 64 x 2: k_wgrad_reduce_adam steps the weights behind their slab sums
}


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["u16", "u32"])
@pytest.mark.parametrize("route", list(TRAINERS))
def test_trainer_step_from_crafted_state(tcnn, oracle, route, state):
    """A 64 x 2 trainer at n = 256, three fused training steps (loss scale 128) from crafted moments, counts and +-0 weights; the gradients
    are the step's own, read back after it."""
    import msgpack
    import torch

    common, lags, _, _, _, _ = STATES[state]
    cfg = TRAINERS[route]
    opt_cfg = cfg["optimizer"]
    tr = tcnn.Trainer(2, 3, cfg, seed=1337)
    n = tr.n_params
    n_matrix = oracle.Trainer(2, 3, cfg, seed=1337).model.network.n_params
    m1, m2, steps = crafted_state(n, common, lags)
    snapshot = msgpack.unpackb(tr.serialize(True), raw=False)
    snapshot["optimizer"] = with_state(snapshot["optimizer"], common, m1, m2, steps)
    tr.deserialize(msgpack.packb(snapshot, use_bin_type=True))
    w = tr.params_full_precision().cpu().numpy()
    w[3::22] = F(0.0)
    w[14::22] = F(-0.0)
    tr.set_params_full_precision(torch.from_numpy(w).cuda())
    ref = reference(opt_cfg, n, n_matrix, common, m1, m2, steps)
    for s in range(3):
        x, t = oracle.synthetic_batch(256, 2, 3, seed=90 + s)
        w_fp, w_half = tr.params_full_precision().cpu().numpy(), tr.params().cpu().numpy().view(np.uint16)
        ctx = tr.training_step(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda())
        g = tr.param_gradients().cpu().numpy().view(np.uint16)
        want = ref.step(tr.default_loss_scale, w_fp, w_half, g)
        got = {"w_fp": tr.params_full_precision().cpu().numpy(), "w_half": tr.params().cpu().numpy().view(np.uint16),
               **optimizer_state(msgpack.packb(msgpack.unpackb(tr.serialize(True), raw=False)["optimizer"], use_bin_type=True))}
        assert_same_state(got, want, f"{route}/{state} step {s + 1}")
        assert np.any(g[:n_matrix] & 0x7FFF) and np.all(want["steps"][:n_matrix] == steps[:n_matrix] + s + 1)
        del ctx
    if route == "prologue":  # (a step whose gradient launch is timed for the scatter plan keeps its finalize launch and runs k_adam)
        assert tr.optimizer_prologue_steps() >= 1 and np.any(want["steps"][n_matrix:] != steps[n_matrix:]) and np.any(want["steps"][n_matrix:] == steps[n_matrix:])
    else:
        assert tr.params_updated_in_flush() == n == n_matrix
