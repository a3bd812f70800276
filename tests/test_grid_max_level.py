"""max_level of the grid encodings on the GPU (the reference's GridEncoding::set_max_level / set_max_level_gpu, grid_interface.h:101-123;
kernels grid.h:67-90, :237-245, :377-384, :482-490).  Every comparison is against the same module or trainer with max_level unset, on
identical inputs: below the cut-off the bits are those of the unrestricted run, above it the outputs are zero, the gradients zero
(Overwrite) or untouched (Accumulate)."""
import numpy as np
import pytest

from conftest import CONFIG_C3A

pytestmark = pytest.mark.gpu

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- the rule in numpy
def threshold(ml, L, F):
    """the reference's fp32 expressions: (ml * (L*F)) / F + 1e-3f"""
    ml = np.asarray(ml, dtype=F32)
    return (ml * F32(L * F)) / F32(F) + F32(1e-3)


def off_mask(ml, L, F, gradient_rule):
    """[n][L] (or [L] for a scalar) bool: level off by the forward rule (l >= t) or the gradient rule (l > t); NaN: every level on"""
    t = threshold(ml, L, F)
    lv = np.arange(L, dtype=F32)
    t = t[..., None]
    with np.errstate(invalid="ignore"):
        return lv > t if gradient_rule else lv >= t


def levels_on(ml, L, F, gradient_rule):
    m = off_mask(ml, L, F, gradient_rule)
    return int(np.argmax(m)) if m.any() else L


def tie_value(L, F):
    """a float32 ml with (ml * L*F) / F + 1e-3f exactly an integer k: level k outputs zeros but receives gradients"""
    for k in range(L // 2, L):
        base = F32((k - 1e-3) / L)
        cand = base
        for _ in range(400):
            for c in (cand, F32(2 * base - cand)):
                if threshold(c, L, F) == F32(k):
                    return float(c), k
            cand = np.nextafter(cand, F32(1), dtype=F32)
    raise AssertionError("no tie value found")


def test_tie_value_of_the_issue():
    v, k = tie_value(16, 2)
    assert threshold(F32(0.4999375), 16, 2) == F32(8.0)
    assert levels_on(F32(0.4999375), 16, 2, False) == 8 and levels_on(F32(0.4999375), 16, 2, True) == 9
    assert threshold(v, 16, 2) == F32(k)


# ---------------------------------------------------------------------------------------------------------------- helpers
def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    a = _np(t)
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32)


def _inputs(n, n_in, width, seed, dtype):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(n, n_in, device="cuda", generator=g) * 0.98 + 0.01
    dy = (torch.rand(n, width, device="cuda", generator=g) * 2 - 1).to(dtype)
    return x.contiguous(), dy.contiguous()


def _module(tcnn, n_in, cfg, dtype=None, seed=1):
    import torch

    enc = tcnn.Encoding(n_in, cfg, seed=seed, dtype=dtype)
    with torch.no_grad():  # parameters of a trained size, so that every level's output differs from zero
        enc.params.copy_((torch.rand_like(enc.params) * 2 - 1))
    return enc


def _level_params(oracle, n_in, cfg):
    ref = oracle.create_encoding(n_in, cfg, alignment=0)
    F = cfg.get("n_features_per_level", 2)
    return (ref.offsets.astype(np.int64) * F), F


def _fwd(native, x, p, need_dx=False):
    xx = x.detach().requires_grad_(need_dx)
    pp = p.detach().requires_grad_(True)
    ctx, out = native.fwd(xx, pp)
    return ctx, out, xx, pp


def _grads(native, x, p, dy, need_dx=False):
    ctx, out, xx, pp = _fwd(native, x, p, need_dx)
    gx, gp = native.bwd(ctx, xx, pp, out, dy)
    return out, gx, gp


FWD_CASES = [
    (2, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16, "per_level_scale": 1.5}, None),
    (3, {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 4, "log2_hashmap_size": 14, "base_resolution": 8, "per_level_scale": 2.0, "interpolation": "Smoothstep"}, None),
    (2, {"otype": "DenseGrid", "n_levels": 6, "n_features_per_level": 1, "base_resolution": 8, "per_level_scale": 1.5}, None),
    (3, {"otype": "TiledGrid", "n_levels": 4, "n_features_per_level": 8, "base_resolution": 8, "per_level_scale": 1.5, "interpolation": "Nearest"}, None),
    (2, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16, "per_level_scale": 1.5}, "float32"),
    (3, {"otype": "HashGrid", "n_levels": 12, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16, "per_level_scale": 1.5}, None),
]


def _settings(L, F):
    return [0.0, 0.3, 0.5, tie_value(L, F)[0], 1.0, 1000.0, float("nan")]


@pytest.mark.parametrize("n_in,cfg,dtype", FWD_CASES)
def test_forward_scalar(tcnn, n_in, cfg, dtype):
    import torch

    dt = getattr(torch, dtype) if dtype else None
    enc = _module(tcnn, n_in, cfg, dt)
    native = enc.native_tcnn_module
    L, F = cfg["n_levels"], cfg["n_features_per_level"]
    x, _ = _inputs(4096, n_in, enc.n_output_dims, 0, torch.half)
    p = enc.params.detach().to(enc.dtype).contiguous()
    with torch.no_grad():
        _, full = native.fwd(x, p)  # inference form (level planes where the grid takes them)
    _, full_aos, _, _ = _fwd(native, x, p, need_dx=True)  # AoS kernel with dy_dx
    for ml in _settings(L, F):
        native.set_max_level(ml)
        with torch.no_grad():
            _, got = native.fwd(x, p)
        _, got_aos, _, _ = _fwd(native, x, p, need_dx=True)
        on = levels_on(F32(ml), L, F, False)
        for a, b in ((got, full), (got_aos, full_aos)):
            assert np.array_equal(_bits(a)[:, : on * F], _bits(b)[:, : on * F]), ml
            assert not np.any(_bits(a)[:, on * F: L * F]), ml
            assert np.array_equal(_bits(a)[:, L * F:], _bits(b)[:, L * F:])
        native.set_max_level(1000.0)


# (n_in, cfg, n, env): each one selects a path of the gradient kernels (the switches are read when the module is created)
C3A_ENC = CONFIG_C3A["encoding"]
GRAD_CASES = [
    ("lists", 2, C3A_ENC, 1 << 18, {}),
    ("bitplanes", 2, C3A_ENC, 1 << 16, {"TCNN_AMD_SCATTER_LISTS": "0"}),
    ("records_off", 2, C3A_ENC, 1 << 16, {"TCNN_AMD_SCATTER_RECORDS": "0"}),
    ("aos_forward", 2, C3A_ENC, 1 << 16, {"TCNN_AMD_GRID_PLANES": "0"}),
    ("rows_forward", 2, C3A_ENC, 1 << 16, {"TCNN_AMD_GRID_ROWS_PLANES": "0"}),
    ("binned", 3, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 4, "log2_hashmap_size": 22, "base_resolution": 16, "per_level_scale": 2.0}, 1 << 12, {}),
    ("f1", 2, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 1, "log2_hashmap_size": 15, "base_resolution": 16, "per_level_scale": 1.5}, 1 << 14, {}),
]
ATOMIC = ("atomic", 2, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16, "per_level_scale": 1.5}, 1 << 14,
          {"TCNN_AMD_GRID_SCATTER": "atomic"})


def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name,n_in,cfg,n,env", GRAD_CASES + [ATOMIC], ids=[c[0] for c in GRAD_CASES + [ATOMIC]])
def test_gradients_scalar(tcnn, oracle, monkeypatch, name, n_in, cfg, n, env):
    import torch

    _env(monkeypatch, env)
    enc = _module(tcnn, n_in, cfg)
    native = enc.native_tcnn_module
    L, F = cfg["n_levels"], cfg["n_features_per_level"]
    starts, _ = _level_params(oracle, n_in, cfg)
    assert starts[-1] == native.n_params()
    x, dy = _inputs(n, n_in, enc.n_output_dims, 1, torch.half)
    p = enc.params.detach().half().contiguous()
    _, _, g_full = _grads(native, x, p, dy)
    exact = name not in ("atomic", "f1")  # (global float atomics, in arbitrary order: F = 1 sums in an fp32 scratch that way)
    for ml in (0.5, tie_value(L, F)[0], 0.3, 0.0):
        native.set_max_level(ml)
        before = native.list_scatters()
        out, _, g = _grads(native, x, p, dy)
        if name == "lists":
            assert native.list_scatters() == before + 1
        on, cut = levels_on(F32(ml), L, F, False), levels_on(F32(ml), L, F, True)
        head = int(starts[cut])
        if exact:
            assert np.array_equal(_bits(g)[:head], _bits(g_full)[:head]), ml
        else:
            a, b = _np(g)[:head].astype(np.float64), _np(g_full)[:head].astype(np.float64)
            assert np.linalg.norm(a - b) <= 2e-2 * np.linalg.norm(b)
        assert not np.any(_bits(g)[head:]), ml  # +0 everywhere (Overwrite)
        assert not np.any(_bits(out)[:, on * F:])
        if cut > on:  # the tie: level `on` outputs zeros and still receives gradients
            lvl = slice(int(starts[on]), int(starts[on + 1]))
            assert np.any(_bits(g)[lvl]) and (not exact or np.array_equal(_bits(g)[lvl], _bits(g_full)[lvl]))
    native.set_max_level(1000.0)


def test_accumulate_leaves_the_off_levels_untouched(tcnn, oracle):
    """Trainer.backward with GRADIENT_ACCUMULATE: the skipped levels' gradients keep their bits, negative zeros included"""
    import torch

    from tinycudann import _C
    from tinycudann.native import GRADIENT_ACCUMULATE, GRADIENT_OVERWRITE, Trainer

    tr = Trainer(2, 1, CONFIG_C3A, seed=3)
    n = 1 << 16
    x = torch.rand(n, 2, device="cuda")
    y = torch.rand(n, 1, device="cuda")
    tr.backward(tr.forward(x, y), x, gradient_mode=GRADIENT_OVERWRITE)
    g0 = tr.param_gradients()
    g0[-64:] = -0.0
    torch.cuda.synchronize()
    _C.memcpy_dtod(_C.lib.tcnn_trainer_param_gradients(tr._h), g0.data_ptr(), g0.numel() * 2)
    tr.set_max_level(0.5)
    tr.backward(tr.forward(x, y), x, gradient_mode=GRADIENT_ACCUMULATE)
    g1 = tr.param_gradients()
    ref = oracle.create_encoding(2, CONFIG_C3A["encoding"], alignment=0)
    F = CONFIG_C3A["encoding"]["n_features_per_level"]
    first = tr.n_params - int(ref.offsets[-1]) * F
    tail = first + int(ref.offsets[levels_on(F32(0.5), 16, 2, True)]) * F
    assert np.array_equal(_bits(g1)[tail:], _bits(g0)[tail:])
    assert np.all(_bits(g1)[-64:] == 0x8000)
    assert not np.array_equal(_bits(g1)[first:tail], _bits(g0)[first:tail])  # the levels that are on did accumulate


def test_per_sample(tcnn, oracle):
    """random ml per row with ties: outputs = unrestricted with the off (row, level) pairs zeroed; parameter gradients = the
    unrestricted run fed with dL/dy masked by the gradient rule, bit for bit; dL/dx and the second-order results likewise"""
    import torch

    cfg = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16, "per_level_scale": 1.5}
    L, F = 16, 2
    tie, _ = tie_value(L, F)
    for env in ({}, {"TCNN_AMD_SCATTER_LISTS": "0"}, {"TCNN_AMD_GRID_SCATTER": "atomic"}):
        mp = pytest.MonkeyPatch()
        for k, v in env.items():
            mp.setenv(k, v)
        try:
            enc = _module(tcnn, 2, cfg)
            native = enc.native_tcnn_module
            n = 1 << 16
            x, dy = _inputs(n, 2, enc.n_output_dims, 5, torch.half)
            rs = np.random.RandomState(7)
            ml = rs.uniform(0, 1, n).astype(F32)
            ml[::7] = F32(tie)
            ml[::11] = F32(1000.0)
            ml[::13] = F32(0.0)
            mlt = _t(ml)
            p = enc.params.detach().half().contiguous()
            fwd_off = np.repeat(off_mask(ml, L, F, False), F, axis=1)
            bwd_off = np.repeat(off_mask(ml, L, F, True), F, axis=1)
            dy_masked = _t(np.where(bwd_off, np.float16(0), _np(dy)))
            out_full, _, g_masked = _grads(native, x, p, dy_masked)
            native.set_max_level_gpu(mlt)
            out, _, g = _grads(native, x, p, dy)
            native.set_max_level_gpu(None)
            want = np.where(fwd_off, np.uint16(0), _bits(out_full))
            assert np.array_equal(_bits(out), want)
            if not env:
                assert np.array_equal(_bits(g), _bits(g_masked))
            else:
                a, b = _np(g).astype(np.float64), _np(g_masked).astype(np.float64)
                assert np.linalg.norm(a - b) <= 2e-2 * np.linalg.norm(b) and (env.get("TCNN_AMD_GRID_SCATTER") or np.array_equal(_bits(g), _bits(g_masked)))
        finally:
            mp.undo()

    # input gradients and the second-order pass (fp32 parameters: the AoS kernel with dy_dx, the atomic gradient kernels)
    enc = _module(tcnn, 2, cfg, torch.float32)
    native = enc.native_tcnn_module
    n = 4096
    x, dy = _inputs(n, 2, enc.n_output_dims, 9, torch.float32)
    ml = np.random.RandomState(3).uniform(0, 1, n).astype(F32)
    ml[::5] = F32(tie)
    p = enc.params.detach().float().contiguous()
    fwd_off = np.repeat(off_mask(ml, L, F, False), F, axis=1)
    bwd_off = np.repeat(off_mask(ml, L, F, True), F, axis=1)
    v = torch.rand(n, 2, device="cuda") - 0.5
    # unrestricted, dL/dy masked by the forward rule (dy_dx is zero there): the same dL/dx
    _, gx_full, _ = _grads(native, x, p, _t(np.where(fwd_off, F32(0), _np(dy))), need_dx=True)
    ctx_f, out_f, xf, pf = _fwd(native, x, p, need_dx=True)
    dyb = _t(np.where(bwd_off, F32(0), _np(dy))).requires_grad_(True)
    ddy_f, dp_f, dx_f = native.bwd_bwd_input(ctx_f, xf, pf, v, dyb)
    native.set_max_level_gpu(_t(ml))
    _, gx, _ = _grads(native, x, p, dy, need_dx=True)
    ctx_r, out_r, xr, pr = _fwd(native, x, p, need_dx=True)
    ddy_r, dp_r, dx_r = native.bwd_bwd_input(ctx_r, xr, pr, v, dy.detach().requires_grad_(True))
    native.set_max_level_gpu(None)
    assert torch.equal(gx, gx_full)
    assert torch.equal(dx_r, dx_f)
    assert np.array_equal(_np(ddy_r), np.where(fwd_off, F32(0), _np(ddy_f)))
    a, b = _np(dp_r).astype(np.float64), _np(dp_f).astype(np.float64)
    assert np.linalg.norm(a - b) <= 2e-2 * np.linalg.norm(b)


def test_python_module_pads_the_per_sample_array(tcnn):
    import torch

    cfg = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 14, "base_resolution": 16, "per_level_scale": 1.5}
    enc = _module(tcnn, 3, cfg)
    n = 1000  # not a multiple of 256
    x = torch.rand(n, 3, device="cuda")
    ml = torch.rand(n, device="cuda")
    full = enc(x)
    enc.set_max_level_gpu(ml)
    assert enc.max_level_gpu is ml
    got = enc(x)
    enc.set_max_level_gpu(None)
    off = np.repeat(off_mask(_np(ml), 8, 2, False), 2, axis=1)
    assert np.array_equal(_bits(got), np.where(off, np.uint16(0), _bits(full)))
    with pytest.raises(RuntimeError, match="float32"):
        enc.set_max_level_gpu(ml.double())
    enc.set_max_level_gpu(ml[: n // 2])
    with pytest.raises(RuntimeError, match="holds"):
        enc(x)
    enc.set_max_level_gpu(None)


def test_autograd_uses_the_setting_of_the_forward_pass(tcnn):
    import torch

    cfg = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5, "interpolation": "Smoothstep"}
    enc = _module(tcnn, 3, cfg, torch.float32)
    x0 = torch.rand(512, 3, device="cuda") * 0.9 + 0.05
    w = torch.rand(enc.n_output_dims, device="cuda") - 0.5

    def run(change_to=None):
        enc.params.grad = None
        x = x0.clone().requires_grad_(True)
        y = enc(x)
        (g,) = torch.autograd.grad((y * w).sum(), x, create_graph=True)
        if change_to is not None:
            enc.set_max_level(change_to)
        (g.square().sum() + (y * w).sum()).backward()
        return y.detach(), x.grad.clone(), enc.params.grad.clone()

    def same(a, b):  # (the grid gradients of fp32 parameters are sums of float atomics in arbitrary order)
        scale = float(b[2].abs().max())
        return torch.equal(a[0], b[0]) and torch.allclose(a[1], b[1], rtol=1e-5, atol=1e-5) and torch.allclose(a[2], b[2], rtol=1e-3, atol=1e-5 * scale)

    enc.set_max_level(0.5)
    want = run()
    got = run(change_to=1000.0)  # changed between forward and backward: the backward passes keep 0.5
    assert enc.max_level == 1000.0
    assert same(got, want)
    full = run()
    assert not torch.equal(full[0], want[0]) and not torch.allclose(full[2], want[2], rtol=1e-3, atol=1e-5 * float(want[2].abs().max()))
    n_on = levels_on(F32(0.5), 8, 2, True)
    assert torch.all(want[0][:, levels_on(F32(0.5), 8, 2, False) * 2:] == 0) and n_on < 8


COMPOSITE_CFG = {
    "loss": {"otype": "L2"},
    "optimizer": CONFIG_C3A["optimizer"],
    "encoding": {"otype": "Composite", "nested": [dict(CONFIG_C3A["encoding"], n_dims_to_encode=3), {"otype": "SphericalHarmonics", "degree": 4, "n_dims_to_encode": 3}]},
    "network": CONFIG_C3A["network"],
}


@pytest.mark.parametrize("which", ["c3a", "composite"])
def test_trainer(tcnn, oracle, which):
    import torch

    from tinycudann.native import Trainer

    cfg, n_in = (CONFIG_C3A, 2) if which == "c3a" else (COMPOSITE_CFG, 6)
    n = 1 << 16 if which == "c3a" else 1 << 14
    tr = Trainer(n_in, 3, cfg, seed=11)
    assert tr.max_level == 1000.0
    snap = tr.serialize()
    tr.set_max_level(0.5)
    assert tr.max_level == 0.5 and tr.serialize() == snap  # not part of snapshots
    x = torch.rand(n, n_in, device="cuda")
    y = torch.rand(n, 3, device="cuda")
    grid_cfg = CONFIG_C3A["encoding"]
    ref = oracle.create_encoding(3 if which == "composite" else 2, grid_cfg, alignment=0)
    F = grid_cfg["n_features_per_level"]
    grid_params = int(ref.offsets[-1]) * F
    first = tr.n_params - grid_params  # the network's parameters first, then the grid's (spherical harmonics have none)
    per_sample = torch.rand(n, device="cuda")
    for setting in ("scalar", "array"):
        if setting == "array":
            tr.set_max_level(1000.0)
            tr.set_max_level_gpu(per_sample)
        ctx = tr.training_step(x, y, run_optimizer=False)
        step_out = ctx.output()[:, :3].float()
        inf = tr.inference(x)
        assert float((step_out - inf).abs().max()) <= 1e-2 * max(1.0, float(inf.abs().max()))
        # Overwrite through the split forward / backward: the off levels' entries are zero
        c = tr.forward(x, y)
        tr.backward(c, x)
        g = _bits(tr.param_gradients())
        if setting == "scalar":
            cut = levels_on(F32(0.5), 16, 2, True)
            assert not np.any(g[first + int(ref.offsets[cut]) * F: first + grid_params])
            assert np.any(g[first: first + int(ref.offsets[cut]) * F])
    tr.set_max_level_gpu(None)
    assert tr.max_level_gpu is None

    # coarse to fine: 50 steps with the cut-off ramping from 0.1 to 1
    losses = []
    for i in range(50):
        tr.set_max_level(0.1 + 0.9 * i / 49)
        losses.append(tr.loss(tr.training_step(x, y)))
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]

    # unset: one step here and one on a fresh trainer loaded with the same state give the same bits
    tr.set_max_level(1000.0)
    state = tr.serialize(serialize_optimizer=True)
    fresh = Trainer(n_in, 3, cfg, seed=11)
    fresh.deserialize(state)
    # (a snapshot holds the half-precision parameters: the two trainers' fp32 masters differ, so their first updates may too -- the
    # gradients of the same parameters and batch may not)
    ca, cb = tr.forward(x, y), fresh.forward(x, y)
    assert torch.equal(ca.output(), cb.output())
    tr.backward(ca, x)
    fresh.backward(cb, x)
    assert np.array_equal(_bits(tr.param_gradients()), _bits(fresh.param_gradients()))
    a = tr.training_step(x, y).output()
    b = fresh.training_step(x, y).output()
    assert torch.equal(a, b)
