"""Grid encodings of 1, 5, 6 and 7 input dimensions on the GPU (k_grid_nd.hip; the 1-D instantiations of k_grid.hip, k_grid_scatter.hip,
k_grid_bin.hip and k_grid_bwdbwd.hip; the rolled corner loops of k_grid_scatter.hip / k_grid_bin.hip) against tests/grid_nd_reference.py,
the numpy restatement that tests/test_grid_nd_reference.py pins to the CPU oracle.

  forward, dy/dx, dL/dx: a fixed order of operations -- bit for bit, half and float.
  parameter gradients, deterministic route (half, two or more features per level): the exact sum of the fp16 products rounded once -- bit for
    bit, twice the same bits, also with stochastic_interpolation and under a max_level cut-off.
  parameter gradients, atomic routes: tests/grid_reference.py's per-element bounds, gamma(k - 1) * sum |terms| at the unit roundoff of the
    additions, no entry excluded.
  second order: ||ours - R64|| <= 2 ||Rh - R64|| per result (tests/test_encoding_second_order.py's criterion: two realisations of the same
    rounding noise differ by sqrt(2) in norm; 2 is that rounded up).  dL_dinput of a Linear grid is exactly zero in ONE dimension only: in
    several the multilinear interpolant has mixed second derivatives (grid.h:560-620 computes them for every interpolation).
Which route a shape takes is asserted on the host by tests/test_grid_nd_host.py (the route functions are pure host code); here the
list-fed kernel's counter is checked to stay 0."""
import numpy as np
import pytest

from grid_nd_reference import PRODUCT_FP32, PRODUCT_HALF, PRODUCT_SCRATCH32, GridND
from grid_reference import MIN_CONTRIBUTION, U16, U32, check_rounded_sum_per_level, check_sum_per_level, edge_x, to_device

pytestmark = pytest.mark.gpu


def _cfg(otype, levels, F, log2_t, base, scale, **extra):
    return dict({"otype": otype, "n_levels": levels, "n_features_per_level": F, "log2_hashmap_size": log2_t, "base_resolution": base, "per_level_scale": scale}, **extra)


# per dimension: a dense level, (from 5-D on) a level whose stride loop exits early, hashed levels
SHAPES = {1: (6, 8, 4, 2.5), 5: (5, 10, 2, 1.5), 6: (4, 10, 2, 1.5), 7: (4, 11, 2, 2.0)}  # (levels, log2 T, base resolution, per-level scale)
FIRST_HASHED = {1: 5, 5: 2, 6: 2, 7: 1}
# (otype, F, extra): every F, hash / dense / tiled, the four hash functions, the three interpolations; output widths 5, 10, 8, 16, 32 ...
KINDS = [
    ("HashGrid", 2, {}), ("HashGrid", 1, {"hash": "Prime", "interpolation": "Smoothstep"}), ("HashGrid", 4, {"hash": "ReversedPrime"}),
    ("HashGrid", 8, {"hash": "Rng"}), ("DenseGrid", 2, {"interpolation": "Smoothstep"}), ("TiledGrid", 4, {"interpolation": "Nearest"}),
    ("HashGrid", 8, {"interpolation": "Nearest"}), ("DenseGrid", 1, {}),
]


def forward_cases():
    for D, (levels, log2_t, base, scale) in SHAPES.items():
        for otype, F, extra in KINDS:
            if extra.get("hash") == "Rng":
                levels_here = FIRST_HASHED[D] + 1  # (the restatement's pcg32 advance is 64 numpy steps per index: one hashed level)
            else:
                levels_here = levels
            yield D, _cfg(otype, levels_here, F, log2_t, base, scale, **extra)


def case_id(v):
    if isinstance(v, int):
        return f"{v}d"
    return f"{v['otype'][:-4]}-L{v['n_levels']}-F{v['n_features_per_level']}-T{v['log2_hashmap_size']}-b{v['base_resolution']}" + "".join(f"-{v[k]}" for k in ("interpolation", "hash") if k in v) + ("-stoch" if v.get("stochastic_interpolation") else "")


_INPUTS = {}


def inputs(D, cfg, n):
    """(restatement, x, params float32, dL/dy float32), computed once per case: n - 256 uniform rows and the 256 edge rows of
    tests/grid_reference.py (0, 1, their neighbours, negatives, > 1); parameters in [-1, 1); dL/dy in [-2, 2), every seventh row zero"""
    key = (D, case_id(cfg), n)
    if key not in _INPUTS:
        ref = GridND(D, cfg)
        rs = np.random.RandomState(17 + D)
        x = np.concatenate([rs.uniform(0, 1, (n - 256, D)), edge_x(256, D)]).astype(np.float32)
        params = rs.uniform(-1, 1, ref.n_params).astype(np.float32)
        dy = rs.uniform(-2, 2, (n, ref.n_output_dims)).astype(np.float32)
        dy[::7] = 0
        for a in (x, params, dy):
            a.setflags(write=False)
        _INPUTS[key] = (ref, x, params, dy)
    return _INPUTS[key]


def module(tcnn, D, cfg, fp32):
    import torch

    enc = tcnn.Encoding(D, cfg, dtype=torch.float32) if fp32 else tcnn.Encoding(D, cfg)
    native = enc.native_tcnn_module
    return enc, native


def same_bits(got, want, what):
    view = np.uint32 if want.dtype == np.float32 else np.uint16
    differ = np.ascontiguousarray(got).view(view) != np.ascontiguousarray(want).view(view)
    assert got.shape == want.shape and not np.any(differ), (
        f"{what}: {int(np.count_nonzero(differ))} of {differ.size} values differ, first at {tuple(np.argwhere(differ)[0])}: got {got[differ][0]!r}, want {want[differ][0]!r}")


# ---------------------------------------------------------------------------------------------------- forward, dy/dx, dL/dx
@pytest.mark.parametrize("fp32", [False, True], ids=["half", "float"])
@pytest.mark.parametrize("D,cfg", list(forward_cases()), ids=case_id)
def test_forward_and_input_gradients_bit_exact(tcnn, D, cfg, fp32):
    n = 512
    ref, x, params, dy = inputs(D, cfg, n)
    T = np.float32 if fp32 else np.float16
    p, d = params.astype(T), dy.astype(T)
    want, want_dy_dx = ref.forward(x, p, want_dy_dx=True)
    enc, native = module(tcnn, D, cfg, fp32)
    assert native.n_output_dims() == ref.n_output_dims and native.n_params() == ref.n_params  # (an Encoding module pads to a multiple of F: nothing)
    xt, pt = to_device(x).requires_grad_(True), to_device(p).requires_grad_(True)
    ctx, out = native.fwd(xt, pt)
    same_bits(out.cpu().numpy(), want, f"{D}-D {case_id(cfg)} output")
    assert np.any(want != 0)
    dx, _ = native.bwd(ctx, xt, pt, out, to_device(d))
    want_dx = ref.backward_input(want_dy_dx, d)
    same_bits(dx.cpu().numpy(), want_dx, f"{D}-D {case_id(cfg)} dL/dx")
    # inference (no context) gives the same bits; dy/dx itself, row by row: d output[k] / d input at backprop_scale 1 is 0 + 1 * dy_dx[k]
    with_out = native.fwd(to_device(x), to_device(p))[1]
    same_bits(with_out.cpu().numpy(), want, "inference output")
    jac, _ = native.input_jacobian(to_device(x), to_device(p), list(range(ref.n_output_dims)), 1.0)
    jac = jac.cpu().numpy()
    assert np.array_equal(jac, want_dy_dx), f"dy/dx: {int(np.count_nonzero(jac != want_dy_dx))} values differ"
    if cfg.get("interpolation") == "Nearest":
        assert not np.any(want_dy_dx) and not np.any(dx.cpu().numpy().view(np.uint32))
    else:
        assert np.any(want_dx != 0)


COMPOSITE_GRID = _cfg("HashGrid", 5, 2, 10, 2, 1.5)
COMPOSITE = {"otype": "Composite", "nested": [dict(COMPOSITE_GRID, n_dims_to_encode=5, dims_to_encode_begin=1), {"otype": "Identity", "n_dims_to_encode": 1, "dims_to_encode_begin": 0}]}


def test_grid_behind_a_composite_slice(tcnn):
    """the grid reads columns 1 .. 5 of six: a sample stride that is not its own width (the kernels' general coordinate path)"""
    n = 512
    ref, x5, params, _ = inputs(5, COMPOSITE_GRID, n)
    x = np.ascontiguousarray(np.concatenate([np.linspace(0, 1, n, dtype=np.float32)[:, None], x5], axis=1))
    native = tcnn.Encoding(6, COMPOSITE).native_tcnn_module
    assert native.n_params() == ref.n_params
    p = params.astype(np.float16)
    out = native.fwd(to_device(x), to_device(p))[1].cpu().numpy()
    want, _ = ref.forward(x5, p)
    same_bits(np.ascontiguousarray(out[:, :ref.n_output_dims]), want, "grid columns of the composite")


# ---------------------------------------------------------------------------------------------------- parameter gradients: the exact route
EXACT_CASES = [
    (5, _cfg("HashGrid", 5, 2, 10, 2, 1.5)),                                  # every level one scatter chunk
    (5, _cfg("HashGrid", 4, 2, 15, 8, 2.0)),                                  # hashed levels of 4 chunks
    (5, _cfg("HashGrid", 4, 2, 18, 8, 2.0)),                                  # levels of 32 chunks: the binned kernels (as a 4-D grid of this shape)
    (5, _cfg("HashGrid", 5, 4, 10, 2, 1.5, interpolation="Smoothstep")),
    (5, _cfg("HashGrid", 5, 2, 10, 2, 1.5, interpolation="Nearest")),
    (5, _cfg("HashGrid", 3, 8, 10, 2, 1.5, hash="Rng")),
    (6, _cfg("HashGrid", 4, 2, 10, 2, 1.5)), (7, _cfg("HashGrid", 4, 4, 11, 2, 2.0)), (7, _cfg("DenseGrid", 3, 2, 11, 2, 2.0)),
    (1, _cfg("HashGrid", 6, 2, 8, 4, 2.5)), (1, _cfg("HashGrid", 6, 8, 8, 4, 2.5, interpolation="Smoothstep")),
]
STOCHASTIC_CASES = [(D, dict(cfg, stochastic_interpolation=True)) for D, cfg in (EXACT_CASES[0], EXACT_CASES[1], EXACT_CASES[2], EXACT_CASES[7], EXACT_CASES[9])]


def _half_gradient(tcnn, D, cfg, x, params_h, dy_h, max_level=None, env=None, monkeypatch=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    native = tcnn.Encoding(D, cfg).native_tcnn_module
    for k in (env or {}):
        monkeypatch.delenv(k)
    if max_level is not None:
        native.set_max_level(max_level)
    xt, pt = to_device(x), to_device(params_h).requires_grad_(True)
    ctx, out = native.fwd(xt, pt)
    _, g = native.bwd(ctx, xt, pt, out, to_device(dy_h))
    assert native.list_scatters() == 0  # hit lists stay with 2 and 3 dimensions
    return g.detach().cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("D,cfg", EXACT_CASES + STOCHASTIC_CASES, ids=case_id)
def test_exact_route_bit_exact_and_deterministic(tcnn, D, cfg):
    n = 512
    ref, x, params, dy = inputs(D, cfg, n)
    p, d = params.astype(np.float16), dy.astype(np.float16)
    want = ref.backward_exact(x, d)
    got = _half_gradient(tcnn, D, cfg, x, p, d)
    differ = got != want
    assert not np.any(differ), f"{int(np.count_nonzero(differ))} of {differ.size} gradient entries differ from the exact sum, first at {int(np.argwhere(differ)[0][0])}"
    assert np.any(want != 0)
    again = _half_gradient(tcnn, D, cfg, x, p, d)
    assert np.array_equal(got, again)


@pytest.mark.parametrize("D,cfg", [EXACT_CASES[1], EXACT_CASES[2], EXACT_CASES[7]], ids=case_id)
def test_exact_route_under_a_max_level_cut_off(tcnn, D, cfg):
    """max_level = 0.5 of four levels: m = 2, so levels l > 2 + 1e-3 receive no gradient (grid.h:237-245) -- level 3's entries are +0"""
    n = 512
    ref, x, params, dy = inputs(D, cfg, n)
    assert ref.n_levels == 4
    p, d = params.astype(np.float16), dy.astype(np.float16)
    masked = d.copy()
    masked[:, 3 * ref.F:] = 0
    want = ref.backward_exact(x, masked)
    first_off = int(ref.offsets[3]) * ref.F
    want[first_off:] = 0  # (Overwrite: +0, whatever the sign of a zero product)
    got = _half_gradient(tcnn, D, cfg, x, p, d, max_level=0.5)
    assert np.array_equal(got, want) and np.any(want[:first_off] != 0)


# ---------------------------------------------------------------------------------------------------- parameter gradients: the atomic routes
ATOMIC_CASES = [
    (5, _cfg("HashGrid", 5, 2, 10, 2, 1.5)), (5, _cfg("HashGrid", 4, 4, 15, 8, 2.0, interpolation="Smoothstep")), (7, _cfg("HashGrid", 4, 2, 11, 2, 2.0)),
    (6, _cfg("DenseGrid", 3, 8, 10, 2, 1.5)), (1, _cfg("HashGrid", 6, 2, 8, 4, 2.5)), (5, _cfg("HashGrid", 5, 2, 10, 2, 1.5, stochastic_interpolation=True)),
]
SCALAR_CASES = [(5, _cfg("HashGrid", 5, 1, 10, 2, 1.5)), (7, _cfg("HashGrid", 4, 1, 11, 2, 2.0, interpolation="Smoothstep")), (1, _cfg("HashGrid", 6, 1, 8, 4, 2.5)),
                (6, _cfg("HashGrid", 4, 1, 10, 2, 1.5, stochastic_interpolation=True))]
ATOMIC_ROWS = 256  # the packed-fp16 bound needs (k - 1) 2^-11 < 1 for every entry: few rows keep the coarse levels' counts below 2049


def _terms(ref, x, dy, product):
    t = ref.backward_terms(x, dy, product)
    assert t["min_nonzero"] >= MIN_CONTRIBUTION
    return t


@pytest.mark.parametrize("D,cfg", ATOMIC_CASES + SCALAR_CASES, ids=case_id)
def test_fp32_grid_gradient_per_element(tcnn, D, cfg):
    """k_grid_nd_bwd<float, float> / k_grid_bwd<float, float, 1, F>: weight * dL/dy in fp32, float atomics"""
    n = ATOMIC_ROWS
    ref, x, params, dy = inputs(D, cfg, n)
    enc, native = module(tcnn, D, cfg, True)
    xt, pt = to_device(x), to_device(params).requires_grad_(True)
    ctx, out = native.fwd(xt, pt)
    _, g = native.bwd(ctx, xt, pt, out, to_device(dy))
    g = g.detach().cpu().numpy()
    records = check_sum_per_level(ref, (g.astype(np.float64), g.view(np.uint32)), _terms(ref, x, dy, PRODUCT_FP32), U32, max_excluded=0, label=f"{D}-D {case_id(cfg)} fp32")
    print(records)
    assert np.any(g != 0)


@pytest.mark.parametrize("D,cfg", ATOMIC_CASES, ids=case_id)
def test_packed_fp16_atomic_gradient_per_element(tcnn, monkeypatch, D, cfg):
    """TCNN_AMD_GRID_SCATTER=atomic: (half)weight * dL/dy in fp16, packed-fp16 atomics; u = 2^-11 and one subnormal spacing to spare"""
    n = ATOMIC_ROWS
    ref, x, params, dy = inputs(D, cfg, n)
    d = dy.astype(np.float16)
    terms = _terms(ref, x, d, PRODUCT_HALF)
    assert int(terms["hits"].max()) < 2049, "the case gives an entry more contributions than the fp16 bound covers"
    bits = _half_gradient(tcnn, D, cfg, x, params.astype(np.float16), d, env={"TCNN_AMD_GRID_SCATTER": "atomic"}, monkeypatch=monkeypatch)
    records = check_sum_per_level(ref, (bits.view(np.float16).astype(np.float64), bits), terms, U16, slack=2.0 ** -24, max_excluded=0, label=f"{D}-D {case_id(cfg)} packed fp16")
    print(records)
    assert np.any(bits != 0)


@pytest.mark.parametrize("D,cfg", SCALAR_CASES, ids=case_id)
def test_scalar_feature_half_gradient_in_rounding_interval(tcnn, D, cfg):
    """one feature per level: an fp32 scratch (weight * (float)dL/dy, float atomics), rounded to half once"""
    n = ATOMIC_ROWS
    ref, x, params, dy = inputs(D, cfg, n)
    d = dy.astype(np.float16)
    bits = _half_gradient(tcnn, D, cfg, x, params.astype(np.float16), d)
    records = check_rounded_sum_per_level(ref, bits, _terms(ref, x, d, PRODUCT_SCRATCH32), label=f"{D}-D {case_id(cfg)} scratch32")
    print(records)
    assert np.any(bits != 0)


# ---------------------------------------------------------------------------------------------------- second order
SECOND_ORDER = [(D, F, interpolation) for D in (1, 5, 7) for interpolation in ("Linear", "Smoothstep") for F in ((2,) if D != 5 else (1, 2, 8))]


@pytest.mark.parametrize("fp32", [False, True], ids=["half", "float"])
@pytest.mark.parametrize("D,F,interpolation", SECOND_ORDER, ids=lambda v: str(v))
def test_second_order_as_close_to_fp64_as_the_rounding_twin(tcnn, D, F, interpolation, fp32):
    levels, log2_t, base, scale = SHAPES[D]
    cfg = _cfg("HashGrid", min(levels, 3 if D == 7 else 4), F, log2_t, base, scale, interpolation=interpolation)
    n = 256
    ref = GridND(D, cfg)
    rs = np.random.RandomState(5)
    T = np.float32 if fp32 else np.float16
    x = rs.uniform(0.02, 0.98, (n, D)).astype(np.float32)
    v = rs.uniform(-1, 1, (n, D)).astype(np.float32)
    params = rs.uniform(-1, 1, ref.n_params).astype(np.float16).astype(T)  # (half-representable: one set serves both precisions)
    dy = rs.uniform(-1, 1, (n, ref.n_output_dims)).astype(np.float16).astype(T)
    truth = ref.second_order(x, v, dy, params, "r64")
    twin = ref.second_order(x, v, dy, params, "rh")

    enc, native = module(tcnn, D, cfg, fp32)
    xt, pt, dt = to_device(x).requires_grad_(True), to_device(params).requires_grad_(True), to_device(dy).requires_grad_(True)
    ctx, _ = native.fwd(xt, pt)
    ddy, dparams, dx = native.bwd_bwd_input(ctx, xt, pt, to_device(v), dt)
    ours = [t.detach().float().cpu().numpy().astype(np.float64) for t in (ddy, dparams, dx)]
    failures = []
    for what, got, r64, rh in zip(("dL_ddLdoutput", "dL_dparams", "dL_dinput"), ours, truth, twin):
        e_ours, e_h, norm = float(np.linalg.norm(got - r64)), float(np.linalg.norm(rh - r64)), float(np.linalg.norm(r64))
        print(f"{D}-D F{F} {interpolation} {'float' if fp32 else 'half'} {what:14s} |ours-R64| {e_ours:.3e}  |Rh-R64| {e_h:.3e}  |R64| {norm:.3e}")
        assert np.all(np.isfinite(got))
        if e_ours > 2.0 * e_h:
            failures.append((what, e_ours, e_h))
        if not np.any(r64) and np.any(got):
            failures.append((what, "nonzero where R64 is exactly zero"))
    assert not failures, failures
    assert np.any(truth[0]) and np.any(truth[1])
    if D == 1 and interpolation == "Linear":
        assert not np.any(dx.cpu().numpy().view(np.uint32))  # no curvature and no second dimension to mix with
    else:
        assert np.any(truth[2])
