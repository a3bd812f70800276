"""stochastic_interpolation of the grid encodings without a GPU: every factory takes the key, the generator behind the draw is the
reference's, and the numpy restatement the GPU tests compare with (tests/grid_stochastic_reference.py) selects what the rule says --
exactly one corner per (sample, level), every corner and both outcomes of the comparison occurring on the inputs those tests use."""
import ctypes as C
import json

import numpy as np
import pytest

import grid_stochastic_reference as gsr
from conftest import CONFIG_C3B

GRID = dict(CONFIG_C3B["encoding"], stochastic_interpolation=True)
NET = CONFIG_C3B["network"]
COMPOSITE = {"otype": "Composite", "nested": [dict(GRID, n_dims_to_encode=3), {"otype": "SphericalHarmonics", "degree": 4, "n_dims_to_encode": 3}]}
REFUSAL = "stochastic_interpolation is not supported"


@pytest.fixture(scope="module")
def lib(tcnn):
    from tinycudann import _C

    return _C


@pytest.mark.parametrize("n_dims,enc", [(2, GRID), (3, dict(GRID, interpolation="Smoothstep")), (4, dict(GRID, interpolation="Nearest")), (6, COMPOSITE)],
                         ids=["2d", "3d-smoothstep", "4d-nearest", "composite"])
def test_modules_take_the_key(lib, n_dims, enc):
    """tcnn_create_encoding (both precisions) and tcnn_create_network_with_input_encoding, the grid alone and nested in a Composite:
    construction touches no device.  The key is no hyperparameter, as in the reference (grid.h:1098-1115)."""
    L = lib.lib
    def without_key(c):
        c = {k: v for k, v in c.items() if k != "stochastic_interpolation"}
        if "nested" in c:
            c["nested"] = [without_key(e) for e in c["nested"]]
        return c

    plain = without_key(enc)
    assert "stochastic_interpolation" in json.dumps(enc) and "stochastic_interpolation" not in json.dumps(plain)
    for precision in (1, 0):
        h, p = C.c_void_p(), C.c_void_p()
        assert L.tcnn_create_encoding(n_dims, json.dumps(enc).encode(), precision, C.byref(h)) == 0, L.tcnn_last_error().decode()
        lib.check(L.tcnn_create_encoding(n_dims, json.dumps(plain).encode(), precision, C.byref(p)))
        try:
            assert L.tcnn_module_hyperparams(h) == L.tcnn_module_hyperparams(p)
            assert L.tcnn_module_n_params(h) == L.tcnn_module_n_params(p) > 0
        finally:
            L.tcnn_module_destroy(h)
            L.tcnn_module_destroy(p)
    h = C.c_void_p()
    assert L.tcnn_create_network_with_input_encoding(n_dims, 16, json.dumps(enc).encode(), json.dumps(NET).encode(), C.byref(h)) == 0, L.tcnn_last_error().decode()
    L.tcnn_module_destroy(h)


def test_create_from_config_takes_the_key(lib):
    """tcnn_create_from_config: a trainer initialises its parameters on the device, so without a GPU the factory fails -- but then with the
    error it gives for the same config without the key, never with a refusal of the key.  (With a GPU it succeeds:
    tests/test_grid_stochastic_gpu.py builds its trainers from such configs.)"""
    L = lib.lib
    outcomes = []
    for enc in (GRID, CONFIG_C3B["encoding"]):
        cfg = dict(CONFIG_C3B, encoding=enc)
        t = C.c_void_p()
        rc = L.tcnn_create_from_config(2, 3, json.dumps(cfg).encode(), C.byref(t))
        msg = "" if rc == 0 else L.tcnn_last_error().decode("utf-8", "replace")
        if rc == 0:
            L.tcnn_trainer_destroy(t)
        outcomes.append((rc, msg))
    assert REFUSAL not in outcomes[0][1] and "stochastic" not in outcomes[0][1], outcomes[0]
    assert outcomes[0] == outcomes[1]


KNOWN_ANSWER_INDICES = [0, 1, 255, 256 * 15 + 7, 2 ** 32 - 1]


def test_random_val_known_answers(oracle):
    """random_val(1337, idx) = pcg32{1337} (stream 1), advance(idx), next_float(): the restatement's draw against the oracle's generator taken
    step by step -- advance(k) is k calls of next_uint -- and, for 2^32 - 1, against the default advance of 2^32 taken one step back."""
    for idx in KNOWN_ANSWER_INDICES[:4]:
        rng = oracle.Pcg32(1337)
        for _ in range(idx):
            rng.next_uint()
        u = rng.next_uint()
        want = np.uint32((u >> 9) | 0x3F800000).view(np.float32) - np.float32(1.0)
        got = gsr.random_val(oracle, idx)
        assert got.dtype == np.float32 and got == want and 0.0 <= got < 1.0, idx
    far = oracle.Pcg32(1337)
    far.advance(2 ** 32 - 1)
    st = far.st.copy()
    far.next_uint()  # now 2^32 steps from the seed
    ahead = oracle.Pcg32(1337)
    ahead.advance(2 ** 32)
    assert np.array_equal(far.st, ahead.st)
    again = oracle.Pcg32(1337)
    again.st[:] = st
    assert gsr.random_val(oracle, 2 ** 32 - 1) == np.float32(again.next_float())
    # the index is computed in uint32
    assert gsr.random_val(oracle, 2 ** 32 + 5) == gsr.random_val(oracle, 5)
    values = {float(gsr.random_val(oracle, i)) for i in KNOWN_ANSWER_INDICES}
    assert len(values) == len(KNOWN_ANSWER_INDICES)


def test_fused_multiply_add_rounds_once():
    """the restatement's fmaf against exact rational arithmetic, on operands chosen to sit on and next to float32 rounding ties"""
    from fractions import Fraction

    rs = np.random.RandomState(5)
    a = rs.uniform(1, 700, 4000).astype(np.float32)
    b = np.concatenate([rs.uniform(-0.5, 1.5, 3000), [0.0, 1.0, 1e-8, 0.5, -0.25, 0.999] * 100, rs.uniform(0, 1e-6, 400)]).astype(np.float32)
    got = gsr.fmaf(a, b, np.float32(0.5))
    for x, y, g in zip(a[::7], b[::7], got[::7]):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(1, 2)
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        err = abs(Fraction(float(g)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):
            assert (int(np.float32(g).view(np.uint32)) & 1) == 0  # a tie goes to even


# the grids of tests/test_grid_stochastic_gpu.py (imported there): small tables, so that many samples meet in one entry
def _grid(otype, n_in, F, interp="Linear", **more):
    cfg = {"otype": otype, "n_levels": 4, "n_features_per_level": F, "base_resolution": 2 + n_in % 3, "per_level_scale": 1.5, "interpolation": interp, "stochastic_interpolation": True}
    if otype == "HashGrid":
        cfg["log2_hashmap_size"] = 4 + F % 5
    cfg.update(more)
    return n_in, cfg


EXACT_CASES = [
    _grid("HashGrid", 2, 2), _grid("HashGrid", 3, 2, "Smoothstep", hash="Prime"), _grid("HashGrid", 4, 2, hash="ReversedPrime"),
    _grid("HashGrid", 3, 4, hash="Rng"), _grid("DenseGrid", 2, 4, "Smoothstep"), _grid("TiledGrid", 3, 8), _grid("HashGrid", 2, 8, "Smoothstep", log2_hashmap_size=8),
    _grid("DenseGrid", 4, 4), _grid("TiledGrid", 4, 8, "Smoothstep"), _grid("DenseGrid", 3, 2, base_resolution=4),
]
ATOMIC_CASES = [_grid("HashGrid", 2, 1), _grid("DenseGrid", 3, 1, "Smoothstep"), _grid("HashGrid", 3, 2), _grid("TiledGrid", 2, 4, "Smoothstep"), _grid("HashGrid", 4, 8)]
BATCHES = (256, 512)


def case_id(case):
    n_in, cfg = case
    return f"{n_in}d-{cfg['otype'][:-4]}-F{cfg['n_features_per_level']}-{cfg['interpolation']}" + (f"-{cfg['hash']}" if "hash" in cfg else "")


_SELECTIONS = {}


def selection_of(oracle, case, n):
    """(oracle encoding, x, selection) of a case at batch size n: computed once, shared, read-only"""
    key = (case_id(case), json.dumps(case[1], sort_keys=True), n)
    if key not in _SELECTIONS:
        n_in, cfg = case
        ref = oracle.create_encoding(n_in, cfg, alignment=0)
        x = gsr.stochastic_rows(oracle, ref, n)
        sel = gsr.selection(oracle, ref, x)
        for a in [x] + list(sel.values()):
            a.setflags(write=False)
        _SELECTIONS[key] = (ref, x, sel)
    return _SELECTIONS[key]


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("case", EXACT_CASES + ATOMIC_CASES, ids=case_id)
def test_restatement_selects_one_corner_and_covers_both_outcomes(oracle, case, n):
    n_in, cfg = case
    ref, x, sel = selection_of(oracle, case, n)
    L, D, C_ = int(ref.g.n_levels), n_in, 1 << n_in
    # one of the cell's 2^D corners, the one the comparisons name
    assert sel["corner"].min() >= 0 and sel["corner"].max() < C_
    level_of = sel["entry"] - ref.offsets[:L].astype(np.int64)[None, :]
    assert np.array_equal(level_of, np.take_along_axis(sel["indices"], sel["corner"][:, :, None], axis=2)[:, :, 0])
    assert np.all(level_of >= 0) and np.all(sel["entry"] < ref.offsets[1: L + 1].astype(np.int64)[None, :])
    for d in range(D):
        upper = (sel["corner"] >> d) & 1
        assert np.array_equal(upper == 0, sel["sample"] >= sel["pos"][:, :, d])
    # the fractions are pos_fract's: in [0, 1], and the cells reproduce the oracle's dense entries where a level is not hashed
    assert np.all((sel["pos"] >= 0) & (sel["pos"] <= 1)) and np.all((sel["sample"] >= 0) & (sel["sample"] < 1))
    res = ref.resolutions.astype(np.int64)
    sizes = np.diff(ref.offsets.astype(np.int64))
    checked = 0
    for l in range(L):
        if res[l] ** D > sizes[l] or cfg["otype"] == "TiledGrid":
            continue
        dense = np.zeros(n, dtype=np.int64)
        for d in range(D):
            dense += sel["cell"][:, l, d].astype(np.int64) * res[l] ** d
        inside = np.all((x >= 0) & (x < 1), axis=1)
        assert np.array_equal(dense[inside] % sizes[l], sel["indices"][inside, l, 0])
        checked += 1
    assert checked > 0 or cfg["otype"] != "DenseGrid"
    # not degenerate: every corner of the coarsest level, and both outcomes in every dimension, on every level
    assert set(np.unique(sel["corner"][:, 0])) == set(range(C_))
    for l in range(L):
        for d in range(D):
            bit = (sel["corner"][:, l] >> d) & 1
            assert bit.min() == 0 and bit.max() == 1, (l, d)
    # the draw of row i on level l is that of index i + l * n: with n = 512 the second level starts at 512, not at a multiple of the other batch
    assert sel["sample"][3, 1] == gsr.random_val(oracle, 3 + n)


def test_restatement_sums(oracle):
    """the two sums on a hand-made selection: exact integer sum rounded once (with and without a previous gradient), and S / A / k"""
    case = EXACT_CASES[0]
    ref, x, sel = selection_of(oracle, case, 256)
    F, L = 2, 4
    dy = np.zeros((256, L * F), dtype=np.uint16)
    dy[:, 0] = oracle.half_bits(np.full(256, 2.0 ** -12, dtype=np.float32))  # 256 x 2^-12 = 2^-4 on level 0, feature 0
    dy[5, 1] = 0x0001  # the smallest subnormal
    g = gsr.exact_half_gradient(oracle, ref, sel, dy)
    lvl0 = slice(0, int(ref.offsets[1]) * F)
    total = oracle.half_to_f32(g[lvl0][0::F]).astype(np.float64).sum()
    assert abs(total - 2.0 ** -4) <= 256 * 2.0 ** -24 and not np.any(g[int(ref.offsets[1]) * F:])
    assert np.count_nonzero(g[lvl0][1::F]) == 1 and g[int(sel["entry"][5, 0]) * F + 1] == 0x0001
    prev = np.full(ref.n_params, 0x3C00, dtype=np.uint16)  # 1.0 everywhere
    g2 = gsr.exact_half_gradient(oracle, ref, sel, dy, previous_bits=prev)
    want = (1.0 + oracle.half_to_f32(g).astype(np.float64)).astype(np.float16).view(np.uint16)
    assert np.array_equal(g2, want)
    off = np.zeros((256, L), dtype=bool)
    off[:, 0] = True
    assert not np.any(gsr.exact_half_gradient(oracle, ref, sel, dy, off=off))
    t = gsr.atomic_terms(oracle, ref, sel, dy)
    assert int(t["hits"][0::F][: int(ref.offsets[1])].sum()) == 256 and t["min_nonzero"] == 2.0 ** -24
    assert np.array_equal(t["hits"][0::F], t["hits"][1::F]) and np.all(t["abs_sum"] >= np.abs(t["sum"]))
