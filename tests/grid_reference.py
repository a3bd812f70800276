"""Shared by the tests of the reference-shaped grid kernels (k_grid_fwd<float>, k_grid_bwd with float atomics or packed-fp16 atomics,
k_grid_bwd_input<float>): the case list, the inputs, and the per-element bound of a sum whose order is not defined.  No GPU in here."""
import numpy as np

U32 = 2.0 ** -24  # unit roundoff of an fp32 addition
U16 = 2.0 ** -11  # unit roundoff of an fp16 addition


def edge_x(n, n_in):
    """rows that run through the special coordinates in every dimension: 0, 1, the float below 1, 0.5, negative, above 1, tiny, 0.999"""
    specials = [0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 0.5, -0.25, 1.5, 1e-8, 0.999]
    x = np.zeros((n, n_in), dtype=np.float32)
    for i in range(n):
        for d in range(n_in):
            x[i, d] = specials[(i // len(specials) ** d) % len(specials)]
    return x


# (n_in, encoding): every <D, F> instantiation family of k_grid_fwd / k_grid_bwd (D = 2, 3, 4; F = 1, 2, 4, 8), hash / dense / tiled, every
# hash function, the three interpolations, and both store paths of k_grid_fwd (row width 3: scalar tail stores; multiples of 8: one
# 16-byte store).  Tables are small: coarse levels collect hundreds of contributions per entry, fine levels a few.
REFERENCE_KERNEL_CASES = [
    (2, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16, "per_level_scale": 1.5}),
    (2, {"otype": "HashGrid", "n_levels": 12, "n_features_per_level": 1, "log2_hashmap_size": 12, "base_resolution": 8, "per_level_scale": 1.4}),
    (2, {"otype": "DenseGrid", "n_levels": 3, "n_features_per_level": 1, "base_resolution": 8, "per_level_scale": 2.0, "interpolation": "Smoothstep"}),
    (2, {"otype": "DenseGrid", "n_levels": 3, "n_features_per_level": 8, "base_resolution": 8, "per_level_scale": 2.0}),
    (3, {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 4, "log2_hashmap_size": 14, "base_resolution": 8, "per_level_scale": 2.0, "interpolation": "Smoothstep"}),
    (3, {"otype": "TiledGrid", "n_levels": 4, "n_features_per_level": 2, "base_resolution": 8, "per_level_scale": 1.5}),
    (3, {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 8, "per_level_scale": 1.5, "hash": "Rng"}),
    (3, {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 8, "per_level_scale": 1.5, "hash": "Prime"}),
    (3, {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 8, "per_level_scale": 1.5, "hash": "ReversedPrime"}),
    (3, {"otype": "HashGrid", "n_levels": 5, "n_features_per_level": 8, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.7, "interpolation": "Nearest"}),
    (4, {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 1, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}),
    (4, {"otype": "TiledGrid", "n_levels": 2, "n_features_per_level": 4, "base_resolution": 4, "per_level_scale": 2.0, "interpolation": "Smoothstep"}),
]


def case_id(case):
    n_in, cfg = case
    extra = "".join(f"-{cfg[k]}" for k in ("interpolation", "hash") if k in cfg)
    return f"{n_in}d-{cfg['otype'][:-4]}-L{cfg['n_levels']}-F{cfg['n_features_per_level']}{extra}"


N_ROWS = 1024
MIN_CONTRIBUTION = 2.0 ** -100  # below this a test would depend on how float atomics treat subnormal sums


def reference_inputs(oracle, ref, n=N_ROWS):
    """(x [n][D], params float32, dL/dy float32 [n][width]): n - 256 uniform rows from pcg32{42} and the 256 edge rows; parameters uniform in
    [-1, 1); dL/dy uniform in [-2, 2) with every seventh row zero.  Round params / dL/dy through oracle.half_bits where half values are needed."""
    n_in = ref.n_in
    x = np.concatenate([oracle.Pcg32(42).uniform_strided((n - 256) * n_in).reshape(n - 256, n_in), edge_x(256, n_in)]).astype(np.float32)
    params = oracle.Pcg32(3).uniform_strided(ref.n_params, -1.0, 1.0).astype(np.float32)
    width = ref.padded_output_width
    dy = oracle.Pcg32(9).uniform_strided(n * width, -2.0, 2.0).reshape(n, width).astype(np.float32)
    dy[::7] = 0
    return x, params, dy


def gamma(m, u):
    """gamma_m = m u / (1 - m u) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1); inf where m u >= 1"""
    m = np.asarray(m, dtype=np.float64)
    mu = m * u
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mu < 1.0, mu / (1.0 - mu), np.inf)


def summation_bound(terms, u):
    """e = gamma(k - 1) * A per parameter: k numbers added in ANY order with k - 1 roundings of unit roundoff u differ from their exact sum
    by at most gamma(k - 1) times the sum of their magnitudes (Higham, section 4.2).  0 for k <= 1; inf where (k - 1) u >= 1."""
    k = terms["hits"].astype(np.float64)
    g = gamma(np.maximum(k - 1.0, 0.0), u)
    with np.errstate(invalid="ignore"):
        return np.where(g == 0.0, 0.0, g * terms["abs_sum"])


def level_slices(ref):
    F = ref.g.n_features_per_level
    off = ref.offsets.astype(np.int64) * F
    return [slice(int(off[l]), int(off[l + 1])) for l in range(ref.g.n_levels)]


def check_sum_per_level(ref, got, terms, u, slack=0.0, max_excluded=0.0, label=""):
    """|got - S| <= gamma(k - 1) * A + slack for every parameter, asserted level by level; untouched entries must be +0.
    got: float64 values and their raw bit patterns (got_bits) as a pair.  Entries whose gamma is undefined are excluded; at most the share
    max_excluded of a level's hit entries may be.  Returns one record per level: (level, worst ratio |got - S| / bound, excluded, hit entries)."""
    values, bits = got
    S, k = terms["sum"], terms["hits"]
    bound = summation_bound(terms, u) + slack
    records = []
    for level, sl in enumerate(level_slices(ref)):
        v, s, kk, b = values[sl].astype(np.float64), S[sl], k[sl], bound[sl]
        assert not np.any(bits[sl][kk == 0]), f"{label} level {level}: an entry that no sample touches is not +0"
        hit = kk > 0
        usable = hit & np.isfinite(b)
        excluded = int(np.count_nonzero(hit & ~usable))
        assert excluded <= max_excluded * int(np.count_nonzero(hit)), f"{label} level {level}: {excluded} of {int(np.count_nonzero(hit))} hit entries have no bound"
        err = np.abs(v - s)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(usable, np.where(err == 0.0, 0.0, err / b), 0.0)
        worst = int(np.argmax(ratio)) if ratio.size else 0
        records.append((level, float(ratio[worst]) if ratio.size else 0.0, excluded, int(np.count_nonzero(hit))))
        assert np.all(np.isfinite(v)) and float(ratio[worst]) <= 1.0, (
            f"{label} level {level}: entry {worst} (k = {int(kk[worst])}) has |got - S| / e = {float(ratio[worst]):.4g} "
            f"(got {v[worst]!r}, S {s[worst]!r}, e {b[worst]!r}); {int(np.count_nonzero(ratio > 1.0))} entries of the level outside")
    return records


def check_rounded_sum_per_level(ref, got_half_bits, terms, label=""):
    """The F = 1 half gradient: an fp32 sum in any order, rounded to half once.  Rounding is monotone, so
    rn_half(S - e) <= got <= rn_half(S + e) with e = gamma(k - 1) * A at u = 2^-24; compared as ordered half values, level by level.
    Returns (level, worst |got - S| / half width of the interval, 0, hit entries) per level."""
    S, k = terms["sum"], terms["hits"]
    e = summation_bound(terms, U32)
    assert np.all(np.isfinite(e))
    lo = (S - e).astype(np.float16).astype(np.float64)  # numpy rounds double -> half once, to nearest even
    hi = (S + e).astype(np.float16).astype(np.float64)
    got = got_half_bits.view(np.float16).astype(np.float64)
    records = []
    for level, sl in enumerate(level_slices(ref)):
        g, kk = got[sl], k[sl]
        assert not np.any(got_half_bits[sl][kk == 0]), f"{label} level {level}: an entry that no sample touches is not +0"
        outside = ~((lo[sl] <= g) & (g <= hi[sl]))
        width = np.maximum((hi[sl] - lo[sl]) / 2, np.abs(S[sl]) * U16)  # (record only)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(width > 0, np.abs(g - S[sl]) / width, 0.0)
        worst = int(np.argmax(np.where(outside, np.inf, ratio))) if ratio.size else 0
        records.append((level, float(ratio[worst]) if ratio.size else 0.0, 0, int(np.count_nonzero(kk > 0))))
        assert not np.any(outside), (
            f"{label} level {level}: entry {worst} (k = {int(kk[worst])}) lies outside [rn_half(S - e), rn_half(S + e)] = "
            f"[{lo[sl][worst]!r}, {hi[sl][worst]!r}]: got {g[worst]!r}, S {S[sl][worst]!r}, e {e[sl][worst]!r}, |got - S| / e = "
            f"{abs(g[worst] - S[sl][worst]) / e[sl][worst] if e[sl][worst] else float('inf'):.4g}; {int(np.count_nonzero(outside))} entries of the level outside")
    return records


def print_records(form, case, records):
    """one line per level (pytest -s): records, not thresholds"""
    for level, worst, excluded, hit in records:
        print(f"parity {form:9s} {case_id(case):40s} level {level:2d}  hit entries {hit:6d}  worst |got-S|/e {worst:8.4f}  excluded {excluded}")


# ------------------------------------------------------------------------------------------------------ what needs the GPU
def to_device(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared references are read-only)


def fp32_module(tcnn, n_in, cfg, params):
    """tcnn.Encoding(dtype=torch.float32) holding the given float32 parameters"""
    import torch

    enc = tcnn.Encoding(n_in, cfg, dtype=torch.float32)
    assert enc.dtype == torch.float32 and enc.params.numel() == params.size
    with torch.no_grad():
        enc.params.copy_(to_device(params))
    return enc


def assert_fp32_forward_bit_exact(tcnn, oracle, case, x, params):
    """k_grid_fwd<float> against orc_grid_forward_f32: the same uint32 patterns, padding columns included, through the module (inference)
    and through native.fwd with a context (the training form of the forward pass).  Returns the oracle's output."""
    import torch

    n_in, cfg = case
    ref = oracle.create_encoding(n_in, cfg, alignment=0)
    enc = fp32_module(tcnn, n_in, cfg, params)
    ref.n_to_pad = enc.n_output_dims - ref.n_output_dims  # the module reports its padded width
    assert 0 <= ref.n_to_pad < 8
    want, _ = ref.forward_f32(x, params)
    with torch.no_grad():
        got = enc(to_device(x))
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert not np.any(differ), (
        f"{case_id(case)}: {int(np.count_nonzero(differ))} outputs of the module differ from the fp32 oracle, first at {tuple(np.argwhere(differ)[0])}: "
        f"got {got[differ][0]!r}, want {want[differ][0]!r}")
    native = enc.native_tcnn_module
    n = x.shape[0]
    assert n % 256 == 0
    ctx, out = native.fwd(to_device(x), to_device(params).requires_grad_(True))
    assert ctx is not None
    out = out.cpu().numpy()
    differ = out.view(np.uint32) != want.view(np.uint32)
    assert not np.any(differ), f"{case_id(case)}: {int(np.count_nonzero(differ))} outputs of native.fwd differ from the fp32 oracle, first at {tuple(np.argwhere(differ)[0])}"
    return want
