"""stochastic_interpolation of the grid encodings (grid.h:284-298) restated in numpy.  No GPU in here.

The rule.  In the parameter-gradient pass, and only there, sample i of a batch of n rows puts its dL/dy of level l on ONE corner of its cell,
with weight 1: sample = random_val(1337, i + l * n) (pcg32{1337}, advance, next_float; the index wraps in uint32), and in EVERY dimension d
the corner is pos_grid[d] if sample >= pos[d], else pos_grid[d] + 1 -- one draw for all dimensions.  pos[d] is pos_fract's fraction
(common_device.h:856-868), smoothstepped for Smoothstep grids.  Nearest returns before the flag is read.

What comes from where.  The inputs are those of tests/grid_reference.py (reference_inputs: pcg32{42} rows plus its edge rows).  The
generator is the oracle's Pcg32, pinned to the reference's own by tests/test_oracle.py.  The corners' table entries are the oracle's
(GridEncoding.forward(want_indices=True): corner c of a cell has bit d set where dimension d takes pos_grid[d] + 1), so no hash is restated
here.  The fractions are computed below in fp32, operation by operation, as pos_fract does: one fused multiply-add, floor, one subtraction;
smoothstep as three fp32 products and one difference (the kernels are compiled with -ffp-contract=off)."""
import numpy as np

from grid_reference import edge_x, level_slices, reference_inputs  # noqa: F401  (re-exported: the tests take their inputs from here)

F32 = np.float32
SEED = 1337


def fmaf(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 arrays: the product of two floats is exact in a double; the sum is rounded to odd in
    double (TwoSum tells whether it was exact), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the correct one."""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.copy().view(np.int64)
    inexact_even = (err != 0) & ((bits & 1) == 0)
    # towards the true value: one unit in the last place up in magnitude if err has the sign of s, else down
    away = (err > 0) == (s > 0)
    bits = np.where(inexact_even, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(F32)


def smoothstep(v):
    v = np.asarray(v, dtype=F32)
    return (v * v) * (F32(3.0) - F32(2.0) * v)


def fractions(oracle, ref, x):
    """pos [n][L][D] float32 as the gradient kernels see it, and pos_grid [n][L][D] uint32"""
    x = np.asarray(x, dtype=F32)
    scale = ref.scales.astype(F32)[None, :, None]
    p = fmaf(np.broadcast_to(scale, (x.shape[0], scale.shape[1], x.shape[1])), x[:, None, :], F32(0.5))
    fl = np.floor(p)
    pos = (p - fl).astype(F32)
    cell = fl.astype(np.int64).astype(np.int32).view(np.uint32)
    if ref.g.interpolation == oracle.INTERP["smoothstep"]:
        pos = smoothstep(pos)
    return pos, cell


def random_val(oracle, idx):
    """common_device.h:333-337 with seed 1337: pcg32{1337}, advance(idx), next_float()"""
    rng = oracle.Pcg32(SEED)
    rng.advance(int(idx) & 0xFFFFFFFF)
    return F32(rng.next_float())


def selection(oracle, ref, x):
    """Which corner every (sample, level) pair selects.  A dict of [n][L] arrays: sample (the draw), corner (bit d: dimension d took
    pos_grid[d] + 1), entry (the selected table entry, counted from the start of the whole table) -- plus pos [n][L][D] and the oracle's
    entries of all corners, indices [n][L][2^D] (relative to their level)."""
    assert ref.g.interpolation != oracle.INTERP["nearest"], "Nearest returns before the flag is read: compare it with a plain Nearest grid"
    x = np.ascontiguousarray(x, dtype=F32)
    n, D = x.shape
    L = int(ref.g.n_levels)
    pos, cell = fractions(oracle, ref, x)
    _, ctx = ref.forward(x, np.zeros(ref.n_params, dtype=np.uint16), want_indices=True)
    indices = ctx["indices"].astype(np.int64)
    sample = np.empty((n, L), dtype=F32)
    for l in range(L):
        for i in range(n):
            sample[i, l] = random_val(oracle, (i + l * n) & 0xFFFFFFFF)
    upper = ~(sample[:, :, None] >= pos)  # NaN fractions (none in the test inputs) would take pos_grid + 1, as the kernel's else branch does
    corner = np.zeros((n, L), dtype=np.int64)
    for d in range(D):
        corner |= upper[:, :, d].astype(np.int64) << d
    entry = np.take_along_axis(indices, corner[:, :, None], axis=2)[:, :, 0] + ref.offsets[:L].astype(np.int64)[None, :]
    return {"sample": sample, "corner": corner, "entry": entry, "pos": pos, "cell": cell, "indices": indices}


def _pairs(sel, ref, off):
    """(row, level, first parameter of the selected entry) of every pair that the gradient rule leaves on"""
    F = int(ref.g.n_features_per_level)
    n, L = sel["entry"].shape
    on = np.ones((n, L), dtype=bool) if off is None else ~np.asarray(off, dtype=bool)
    rows, levels = np.nonzero(on)
    return rows, levels, sel["entry"][rows, levels] * F, F


def exact_half_gradient(oracle, ref, sel, dy_bits, previous_bits=None, off=None):
    """Half grids with two or more features per level: the exact sum of the selected dL/dy halves per parameter in units of 2^-24, rounded
    to half once -- the convention of orc_grid_backward_exact.  previous_bits (GradientMode::Accumulate): the gradient already there joins
    the sum exactly, before the rounding.  off [n][L]: pairs a max_level cut-off skips.  Returns uint16 [n_params]."""
    dy = oracle.half_to_f32(np.ascontiguousarray(dy_bits)).astype(np.float64) * 2.0 ** 24
    assert np.all(dy == np.rint(dy))
    dy = dy.astype(np.int64)
    total = np.zeros(ref.n_params, dtype=np.int64)
    if previous_bits is not None:
        prev = oracle.half_to_f32(np.ascontiguousarray(previous_bits)).astype(np.float64) * 2.0 ** 24
        total += prev.astype(np.int64)
    rows, levels, first, F = _pairs(sel, ref, off)
    for f in range(F):
        np.add.at(total, first + f, dy[rows, levels * F + f])
    assert np.all(np.abs(total) < 2 ** 52)
    return (total.astype(np.float64) * 2.0 ** -24).astype(np.float16).view(np.uint16)  # (numpy rounds double -> half once, to nearest even)


def atomic_terms(oracle, ref, sel, dy, off=None):
    """The atomic families: per parameter the exact sum S of the selected dL/dy values (each added as it is: the weight is 1.0), the sum of
    their magnitudes and the number k of pairs that select the parameter's entry -- the dict tests/grid_reference.py's bounds take.
    dy: float32 [n][width], or half bits."""
    dy = np.ascontiguousarray(dy)
    v = (oracle.half_to_f32(dy) if dy.dtype == np.uint16 else dy.astype(F32)).astype(np.float64)
    s = np.zeros(ref.n_params, dtype=np.float64)
    a = np.zeros(ref.n_params, dtype=np.float64)
    k = np.zeros(ref.n_params, dtype=np.uint32)
    rows, levels, first, F = _pairs(sel, ref, off)
    smallest = np.inf
    for f in range(F):
        c = v[rows, levels * F + f]
        np.add.at(s, first + f, c)  # in double: exact for halves (multiples of 2^-24 below 2^11), within 2^-53 relative for floats
        np.add.at(a, first + f, np.abs(c))
        np.add.at(k, first + f, 1)
        if np.any(c != 0):
            smallest = min(smallest, float(np.abs(c[c != 0]).min()))
    return {"sum": s, "abs_sum": a, "hits": k, "min_nonzero": smallest}


# ------------------------------------------------------------------------------------------------------ the GPU tests' inputs
def stochastic_rows(oracle, ref, n):
    """x [n][D]: n - 64 rows from pcg32{42} and the first 64 edge rows of grid_reference.py (0, 1, the float below 1, 0.5, negative, above 1,
    tiny, 0.999 in every dimension)."""
    D = ref.n_in
    body = oracle.Pcg32(42).uniform_strided((n - 64) * D).reshape(n - 64, D)
    return np.concatenate([body, edge_x(64, D)]).astype(F32)


def stochastic_gradients(oracle, n, width, seed=9):
    """dL/dy as half bits [n][width]: mixed sign and magnitude -- uniform in [-2, 2) scaled by 2^-e, e cycling through 0 .. 23 along a row's
    columns shifted by the row (so the smallest are fp16 subnormals), every seventh row zero, every fifth column of every third row -0."""
    v = oracle.Pcg32(seed).uniform_strided(n * width, -2.0, 2.0).reshape(n, width).astype(np.float64)
    e = (np.arange(width)[None, :] + np.arange(n)[:, None]) % 24
    bits = oracle.half_bits((v * 2.0 ** -e).astype(F32))
    bits[::7] = 0
    bits[::3, ::5] = 0x8000
    return bits
