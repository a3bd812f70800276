"""Frequency, TriangleWave and SphericalHarmonics at first order, element by element (k_frequency_fwd, k_trianglewave_fwd,
k_periodic_bwd_input, k_sh_fwd, k_sh_bwd_input in k_encodings.hip).

Every output element, every entry of the Jacobian (read out of the backward pass with a one-hot dL_dy) and every element of a dense
dL_dx is compared on its own with R64, the fp64 value on the kernels' float constants (tests/analytic_encoding_reference.py):
  Frequency           inside a derived bound (frequency_bounds, dense_bound: the argument's two roundings, sinf / cosf within their
                      measured float steps, the roundings of the sum);
  TriangleWave        the bits of Rf32, the fp32 restatement: every operation after the argument is exact or rounds as Rf32 does, every
                      Jacobian entry is +-2^(k+1) exactly, so the dense sum in the kernel's order has Rf32's bits too;
  SphericalHarmonics  per column as close to R64 as Rf32 is, up to the margin of column_bar (degree 1: a constant, Rf32's bits).
One criterion over a whole matrix (max |got - want| <= 2e-3 max |want|) cannot see a low-frequency column next to one whose derivative is
2^11 pi: the four mutants below pass it and fail here.  The input set covers [0, 1), [-4, 4), every kink with its float neighbours,
negative inputs and arguments up to 255.75 * 2^11 pi; inputs() says what is out of scope."""
import functools
import types

import pytest

import analytic_encoding_reference as ref

gpu = pytest.mark.gpu

CASES = {
    "frequency_12x3": (3, {"otype": "Frequency", "n_frequencies": 12}),
    "frequency_1x1": (1, {"otype": "Frequency", "n_frequencies": 1}),
    "trianglewave_12x2": (2, {"otype": "TriangleWave", "n_frequencies": 12}),
    "sh_1": (3, {"otype": "SphericalHarmonics", "degree": 1}),
    "sh_4": (3, {"otype": "SphericalHarmonics", "degree": 4}),
    "sh_8": (3, {"otype": "SphericalHarmonics", "degree": 8}),
}
PERIODIC = [c for c in CASES if not c.startswith("sh")]
FREQUENCY = [c for c in CASES if c.startswith("frequency")]
PRECISIONS = ["half", "float32"]


def _is_sh(case):
    return CASES[case][1]["otype"] == "SphericalHarmonics"


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Everything the tests of one case compare with, computed once on the CPU and never written to: the input set, R64 and Rf32 of the
    values ("half": rounded where the kernel stores a half), of the Jacobian (periodic: the band dy_dx [n][D P]; SH: [n][W][3]) and
    Frequency's bounds"""
    n_in, cfg = CASES[case]
    r = types.SimpleNamespace(case=case, n_in=n_in, cfg=cfg, x=ref.inputs(cfg, n_in), width=ref._width(cfg, n_in))
    r.y64 = ref.values(cfg, r.x, "r64f")
    r.y32 = {"float32": ref.values(cfg, r.x, "f32"), "half": ref.values(cfg, r.x, "half")}
    if _is_sh(case):
        r.J64 = ref.jacobian(cfg, r.x)
        r.J32 = ref.sh_first_order(r.x, None, cfg["degree"], "f32")[0]
    else:
        r.P = ref.outputs_per_input(cfg)
        r.band64, r.band32 = ref.dy_dx(cfg, r.x, "r64f"), ref.dy_dx(cfg, r.x, "f32")
        if cfg["otype"] == "Frequency":
            r.value_bound = {}
            for precision in PRECISIONS:
                r.value_bound[precision], r.band_bound, r.arg = ref.frequency_bounds(cfg, r.x, precision == "half")
    return r


@functools.lru_cache(maxsize=None)
def _dense_dy(width, scale):
    """dL_dy [N_ROWS][width]: multiples of 2^-10 in [-1, 1) (half-representable: one dy serves both precisions), times the loss scale"""
    import torch

    g = torch.Generator().manual_seed(1000 + width)
    return torch.randint(-1024, 1024, (ref.N_ROWS, width), generator=g).float() / 1024.0 * scale


# ---------------------------------------------------------------------------------------------------- the comparisons
def _column_x(r, column):
    """the input dim an output column of a periodic encoding reads (SH: every column reads all three)"""
    return None if _is_sh(r.case) else column // r.P


def _worst(r, what, got, want, bound, column_of=lambda j: j):
    """(worst ratio |got - want| / bound, the report of that element).  got, want, bound: [n][columns] (fp64)"""
    ratio = (got.double() - want).abs() / bound
    flat = int(ratio.argmax())
    i, j = flat // ratio.shape[1], flat % ratio.shape[1]
    a = _column_x(r, column_of(j))
    x = r.x[i].tolist() if a is None else float(r.x[i, a])
    where = f"column {j}" if column_of(j) == j or not _is_sh(r.case) else f"column {column_of(j)} d/d{'xyz'[j % 3]}"
    report = f"{r.case} {what}: worst ratio {float(ratio[i, j]):.3f} at (row {i}, {where}, x {x!r}, got {float(got[i, j])!r}, want {float(want[i, j])!r}, bound {float(bound[i, j]):.3e})"
    return float(ratio[i, j]), report


def _same_bits(r, what, got, want, zero_sign=True):
    """None, or the report of the first element whose bits differ.  zero_sign=False: +0 and -0 count as equal."""
    import torch

    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    view = torch.int16 if got.dtype == torch.half else torch.int32
    differ = got.contiguous().view(view) != want.contiguous().view(view)
    if not zero_sign:
        differ &= ~((got == 0) & (want == 0))
    if not bool(differ.any()):
        return None
    i, j = [int(t) for t in differ.reshape(got.shape[0], -1).nonzero()[0]]
    g, w = got.reshape(got.shape[0], -1), want.reshape(got.shape[0], -1)
    return f"{r.case} {what}: {int(differ.sum())} elements differ, the first at (row {i}, column {j}, x {r.x[i].tolist()!r}, got {float(g[i, j])!r}, want {float(w[i, j])!r}, bound: equal bits)"


def _sh_bound(rf32, r64, half=False):
    """column_bar as a bound per element (SH values [n][W], Jacobian [n][W * 3], dense dL_dx [n][3]); E per column beside it"""
    E, bar = ref.column_bar(rf32, r64)
    bound = bar.unsqueeze(0).expand_as(r64)
    return E, (bound + ref._half_ulp(r64) if half else bound)


def _per_degree(E, got, r64):
    """SH: the worst column of every degree l by max_i |ours - R64| / E_j (columns l^2 .. l^2 + 2l; trailing dims belong to the column).
    A column with E_j = 0 (Rf32 exact on every row) is listed only if ours is not exact there."""
    import math

    err = (got.double() - r64).abs().amax(dim=0)
    parts = []
    for l in range(math.isqrt(E.shape[0] - 1) + 1):
        block_e, block_err = E[l * l:(l + 1) * (l + 1)].reshape(-1), err[l * l:(l + 1) * (l + 1)].reshape(-1)
        ratio = block_err / block_e
        ratio[(block_e == 0) & (block_err == 0)] = 0.0
        k = int(ratio.argmax())
        per = block_e.numel() // (2 * l + 1)
        parts.append(f"l={l}: {float(ratio[k]):.2f} (column {l * l + k // per}{'' if per == 1 else ' d/d' + 'xyz'[k % per]})")
    return "; ".join(parts)


def check_values(r, precision, got):
    """a. every output element: (ok, lines to print / report)"""
    want32 = r.y32[precision]
    got = got.cpu()
    otype = r.cfg["otype"]
    if otype == "Frequency":
        ratio, report = _worst(r, f"{precision} values", got, r.y64, r.value_bound[precision])
        return ratio <= 1.0, [report]
    if otype == "TriangleWave" or r.cfg["degree"] == 1:
        report = _same_bits(r, f"{precision} values", got, want32.to(got.dtype))
        return report is None, [report or f"{r.case} {precision} values: the bits of Rf32 in all {got.numel()} elements"]
    _, bound = _sh_bound(r.y32["float32"], r.y64, half=precision == "half")  # fp32's E_j; a stored half adds half a half-ulp at the element
    ratio, report = _worst(r, f"{precision} values", got, r.y64, bound)
    # (the ratio to print: against E_j of the restatement in the SAME precision -- in half both are the rounding to half, not fp32's)
    return ratio <= 1.0, [report, f"{r.case} {precision} values ours / E_j: {_per_degree(ref.column_bar(want32, r.y64)[0], got, r.y64)}"]


def check_jacobian(r, got, what="Jacobian"):
    """b. every entry: periodic got [n][D P] (the band), SH got [n][W][3], fp32 from the kernel"""
    import torch

    otype = r.cfg["otype"]
    if otype == "Frequency":
        ratio, report = _worst(r, what, got, r.band64, r.band_bound)
        return ratio <= 1.0, [report]
    if otype == "TriangleWave":
        report = _same_bits(r, what, got, r.band32)
        exact = bool((got.abs() == torch.pow(2.0, torch.arange(r.P).float() + 1).repeat(r.n_in)[None, :]).all())
        return report is None and exact, [report or f"{r.case} {what}: +-2^(k+1) with the rule's sign in all {got.numel()} entries"]
    n, W = got.shape[0], got.shape[1]
    E, bound = _sh_bound(r.J32.reshape(n, W * 3), r.J64.reshape(n, W * 3))
    ratio, report = _worst(r, what, got.reshape(n, W * 3), r.J64.reshape(n, W * 3), bound, column_of=lambda j: j // 3)
    return ratio <= 1.0, [report, f"{r.case} {what} ours / E_ja: {_per_degree(E.reshape(W, 3), got, r.J64)}"]


def dense_reference(r, dy):
    """(R64's dL_dx [n][D] for dy, Rf32's in the kernel's order)"""
    import torch

    if _is_sh(r.case):
        return torch.einsum("ij,ija->ia", dy.double(), r.J64), ref.sh_first_order(r.x, dy, r.cfg["degree"], "f32")[1]
    return ref.dense_sum(dy, r.band64, r.P, torch.float64), ref.dense_sum(dy, r.band32, r.P, torch.float32)


def check_dense(r, dy, got, what="dense dL_dx"):
    """c. every element of dL_dx for a dense dy"""
    want64, want32 = dense_reference(r, dy)
    otype = r.cfg["otype"]
    if otype == "Frequency":
        ratio, report = _worst(r, what, got, want64, ref.dense_bound(dy, r.band64, r.band_bound, r.P), column_of=lambda a: a * r.P)
        return ratio <= 1.0, [report]
    if otype == "TriangleWave":
        report = _same_bits(r, what, got, want32)
        return report is None, [report or f"{r.case} {what}: the bits of Rf32's sum in all {got.numel()} elements"]
    E, bound = _sh_bound(want32, want64)
    ratio, report = _worst(r, what, got, want64, bound)
    err = (got.double() - want64).abs().amax(dim=0)
    return ratio <= 1.0, [report, f"{r.case} {what} ours / E_a: " + ", ".join(f"{float(e / E_a) if E_a > 0 else float(e > 0):.2f}" for e, E_a in zip(err, E))]


def old_criterion_accepts(got, want):
    """test_encoding_forward_backward_match_oracle's: one number for the whole matrix"""
    return float((got.double() - want).abs().max()) <= 2e-3 * max(1.0, float(want.abs().max()))


# ---------------------------------------------------------------------------------------------------- CPU: the references
@pytest.mark.parametrize("case", list(CASES))
def test_r64_jacobian_matches_autograd(case):
    """The closed-form Jacobians (and sh_eval's hand-written derivative recurrence, restated in fp64) against torch.autograd on the
    fp64 values.  TriangleWave on the rows that sit on no kink of any frequency (2 val is no integer): there autograd's sign of |.| is
    the kernel's rule, to the bit; negative inputs are among them."""
    import torch

    r = _reference(case)
    if _is_sh(case):
        hand, _ = ref.sh_first_order(r.x, None, r.cfg["degree"], "r64f")
        excess = (hand - r.J64).abs() - 1e-12 * (1.0 + r.J64.abs())
        print(f"{case}: |recurrence - autograd| max {float((hand - r.J64).abs().max()):.3e}, max |J| {float(r.J64.abs().max()):.3e}")
        assert float(excess.max()) <= 0
        assert bool(r.J64.any()) == (r.cfg["degree"] > 1)  # degree 1: a constant
        dy = _dense_dy(r.width, 1.0)
        _, dense = ref.sh_first_order(r.x, dy, r.cfg["degree"], "r64f")
        want = dense_reference(r, dy)[0]
        assert float(((dense - want).abs() - 1e-12 * (1.0 + torch.einsum("ij,ija->ia", dy.double().abs(), r.J64.abs()))).max()) <= 0
        return
    xp = r.x.double().requires_grad_(True)
    y = ref.values(r.cfg, xp, "r64f")
    D, P = r.n_in, r.P
    auto = torch.zeros(ref.N_ROWS, D * P, dtype=torch.float64)
    for k in range(P):
        (g,) = torch.autograd.grad(y[:, k::P].sum(), xp, retain_graph=True)  # column a P + k reads input a alone
        auto[:, k::P] = g
    rows = torch.ones(ref.N_ROWS, dtype=torch.bool)
    if r.cfg["otype"] == "TriangleWave":
        for k in range(r.cfg["n_frequencies"]):
            twice = ref._triangle_val(r.x, k, torch.float64) * 2.0
            rows &= (twice != torch.floor(twice)).all(dim=1)
        assert int(rows.sum()) >= ref.N_ROWS // 2 and bool((r.x[rows] < 0).any()) and not bool(rows.all())
        assert torch.equal(auto[rows], r.band64[rows])
        assert bool((r.band64.abs() == torch.pow(2.0, torch.arange(P).double() + 1).repeat(D)[None, :]).all())
    else:
        excess = (auto - r.band64).abs() - 1e-12 * (1.0 + r.band64.abs())
        assert float(excess.max()) <= 0
    J = ref.jacobian(r.cfg, r.x)
    assert J.shape == (ref.N_ROWS, D * P, D) and all(torch.equal(J[:, a * P:(a + 1) * P, a], r.band64[:, a * P:(a + 1) * P]) for a in range(D))
    assert int((J != 0).sum()) == int((r.band64 != 0).sum())  # nothing outside the band


def test_input_sets_hold_what_they_promise():
    import numpy as np
    import torch

    for case in PERIODIC:
        r = _reference(case)
        flat = r.x.reshape(-1)
        F = r.cfg["n_frequencies"]
        for special in ref.periodic_specials(F):
            assert bool(((flat == float(special)) & (torch.signbit(flat) == bool(np.signbit(special)))).any()), (case, special)
        for k in range(F):  # a kink of every frequency on both sides of zero, and both float neighbours
            for m in (-3, 3):
                kink = np.float32(m * 2.0 ** -(k + 1))
                for v in (np.nextafter(kink, np.float32(-np.inf)), kink, np.nextafter(kink, np.float32(np.inf))):
                    assert bool((flat == float(v)).any()), (case, k, m)
        assert bool(((flat >= 0) & (flat < 1)).sum() >= 100) and bool((flat < -1).sum() >= 20) and float(flat.abs().max()) == 255.75
    r = _reference("sh_8")
    for point in ([0, 0, 0], [1, 1, 1], [1, 0, 1], [0.5, 0.5, 0], [1, 0.5, 0.5], [0.5, 0.5, 0.5]):
        assert bool((r.x == torch.tensor(point, dtype=torch.float32)).all(dim=1).any()), point
    on_sphere = ((r.x.double() * 2 - 1).norm(dim=1) - 1).abs() < 1e-6
    assert int(on_sphere.sum()) >= 241 and float(r.x.min()) >= 0 and float(r.x.max()) <= 1


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", FREQUENCY)
def test_rf32_stays_inside_the_frequency_bounds(case, precision):
    """The bounds are not vacuous and not too tight for a correct implementation: the fp32 restatement (the host's sinf / cosf) is
    inside them on the whole input set -- values, dy_dx and the dense sum at both loss scales; the worst ratios are printed"""
    r = _reference(case)
    ok, lines = check_values(r, precision, r.y32[precision].half() if precision == "half" else r.y32[precision])
    results = [(ok, lines)]
    results.append(check_jacobian(r, r.band32, "dy_dx"))
    for scale in (1.0, 128.0):
        dy = _dense_dy(r.width, scale)
        results.append(check_dense(r, dy, dense_reference(r, dy)[1], f"dense dL_dx at loss scale {scale:g}"))
    for _, lines in results:
        print("\n".join("Rf32 " + line for line in lines))
    assert all(ok for ok, _ in results)


def _swapped(t, i, j):
    out = t.clone()
    out[:, i], out[:, j] = t[:, j], t[:, i]
    return out


def _mutant(name):
    """(reference of the case, the mutated Jacobian of Rf32: the band of a periodic encoding, [n][W][3] of SH)"""
    if name == "trianglewave_k0_slope_sign":
        r = _reference("trianglewave_12x2")
        band = r.band32.clone()
        band[:, 0::r.P] = -band[:, 0::r.P]
        return r, band
    if name == "frequency_k1_dy_dx_halved":
        r = _reference("frequency_12x3")
        band = r.band32.clone()
        for phase in range(2):
            band[:, 2 + phase::r.P] = 0.5 * band[:, 2 + phase::r.P]
        return r, band
    if name == "frequency_k0_sine_cosine_paired_crosswise":  # dL_dy of the sine column meets dy_dx of the cosine column and back
        r = _reference("frequency_12x3")
        band = r.band32
        for a in range(r.n_in):
            band = _swapped(band, a * r.P, a * r.P + 1)
        return r, band
    r = _reference("sh_8")
    if name == "sh_l7_m1_columns_swapped_in_the_gradient":
        return r, _swapped(r.J32, 7 * 7 + 7 + 1, 7 * 7 + 7 - 1)
    assert name == "sh_l1_gradient_halved"
    J = r.J32.clone()
    J[:, 1:4] = 0.5 * J[:, 1:4]
    return r, J


MUTANTS = ["trianglewave_k0_slope_sign", "frequency_k1_dy_dx_halved", "frequency_k0_sine_cosine_paired_crosswise", "sh_l1_gradient_halved"]


@pytest.mark.parametrize("name", MUTANTS)
def test_mutants_pass_the_global_criterion_and_fail_per_element(name):
    """A wrong backward pass that the one-number criterion accepts on a dense dL_dy and that each per-element comparison rejects: the
    gap these tests close.  For SphericalHarmonics the mutant is a wrong factor in the degree-1 columns (entries about 1 beside
    degree-7 entries in the hundreds): swapping the columns l^2 + l +- m of l = 7, m = 1 moves dL_dx by 163 where the old tolerance is
    0.64, and the old criterion rejects that already (test_the_old_criterion_sees_a_swap_of_high_degree_columns)."""
    import torch

    r, mutated = _mutant(name)
    dy = _dense_dy(r.width, 1.0)
    want64, _ = dense_reference(r, dy)
    if _is_sh(r.case):
        dense = torch.einsum("ij,ija->ia", dy, mutated)
        unit_rows = slice(8 + 6 + 1 + 241, ref.N_ROWS)  # the uniform draws in [0, 1)^3
    else:
        dense = ref.dense_sum(dy, mutated, r.P, torch.float32)
        unit_rows = slice(0, 100)
    assert bool(((r.x[unit_rows] >= 0) & (r.x[unit_rows] < 1)).all())
    # the old test's rows, [0, 1), against R64; and on the whole set what the mutation itself adds to the unmutated Rf32 (there fp32
    # is far from R64 of its own accord: at |x| = 255.75 the argument's rounding alone moves a 2^11 pi column by hundreds)
    delta = float((dense[unit_rows].double() - want64[unit_rows]).abs().max())
    added = float((dense.double() - dense_reference(r, dy)[1].double()).abs().max())
    tolerance = [2e-3 * max(1.0, float(w.abs().max())) for w in (want64[unit_rows], want64)]
    print(f"{name}: dense dL_dx, rows in [0, 1): max |mutant - R64| {delta:.3e}, the old tolerance {tolerance[0]:.3e}; all rows: max |mutant - Rf32| {added:.3e}, the old tolerance {tolerance[1]:.3e}")
    assert delta > 0 and added > 0
    assert old_criterion_accepts(dense[unit_rows], want64[unit_rows]) and added <= tolerance[1]
    ok_jacobian, lines_jacobian = check_jacobian(r, mutated)
    ok_dense, lines_dense = check_dense(r, dy, dense)
    print("\n".join(lines_jacobian + lines_dense))
    assert not ok_jacobian and not ok_dense
    # and the comparisons accept what is not mutated
    unmutated = r.J32 if _is_sh(r.case) else r.band32
    assert check_jacobian(r, unmutated)[0] and check_dense(r, dy, dense_reference(r, dy)[1])[0]


def test_the_old_criterion_sees_a_swap_of_high_degree_columns():
    """Why the SH mutant above is not the swap of l = 7, m = 1: the one-number criterion rejects that one; so do the new comparisons"""
    import torch

    r, mutated = _mutant("sh_l7_m1_columns_swapped_in_the_gradient")
    dy = _dense_dy(r.width, 1.0)
    dense = torch.einsum("ij,ija->ia", dy, mutated)
    assert not old_criterion_accepts(dense, dense_reference(r, dy)[0])
    assert not check_jacobian(r, mutated)[0] and not check_dense(r, dy, dense)[0]


# ---------------------------------------------------------------------------------------------------- GPU
def _dtype(precision):
    import torch

    return torch.half if precision == "half" else torch.float32


def _forward(tcnn, n_in, cfg, precision, x, params=None):
    """(native module, context, x and the parameters on the device, output) of one fwd call that prepares input gradients"""
    import torch

    native = tcnn.Encoding(n_in, cfg, dtype=_dtype(precision)).native_tcnn_module
    xt = x.cuda().requires_grad_(True)
    if params is None:
        params = torch.zeros(native.n_params(), dtype=_dtype(precision), device="cuda")
    ctx, y = native.fwd(xt, params)
    return native, ctx, xt, params, y


def _case_forward(tcnn, case, precision):
    r = _reference(case)
    run = _forward(tcnn, r.n_in, r.cfg, precision, r.x)
    assert run[4].shape == (ref.N_ROWS, r.width) and run[4].dtype == _dtype(precision)
    return (r,) + run


def _report(ok, lines):
    print("\n".join("PER_ELEMENT " + line for line in lines))
    assert ok, "\n".join(lines)


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_values_per_element(tcnn, case, precision):
    r, _, _, _, _, y = _case_forward(tcnn, case, precision)
    _report(*check_values(r, precision, y.detach()))


def _one_hot_jacobian(r, native, ctx, xt, params, y, hot):
    """The Jacobian out of the backward pass: dL_dy holds `hot` in one column per input dim (periodic: column a P + k for every a in
    call k; SH: column j in call j) and +0 elsewhere, so dL_dx is hot * dy_dx of that column -- the other terms are 0 * finite, and
    for a power of two `hot` the product is exact"""
    import torch

    calls = r.width if _is_sh(r.case) else r.P
    out = []
    for k in range(calls):
        dy = torch.zeros_like(y)
        if _is_sh(r.case):
            dy[:, k] = hot
        else:
            dy[:, k::r.P] = hot
        dx, _ = native.bwd(ctx, xt, params, y, dy)
        assert dx.dtype == torch.float32 and dx.shape == (ref.N_ROWS, r.n_in)
        out.append(dx)
    stacked = torch.stack(out, dim=1 if _is_sh(r.case) else 2).cpu()  # SH [n][W][3]; periodic [n][D][P]
    return stacked if _is_sh(r.case) else stacked.reshape(ref.N_ROWS, r.n_in * r.P)


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_jacobian_per_entry_by_one_hot_dL_dy(tcnn, case, precision):
    """One backward call per output-per-input index (SH: per column) with the hot value 1, compared entry by entry; once more with
    -0.5, which must give -0.5 times the first run bit for bit (the scaling is exact).  Where an entry is zero the sign of the zero is
    left open: SH's accumulators start at +0 and add (hot * 0) + (0 * finite), whose sign follows the operands, not the product."""
    r, native, ctx, xt, params, y = _case_forward(tcnn, case, precision)
    first = _one_hot_jacobian(r, native, ctx, xt, params, y, 1.0)
    _report(*check_jacobian(r, first, f"{precision} Jacobian"))
    second = _one_hot_jacobian(r, native, ctx, xt, params, y, -0.5)
    report = _same_bits(r, "Jacobian with the hot value -0.5 against -0.5 times the first run", second, -0.5 * first, zero_sign=False)
    assert report is None, report
    if case != "sh_1":
        assert float(first.abs().sum()) > 0


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_dense_dL_dx_per_element(tcnn, case, precision):
    """dL_dy dense in [-1, 1), and once at loss scale 128"""
    r, native, ctx, xt, params, y = _case_forward(tcnn, case, precision)
    for scale in (1.0, 128.0):
        dy = _dense_dy(r.width, scale)
        dx, _ = native.bwd(ctx, xt, params, y, dy.to(_dtype(precision)).cuda())
        _report(*check_dense(r, dy, dx.cpu(), f"{precision} dense dL_dx at loss scale {scale:g}"))


GRID_F8 = {"otype": "HashGrid", "n_levels": 1, "n_features_per_level": 8, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("behind", ["last", "padded"])
@pytest.mark.parametrize("case", list(CASES))
def test_nested_behind_identity_has_the_bits_of_the_encoding_alone(tcnn, case, precision, behind):
    """Composite[Identity on 3 dims, the encoding]: its input view starts at column 3 of rows 3 + n_in floats apart ("last"), its
    output at column 3.  "padded": a grid with 8 features per level on three more dims follows, so the encoding is padded until
    3 + its width is a multiple of 8 (rows 6 + n_in apart).  Live output columns and dL_dx[:, 3:3 + n_in] have the bits of the
    encoding alone; the padding columns hold ones (SH: they come first) and take no part in dL_dx."""
    import torch

    r, native, ctx, xt, params, y = _case_forward(tcnn, case, precision)
    dtype = _dtype(precision)
    g = torch.Generator().manual_seed(7)
    nested = [{"n_dims_to_encode": 3, "otype": "Identity"}, {"n_dims_to_encode": r.n_in, **r.cfg}]
    columns = [torch.rand(ref.N_ROWS, 3, generator=g), r.x]
    pad = 0
    if behind == "padded":
        nested.append({"n_dims_to_encode": 3, **GRID_F8})
        columns.append(torch.rand(ref.N_ROWS, 3, generator=g))
        pad = -(3 + r.width) % 8
        assert pad > 0
    n_all = sum(c.shape[1] for c in columns)
    enc = tcnn.Encoding(n_all, {"otype": "Composite", "nested": nested}, dtype=dtype)
    assert enc.n_output_dims == 3 + r.width + pad + (8 if behind == "padded" else 0)
    p_all = (torch.rand(enc.native_tcnn_module.n_params(), generator=g) * 2 - 1).to(dtype).cuda()
    _, ctx_all, x_all, _, y_all = _forward(tcnn, n_all, {"otype": "Composite", "nested": nested}, precision, torch.cat(columns, dim=1), p_all)
    first = r.cfg["otype"] == "SphericalHarmonics"
    live = slice(3 + pad, 3 + pad + r.width) if first else slice(3, 3 + r.width)
    padding = slice(3, 3 + pad) if first else slice(3 + r.width, 3 + r.width + pad)
    report = _same_bits(r, f"{behind} nested values", y_all[:, live].detach().cpu(), y.detach().cpu())
    assert report is None, report
    assert bool((y_all[:, padding] == 1).all()) and torch.equal(y_all[:, :3].detach().float().cpu(), columns[0].to(dtype).float())

    dy = _dense_dy(r.width, 1.0)
    dy_all = _dense_dy(enc.n_output_dims, 1.0).clone()  # (dense in the padding columns too: they must not reach dL_dx)
    dy_all[:, live] = dy
    dx, _ = native.bwd(ctx, xt, params, y, dy.to(dtype).cuda())
    dx_all, _ = enc.native_tcnn_module.bwd(ctx_all, x_all, p_all, y_all, dy_all.to(dtype).cuda())
    report = _same_bits(r, f"{behind} nested dL_dx", dx_all[:, 3:3 + r.n_in].cpu(), dx.cpu())
    assert report is None, report
    assert torch.equal(dx_all[:, :3].cpu(), dy_all[:, :3].to(dtype).float())  # Identity: scale 1
    if case != "sh_1":
        assert float(dx.abs().sum()) > 0


def _trainer_config(cfg, precision):
    return {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2},
            "encoding": cfg, "network": {"otype": "FullyFusedMLP" if precision == "half" else "CutlassMLP", "activation": "ReLU",
                                         "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}}


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_trainer_reads_soa_input_like_aos(tcnn, case, precision):
    """Trainer (native.py): the encoding in front of a small MLP -- FullyFusedMLP in half; an fp32 trainer has no FullyFusedMLP, there
    CutlassMLP -- fed with [n][n_in] as LAYOUT_AOS and with the transposed [n_in][n] as LAYOUT_SOA (the encoding reads its inputs n
    floats apart).  Outputs agree bit for bit, and so does dL_dinput, which training_step returns in the input's layout."""
    import torch

    from tinycudann.native import LAYOUT_AOS, LAYOUT_SOA

    r = _reference(case)
    dtype = _dtype(precision)
    tr = tcnn.Trainer(r.n_in, 3, _trainer_config(r.cfg, precision), seed=1337, dtype=dtype)
    dy = (_dense_dy(tr.padded_output_width, 1.0) / ref.N_ROWS).to(dtype).cuda()
    x = r.x.cuda()
    runs = {}
    for layout, xin in ((LAYOUT_AOS, x), (LAYOUT_SOA, x.t().contiguous())):
        dx = torch.zeros_like(xin)
        ctx = tr.training_step(xin, None, run_optimizer=False, dL_dinput=dx, external_dL_dy=dy, input_layout=layout)
        runs[layout] = (ctx.output().cpu(), (dx if layout == LAYOUT_AOS else dx.t().contiguous()).cpu())
    (out_aos, dx_aos), (out_soa, dx_soa) = runs[LAYOUT_AOS], runs[LAYOUT_SOA]
    report = _same_bits(r, "trainer output, SoA against AoS", out_soa, out_aos) or _same_bits(r, "trainer dL_dinput, SoA against AoS", dx_soa, dx_aos)
    assert report is None, report
    assert float(out_aos.float().abs().sum()) > 0 and bool(torch.isfinite(out_aos.float()).all())
    if case != "sh_1":
        assert float(dx_aos.abs().sum()) > 0


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_300_rows_are_the_first_300_of_512(tcnn, case, precision):
    """tcnn.Encoding pads 300 rows to the batch granularity's 512 and returns 300: output and x.grad have the bits of the first 300
    rows of the 512-row call (every row is computed on its own)"""
    import torch

    r = _reference(case)
    dtype = _dtype(precision)
    enc = tcnn.Encoding(r.n_in, r.cfg, dtype=dtype)
    dy = _dense_dy(r.width, 1.0).to(dtype).cuda()
    got = {}
    for n in (300, ref.N_ROWS):
        x = r.x[:n].cuda().requires_grad_(True)
        y = enc(x)
        assert y.shape == (n, r.width) and y.dtype == dtype
        y.backward(dy[:n])
        assert x.grad.shape == (n, r.n_in) and x.grad.dtype == torch.float32
        got[n] = (y.detach().cpu(), x.grad.cpu())
    report = _same_bits(r, "300-row output", got[300][0], got[ref.N_ROWS][0][:300]) or _same_bits(r, "300-row x.grad", got[300][1], got[ref.N_ROWS][1][:300])
    assert report is None, report
    ok, lines = check_values(r, precision, torch.cat([got[300][0], got[ref.N_ROWS][0][300:]]))
    assert ok, lines
