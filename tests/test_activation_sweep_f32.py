"""Every activation over a wide float32 range, in the fp32 MLP kernels (k_mlp_layers.hip).

The fp32 networks instantiate activation_fwd<float>, activation_bwd<float>, act_d1, act_d2 and expf_near_zero of mlp_device.h in
k_layer_gemm<float> (the narrow tile <1,4,4,4> and the wide one <2,2,4,4>, the first-order and the second-order epilogue of each),
k_layer_delta<float> and k_act_bwd_output<float>.  tests/test_fp32_network.py feeds them pre-activations within about |z| < 2 and judges a tensor
by its maximum; here 65 536 floats from the smallest subnormal to the largest finite float go through each activation, in the setting of
tests/activation_sweep_f32.py (identity weights: every tensor is an elementwise function of x, dL/dy and the tangent v), and every single
float is judged: expf's overflow at 88.72 (8.872 for Softplus), its subnormal results and its underflow, the 2^-6 switch inside
expf_near_zero, Squareplus' cancellation for negative arguments, 1 - y y and 1 - s in saturation, sinf / cosf of k pi / 2 up to k = 2^40 and
beyond, fp32 subnormals through v_mfma_f32_16x16x4_f32, inf * 0 in the backward expressions.

The bar is set membership (tests/activation_sweep_f32.py): the device's float is bit for bit one of the candidates of the restatement, signs
of zero included -- one value for None, ReLU, LeakyReLU and Squareplus, which call no libm function -- on every row that is finite in the
restatement; on the other rows the class (finite, +inf, -inf, NaN) of every element is the restatement's.  Per width (48 and 144) and case
(hidden activation A with output None; hidden None with output activation B) in one hidden layer:
  * native.fwd with a context, and without one (inference), whose bits equal the training forward's on every row;
  * native.bwd: dL/dinput against activation_bwd of the device's OWN forward output (a Sine hidden layer: from the pre-activation);
  * native.bwd_bwd_input: dL/d(dL/doutput) = a'(x) v and the second-order dL/dinput = a''(x) dL/dy v;
  * every pass twice, the same bits.
Squareplus in two hidden layers runs through bwd_bwd_input as well: the only curved activation without a libm call, so the only one that
holds LG_CURVATURE's c + d1 * acc with a curved d1 bit for bit through A(A(x)).

Not judged: parameter gradients, sums over the 4096 rows here (tests/test_fp32_network.py bounds them).  k_layer_delta<float> runs in every
(None, B) case and is restated (activation_sweep_f32.delta, held against float64 below), but its result d_K = a'(z_K) dL/dy reaches only the
parameter gradients; what it calls, act_d1, is judged through dL/d(dL/doutput).  The fp32 Trainer is held bit for bit against the module
(tests/test_fp32_training.py), so it is covered by this sweep.  Measured shares: profiles/activation_sweep_f32.txt.
"""
import math
import os
import re

import numpy as np
import pytest

import activation_sweep as sw
import activation_sweep_f32 as s32
from conftest import ROOT

gpu = pytest.mark.gpu
F = np.float32
CASES = sw.cases()
TENSORS = ("out", "dx", "ddy", "dx2")
CASE_IDS = [sw.case_id(c) for c in CASES]


# ---------------------------------------------------------------------------------------------------- CPU: the setting
def test_the_sweep_holds_what_it_lists():
    x = s32.sweep_x()
    n = s32.sweep_count()
    v = x.ravel()[:n]
    assert x.shape == (4096, 16) and x.dtype == F and np.all(np.isfinite(x))
    assert n >= 65536 - 16 and not s32.bits(x.ravel()[n:]).any()  # zero-padded, by less than a row
    o = s32.ordered(v)
    assert np.all(np.diff(o) >= 0) and np.count_nonzero(np.diff(o) == 0) == 1  # ascending; -0 and +0 are the one pair of equals
    have = set(s32.bits(v).tolist())
    holds = lambda a: set(s32.bits(np.asarray(a, dtype=F)).tolist()) <= have
    assert holds([0.0, -0.0])
    for sign in (F(1), F(-1)):
        b = s32.binade_boundaries()
        assert b.size == 277 and b[0] == F(2.0 ** -149) and b[-1] == F(2.0 ** 127)
        assert holds(sign * b) and holds(sign * np.nextafter(b, F(np.inf))) and holds(sign * np.nextafter(b, F(0))[1:])
        assert holds([sign * np.finfo(F).max])
        t = np.asarray([88.7228, 8.87228, 87.3365, 103.972, 8.73365, 10.3972, 2.0 ** -6, 2.0 ** -6 / 10, 65504.0] + [2.0 ** j * math.pi / 2 for j in range(41)])
        mine = s32.thresholds().astype(np.float64)
        assert mine.size == t.size and all(np.min(np.abs(mine - u) / u) < 1e-6 for u in t)
        th = s32.thresholds()
        assert holds(sign * th) and holds(sign * np.nextafter(th, F(np.inf))) and holds(sign * np.nextafter(th, F(0)))
    # the dense part: every binade of [2^-12, 2^7) holds the same number of floats (+- 1, and the fixed ones), no two of them farther apart
    # than two of its even spacings
    mag = np.abs(v.astype(np.float64))
    counts = []
    for e in s32.DENSE_BINADES:
        inside = np.sort(mag[(v > 0) & (mag >= 2.0 ** e) & (mag < 2.0 ** (e + 1))])
        counts.append(inside.size)
        assert np.max(np.diff(inside)) <= 2 * 2.0 ** e / (inside.size - 40)
    assert min(counts) > 1600 and max(counts) - min(counts) <= 40
    assert np.array_equal(np.sort(-v[v < 0]), np.sort(v[v > 0]))  # each sign gets the same


def test_dL_dy_and_the_tangent_stay_in_range():
    g, v = s32.dy(), s32.tangent()
    assert not np.array_equal(g, v) and np.array_equal(s32.bits(g), s32.bits(s32.dy()))  # two seeds, fixed
    for a in (g, v):
        mag = np.abs(a.astype(np.float64))
        assert a.dtype == F and np.all(mag >= 2.0 ** -10) and np.all(mag < 2.0 ** 4)
        exps = np.unique(np.floor(np.log2(mag)))
        assert exps.min() == -10 and exps.max() == 3 and exps.size == 14
        assert np.any(a < 0) and np.any(a > 0) and np.unique(s32.bits(a) & 0x7FFFFF).size > 60000


def test_the_allowances_are_the_measured_ones():
    """K_f of activation_sweep_f32 is what profiles/libm_f32_ulp.txt records, and no more than the few ulp test_fp32_network.py allows; the
    profile's one other constant, powf in Adam's debiasing factor, is the K_POWF of adam_reference"""
    import adam_reference

    text = open(os.path.join(ROOT, "profiles", "libm_f32_ulp.txt")).read()
    measured = {name: int(k) for name, k in re.findall(r"^K_(\w+)\s*= (\d+)$", text, flags=re.M)}
    mine = {"EXPF": s32.K_EXPF, "LOGF": s32.K_LOGF, "SINF": s32.K_SINF, "COSF": s32.K_COSF, "TANHF": s32.K_TANHF}
    assert measured == {**mine, "POWF": adam_reference.K_POWF}
    assert all(0 <= k <= s32.MAX_K for k in mine.values())


def test_candidates_are_float_steps():
    a = np.asarray([[0.0, -0.0, 1.0, -1.0, np.finfo(F).max, 2.0 ** -149, np.inf, np.nan]], dtype=F)
    up, down = s32.moved(a, 1)[0], s32.moved(a, -1)[0]
    assert np.array_equal(up[:6], np.asarray([2.0 ** -149, 2.0 ** -149, 1 + 2.0 ** -23, -1 + 2.0 ** -24, np.inf, 2.0 ** -148], dtype=F))
    assert np.array_equal(down[:6], np.asarray([-2.0 ** -149, -2.0 ** -149, 1 - 2.0 ** -24, -1 - 2.0 ** -23, np.finfo(F).max * (1 - 2.0 ** -24), 0.0], dtype=F))
    assert up[6] == np.inf and down[6] == np.inf and np.isnan(up[7]) and np.isnan(down[7])
    c = s32.candidates(np.exp, 2, np.asarray([[[1.0, 0.0]]], dtype=F))
    assert c.shape == (5, 1, 2) and np.array_equal(s32.ordered(c[:, 0, 0]) - s32.ordered(c[0, 0, 0]), [0, -1, 1, -2, 2]) and c[0, 0, 1] == 1
    got = np.asarray([[1.0, -0.0, np.nan]], dtype=F)
    cands = np.asarray([[[1.0, 0.0, np.nan]], [[2.0, -0.0, 1.0]]], dtype=F)
    assert s32.member(got, cands).tolist() == [[[True, False, True]], [[False, True, False]]]  # signs of zero count, NaN matches NaN


def test_a_product_with_the_identity_weights():
    """activation_sweep_f32.product against the fmaf chain it stands for, in float64 numpy on values that are exact there"""
    rs = np.random.RandomState(3)
    a = rs.uniform(-4, 4, (64, 16)).astype(F)
    a[1, 3], a[2, 5], a[3, 7], a[4, 2], a[4, 9], a[5, 0] = -0.0, np.inf, np.nan, np.inf, -np.inf, 2.0 ** -149
    for width in (16, 48, 144):
        w = np.zeros((16, width))
        for c in range(16):
            w[c, sw.neuron_of(c, width)] = 1.0
        with np.errstate(invalid="ignore"):
            chain = np.zeros((64, width))
            for k in range(16):  # acc = fmaf(a[k], w[k], acc), ascending k, from +0
                chain = a[:, k:k + 1].astype(np.float64) * w[k:k + 1] + chain
        want = chain[:, [sw.neuron_of(c, width) for c in range(16)]].astype(F)
        got = s32.product(a[None])[0]
        assert np.array_equal(s32.bits(got)[~np.isnan(want)], s32.bits(want)[~np.isnan(want)]) and np.array_equal(np.isnan(got), np.isnan(want))
    assert not np.signbit(got[1, 3]) and got[5, 0] == F(2.0 ** -149) and np.isnan(got[2, 0]) and got[2, 5] == np.inf and np.isnan(got[4, 2])


# ---------------------------------------------------------------------------------------------------- CPU: the restatement against float64
BOUND = 2.0 ** -16
"""relative, where the expression is well conditioned.  Every expression is at most eight float roundings (2^-24 each) and on the ranges below no
step magnifies a relative error by more than Softplus' rounding of 10 x ahead of expf does: |10 x| <= 89 times 2^-24, below 2^-17.  The bar is
32 times finer than a rounding to half and far below any error in a formula; it is not meant to see a last bit."""


def _exact(act, x):
    """(a, a', a'') of the mathematical function in float64, written independently of the kernels' expressions"""
    with np.errstate(all="ignore"):
        one, zero = np.ones_like(x), np.zeros_like(x)
        if act == "None":
            return x, one, zero
        if act == "ReLU":
            return np.maximum(x, 0), (x > 0) * one, zero
        if act == "LeakyReLU":
            return np.where(x > 0, x, x / 100), np.where(x > 0, 1.0, 1 / 100), zero
        if act == "Exponential":
            return np.exp(x), np.exp(x), np.exp(x)
        if act == "Sine":
            return np.sin(x), np.cos(x), -np.sin(x)
        if act == "Sigmoid":
            d1 = 1 / (2 * np.cosh(x / 2)) ** 2
            return np.exp(-np.logaddexp(0, -x)), d1, -d1 * np.tanh(x / 2)
        if act == "Squareplus":
            q = np.hypot(10 * x, 2)
            return np.where(x >= 0, (10 * x + q) / 20, 0.2 / (q - 10 * x)), np.where(x >= 0, (10 * x + q) / (2 * q), 2 / (q * (q - 10 * x))), 20 / q ** 3
        if act == "Softplus":
            return np.logaddexp(0, 10 * x) / 10, np.exp(-np.logaddexp(0, -10 * x)), 10 / (2 * np.cosh(5 * x)) ** 2
        if act == "Tanh":
            return np.tanh(x), 1 / np.cosh(x) ** 2, -2 * np.tanh(x) / np.cosh(x) ** 2
    raise ValueError(act)


# where each expression is well conditioned, as a rule on x: (lowest, highest) pairs
EVERYWHERE = [(-np.inf, np.inf)]
WELL_CONDITIONED = {
    "fwd": {"None": EVERYWHERE, "ReLU": EVERYWHERE, "LeakyReLU": EVERYWHERE, "Exponential": [(-87, 87)], "Sine": EVERYWHERE, "Sigmoid": [(-87, np.inf)],
            "Squareplus": [(0, 1e18)], "Softplus": [(0, 8.8)], "Tanh": EVERYWHERE},
    # a' from the forward output (Sine: from the pre-activation), times dL/dy (|dL/dy| < 16: Exponential stays below the overflow)
    "bwd": {"None": EVERYWHERE, "ReLU": EVERYWHERE, "LeakyReLU": EVERYWHERE, "Exponential": [(-80, 80)], "Sine": EVERYWHERE, "Sigmoid": [(-87, 1)],
            "Squareplus": [(0, 1e18)], "Softplus": [(0, 8.8)], "Tanh": [(-1, 1)]},
    # 1 - s, 1 - t t and Squareplus' 1 + y / sqrt(..) cancel on the other side
    "d1": {"None": EVERYWHERE, "ReLU": EVERYWHERE, "LeakyReLU": EVERYWHERE, "Exponential": [(-87, 87)], "Sine": EVERYWHERE, "Sigmoid": [(-87, 1)],
           "Squareplus": [(0, 1e18)], "Softplus": [(-8.7, 8.7)], "Tanh": [(-1, 1)]},
    # 1 - 2 s cancels around zero
    "d2": {"Exponential": [(-87, 87)], "Sine": EVERYWHERE, "Sigmoid": [(-8, -0.5), (0.5, 1)], "Squareplus": [(-1e6, 1e6)], "Softplus": [(-8.7, 0.1)], "Tanh": [(-1, 1)]},
}


def _assert_close(what, got, want, x, ranges):
    got, want = got.astype(np.float64), np.asarray(want, dtype=np.float64)
    inside = np.zeros(x.shape, dtype=bool)
    for lo, hi in ranges:
        inside |= (x >= lo) & (x <= hi)
    with np.errstate(invalid="ignore"):
        judged = inside & (np.abs(want) >= 2.0 ** -100) & (np.abs(want) <= 2.0 ** 120)  # normal numbers on both sides
    assert np.count_nonzero(judged) >= 1000, (what, int(np.count_nonzero(judged)))
    err = np.abs(got[judged] - want[judged]) / np.abs(want[judged])
    worst = float(err.max())
    print(f"{what}: {int(np.count_nonzero(judged))} judged, largest relative error {worst:.3e}")
    assert worst <= BOUND, f"{what}: relative error {worst} at x = {float(x[judged][np.argmax(err)])!r}"


@pytest.mark.parametrize("act", sw.ACTIVATIONS)
def test_restatement_is_the_mathematical_function(act):
    """the j = 0 restatement of activation_fwd, activation_bwd (from the restated output; a Sine hidden layer from the pre-activation), act_d1,
    act_d2, k_layer_delta<float> and the epilogue's products against float64, so that a restatement that copies a kernel's bug does not pass"""
    m = s32.ONE_CANDIDATE
    x32, g32, v32 = s32.sweep_x(), s32.dy(), s32.tangent()
    x, g, v = (a.astype(np.float64) for a in (x32, g32, v32))
    a0, a1, a2 = _exact(act, x)
    with np.errstate(all="ignore"):
        _restatement_against(act, m, x32, g32, v32, x, g, v, a0, a1, a2)


def _restatement_against(act, m, x32, g32, v32, x, g, v, a0, a1, a2):
    y = s32.activation_fwd(m, act, x32[None])
    _assert_close(f"{act} forward", y[0], a0, x, WELL_CONDITIONED["fwd"][act])
    bwd = s32.sine_bwd(m, g32[None], x32[None]) if act == "Sine" else s32.activation_bwd(m, act, g32[None], y)
    _assert_close(f"{act} backward", bwd[0], a1 * g, x, WELL_CONDITIONED["bwd"][act])
    aux = x32[None] if act in s32.CURVATURE else y
    _assert_close(f"{act} delta", s32.delta(m, act, g32[None], aux)[0], a1 * g, x, WELL_CONDITIONED["d1"][act])
    _assert_close(f"{act} d1 * acc", (s32.act_d1(m, act, aux) * v32[None])[0], a1 * v, x, WELL_CONDITIONED["d1"][act])
    if act in s32.CURVATURE:
        _assert_close(f"{act} (d2 * g) * acc", (s32.act_d2(m, act, aux) * g32[None] * v32[None])[0], a2 * g * v, x, WELL_CONDITIONED["d2"][act])
    else:
        assert not s32.bits(s32.act_d2(m, act, aux)).any()


def test_expf_near_zero_is_restated_exactly():
    """the polynomial branch has no libm call: one candidate however wide the allowance, within a float step of exp below 2^-6, and expf beyond"""
    x32 = s32.sweep_x()
    wide = s32.expf_near_zero(s32.Libm(ks={"expf": 2, "logf": 0, "sinf": 0, "cosf": 0, "tanhf": 0}), x32[None])
    assert wide.shape[0] == 5
    small = np.abs(x32) < F(2.0 ** -6)
    assert np.count_nonzero(small) > 20000 and np.count_nonzero(~small) > 20000
    assert all(np.array_equal(s32.bits(wide[j][small]), s32.bits(wide[0][small])) for j in range(5))
    with np.errstate(over="ignore"):
        exact = np.exp(x32.astype(np.float64))
        correctly_rounded = exact.astype(F)
    assert np.max(np.abs(s32.ordered(wide[0][small]) - s32.ordered(correctly_rounded[small]))) <= 1
    assert np.mean(s32.bits(wide[0][small]) == s32.bits(correctly_rounded[small])) > 0.9999
    finite = ~small & np.isfinite(correctly_rounded)
    assert np.array_equal(s32.ordered(wide[:, finite]) - s32.ordered(correctly_rounded[finite])[None], np.repeat([[0], [-1], [1], [-2], [2]], np.count_nonzero(finite), axis=1))


NP_ACTIVATIONS = [a for a in sw.ACTIVATIONS if a != "LeakyReLU"]  # test_fp32_network's restatement has no LeakyReLU


@pytest.mark.parametrize("act", NP_ACTIVATIONS)
def test_restatement_reproduces_the_float32_restatement_of_test_fp32_network(act):
    """_np_act, _np_d1 and _np_d2 of tests/test_fp32_network.py in float32 on the sweep's elements of [-2, 2] are among the candidates, with
    the allowance MAX_K for every function: the host's float32 libm is not the device's, and numpy documents its own at up to three steps.  (Sigmoid' and '' below 2^-6: the kernels' expf_near_zero is no libm call and
    has one candidate, _np_d1 calls np.exp; left out.)"""
    from test_fp32_network import _np_act, _np_d1, _np_d2

    x = s32.sweep_x()
    inside = np.abs(x) <= 2
    m = s32.Libm(ks={name: s32.MAX_K for name in s32.Libm().k})
    with np.errstate(all="ignore"):
        for what, mine, theirs in (("a", s32.activation_fwd(m, act, x[None]), _np_act(act, x)), ("a'", s32.act_d1(m, act, x[None]), _np_d1(act, x)),
                                   ("a''", s32.act_d2(m, act, x[None]), _np_d2(act, x))):
            judged = inside & ~(np.abs(x) < 2.0 ** -6) if act == "Sigmoid" and what != "a" else inside
            ok = s32.member(theirs + F(0), mine + F(0)).any(axis=0)  # (+0 and -0 as one: np.where picks its zeros elsewhere)
            assert np.count_nonzero(judged) > 15000 and ok[judged].all(), (act, what, int(np.count_nonzero(~ok[judged])))


def _runs(mask):
    """lengths of the contiguous runs of True in a flat boolean array"""
    edges = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    return np.flatnonzero(edges == -1) - np.flatnonzero(edges == 1)


@pytest.mark.parametrize("case", CASES + [("Squareplus", "None", 2)], ids=CASE_IDS + ["squareplus-none-2"])
def test_few_rows_leave_the_bit_comparison(case):
    """A condition on the restatement alone, so that the GPU tests cannot end up comparing nothing: per tensor, a contiguous run of m
    non-finite elements of the elementwise result (the sweep ascends: expf's overflow is one run) takes at most ceil(m / 16) + 2 rows out of the
    bit comparison, and in all at most 15 % of the rows leave it for Exponential and Softplus, 2 % for the others."""
    hidden = case[2] if len(case) == 3 else 1
    case = case[:2]
    r, e = s32.restatement(case, hidden, 0), s32.restatement(case, hidden, 0, elementwise=True)
    cap = s32.MAX_SHARE_OUTSIDE.get(sw.curved(case), 0.02)
    for t in TENSORS:
        outside = int(np.count_nonzero(~s32.finite_rows(r[t][0])))
        runs = _runs(~np.isfinite(e[t][0]).ravel())
        allowed = int(sum(-(-int(m) // 16) + 2 for m in runs))
        print(f"{sw.case_id(case)} x{hidden} {t}: {outside} rows outside, {runs.size} runs of non-finite elements allow {allowed}")
        assert outside <= allowed and outside <= cap * 4096, (t, outside, allowed)
        assert np.any(r[t][0][s32.finite_rows(r[t][0])] != 0) or (t == "dx2" and sw.curved(case) not in s32.CURVATURE)


# ---------------------------------------------------------------------------------------------------- GPU
def _t(a, grad=False):
    import torch

    return torch.from_numpy(np.array(a, dtype=F, copy=True)).cuda().requires_grad_(grad)


def _module(tcnn, width, hidden, case):
    from test_fp32_network import FP32, _create, _layer_sizes

    native = _create(tcnn, 16, 16, s32.network_config(width, hidden, case), FP32)
    w = sw.identity_weights(s32.layer_slices(_layer_sizes(native)), width)
    assert native.n_params() == w.size and native.param_precision() == FP32
    return native, w


def _passes(native, w, first_order=True):
    """forward (training and inference), backward and backward_backward_input, all of it twice: [{name: float32 numpy}] * 2"""
    import torch

    runs = []
    for _ in range(2):
        xt, pt, dyt = _t(s32.sweep_x(), True), _t(w), _t(s32.dy(), True)
        ctx, out = native.fwd(xt, pt)
        no_ctx, inferred = native.fwd(_t(s32.sweep_x()), pt)
        assert ctx is not None and no_ctx is None
        got = {"out": out, "inferred": inferred}
        if first_order:
            got["dx"], dp = native.bwd(ctx, xt, pt, out, dyt)
            assert dp is None
        got["ddy"], dp2, got["dx2"] = native.bwd_bwd_input(ctx, xt, pt, _t(s32.tangent()), dyt)
        assert dp2 is None
        torch.cuda.synchronize()
        runs.append({k: t.detach().cpu().numpy() for k, t in got.items()})
    return runs


def _assert_two_runs_agree(what, runs):
    for k in runs[0]:
        assert runs[0][k].dtype == F and np.array_equal(s32.bits(runs[0][k]), s32.bits(runs[1][k])), f"{what} {k}: two runs differ"


@gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("width", s32.WIDTHS)
def test_activation_sweep_f32(tcnn, width, case):
    what = f"layers{width} {sw.case_id(case)}"
    native, w = _module(tcnn, width, 1, case)
    runs = _passes(native, w)
    got = runs[0]
    r = s32.restatement(case)
    s32.compare(got["out"], r["out"], r["out"][0], what + " forward")
    assert np.array_equal(s32.bits(got["inferred"]), s32.bits(got["out"])), f"{what}: inference is not the training forward"
    dx = s32.backward(s32.Libm(), case, s32.sweep_x(), s32.dy(), own_output=got["out"])
    s32.compare(got["dx"], dx, r["dx"][0], what + " backward")
    s32.compare(got["ddy"], r["ddy"], r["ddy"][0], what + " dL_ddLdoutput")
    s32.compare(got["dx2"], r["dx2"], r["dx2"][0], what + " dL_dinput2")
    _assert_two_runs_agree(what, runs)


@gpu
@pytest.mark.parametrize("width", s32.WIDTHS)
def test_squareplus_twice_through_the_curvature_pass(tcnn, width):
    """Squareplus(Squareplus(x)): LG_CURVATURE's c + d1 * acc with a curved d1, bit for bit"""
    case = ("Squareplus", "None")
    what = f"layers{width}x2 {sw.case_id(case)}"
    native, w = _module(tcnn, width, 2, case)
    runs = _passes(native, w, first_order=False)
    r = s32.restatement(case, hidden=2)
    assert all(r[t].shape[0] == 1 for t in TENSORS)
    s32.compare(runs[0]["out"], r["out"], r["out"][0], what + " forward")
    assert np.array_equal(s32.bits(runs[0]["inferred"]), s32.bits(runs[0]["out"]))
    s32.compare(runs[0]["ddy"], r["ddy"], r["ddy"][0], what + " dL_ddLdoutput")
    s32.compare(runs[0]["dx2"], r["dx2"], r["dx2"][0], what + " dL_dinput2")
    _assert_two_runs_agree(what, runs)
