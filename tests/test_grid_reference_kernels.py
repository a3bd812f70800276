"""The reference-shaped grid kernels of k_grid.hip -- k_grid_fwd<float>, k_grid_bwd with float atomics (fp32 grids, and the fp32 scratch
of every half grid with one feature per level), k_grid_bwd with packed-fp16 atomics (TCNN_AMD_GRID_SCATTER=atomic, and every grid the
LDS scatter cannot take) and k_grid_bwd_input<float> -- against the oracle's restatement of the reference's T = float instantiation
(oracle.GridEncoding.forward_f32 / backward_input_f32 / backward_terms, pinned on the CPU by tests/test_oracle.py).

No tolerance here is a measured number:
  a. the fp32 forward pass and b. the fp32 dL/dx have a fixed order of operations (fp32 weight product in dimension order, an explicit fmaf
     chain in corner order, a fixed summation order; -ffp-contract=off): bit for bit.
  c. dL/dparams is a sum of k contributions by atomics in an order nobody fixes.  With S their exact sum, A the sum of their magnitudes
     and u the unit roundoff of one addition, ANY order gives |got - S| <= gamma(k - 1) * A, gamma(m) = m u / (1 - m u): asserted for every
     parameter and reported per level.  The F = 1 half gradient is the fp32 sum rounded to half once; rounding is monotone, so it lies in
     [rn_half(S - e), rn_half(S + e)].  The packed-fp16 form adds in fp16 (u = 2^-11), with one subnormal spacing (2^-24) to spare.
Every test first asserts on the CPU that no non-zero contribution is smaller than 2^-100: sums of such numbers stay normal in fp32, and
how the float atomics treat subnormals stays out of the comparison.

GradientMode::Accumulate of these routes is reachable through a Trainer only, and checking it needs dL/dy of the encoding, which the
trainer does not expose: out of scope here.
"""
import numpy as np
import pytest

from grid_reference import (MIN_CONTRIBUTION, REFERENCE_KERNEL_CASES, U16, U32, assert_fp32_forward_bit_exact, case_id, check_rounded_sum_per_level,
                            check_sum_per_level, fp32_module, print_records, reference_inputs, to_device)

pytestmark = pytest.mark.gpu

SCALAR_CASES = [c for c in REFERENCE_KERNEL_CASES if c[1]["n_features_per_level"] == 1]
PACKED_CASES = [c for c in REFERENCE_KERNEL_CASES if c[1]["n_features_per_level"] >= 2]
PADDED_CASE, PADDED_ROWS = REFERENCE_KERNEL_CASES[4], 1000  # 3-D, F = 4, Smoothstep: the module pads 1000 rows to 1024

_REFERENCES = {}


class _Reference:
    """What the oracle says about one case: computed once, shared by the tests of the case, never written to."""

    def __init__(self, oracle, case, n):
        n_in, cfg = case
        self.ref = ref = oracle.create_encoding(n_in, cfg, alignment=0)
        self.x, self.params, self.dy = reference_inputs(oracle, ref, n)
        self.params_h, self.dy_h = oracle.half_bits(self.params), oracle.half_bits(self.dy)
        self.nearest = ref.g.interpolation == oracle.INTERP["nearest"]
        self.out, ctx = ref.forward_f32(self.x, self.params, want_dy_dx=True)
        self.dL_dx = ref.backward_input_f32(ctx, self.dy)
        self._oracle, self._terms = oracle, {}
        for a in (self.x, self.params, self.dy, self.params_h, self.dy_h, self.out, self.dL_dx):
            a.setflags(write=False)

    def terms(self, product):
        if product not in self._terms:
            t = self.ref.backward_terms(self.x, self.dy if product == self._oracle.PRODUCT_FP32 else self.dy_h, product)
            assert t["min_nonzero"] >= MIN_CONTRIBUTION, "a contribution below 2^-100: the comparison would depend on subnormal handling"
            for a in (t["sum"], t["abs_sum"], t["hits"]):
                a.setflags(write=False)
            self._terms[product] = t
        return self._terms[product]


def _reference(oracle, case, n=1024):
    key = (case_id(case), n)
    if key not in _REFERENCES:
        _REFERENCES[key] = _Reference(oracle, case, n)
    return _REFERENCES[key]


def _assert_same_bits(got, want, what):
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert not np.any(differ), f"{what}: {int(np.count_nonzero(differ))} of {differ.size} values differ, first at {tuple(np.argwhere(differ)[0])}: got {got[differ][0]!r}, want {want[differ][0]!r}"


def _fp32_pass(tcnn, r, case, with_x, rows=None):
    """forward and backward through the fp32 module; (output, x.grad or None, params.grad as (float64 values, uint32 bits))"""
    n_in, cfg = case
    enc = fp32_module(tcnn, n_in, cfg, r.params)
    assert enc.loss_scale == 1.0  # (an fp32 module scales nothing: dL/dy reaches the kernels as given)
    xt = to_device(r.x[:rows]).requires_grad_(with_x)
    out = enc(xt)
    out.backward(to_device(r.dy[:rows, : enc.n_output_dims]))
    g = enc.params.grad.detach().cpu().numpy()
    return out.detach().cpu().numpy(), (xt.grad.detach().cpu().numpy() if with_x else None), (g.astype(np.float64), g.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- a. fp32 forward
@pytest.mark.parametrize("case", REFERENCE_KERNEL_CASES, ids=case_id)
def test_fp32_forward_bit_exact(tcnn, oracle, case):
    """k_grid_fwd<float, D, F> (grid.h:49-169 with T = float): the oracle's bits, through the module and through native.fwd."""
    r = _reference(oracle, case)
    want = assert_fp32_forward_bit_exact(tcnn, oracle, case, r.x, r.params)
    assert np.array_equal(want.view(np.uint32), r.out.view(np.uint32)) and np.any(want != 0)


# ---------------------------------------------------------------------------------------------------- b. fp32 dL/dx (and c for that pass)
@pytest.mark.parametrize("case", REFERENCE_KERNEL_CASES, ids=case_id)
def test_fp32_input_gradient_bit_exact(tcnn, oracle, case):
    """x.grad of an fp32 module (k_grid_fwd<float>'s dy_dx, grid.h:172-211, then k_grid_bwd_input<float>, grid.h:323-349) against
    forward_f32(want_dy_dx) -> backward_input_f32: the same bits; Nearest: zeros.  The parameter gradient of this pass is held like
    that of any other pass (c)."""
    r = _reference(oracle, case)
    out, dx, g = _fp32_pass(tcnn, r, case, with_x=True)
    _assert_same_bits(out, r.out, f"{case_id(case)} output")
    _assert_same_bits(dx, r.dL_dx, f"{case_id(case)} dL/dx")
    if r.nearest:
        assert not np.any(dx.view(np.uint32))
    else:
        assert np.any(r.dL_dx != 0)
    check_sum_per_level(r.ref, g, r.terms(oracle.PRODUCT_FP32), U32, label=f"{case_id(case)} fp32 (pass with dL/dx)")


# ---------------------------------------------------------------------------------------------------- c. dL/dparams, three atomic forms
@pytest.mark.parametrize("case", REFERENCE_KERNEL_CASES, ids=case_id)
def test_fp32_param_gradient_per_element(tcnn, oracle, case):
    """k_grid_bwd<float, float> (grid.h:254 with T = GRAD_T = float: weight * dL/dy in fp32, float atomics):
    |got - S| <= gamma(k - 1) * A at u = 2^-24 for every parameter, level by level; untouched entries +0."""
    r = _reference(oracle, case)
    _, _, g = _fp32_pass(tcnn, r, case, with_x=False)
    records = check_sum_per_level(r.ref, g, r.terms(oracle.PRODUCT_FP32), U32, label=f"{case_id(case)} fp32")
    print_records("fp32", case, records)
    assert np.any(g[0] != 0)


def _half_native_pass(tcnn, r, case, env, monkeypatch):
    """forward and backward of the half grid through the native module (no loss scale in between); (dL/dparams bits, list_scatters())"""
    n_in, cfg = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    native = tcnn.Encoding(n_in, cfg).native_tcnn_module
    for k in env:
        monkeypatch.delenv(k)
    xt, pt = to_device(r.x), to_device(r.params_h.view(np.float16)).requires_grad_(True)
    ctx, out = native.fwd(xt, pt)
    assert native.n_output_dims() == r.dy_h.shape[1]
    _, g = native.bwd(ctx, xt, pt, out, to_device(r.dy_h.view(np.float16)))
    return g.detach().cpu().numpy().view(np.uint16), native.list_scatters()


@pytest.mark.parametrize("case", SCALAR_CASES, ids=case_id)
def test_scalar_feature_half_gradient_in_rounding_interval(tcnn, oracle, monkeypatch, case):
    """n_features_per_level == 1 (grid.h:660, 850-886: k_grid_bwd<half, float> into an fp32 scratch, weight * (float)dL/dy, one cast):
    rn_half(S - e) <= got <= rn_half(S + e) as ordered half values, e = gamma(k - 1) * A at u = 2^-24."""
    r = _reference(oracle, case)
    terms = r.terms(oracle.PRODUCT_SCRATCH32)
    bits, _ = _half_native_pass(tcnn, r, case, {}, monkeypatch)
    records = check_rounded_sum_per_level(r.ref, bits, terms, label=f"{case_id(case)} scratch32")
    print_records("scratch32", case, records)
    assert np.any(bits != 0)


@pytest.mark.parametrize("case", PACKED_CASES, ids=case_id)
def test_packed_fp16_atomic_gradient_per_element(tcnn, oracle, monkeypatch, case):
    """k_grid_bwd<half, half> (grid.h:254: (half)weight * dL/dy in fp16, packed-fp16 atomics), taken under TCNN_AMD_GRID_SCATTER=atomic:
    |got - S| <= gamma(k - 1) * A + 2^-24 at u = 2^-11 (the second term: one spacing of the fp16 subnormals).  Entries with
    (k - 1) u >= 1 have no bound and are left out: at most 5 % of a level's hit entries."""
    r = _reference(oracle, case)
    terms = r.terms(oracle.PRODUCT_HALF)
    bits, lists = _half_native_pass(tcnn, r, case, {"TCNN_AMD_GRID_SCATTER": "atomic"}, monkeypatch)
    assert lists == 0
    got = (bits.view(np.float16).astype(np.float64), bits)
    records = check_sum_per_level(r.ref, got, terms, U16, slack=2.0 ** -24, max_excluded=0.05, label=f"{case_id(case)} packed fp16")
    print_records("packed16", case, records)
    print(f"parity packed16  {case_id(case):40s} excluded entries in all: {sum(rec[2] for rec in records)}")
    assert np.any(bits != 0)


# ---------------------------------------------------------------------------------------------------- a batch the module pads
def test_fp32_padded_batch(tcnn, oracle):
    """1000 rows through tcnn.Encoding: the module pads to 1024; the 24 extra rows reach neither the output, nor dL/dx, nor a gradient
    entry (hits and sums of the oracle come from the 1000 rows alone)."""
    case = PADDED_CASE
    r = _reference(oracle, case, PADDED_ROWS)
    out, dx, g = _fp32_pass(tcnn, r, case, with_x=True)
    assert out.shape[0] == PADDED_ROWS and dx.shape[0] == PADDED_ROWS
    _assert_same_bits(out, r.out, "output")
    _assert_same_bits(dx, r.dL_dx, "dL/dx")
    check_sum_per_level(r.ref, g, r.terms(oracle.PRODUCT_FP32), U32, label=f"{case_id(case)} fp32, 1000 rows")


# ---------------------------------------------------------------------------------------------------- OneBlob and Identity in fp32
ANALYTIC_CASES = [
    (2, {"otype": "OneBlob", "n_bins": 4}), (3, {"otype": "OneBlob", "n_bins": 16}), (2, {"otype": "OneBlob", "n_bins": 64}),
    (3, {"otype": "Identity", "scale": 2.0, "offset": -0.5}),
]


@pytest.mark.parametrize("n_in,cfg", ANALYTIC_CASES, ids=lambda v: v if isinstance(v, int) else f"{v['otype']}{v.get('n_bins', '')}")
def test_analytic_encodings_fp32(tcnn, oracle, n_in, cfg):
    """OneBlob / Identity with dtype=torch.float32: both precisions compute in fp32 and the half kernel rounds once at the end, so the fp32
    output rounded once to half has the half oracle's bits; dL/dx for half-representable dL/dy equals orc_*_backward_input bit for bit."""
    import torch

    n = 1024
    ref = oracle.create_encoding(n_in, cfg, alignment=0)
    x, _, _ = reference_inputs(oracle, ref, n)
    enc = tcnn.Encoding(n_in, cfg, dtype=torch.float32)
    ref.n_to_pad = enc.n_output_dims - ref.n_output_dims
    width = ref.padded_output_width
    dy_h = oracle.half_bits(oracle.Pcg32(9).uniform_strided(n * width, -2.0, 2.0).reshape(n, width))
    dy_h[::7] = 0
    want, ctx = ref.forward(x, want_dy_dx=True)
    want_dx = ref.backward(x, ctx, dy_h, want_dL_dx=True)
    xt = to_device(x).requires_grad_(True)
    out = enc(xt)
    assert out.dtype == torch.float32
    out.backward(to_device(oracle.half_to_f32(dy_h)))
    got = oracle.half_bits(out.detach().cpu().numpy())
    differ = got != want
    assert not np.any(differ), f"{int(np.count_nonzero(differ))} of {differ.size} outputs differ from the half oracle after one rounding"
    _assert_same_bits(xt.grad.detach().cpu().numpy(), want_dx, "dL/dx")
    assert np.any(want_dx != 0)
