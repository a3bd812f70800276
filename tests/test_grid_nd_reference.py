"""Pins tests/grid_nd_reference.py -- the numpy restatement of the reference's grid encoding for 1 to 7 input dimensions, the yardstick of
the 1-, 5-, 6- and 7-dimensional kernels -- to the CPU oracle where both exist: 2, 3 and 4 dimensions, on the cases of
tests/grid_reference.py.  Bit for bit: the level table, the forward pass in half and in float, dy/dx, dL/dx and the exact sum of the
gradient's fp16 products.  The terms of the atomic routes' bounds agree to the last bits of a double sum.  No GPU."""
import numpy as np
import pytest

from grid_nd_reference import DIMS_MESSAGE, PRODUCT_FP32, PRODUCT_HALF, PRODUCT_SCRATCH32, GridND, fma, ordered_sum, random_val
from grid_reference import REFERENCE_KERNEL_CASES, case_id, reference_inputs

N = 512  # 256 uniform rows and the 256 edge rows


@pytest.fixture(scope="module", params=REFERENCE_KERNEL_CASES, ids=case_id)
def pair(request, oracle):
    n_in, cfg = request.param
    ref = oracle.create_encoding(n_in, cfg, alignment=0)
    nd = GridND(n_in, cfg)
    x, params, dy = reference_inputs(oracle, ref, N)
    return oracle, ref, nd, x, params, dy


def test_level_table(pair):
    _, ref, nd, _, _, _ = pair
    assert nd.n_params == ref.n_params and nd.n_output_dims == ref.n_output_dims
    assert np.array_equal(nd.offsets, ref.offsets)
    assert np.array_equal(np.array(nd.scales, dtype=np.float32).view(np.uint32), ref.scales.view(np.uint32))
    assert np.array_equal(np.array(nd.resolutions, dtype=np.uint32), ref.resolutions)


def test_forward_half_and_input_gradients(pair):
    oracle, ref, nd, x, params, dy = pair
    ph, dyh = oracle.half_bits(params), oracle.half_bits(dy)
    want, ctx = ref.forward(x, ph, want_dy_dx=True)
    got, dy_dx = nd.forward(x, ph.view(np.float16), want_dy_dx=True)
    assert np.array_equal(got.view(np.uint16), want)
    assert np.array_equal(dy_dx.view(np.uint32), ctx["dy_dx"].view(np.uint32))
    want_dx = ref.backward(x, ctx, dyh, want_dL_dx=True)
    assert np.array_equal(nd.backward_input(dy_dx, dyh.view(np.float16)).view(np.uint32), want_dx.view(np.uint32))


def test_forward_float_and_input_gradients(pair):
    _, ref, nd, x, params, dy = pair
    want, ctx = ref.forward_f32(x, params, want_dy_dx=True)
    got, dy_dx = nd.forward(x, params, want_dy_dx=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dy_dx.view(np.uint32), ctx["dy_dx"].view(np.uint32))
    assert np.array_equal(nd.backward_input(dy_dx, dy).view(np.uint32), ref.backward_input_f32(ctx, dy).view(np.uint32))


def test_gradient_exact_sum_and_terms(pair):
    oracle, ref, nd, x, _, dy = pair
    dyh = oracle.half_bits(dy)
    want = ref.backward_exact(x, dyh, np.zeros(ref.n_params, dtype=np.uint16))
    assert np.array_equal(nd.backward_exact(x, dyh.view(np.float16)), want)
    for product, grads in ((PRODUCT_HALF, dyh.view(np.float16)), (PRODUCT_SCRATCH32, dyh.view(np.float16)), (PRODUCT_FP32, dy)):
        assert product == {PRODUCT_HALF: oracle.PRODUCT_HALF, PRODUCT_SCRATCH32: oracle.PRODUCT_SCRATCH32, PRODUCT_FP32: oracle.PRODUCT_FP32}[product]
        a = nd.backward_terms(x, grads, product)
        b = ref.backward_terms(x, grads if product == PRODUCT_FP32 else dyh, product)
        assert np.array_equal(a["hits"], b["hits"]) and a["min_nonzero"] == b["min_nonzero"]
        assert np.allclose(a["sum"], b["sum"], rtol=0, atol=1e-12 * max(1.0, float(np.max(b["abs_sum"]))))
        assert np.allclose(a["abs_sum"], b["abs_sum"], rtol=1e-12, atol=0)


def test_random_val_is_the_oracles(oracle):
    idx = np.array([0, 1, 2, 1000, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    for i, got in zip(idx, random_val(idx)):
        rng = oracle.Pcg32(1337)
        rng.advance(int(i))
        assert np.float32(rng.next_float()) == got


def test_dimension_limits_and_helpers():
    for n_in in (0, 8):
        with pytest.raises(RuntimeError, match=DIMS_MESSAGE.replace(".", r"\.")):
            GridND(n_in, {"otype": "HashGrid"})
    for n_in in range(1, 8):
        assert GridND(n_in, {"otype": "HashGrid", "n_levels": 4, "log2_hashmap_size": 10, "base_resolution": 2}).n_in == n_in
    # a fused multiply-add whose float64 sum is inexact and lands on a float32 tie: one rounding, not two.  (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24
    # lies midway between two floats; the addend 2^-80, lost in float64, decides the direction
    a = np.array([1 + 2.0 ** -12], dtype=np.float32)
    assert fma(a, a, np.array([2.0 ** -80], dtype=np.float32), np.float32)[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert fma(a, a, np.array([-(2.0 ** -80)], dtype=np.float32), np.float32)[0] == np.float32(1 + 2.0 ** -11)
    assert ordered_sum(np.array([1, 0, 1]), np.array([1.0, 2.0, 2.0 ** -12]), 2, np.float16).tolist() == [2.0, 1.0]
