"""The Adam kernels' exact fast square root and division (adam_device.h) against sqrtf and `/`, on the device, input by input.

The kernels take learning_rate / (sqrtf(second_moment) + epsilon) through a hardware approximation with fused residual corrections wherever a
range test on the operands holds, and through the plain expressions elsewhere.  tcnn_adam_math_sweep runs those very functions -- range test
included -- beside the plain expressions, compares the bits in the kernel and reports how many inputs differ and the smallest of them.
Expected: none.  Nothing is stored per element; each sweep is one launch."""
import ctypes as C
import time

import numpy as np
import pytest

SWEEP_SQRT, SWEEP_DIV_GRID, SWEEP_DIV_PAIRS = 0, 1, 2


def _sweep(tcnn, what, first=0, count=0, n_numerators=0, lo=0.0, hi=0.0, seed=0):
    import torch

    from tinycudann import _C

    torch.cuda.init()
    bad, first_bad = C.c_uint64(), C.c_uint64()
    t0 = time.perf_counter()
    _C.check(_C.lib.tcnn_adam_math_sweep(None, what, first, count, n_numerators, lo, hi, seed, C.byref(bad), C.byref(first_bad)))
    print(f"SWEEP what={what} first={first:#x} count={count:#x}: {bad.value} mismatches, first {first_bad.value:#x}, {time.perf_counter() - t0:.3f} s")
    return bad.value, first_bad.value


def _describe(first_bad, pair):
    if not pair:
        return f"x = {np.uint32(first_bad).view(np.float32)!r} ({first_bad:#010x})"
    d, n = np.uint32(first_bad >> 32).view(np.float32), np.uint32(first_bad & 0xFFFFFFFF).view(np.float32)
    return f"n = {n!r} ({first_bad & 0xFFFFFFFF:#010x}), d = {d!r} ({first_bad >> 32:#010x})"


@pytest.mark.gpu
def test_fast_square_root_on_every_positive_finite_float(tcnn):
    """every pattern from the smallest denormal to the largest finite float: 2^31 - 2^23 - 1 inputs"""
    bad, first_bad = _sweep(tcnn, SWEEP_SQRT, first=1, count=0x7F800000 - 1)
    assert bad == 0, f"{bad} square roots differ from sqrtf, first at {_describe(first_bad, False)}"


@pytest.mark.gpu
def test_fast_division_on_every_denominator(tcnn):
    """All 2^32 denominator patterns -- zeros, denormals, negatives, infinities and NaN take the plain expression, as in the kernels -- against
    1000 numerators across learning_rate * debias: learning rates of 1e-6 .. 1 times debias factors of 0.3 .. 3.2 lie within 2^-22 .. 2^2."""
    bad, first_bad = _sweep(tcnn, SWEEP_DIV_GRID, first=0, count=1 << 32, n_numerators=1000, lo=2.0 ** -22, hi=4.0, seed=20240917)
    assert bad == 0, f"{bad} quotients differ from n / d, first at {_describe(first_bad, True)}"


@pytest.mark.gpu
def test_fast_division_on_seeded_pairs(tcnn):
    """2^26 pairs drawn around both range tests' edges (numerators of 2^-70 .. 2^70 against the test's 2^-64 .. 2^64, denominators of
    2^-54 .. 2^24 against 2^-48 .. 2^18), a quarter of each operand negative"""
    bad, first_bad = _sweep(tcnn, SWEEP_DIV_PAIRS, count=1 << 26, seed=7)
    assert bad == 0, f"{bad} quotients differ from n / d, first at {_describe(first_bad, True)}"


@pytest.mark.gpu
def test_the_sweep_rejects_what_it_cannot_run(tcnn):
    from tinycudann import _C

    bad, first_bad = C.c_uint64(), C.c_uint64()
    assert _C.lib.tcnn_adam_math_sweep(None, 3, 0, 1, 0, 0.0, 0.0, 0, C.byref(bad), C.byref(first_bad)) != 0
    assert _C.lib.tcnn_adam_math_sweep(None, SWEEP_SQRT, 1 << 31, (1 << 31) + 1, 0, 0.0, 0.0, 0, C.byref(bad), C.byref(first_bad)) != 0
    assert _C.lib.tcnn_adam_math_sweep(None, SWEEP_DIV_GRID, 0, 16, 0, 1.0, 2.0, 0, C.byref(bad), C.byref(first_bad)) != 0
    assert _sweep(tcnn, SWEEP_SQRT, first=0x3F800000, count=0) == (0, 2 ** 64 - 1)
