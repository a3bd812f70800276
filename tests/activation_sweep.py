"""Every finite fp16 value through one activation function: the inputs, weights, yardsticks and comparison of tests/test_activation_sweep.py.

A plain module the tests import (no fixtures, no GPU).  The setting: an Identity encoding of 16 inputs, hidden layers of width W, 16 outputs.
Every weight matrix is zero except for sixteen ones: input column c feeds hidden neuron neuron_of(c, W), which feeds output c, so every matrix
product is one value times one plus zeros and the network's output is the activation of its input, element by element.  x holds the 63 488
finite halves once, ascending, zero-padded to 4096 x 16.  Two families of cases: (activation A, output activation None) and (activation
None, output activation B).
"""
import functools
from itertools import repeat

import numpy as np

N_ROWS, N_COLS = 4096, 16
FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
ACTIVATIONS = ["None", "ReLU", "LeakyReLU", "Exponential", "Sine", "Sigmoid", "Squareplus", "Softplus", "Tanh"]
EXACT = ("None", "ReLU", "LeakyReLU", "Squareplus")  # *, +, sqrtf and / only: correctly rounded on both sides
# at most this share of the rows may leave the bit comparison (an expf that overflows a half makes its whole row NaN in the product)
MAX_SHARE_OUTSIDE = {"Exponential": 0.21, "Softplus": 0.21}
MIN_SHARE_IDENTICAL = 0.999  # of the halves where device and host libm may differ in the last float bit; every other one an adjacent half


def cases(hidden_activations=ACTIVATIONS, output_activations=ACTIVATIONS):
    """(activation, output activation) of both families, None / None once"""
    return [(a, "None") for a in hidden_activations] + [("None", b) for b in output_activations if b != "None"]


def case_id(case):
    return f"{case[0].lower()}-{case[1].lower()}"


def curved(case):
    """the activation of the case that is not None (None for None / None)"""
    return case[0] if case[0] != "None" else case[1]


def sweep_bits():
    """[4096][16] uint16: every finite half once in ascending order (-65504 .. -0, +0 .. 65504), then +0"""
    neg = np.arange(0xFBFF, 0x7FFF, -1, dtype=np.int64)
    pos = np.arange(0x0000, 0x7C00, dtype=np.int64)
    out = np.zeros(N_ROWS * N_COLS, dtype=np.uint16)
    out[:neg.size + pos.size] = np.concatenate([neg, pos])
    return out.reshape(N_ROWS, N_COLS)


def sweep_x():
    """the sweep as float32, which the Identity encoding casts back to half exactly"""
    return np.ascontiguousarray(sweep_bits().view(np.float16).astype(np.float32))


def dy_bits(seed=7, n_out=N_COLS):
    """[4096][16] uint16: dL/dy, signed halves with exponents 2^-10 .. 2^3 and random mantissas (2^-10 <= |dL/dy| < 2^4), zero beyond n_out"""
    rs = np.random.RandomState(seed)
    sign = rs.randint(0, 2, size=(N_ROWS, N_COLS)).astype(np.uint16) << 15
    exponent = (rs.randint(-10, 4, size=(N_ROWS, N_COLS)) + 15).astype(np.uint16) << 10
    out = sign | exponent | rs.randint(0, 1024, size=(N_ROWS, N_COLS)).astype(np.uint16)
    out[:, n_out:] = 0
    return np.ascontiguousarray(out)


def neuron_of(c, width):
    """the hidden neuron input column c feeds: one in every 16-wide tile of layers up to 256 wide, spread evenly beyond"""
    return c * width // N_COLS


def identity_weights(slices, width):
    """float32 parameters in the layout of grad_checks.layer_slices: ones at (neuron_of(c), c) of the first matrix, (neuron_of(c), neuron_of(c))
    of the hidden ones and (c, neuron_of(c)) of the last, zero elsewhere"""
    w = np.zeros(sum(r * c for _, r, c in slices), dtype=np.float32)
    last = len(slices) - 1
    for l, (off, rows, cols) in enumerate(slices):
        m = w[off:off + rows * cols].reshape(rows, cols)
        for c in range(N_COLS):
            m[c if l == last else neuron_of(c, width), c if l == 0 else neuron_of(c, width)] = 1.0
    return w


def network_config(width, hidden, case):
    otype = "FullyFusedMLP" if width in (16, 32, 64, 128) and case[0] != "Sine" else "CutlassMLP"
    return {"otype": otype, "activation": case[0], "output_activation": case[1], "n_neurons": width, "n_hidden_layers": hidden}


def trainer_config(width, hidden, case):
    return {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6},
            "encoding": {"otype": "Identity"}, "network": network_config(width, hidden, case)}


# ---------------------------------------------------------------------------------------------------- the yardsticks
def elementwise_forward(oracle, activation, bits):
    """orc_activation on every element of a uint16 array"""
    fn, act = oracle.lib().orc_activation, oracle.ACT[activation.lower()]
    flat = np.ascontiguousarray(bits, dtype=np.uint16).ravel().tolist()
    return np.fromiter(map(fn, repeat(act), flat), dtype=np.uint16, count=len(flat)).reshape(np.shape(bits))


def elementwise_backward(oracle, activation, grad_bits, forward_bits):
    """orc_activation_backward(dL/dy, forward output) on every element: the derivative from the forward output (Sine: the gradient itself)"""
    fn, act = oracle.lib().orc_activation_backward, oracle.ACT[activation.lower()]
    g = np.ascontiguousarray(grad_bits, dtype=np.uint16).ravel().tolist()
    f = np.ascontiguousarray(forward_bits, dtype=np.uint16).ravel().tolist()
    return np.fromiter(map(fn, repeat(act), g, f), dtype=np.uint16, count=len(g)).reshape(np.shape(grad_bits))


def sine_backward_from_preactivation(grad_bits, z_bits):
    """hmul(dL/dy, half(cosf(z))) in float32 numpy: what the layer-by-layer path computes for a Sine layer from the stored pre-activation
    (the oracle differentiates from outputs and has none)"""
    z = np.asarray(z_bits, dtype=np.uint16).view(np.float16).astype(np.float32)
    c = np.cos(z).astype(np.float16).astype(np.float32)
    g = np.asarray(grad_bits, dtype=np.uint16).view(np.float16).astype(np.float32)
    return (g * c).astype(np.float16).view(np.uint16)  # the float product of two halves is exact: one rounding, as __hmul


def oracle_step(oracle, width, hidden, case):
    """one oracle training step of the setting: {"out", "dx"} as uint16 [4096][16]; dx is dL/dinput (the oracle's float32 holds halves)"""
    ref = oracle.Trainer(N_COLS, N_COLS, trainer_config(width, hidden, case), seed=1337)
    net = ref.model.network
    assert net.padded_output_width == N_COLS and ref.model.encoding.n_params == 0
    from grad_checks import layer_slices

    ref.params = oracle.half_bits(identity_weights(layer_slices(net), width))
    res = ref.training_step(sweep_x(), None, run_optimizer=False, want_dL_dx=True, external_dL_dy=dy_bits())
    return {"out": res["output"].copy(), "dx": float_to_half_bits(res["dL_dinput"])}


@functools.lru_cache(maxsize=None)
def _reference(oracle, hidden, case):
    return oracle_step(oracle, N_COLS, hidden, case)


def reference(oracle, hidden, case):
    """The oracle network's step at width 16, computed once per case: the zeros of a wider layer add nothing to any sum, and an infinite
    neuron meets as many zero weights, so the result is the same at every width (tests/test_activation_sweep.py asserts it on the CPU)."""
    return _reference(oracle, hidden, tuple(case))


# ---------------------------------------------------------------------------------------------------- second order
K_ACT = np.float32(10.0)


def _rounded(fn):
    """a float32 libm function as its float64 value rounded once: the same on every host"""
    def f(x):
        with np.errstate(over="ignore", invalid="ignore"):
            return fn(x.astype(np.float64)).astype(np.float32)
    return f


_exp, _sin, _cos, _tanh = _rounded(np.exp), _rounded(np.sin), _rounded(np.cos), _rounded(np.tanh)


def _logistic(x):
    return np.float32(1) / (np.float32(1) + _exp(-x))


def act_d1_d2(activation, x):
    """a'(z) and a''(z) as act_d1 / act_d2 of mlp_device.h write them: float32, one IEEE operation after the other in the kernels' order"""
    one, two = np.float32(1), np.float32(2)
    if activation == "Exponential":
        return _exp(x), _exp(x)
    if activation == "Sine":
        return _cos(x), -_sin(x)
    if activation == "Sigmoid":
        s = _logistic(x)
        return s * (one - s), s * (one - s) * (one - two * s)
    if activation == "Squareplus":
        y = x * K_ACT
        q = y * y + np.float32(4)
        return np.float32(0.5) * (one + y / np.sqrt(q)), two * K_ACT / (q * np.sqrt(q))
    if activation == "Softplus":
        s = _logistic(x * K_ACT)
        return s, K_ACT * s * (one - s)
    if activation == "Tanh":
        t = _tanh(x)
        return one - t * t, -two * t * (one - t * t)
    raise ValueError(activation)


def through_identity_weights(a):
    """what a product with the setting's weights makes of [4096][16] float32 values: itself, and NaN wherever another element of the row is not
    finite (0 * inf)"""
    bad = ~np.isfinite(a)
    others = bad.sum(axis=1, keepdims=True) - bad > 0
    return np.where(others, np.float32(np.nan), a)


def second_order_restatement(activation, x_bits, dy_bits_, v_bits):
    """The recipe of Network::second_order_* (test_network_second_order._restate(half=True)) for one hidden layer in this setting, in float32 numpy:
    dL/d(dL/doutput) = half(a'(z) v) and dL/dinput = half(a''(z) g v), the float products in the order of second_order_epilogue
    (k_mlp_layers.hip), uint16 [4096][16] each.  torch's float32 functions, which _restate calls, are vectorised differently from host to host:
    on one of two hosts its Squareplus a' -- *, +, / and sqrt only -- matched the IEEE evaluation on 99.3 % of the sweep's halves."""
    f = lambda b: np.asarray(b, dtype=np.uint16).view(np.float16).astype(np.float32)
    z, g, v = f(x_bits), f(dy_bits_), f(v_bits)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d1, d2 = act_d1_d2(activation, z)
        h = lambda a: a.astype(np.float16).astype(np.float32)
        u = through_identity_weights(h(d1 * v))      # the output layer has no activation: u_2 = W_2 u_1
        r = through_identity_weights(h(d2 * g * v))  # p_0 = r_0, dS/dinput = p_0 W_0
    return float_to_half_bits(u), float_to_half_bits(r)


# ---------------------------------------------------------------------------------------------------- classes and the comparison
def float_to_half_bits(a):
    """float32 values that are halves -> their uint16 bits (asserted: nothing is rounded; NaN stays NaN)"""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
    back = h.astype(np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(back)) and np.array_equal(a[~np.isnan(a)], back[~np.isnan(a)]), "not half values"
    return np.ascontiguousarray(h).view(np.uint16)


def classes(bits):
    """FINITE, POS_INF, NEG_INF or NAN of every half"""
    bits = np.asarray(bits, dtype=np.uint16)
    mag = bits & 0x7FFF
    out = np.full(bits.shape, FINITE, dtype=np.uint8)
    out[bits == 0x7C00] = POS_INF
    out[bits == 0xFC00] = NEG_INF
    out[mag > 0x7C00] = NAN
    return out


def finite_rows(*bit_arrays):
    """boolean [rows]: every element of the row is finite in every array"""
    ok = np.ones(np.shape(bit_arrays[0])[0], dtype=bool)
    for b in bit_arrays:
        ok &= np.all(classes(b) == FINITE, axis=1)
    return ok


def ordered(bits):
    """sign-magnitude halves as ordered integers: neighbours differ by one, +0 and -0 are the same number"""
    h = np.asarray(bits, dtype=np.uint16).astype(np.int32)
    return np.where(h & 0x8000, -(h & 0x7FFF), h & 0x7FFF)


def compare(got, want, rows, want_outside, exact, what=""):
    """got against want (uint16 [4096][16]) on the rows of the boolean mask `rows`, +0 and -0 equal: bit-identical where `exact`, else at least
    99.9 % identical and the others adjacent halves; on the other rows the class of every element of got is that of `want_outside`.
    Returns (elements compared, share identical, largest distance in half steps) -- measured before anything is asserted."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    assert got.shape == want.shape == (N_ROWS, N_COLS) and rows.shape == (N_ROWS,)
    g, w = got[rows], want[rows]
    steps = np.abs(ordered(g) - ordered(w))
    steps[classes(g) != classes(w)] = 1 << 16  # an infinity or NaN on one side only
    steps[(classes(g) == NAN) & (classes(w) == NAN)] = 0
    share, worst = float(np.mean(steps == 0)), int(steps.max())
    stats = (int(steps.size), share, worst)
    print(f"{what}: {steps.size} elements, {share:.6f} identical, at most {worst} half steps apart, {int(np.count_nonzero(~rows))} rows by class")
    outside = ~rows
    assert np.array_equal(classes(got[outside]), classes(want_outside[outside])), f"{what}: classes differ on the rows outside the finite comparison"
    if worst > 0:
        r, c = np.unravel_index(int(np.argmax(steps)), steps.shape)
        first = f"row {int(np.flatnonzero(rows)[r])}, column {c}: got 0x{int(g[r, c]):04x}, want 0x{int(w[r, c]):04x}"
    if exact:
        assert worst == 0, f"{what}: {int(np.count_nonzero(steps))} of {steps.size} halves differ, by up to {worst} steps; worst: {first}"
    else:
        assert share >= MIN_SHARE_IDENTICAL, f"{what}: only {share:.6f} of {steps.size} halves identical; worst: {first}"
        assert worst <= 1, f"{what}: {worst} half steps apart; {first}"
    return stats
