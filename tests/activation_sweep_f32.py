"""A wide float32 range through one activation function of the fp32 networks: the inputs, the yardstick and the comparison of
tests/test_activation_sweep_f32.py.

A plain module the tests import (no fixtures, no GPU), in the setting of tests/activation_sweep.py: a CutlassMLP of 16 inputs, hidden layers
of width W and 16 outputs created with precision fp32 (k_mlp_layers.hip), every weight matrix zero except for sixteen ones, so that every
matrix product is one value times one plus zeros and every tensor is an elementwise function of x, dL/dy and the tangent v.

The yardstick restates every expression of mlp_device.h and of the epilogues of k_mlp_layers.hip in float32 numpy, one IEEE operation after
the other in the kernels' order (the file is built with -ffp-contract=off: a product and a sum are two roundings).  *, +, / and sqrtf are
correctly rounded on both sides.  A call of expf, logf, sinf, cosf or tanhf is not: it yields 2 K_f + 1 CANDIDATES, the correctly rounded
value (the float64 value rounded once) moved j float steps, j = -K_f .. K_f, and the candidates are carried through the rest of the expression.
The bar is set membership: the device's float is bit for bit one of the candidates, signs of zero included, NaN matching NaN.  Without a libm
call (None, ReLU, LeakyReLU, Squareplus) the set is one value.  K_f is a property of the platform's libm, measured against the float64 value
by tools/ubench/libm_f32.hip and tools/libm_f32_ulp.py -- never against a kernel of this project -- and recorded in profiles/libm_f32_ulp.txt.

Arrays of candidates carry them on a leading axis, [C][4096][16], the j = 0 candidate first.
"""
import functools

import numpy as np

import activation_sweep as sw
from activation_sweep import ACTIVATIONS, EXACT, FINITE, N_COLS, N_ROWS, NAN, NEG_INF, POS_INF, case_id, cases, curved, identity_weights, neuron_of, through_identity_weights  # noqa: F401

F = np.float32
K_ACT = F(10.0)

# The largest distance, in float steps, of the device's libm from the correctly rounded value: profiles/libm_f32_ulp.txt (an MI355X, ROCm's
# ocml as hipcc links it with build.py's FLAGS), over the sweep and over the arguments the expressions pass.  Above MAX_K it would be a finding.
K_EXPF = 1
K_LOGF = 2
K_SINF = 1
K_COSF = 2
K_TANHF = 1
MAX_K = 4  # the "few ulp" tests/test_fp32_network.py allows the device's libm in its factor 4

WIDTHS = (48, 144)  # k_layer_gemm<float,1,4,4,4> and <float,2,2,4,4>
CURVATURE = ("Exponential", "Sine", "Sigmoid", "Squareplus", "Softplus", "Tanh")
MAX_SHARE_OUTSIDE = {"Exponential": 0.15, "Softplus": 0.15}  # of the rows; 0.02 for the others
DENSE_BINADES = range(-12, 7)  # the dense part: 2^-12 <= |x| < 2^7


# ---------------------------------------------------------------------------------------------------- the inputs
def _with_neighbours(v):
    v = np.asarray(v, dtype=F)
    out = np.concatenate([v, np.nextafter(v, F(-np.inf)), np.nextafter(v, F(np.inf))])
    return out[np.isfinite(out) & (out > 0)]


def binade_boundaries():
    """2^e for e = -149 .. 127"""
    return np.ldexp(F(1), np.arange(-149, 128)).astype(F)


def thresholds():
    """the magnitudes at which an expression of mlp_device.h changes its behaviour: expf overflows behind 88.7228 = log(FLT_MAX) (Softplus:
    a tenth of it), gives subnormals below -87.3365 = log(2^-126) and zero below -103.972 = log(2^-150); expf_near_zero switches at 2^-6
    (Softplus' argument is -10 y); sinf / cosf reduce k pi / 2, k = 2^j for j = 0 .. 40; 65504 is where the half networks end"""
    ln = lambda v: np.log(np.float64(v))
    t = [ln(np.finfo(F).max), 126 * ln(2), 150 * ln(2), 2.0 ** -6]
    t = t + [v / 10 for v in t] + [65504.0] + [2.0 ** j * np.pi / 2 for j in range(41)]
    return np.asarray(t, dtype=np.float64).astype(F)


def fixed_magnitudes():
    """boundaries and thresholds with their two float neighbours, and the largest finite float: unique, ascending, positive"""
    return np.unique(np.concatenate([_with_neighbours(binade_boundaries()), _with_neighbours(thresholds()), [np.finfo(F).max]]).astype(F))


def dense_magnitudes(n, seed=5):
    """n floats over the binades of [2^-12, 2^7): in each binade evenly spaced mantissas with random low bits"""
    rs = np.random.RandomState(seed)
    binades = list(DENSE_BINADES)
    out = []
    for i, e in enumerate(binades):
        m = n // len(binades) + (1 if i < n % len(binades) else 0)
        start = (np.arange(m, dtype=np.int64) << 23) // m
        width = np.diff(np.append(start, 1 << 23))
        mantissa = start + (rs.random_sample(m) * width).astype(np.int64)
        out.append((((e + 127) << 23) | mantissa).astype(np.uint32).view(F))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def _sweep():
    fixed = fixed_magnitudes()
    n_dense = (N_ROWS * N_COLS - 2 * fixed.size - 2) // 2
    pos = np.unique(np.concatenate([fixed, dense_magnitudes(n_dense)]))
    values = np.concatenate([-pos[::-1], [F(-0.0), F(0.0)], pos]).astype(F)
    out = np.zeros(N_ROWS * N_COLS, dtype=F)
    out[:values.size] = values
    out.setflags(write=False)
    return out.reshape(N_ROWS, N_COLS), int(values.size)


def sweep_x():
    """[4096][16] float32, ascending, zero-padded"""
    return _sweep()[0]


def sweep_count():
    """how many elements of sweep_x() are the sweep (the rest is padding)"""
    return _sweep()[1]


def random_f32(seed):
    """[4096][16] float32: a random sign, exponents 2^-10 .. 2^3, random 23-bit mantissas"""
    rs = np.random.RandomState(seed)
    shape = (N_ROWS, N_COLS)
    sign = rs.randint(0, 2, size=shape).astype(np.uint32) << 31
    exponent = (rs.randint(-10, 4, size=shape) + 127).astype(np.uint32) << 23
    return np.ascontiguousarray(sign | exponent | rs.randint(0, 1 << 23, size=shape).astype(np.uint32)).view(F)


def dy():
    return random_f32(7)


def tangent():
    return random_f32(11)


def network_config(width, hidden, case):
    return {"otype": "CutlassMLP", "activation": case[0], "output_activation": case[1], "n_neurons": width, "n_hidden_layers": hidden}


def layer_slices(layer_sizes):
    """(offset, rows, cols) of every weight matrix from the module's (rows, cols) list: what identity_weights takes"""
    out, at = [], 0
    for rows, cols in layer_sizes:
        out.append((at, rows, cols))
        at += rows * cols
    return out


# ---------------------------------------------------------------------------------------------------- candidates
def ordered(a):
    """floats as ordered integers: neighbours differ by one, +0 and -0 are the same number"""
    i = np.ascontiguousarray(a, dtype=F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def moved(a, j):
    """a moved j float steps (beyond the largest finite float: infinity); what is not finite stays"""
    if j == 0:
        return a
    t = np.clip(ordered(a) + j, -0x7F800000, 0x7F800000)
    bits = np.where(t < 0, (-t) | 0x80000000, t).astype(np.uint32)
    return np.where(np.isfinite(a), bits.view(F), a)


def candidates(fn, k, x):
    """A libm call on candidates x [C][..]: [(2 k + 1) C][..], the float64 value rounded once moved 0, -1, +1, .. -k, +k float steps"""
    r = sw._rounded(fn)(x)
    out = [r] + [moved(r, s * j) for j in range(1, k + 1) for s in (-1, 1)]
    return np.concatenate(out, axis=0)


class Libm:
    """the five functions with the allowance k_f of each (scale 0: the j = 0 candidate alone)"""

    def __init__(self, scale=1, ks=None):
        ks = ks or {"expf": K_EXPF, "logf": K_LOGF, "sinf": K_SINF, "cosf": K_COSF, "tanhf": K_TANHF}
        self.k = {name: k * scale for name, k in ks.items()}

    def expf(self, x):
        return candidates(np.exp, self.k["expf"], x)

    def logf(self, x):
        return candidates(np.log, self.k["logf"], x)

    def sinf(self, x):
        return candidates(np.sin, self.k["sinf"], x)

    def cosf(self, x):
        return candidates(np.cos, self.k["cosf"], x)

    def tanhf(self, x):
        return candidates(np.tanh, self.k["tanhf"], x)

    def spread(self, name, a):
        """a [C][..] repeated to line up with the candidates of a call of `name` on C candidates"""
        return np.concatenate([a] * (2 * self.k[name] + 1), axis=0)


ONE_CANDIDATE = Libm(0)


def _quiet(fn):
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
            return fn(*args, **kwargs)
    return wrapped


# ---------------------------------------------------------------------------------------------------- mlp_device.h, restated
@_quiet
def expf_near_zero(m, x):
    small = np.abs(x) < F(2.0 ** -6)
    lo = x * x * (F(0.5) + x * (F(1) / F(6) + x * (F(1) / F(24) + x * (F(1) / F(120)))))
    s = F(1) + x
    e = x - (s - F(1))
    poly = s + (e + lo)
    return np.where(m.spread("expf", small), m.spread("expf", poly), m.expf(x))


@_quiet
def logistic(m, x):
    return F(1) / (F(1) + m.expf(-x))


@_quiet
def activation_fwd(m, act, z):
    if act == "None":
        return z
    if act == "ReLU":
        return np.where(z > 0, z, F(0))
    if act == "LeakyReLU":
        return z * np.where(z > 0, F(1), F(0.01))
    if act == "Exponential":
        return m.expf(z)
    if act == "Sine":
        return m.sinf(z)
    if act == "Sigmoid":
        return logistic(m, z)
    if act == "Squareplus":
        y = z * K_ACT
        return F(0.5) * (y + np.sqrt(y * y + F(4))) / K_ACT
    if act == "Softplus":
        return m.logf(m.expf(z * K_ACT) + F(1)) / K_ACT
    if act == "Tanh":
        return m.tanhf(z)
    raise ValueError(act)


@_quiet
def activation_bwd(m, act, grad, y):
    """the derivative from the forward OUTPUT y; Sine, which has none, passes the gradient on like None"""
    if act in ("None", "Sine"):
        return grad
    if act == "ReLU":
        return np.where(y > 0, grad, grad * F(0))
    if act == "LeakyReLU":
        return grad * np.where(y > 0, F(1), F(0.01))
    if act == "Exponential":
        return grad * y
    if act == "Sigmoid":
        return grad * (y * (F(1) - y))
    if act == "Squareplus":
        t = y * K_ACT
        return grad * (t * t / (t * t + F(1)))
    if act == "Softplus":
        return grad * (F(1) - expf_near_zero(m, -y * K_ACT))
    if act == "Tanh":
        return grad * (F(1) - y * y)
    raise ValueError(act)


@_quiet
def sine_bwd(m, grad, z):
    """a Sine hidden layer: from the stored pre-activation (the LG_BWD epilogue of k_layer_gemm<float>)"""
    return grad * m.cosf(z)


@_quiet
def act_d1(m, act, x):
    """a'(x); x: the pre-activation, for ReLU / LeakyReLU the output (the same sign)"""
    if act == "None":
        return np.ones_like(x[:1])  # (takes no argument at all)
    if act == "ReLU":
        return np.where(x > 0, F(1), F(0))
    if act == "LeakyReLU":
        return np.where(x > 0, F(1), F(0.01))
    if act == "Exponential":
        return m.expf(x)
    if act == "Sine":
        return m.cosf(x)
    if act == "Sigmoid":
        s = F(1) / (F(1) + expf_near_zero(m, -x))
        return s * (F(1) - s)
    if act == "Squareplus":
        y = x * K_ACT
        return F(0.5) * (F(1) + y / np.sqrt(y * y + F(4)))
    if act == "Softplus":
        return logistic(m, x * K_ACT)
    if act == "Tanh":
        t = m.tanhf(x)
        return F(1) - t * t
    raise ValueError(act)


@_quiet
def act_d2(m, act, x):
    if act in ("None", "ReLU", "LeakyReLU"):
        return np.zeros_like(x)
    if act == "Exponential":
        return m.expf(x)
    if act == "Sine":
        return -m.sinf(x)
    if act == "Sigmoid":
        s = F(1) / (F(1) + expf_near_zero(m, -x))
        return s * (F(1) - s) * (F(1) - F(2) * s)
    if act == "Squareplus":
        y = x * K_ACT
        q = y * y + F(4)
        return F(2) * K_ACT / (q * np.sqrt(q))
    if act == "Softplus":
        s = logistic(m, x * K_ACT)
        return K_ACT * s * (F(1) - s)
    if act == "Tanh":
        t = m.tanhf(x)
        return F(-2) * t * (F(1) - t * t)
    raise ValueError(act)


# ---------------------------------------------------------------------------------------------------- the passes of Network, restated
_POISON = [True]  # False: the elementwise function alone, as if no other element of a row reached a product (restatement(elementwise=True))


@_quiet
def product(a):
    """A layer product with the setting's weights on candidates [C][4096][16]: one accumulator from +0, fmaf(a, 1, acc) for the element's own
    value and fmaf(b, 0, acc) for every other one of the row -- the value itself with -0 turned into +0, and NaN wherever another element
    of the row is not finite (through_identity_weights; decided on the j = 0 candidate)"""
    a = a + F(0)
    if not _POISON[-1]:
        return a
    poisoned = np.isnan(through_identity_weights(a[0])) & ~np.isnan(a[0])
    return np.where(poisoned[None], F(np.nan), a)


def _acts(case, hidden):
    return [case[0]] * hidden + [case[1]]


@_quiet
def forward(m, case, x, hidden=1):
    """Network::forward_layers: (output, pre-activations z_l, activations h_l) as candidates"""
    h, zs, hs = x[None], [], []
    for act in _acts(case, hidden):
        zs.append(product(h))
        h = activation_fwd(m, act, zs[-1])
        hs.append(h)
    return h, zs, hs


@_quiet
def backward(m, case, x, g, hidden=1, own_output=None):
    """Network::backward's dL/dinput.  own_output: the device's forward output, which then stands for the activations the derivative is taken
    from -- the output layer's (k_act_bwd_output<float>) or, with an output activation of None behind one hidden layer, the hidden layer's: the
    output is their product with the identity, the same values wherever its row is finite; on its other rows the hidden activations cannot
    be seen, and the restatement's candidates stand for them"""
    acts = _acts(case, hidden)
    _, zs, hs = forward(m, case, x, hidden)
    if own_output is not None:
        assert hidden == 1
        if case[1] == "None":
            hs[0] = np.where(finite_rows(own_output)[None, :, None], own_output[None], hs[0])
        else:
            hs[1] = own_output[None]
    d = activation_bwd(m, acts[-1], g[None], hs[-1])
    for l in range(len(acts) - 1, 0, -1):
        acc = product(d)
        d = sine_bwd(m, acc, zs[l - 1]) if acts[l - 1] == "Sine" else activation_bwd(m, acts[l - 1], acc, hs[l - 1])
    return product(d)


@_quiet
def delta(m, act, g, aux):
    """k_layer_delta<float>"""
    return act_d1(m, act, aux) * g


@_quiet
def second_order(m, case, x, g, v, hidden=1):
    """Network::second_order_begin / _finish: (dL/d(dL/doutput), dL/dinput) as candidates, the products of second_order_epilogue_f32 in its
    order: (d2 * g) * acc, d1 * acc and c + d1 * acc"""
    acts = _acts(case, hidden)
    K = len(acts)
    _, zs, hs = forward(m, case, x, hidden)
    aux = [zs[l] if acts[l] in CURVATURE else hs[l] for l in range(K)]
    gs = [None] * K
    gs[K - 1] = g[None]
    d = g[None] if acts[K - 1] == "None" else delta(m, acts[K - 1], g[None], aux[K - 1])
    for l in range(K - 1, 0, -1):  # LG_BWD_KEEP
        acc = product(d)
        gs[l - 1] = acc
        d = act_d1(m, acts[l - 1], aux[l - 1]) * acc
    u, r = v[None], [None] * K
    for l in range(K):  # LG_TANGENT
        acc = product(u)
        if acts[l] in CURVATURE:
            r[l] = act_d2(m, acts[l], aux[l]) * gs[l] * acc
        u = act_d1(m, acts[l], aux[l]) * acc
    top = [l for l in range(K) if acts[l] in CURVATURE]
    if not top:
        return u, np.zeros_like(x)[None]  # nothing is launched: the result stays +0
    p = r[top[-1]]
    for l in range(top[-1], 0, -1):  # LG_CURVATURE
        acc = product(p)
        c = r[l - 1] if acts[l - 1] in CURVATURE else F(0)
        p = c + act_d1(m, acts[l - 1], aux[l - 1]) * acc
    return u, product(p)


@functools.lru_cache(maxsize=None)
def _restatement(case, hidden, scale, elementwise):
    m = Libm(scale)
    x, g, v = sweep_x(), dy(), tangent()
    _POISON.append(not elementwise)
    try:
        out, _, _ = forward(m, case, x, hidden)
        ddy, dx2 = second_order(m, case, x, g, v, hidden)
        r = {"out": out, "dx": backward(ONE_CANDIDATE, case, x, g, hidden), "ddy": ddy, "dx2": dx2}
    finally:
        _POISON.pop()
    for a in r.values():
        a.setflags(write=False)
    return r


def restatement(case, hidden=1, scale=1, elementwise=False):
    """{"out", "ddy", "dx2"}: candidates of the forward output and the two second-order results; "dx": the first-order dL/dinput from the
    restatement's own j = 0 forward (the rows and classes of the backward comparison; its candidates come from the device's output).
    scale 0: the j = 0 candidate alone.  elementwise: without the NaN that a product spreads over a row.  Computed once per case: the width
    does not enter."""
    return _restatement(tuple(case), hidden, scale, elementwise)


# ---------------------------------------------------------------------------------------------------- classes and the comparison
def classes(a):
    """FINITE, POS_INF, NEG_INF or NAN of every float"""
    a = np.asarray(a, dtype=F)
    out = np.full(a.shape, FINITE, dtype=np.uint8)
    out[a == np.inf] = POS_INF
    out[a == -np.inf] = NEG_INF
    out[np.isnan(a)] = NAN
    return out


def finite_rows(a):
    return np.all(np.isfinite(a), axis=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def member(got, cands):
    """boolean [C][..]: got is bit for bit the candidate (NaN matches NaN)"""
    return (bits(got)[None] == bits(cands)) | (np.isnan(got)[None] & np.isnan(cands))


def compare(got, cands, reference, what=""):
    """got [4096][16] against the candidates [C][4096][16] on the rows that are finite in `reference` (the restatement's j = 0 result): bit
    for bit one of them.  On the other rows the class of every element is the reference's.
    Returns (elements compared, share equal to the j = 0 candidate, rows judged by class) -- printed before anything is asserted."""
    got = np.asarray(got, dtype=F)
    assert got.shape == reference.shape == (N_ROWS, N_COLS) and cands.shape[1:] == got.shape
    rows = finite_rows(reference)
    hit = member(got[rows], cands[:, rows])
    ok = hit.any(axis=0)
    stats = (int(ok.size), float(np.mean(hit[0])) if ok.size else 1.0, int(np.count_nonzero(~rows)))
    print(f"sweep_f32 {what}: compared {stats[0]} at_j0 {stats[1]:.6f} by_class {stats[2]} candidates {cands.shape[0]} outside_the_set {int(np.count_nonzero(~ok))}")
    assert np.array_equal(classes(got[~rows]), classes(reference[~rows])), f"{what}: classes differ on the rows outside the bit comparison"
    if not ok.all():
        r, c = np.argwhere(~ok)[0]
        row = int(np.flatnonzero(rows)[r])
        near = ", ".join(f"0x{int(b):08x}" for b in bits(cands[:, row, c])[:5])
        raise AssertionError(f"{what}: {int(np.count_nonzero(~ok))} of {ok.size} floats are none of their {cands.shape[0]} candidates; first: row {row}, column {c}, "
                             f"x = {float(sweep_x()[row, c])!r}: got 0x{int(bits(got)[row, c]):08x} ({float(got[row, c])!r}), candidates {near}")
    return stats
