"""Full-precision (fp32) networks: tcnn_create_network_precision / tcnn_create_network_with_input_encoding_precision and
tcnn.Network / tcnn.NetworkWithInputEncoding(dtype=torch.float32) -- Network{json, Precision::Fp32} on the fp32 instantiation of
the layer kernels (tiny-cuda-nn_amd/csrc/k_mlp_layers.hip, LayerElem<float>) and the fp32 weight gradients (k_mlp_layers_f32.hip).

Three yardsticks, none of them the kernels themselves:
  * activations None and ReLU: tests/cpp/mlp_f32_reference.cpp, the kernels' contract restated with std::fmaf (one accumulator per
    element from +0, products in ascending k).  Output, dL/dinput and the second-order dL/d(dL/doutput) are compared bit for bit.
  * curved activations: a numpy restatement of the passes in float64 (ref64) and the same restatement with every array and operation in
    np.float32, whose error is e32.  Bar per tensor: max|got - ref64| <= 4 e32 + 2^-24 max|ref64|; the factor 4 covers the summation
    order and the device's expf / tanhf / sinf being a few ulp from correctly rounded.  Guard: 4 e32 < 2^-13 max|ref64|, so that the bar
    can never admit an intermediate that was rounded to half (2^-11 relative).
  * weight gradients: per element |got - S| <= gamma(n) sum_s |d x|, gamma(n) = n u / (1 - n u), u = 2^-24, S the float64 sum --
    a bound that holds for any order of summation.
"""
import ctypes as C
import json
import os
import pickle
import subprocess

import numpy as np
import pytest

from conftest import ROOT

gpu = pytest.mark.gpu
FP32, FP16 = 0, 1
K_ACT = 10.0
U = 2.0 ** -24
SRC = os.path.join(ROOT, "tests", "cpp", "mlp_f32_reference.cpp")


def _net(width, hidden, act="ReLU", out_act="None", otype="CutlassMLP"):
    return {"otype": otype, "activation": act, "output_activation": out_act, "n_neurons": width, "n_hidden_layers": hidden}


HASHGRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}


def _create(tcnn, n_in, n_out, net, precision, enc=None, new=True):
    """A native module through the C factories (new: the ones that take a precision)"""
    from tinycudann import _C, modules

    L = _C.lib
    if enc is None:
        if new:
            return modules._create(L.tcnn_create_network_precision, n_in, n_out, _C.to_json_bytes(net), precision)
        return modules._create(L.tcnn_create_network, n_in, n_out, _C.to_json_bytes(net))
    if new:
        return modules._create(L.tcnn_create_network_with_input_encoding_precision, n_in, n_out, _C.to_json_bytes(enc), _C.to_json_bytes(net), precision)
    return modules._create(L.tcnn_create_network_with_input_encoding, n_in, n_out, _C.to_json_bytes(enc), _C.to_json_bytes(net))


def _layer_sizes(native):
    from tinycudann import _C

    n = C.c_size_t()
    _C.check(_C.lib.tcnn_module_layer_sizes(native._h, None, 0, C.byref(n)))
    flat = (C.c_uint32 * max(2 * n.value, 1))()
    _C.check(_C.lib.tcnn_module_layer_sizes(native._h, flat, n.value, C.byref(n)))
    return [(int(flat[2 * i]), int(flat[2 * i + 1])) for i in range(n.value)]


# ---------------------------------------------------------------------------------------------------- CPU: the surface
def test_precision_factories_are_declared_exported_and_bound(tcnn):
    from tinycudann import _C

    header = open(os.path.join(ROOT, "include", "tcnn_amd.h")).read()
    for name in ("tcnn_create_network_with_input_encoding_precision", "tcnn_create_network_precision"):
        assert name + "(" in header
        assert hasattr(_C.lib, name) and name in _C._SIGNATURES


CPU_CASES = [
    ("identity_64x2", 3, 3, None, _net(64, 2)),
    ("frequency_48x3_sine", 3, 4, {"otype": "Frequency", "n_frequencies": 4}, _net(48, 3, "Sine")),
    ("hashgrid_32x1", 3, 1, HASHGRID, _net(32, 1)),
]


@pytest.mark.parametrize("name,n_in,n_out,enc,net", CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_fp32_modules_are_built_without_a_device(tcnn, name, n_in, n_out, enc, net):
    """(this test runs where there is no GPU: construction touches none)"""
    full = _create(tcnn, n_in, n_out, net, FP32, enc)
    half = _create(tcnn, n_in, n_out, net, FP16, enc, new=False)
    assert full.param_precision() == FP32 and full.output_precision() == FP32
    assert half.param_precision() == FP16 and half.output_precision() == FP16
    assert full.n_params() == half.n_params() and full.n_params() > 0
    assert _layer_sizes(full) == _layer_sizes(half) and len(_layer_sizes(full)) == net["n_hidden_layers"] + 1
    assert full.n_input_dims() == half.n_input_dims() and full.n_output_dims() == half.n_output_dims()
    assert full.hyperparams() == half.hyperparams()
    # precision 1 through the new functions builds what the old ones build
    same = _create(tcnn, n_in, n_out, net, FP16, enc)
    assert same.param_precision() == FP16 and same.n_params() == half.n_params()
    assert json.dumps(same.hyperparams(), sort_keys=True) == json.dumps(half.hyperparams(), sort_keys=True)


def test_fp32_refusals(tcnn):
    from tinycudann import _C

    with pytest.raises(RuntimeError, match="FullyFusedMLP can only be used if the network precision is set to __half."):
        _create(tcnn, 32, 3, _net(64, 2, otype="FullyFusedMLP"), FP32)
    with pytest.raises(RuntimeError, match="FullyFusedMLP can only be used if the network precision is set to __half."):
        _create(tcnn, 3, 3, _net(64, 2, otype="FullyFusedMLP"), FP32, HASHGRID)
    with pytest.raises(RuntimeError, match="this build provides the half-precision form"):
        _create(tcnn, 3, 3, _net(64, 2), FP32, {"otype": "PPNG3"})
    with pytest.raises(RuntimeError, match="Unknown precision"):
        _create(tcnn, 32, 3, _net(64, 2), 7)
    assert _C.lib.tcnn_preferred_precision() == FP16
    # the half factories take FullyFusedMLP as before
    assert _create(tcnn, 32, 3, _net(64, 2, otype="FullyFusedMLP"), FP16).param_precision() == FP16


def test_python_dtype_keyword_is_checked_before_anything_is_built(tcnn):
    """(a bad dtype raises the ValueError of Encoding, before the GPU is asked for)"""
    import torch

    for cls, args in ((tcnn.Network, (32, 3, _net(64, 2))), (tcnn.NetworkWithInputEncoding, (3, 3, HASHGRID, _net(64, 2)))):
        with pytest.raises(ValueError, match="only supports fp32 or fp16 precision"):
            cls(*args, dtype=torch.bfloat16)


# ---------------------------------------------------------------------------------------------------- the passes on the GPU
def _t(a, grad=False):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _passes(native, x, params, dy, v, want_params=True):
    """forward, backward and backward_backward_input of one module; numpy results"""
    xt, pt = _t(x, True), _t(params, want_params)
    ctx, out = native.fwd(xt, pt)
    dyt = _t(dy, True)
    dx, dp = native.bwd(ctx, xt, pt, out, dyt)
    ddy, dp2, dx2 = native.bwd_bwd_input(ctx, xt, pt, _t(v), dyt)
    cpu = lambda t: None if t is None else t.detach().cpu().numpy()
    return {"out": cpu(out), "dx": cpu(dx), "dp": cpu(dp), "ddy": cpu(ddy), "dp2": cpu(dp2), "dx2": cpu(dx2)}


def _case(n, n_in, width, hidden, n_out, seed, dy_in_padding=True):
    rs = np.random.RandomState(seed)
    pad_out = -(-n_out // 16) * 16
    dims = [n_in] + [width] * hidden + [pad_out]
    Ws = []
    for cols, rows in zip(dims[:-1], dims[1:]):
        s = (6.0 / (cols + rows)) ** 0.5
        Ws.append(rs.uniform(-s, s, (rows, cols)).astype(np.float32))
    x = rs.uniform(-1, 1, (n, n_in)).astype(np.float32)
    v = rs.uniform(-1, 1, (n, n_in)).astype(np.float32)
    dy = rs.uniform(-1, 1, (n, pad_out)).astype(np.float32)
    if not dy_in_padding:
        dy[:, n_out:] = 0
    return Ws, x, v, dy


def _flat(Ws):
    return np.concatenate([W.reshape(-1) for W in Ws])


@pytest.fixture(scope="module")
def reference_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mlp_f32_reference") / "mlp_f32_reference")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-O2", "-ffp-contract=off", SRC, "-o", out])
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# (id, n, n_in, width, hidden, n_out): the smallest shapes that cross each boundary of the layer kernel's tiling, which is the half
# kernel's (K staged 32 deep; 64 outputs x 256 samples per workgroup up to 64 outputs, else 128 x 128)
EXACT_SHAPES = [
    ("one_tile_short_k", 256, 16, 16, 1, 1),       # one tile, K shorter than a stage
    ("partial_stage_partial_tile", 256, 32, 48, 2, 3),  # one whole and one partial K stage, a partly skipped output tile
    ("wide_tile_second_block", 256, 16, 144, 1, 17),    # the wide tile, a second output block of 16 rows, padded output 32
    ("no_hidden_layer", 256, 64, 64, 0, 16),
    ("two_sample_blocks", 512, 32, 80, 3, 5),
]


@gpu
@pytest.mark.parametrize("act", ["None", "ReLU"])
@pytest.mark.parametrize("name,n,n_in,width,hidden,n_out", EXACT_SHAPES, ids=[c[0] for c in EXACT_SHAPES])
def test_layers_are_fmaf_chains_bit_for_bit(tcnn, reference_program, tmp_path, name, n, n_in, width, hidden, n_out, act):
    Ws, x, v, dy = _case(n, n_in, width, hidden, n_out, seed=11)
    pad_out = dy.shape[1]
    d = str(tmp_path)
    with open(os.path.join(d, "spec.txt"), "w") as f:
        f.write(f"{n} {n_in} {width} {hidden} {pad_out} {0 if act == 'None' else 1}\n")
    for fname, a in (("x", x), ("w", _flat(Ws)), ("dy", dy), ("v", v)):
        a.tofile(os.path.join(d, fname + ".bin"))
    subprocess.check_call([reference_program, d], timeout=300)
    load = lambda fname, cols: np.fromfile(os.path.join(d, fname + ".bin"), dtype=np.float32).reshape(n, cols)
    native = _create(tcnn, n_in, n_out, _net(width, hidden, act), FP32)
    assert native.n_params() == _flat(Ws).size
    got = _passes(native, x, _flat(Ws), dy, v)
    want_out, want_dx, want_ddy = load(f"h_{hidden}", pad_out), load("g_0", n_in), load(f"u_{hidden}", pad_out)
    for what, a, b in (("output", got["out"], want_out), ("dL_dinput", got["dx"], want_dx), ("dL_ddLdoutput", got["ddy"], want_ddy)):
        differ = _bits(a) != _bits(b)
        assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} elements differ, max |difference| {np.abs(a - b).max()}"
    assert not _bits(got["dx2"]).any(), "the second-order dL_dinput of a piecewise linear network is exactly +0"


@gpu
def test_initial_parameters_are_the_half_modules_master_vector(tcnn):
    cfg = _net(48, 2)
    for enc in (None, HASHGRID):
        a = _create(tcnn, 3 if enc else 32, 3, cfg, FP32, enc).initial_params(1337)
        b = _create(tcnn, 3 if enc else 32, 3, cfg, FP16, enc, new=False).initial_params(1337)
        assert a.dtype == b.dtype and np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------- curved activations
def _np_act(name, z):
    one = z.dtype.type(1)
    k = z.dtype.type(K_ACT)
    if name == "None":
        return z
    if name == "ReLU":
        return np.where(z > 0, z, z.dtype.type(0))
    if name == "Exponential":
        return np.exp(z)
    if name == "Sine":
        return np.sin(z)
    if name == "Sigmoid":
        return one / (one + np.exp(-z))
    if name == "Squareplus":
        y = z * k
        return z.dtype.type(0.5) * (y + np.sqrt(y * y + z.dtype.type(4))) / k
    if name == "Softplus":
        return np.log(np.exp(z * k) + one) / k
    if name == "Tanh":
        return np.tanh(z)
    raise ValueError(name)


def _np_d1(name, x):
    t = x.dtype.type
    if name == "None":
        return np.ones_like(x)
    if name == "ReLU":
        return np.where(x > 0, t(1), t(0))
    if name == "Exponential":
        return np.exp(x)
    if name == "Sine":
        return np.cos(x)
    if name == "Sigmoid":
        s = t(1) / (t(1) + np.exp(-x))
        return s * (t(1) - s)
    if name == "Squareplus":
        y = x * t(K_ACT)
        return t(0.5) * (t(1) + y / np.sqrt(y * y + t(4)))
    if name == "Softplus":
        return t(1) / (t(1) + np.exp(-(x * t(K_ACT))))
    if name == "Tanh":
        th = np.tanh(x)
        return t(1) - th * th
    raise ValueError(name)


def _np_d2(name, x):
    t = x.dtype.type
    if name in ("None", "ReLU"):
        return np.zeros_like(x)
    if name == "Exponential":
        return np.exp(x)
    if name == "Sine":
        return -np.sin(x)
    if name == "Sigmoid":
        s = t(1) / (t(1) + np.exp(-x))
        return s * (t(1) - s) * (t(1) - t(2) * s)
    if name == "Squareplus":
        y = x * t(K_ACT)
        q = y * y + t(4)
        return t(2) * t(K_ACT) / (q * np.sqrt(q))
    if name == "Softplus":
        s = t(1) / (t(1) + np.exp(-(x * t(K_ACT))))
        return t(K_ACT) * s * (t(1) - s)
    if name == "Tanh":
        th = np.tanh(x)
        return t(-2) * th * (t(1) - th * th)
    raise ValueError(name)


def _np_bwd_from_output(name, g, y, z):
    """activation_bwd of the kernels: the derivative from the forward OUTPUT (Sine: from the pre-activation)"""
    t = y.dtype.type
    if name == "None":
        return g
    if name == "ReLU":
        return np.where(y > 0, g, g * t(0))
    if name == "Exponential":
        return g * y
    if name == "Sine":
        return g * np.cos(z)
    if name == "Sigmoid":
        return g * (y * (t(1) - y))
    if name == "Squareplus":
        q = y * t(K_ACT)
        return g * (q * q / (q * q + t(1)))
    if name == "Softplus":
        return g * (t(1) - np.exp(-y * t(K_ACT)))
    if name == "Tanh":
        return g * (t(1) - y * y)
    raise ValueError(name)


def _curved(name):
    return name not in ("None", "ReLU")


def _restate(Ws, acts, x, dy, v, dt):
    """Network::forward / backward / second_order_* on numpy arrays of dtype dt (v: the tangent at the network's input).  Returns the
    results and, for the weight-gradient bounds, the operands of every weight-gradient product."""
    Ws = [W.astype(dt) for W in Ws]
    K = len(Ws)
    h, z = [x.astype(dt)], []
    for W, a in zip(Ws, acts):
        z.append(h[-1] @ W.T)
        h.append(_np_act(a, z[-1]))
    r = {"out": h[-1]}
    # first order, as Network::backward
    dO = [None] * K
    dO[K - 1] = _np_bwd_from_output(acts[K - 1], dy.astype(dt), h[K], z[K - 1])
    for k in range(K - 1, 0, -1):
        dO[k - 1] = _np_bwd_from_output(acts[k - 1], dO[k] @ Ws[k], h[k], z[k - 1])
    r["dx"] = dO[0] @ Ws[0]
    r["dp"] = np.concatenate([(dO[k].T @ h[k]).reshape(-1) for k in range(K)])
    r["dp_terms"] = [[(dO[k], h[k])] for k in range(K)]
    # second order, as Network::second_order_begin / _finish
    aux = [z[k] if _curved(acts[k]) else h[k + 1] for k in range(K)]
    g, d = [None] * K, [None] * K
    g[K - 1] = dy.astype(dt)
    for k in range(K - 1, -1, -1):
        d[k] = g[k] if acts[k] == "None" and k == K - 1 else _np_d1(acts[k], aux[k]) * g[k]
        if k > 0:
            g[k - 1] = d[k] @ Ws[k]
    u, rr = [v.astype(dt)], [None] * K
    for k in range(K):
        zdot = u[-1] @ Ws[k].T
        u.append(_np_d1(acts[k], aux[k]) * zdot)
        if _curved(acts[k]):
            rr[k] = _np_d2(acts[k], aux[k]) * g[k] * zdot
    r["ddy"] = u[-1]
    terms = [[(d[k], u[k])] for k in range(K)]
    dx2 = np.zeros_like(h[0])
    curved = [k for k in range(K) if _curved(acts[k])]
    if curved:
        top = curved[-1]
        p = [None] * K
        p[top] = rr[top]
        for k in range(top, 0, -1):
            back = _np_d1(acts[k - 1], aux[k - 1]) * (p[k] @ Ws[k])
            p[k - 1] = (rr[k - 1] + back) if rr[k - 1] is not None else back
        for k in range(top + 1):
            terms[k].append((p[k], h[k]))
        dx2 = p[0] @ Ws[0]
    r["dx2"] = dx2
    r["dp2"] = np.concatenate([sum(a.T @ b for a, b in terms[k]).reshape(-1) for k in range(K)])
    r["dp2_terms"] = terms
    return r


def _assert_within_fp32_bar(what, got, ref64, ref32):
    scale = np.abs(ref64).max()
    e32 = np.abs(ref32.astype(np.float64) - ref64).max()
    err = np.abs(got.astype(np.float64) - ref64).max()
    print(f"{what}: max|ref64| {scale:.3e}  e32 {e32:.3e}  error {err:.3e}  bar {4 * e32 + U * scale:.3e}")
    assert 4 * e32 < 2.0 ** -13 * scale, f"{what}: the yardstick is too coarse to tell fp32 from half: e32 = {e32}, max|ref64| = {scale}"
    assert err <= 4 * e32 + U * scale, f"{what}: error {err} against e32 = {e32}, max|ref64| = {scale}"


CURVED = ["Tanh", "Sigmoid", "Softplus", "Squareplus", "Exponential", "Sine"]
CURVED_SHAPES = [("48x2", 32, 48, 2, 3), ("144x3", 32, 144, 3, 17)]


@gpu
@pytest.mark.parametrize("act", CURVED)
@pytest.mark.parametrize("name,n_in,width,hidden,n_out", CURVED_SHAPES, ids=[c[0] for c in CURVED_SHAPES])
def test_curved_activations_against_the_fp32_yardstick(tcnn, name, n_in, width, hidden, n_out, act):
    n = 256
    Ws, x, v, dy = _case(n, n_in, width, hidden, n_out, seed=23)
    acts = [act] * hidden + ["None"]
    ref64, ref32 = _restate(Ws, acts, x, dy, v, np.float64), _restate(Ws, acts, x, dy, v, np.float32)
    got = _passes(_create(tcnn, n_in, n_out, _net(width, hidden, act), FP32), x, _flat(Ws), dy, v)
    for key in ("out", "dx", "ddy", "dx2"):
        _assert_within_fp32_bar(f"{act} {name} {key}", got[key], ref64[key], ref32[key])
    # the third result of backward_backward_input, the parameter gradients: on the scale of each layer's matrix
    at = 0
    for k, W in enumerate(Ws):
        sl = slice(at, at + W.size)
        _assert_within_fp32_bar(f"{act} {name} dp2 layer {k}", got["dp2"][sl], ref64["dp2"][sl], ref32["dp2"][sl])
        at += W.size


# ---------------------------------------------------------------------------------------------------- weight gradients
def _wgrad_bound(terms, n):
    """S = the float64 sum over the terms of d^T x, and gamma(n) sum|d x| (the terms' bounds added)"""
    gamma = n * U / (1 - n * U)
    S = sum(a.T @ b for a, b in terms)
    A = sum(np.abs(a).T @ np.abs(b) for a, b in terms)
    return S.reshape(-1), (gamma * A).reshape(-1)


@gpu
@pytest.mark.parametrize("n", [256, 1024])
@pytest.mark.parametrize("act", ["ReLU", "Tanh"])
def test_weight_gradients_within_the_any_order_bound(tcnn, n, act):
    """32 -> 144 x 2 -> 17: panels of 128 and of 16 rows and columns, padded output rows; first order (one product per layer) and second
    order (Tanh: two products per layer, their bounds added).  S and sum|d x| are float64 sums over the float64 restatement's operands.
    Padded ROWS (the output layer's rows past n_output_dims) are exactly zero when dL/doutput is zero there; this module has no padded
    columns (n_input_dims is a multiple of 16; an Identity encoding pads with ones, whose weight gradients are not zero)."""
    n_in, width, hidden, n_out = 32, 144, 2, 17
    Ws, x, v, dy = _case(n, n_in, width, hidden, n_out, seed=31, dy_in_padding=False)
    acts = [act] * hidden + ["None"]
    ref64 = _restate(Ws, acts, x, dy, v, np.float64)
    native = _create(tcnn, n_in, n_out, _net(width, hidden, act), FP32)
    got = _passes(native, x, _flat(Ws), dy, v)
    again = _passes(native, x, _flat(Ws), dy, v)
    for key in ("dp", "dp2"):
        assert np.array_equal(_bits(got[key]), _bits(again[key])), f"{key}: two runs differ"
        at = 0
        for k, W in enumerate(Ws):
            S, bound = _wgrad_bound(ref64[key + "_terms"][k], n)
            err = np.abs(got[key][at:at + W.size].astype(np.float64) - S)
            print(f"{act} n={n} {key} layer {k}: max|S| {np.abs(S).max():.3e}  max error {err.max():.3e}  max error / bound {(err / np.maximum(bound, 1e-300)).max():.3e}")
            assert (err <= bound).all(), f"{key} layer {k}: |got - S| exceeds gamma(n) sum|d x| at {int((err > bound).sum())} of {err.size} elements"
            at += W.size
        last = got[key][-Ws[-1].size:].reshape(Ws[-1].shape)
        assert not (last[n_out:] != 0).any(), f"{key}: padded output rows are not zero"
        assert (last[:n_out] != 0).any()


@gpu
def test_accumulate_adds_the_overwrite_result(tcnn):
    """TCNN_GRADIENT_ACCUMULATE onto a known buffer = that buffer + the Overwrite result, within one more rounding (u = 2^-24) per
    element.  A ReLU network: one product per layer, so that Accumulate is one addition onto the buffer."""
    import torch

    from tinycudann import _C

    n, n_in, width, hidden, n_out = 256, 32, 144, 2, 17
    Ws, x, v, dy = _case(n, n_in, width, hidden, n_out, seed=37)
    native = _create(tcnn, n_in, n_out, _net(width, hidden, "ReLU"), FP32)
    xt, pt, dyt, vt = _t(x, True), _t(_flat(Ws), True), _t(dy), _t(v)
    ctx, out = native.fwd(xt, pt)
    stream = torch.cuda.current_stream().cuda_stream
    base = np.random.RandomState(3).uniform(-1, 1, pt.numel()).astype(np.float32)
    results = []
    for mode, start in ((1, np.full_like(base, np.nan)), (2, base)):  # TCNN_GRADIENT_OVERWRITE, TCNN_GRADIENT_ACCUMULATE
        buf = _t(start)
        _C.check(_C.lib.tcnn_module_backward_backward_input_mode(native._h, stream, ctx._h, n, vt.data_ptr(), xt.data_ptr(), dyt.data_ptr(), buf.data_ptr(), None, None, pt.data_ptr(), mode))
        results.append(buf.cpu().numpy().astype(np.float64))
    overwrite, accumulate = results
    assert np.isfinite(overwrite).all() and (overwrite != 0).any()
    want = base.astype(np.float64) + overwrite
    assert (np.abs(accumulate - want) <= U * np.abs(want)).all()


# ---------------------------------------------------------------------------------------------------- behind encodings, through torch
def _frequency_np(x, n_frequencies, dt):
    """k_frequency_fwd in dtype dt: per input dim and frequency f the columns sin(arg), sin(arg + pi / 2), arg = (2^f x) pi; padded with
    ones to a multiple of 16.  Returns the batch and d(column)/d(its input dim)."""
    n, d = x.shape
    t = np.dtype(dt).type
    pi = t(np.pi)
    cols, ders, dims = [], [], []
    for j in range(d):
        for f in range(n_frequencies):
            for phase in (t(0), pi / t(2)):
                arg = (x[:, j].astype(dt) * t(2.0 ** f)) * pi + phase
                cols.append(np.sin(arg))
                ders.append(t(2.0 ** f) * pi * np.cos(arg))
                dims.append(j)
    pad = -(-len(cols) // 16) * 16 - len(cols)
    e = np.stack(cols + [np.ones(n, dtype=dt)] * pad, axis=1)
    return e, np.stack(ders, axis=1), np.array(dims)


@gpu
def test_frequency_softplus_through_torch_double_backward(tcnn):
    """Frequency -> 64 x 2 Softplus with dtype=torch.float32 through autograd: forward, backward (dL/dinput and dL/dparams) and double
    backward (the gradient of <v, dL/dinput> with respect to dL/doutput) against the 4 e32 bar; encoding and network are both restated."""
    import torch

    n, n_in, n_out, width, hidden, n_freq = 256, 3, 3, 64, 2, 4
    model = tcnn.NetworkWithInputEncoding(n_in, n_out, {"otype": "Frequency", "n_frequencies": n_freq}, _net(width, hidden, "Softplus"), dtype=torch.float32)
    assert model.params.dtype == torch.float32 and model.dtype == torch.float32 and model.loss_scale == 1.0
    rs = np.random.RandomState(5)
    x = rs.uniform(0, 1, (n, n_in)).astype(np.float32)
    dy = rs.uniform(-1, 1, (n, n_out)).astype(np.float32)
    v = rs.uniform(-1, 1, (n, n_in)).astype(np.float32)
    xt, dyt = _t(x, True), _t(dy, True)
    out = model(xt)
    assert out.dtype == torch.float32 and out.shape == (n, n_out)
    dx, dp = torch.autograd.grad(out, (xt, model.params), dyt, create_graph=True)
    (ddy,) = torch.autograd.grad((dx * _t(v)).sum(), dyt)
    assert dx.dtype == dp.dtype == ddy.dtype == torch.float32

    p = model.params.detach().cpu().numpy()
    dims = [32, width, width, 16]
    Ws, at = [], 0
    for cols, rows in zip(dims[:-1], dims[1:]):
        Ws.append(p[at:at + rows * cols].reshape(rows, cols))
        at += rows * cols
    assert at == p.size
    dy_pad = np.zeros((n, 16), dtype=np.float32)
    dy_pad[:, :n_out] = dy
    acts = ["Softplus"] * hidden + ["None"]
    refs = {}
    for dt in (np.float64, np.float32):
        e, de, dim_of = _frequency_np(x, n_freq, dt)
        assert e.shape == (n, 32)
        t = np.zeros_like(e)  # t = J_enc v
        t[:, :de.shape[1]] = de * v.astype(dt)[:, dim_of]
        r = _restate(Ws, acts, e, dy_pad, t, dt)
        dL_de = r["dx"][:, :de.shape[1]] * de
        r["dL_dinput"] = np.stack([dL_de[:, dim_of == j].sum(axis=1) for j in range(n_in)], axis=1)
        refs[dt] = r
    r64, r32 = refs[np.float64], refs[np.float32]
    _assert_within_fp32_bar("output", out.detach().cpu().numpy(), r64["out"][:, :n_out], r32["out"][:, :n_out])
    _assert_within_fp32_bar("dL_dinput", dx.detach().cpu().numpy(), r64["dL_dinput"], r32["dL_dinput"])
    at = 0
    for k, W in enumerate(Ws):
        sl = slice(at, at + W.size)
        _assert_within_fp32_bar(f"dL_dparams layer {k}", dp.detach().cpu().numpy()[sl], r64["dp"][sl], r32["dp"][sl])
        at += W.size
    _assert_within_fp32_bar("dL_ddLdoutput", ddy.cpu().numpy(), r64["ddy"][:, :n_out], r32["ddy"][:, :n_out])


COMPOSITE = {
    "otype": "Composite",
    "nested": [dict(HASHGRID, n_dims_to_encode=3), {"otype": "SphericalHarmonics", "degree": 3}],
}


@gpu
def test_composite_grid_and_spherical_harmonics_in_front(tcnn):
    """Composite(HashGrid fp32, SphericalHarmonics) -> 64 x 2 ReLU.  The parameter vector is the network's weights, then the grid's
    table: the module's output equals tcnn.Network(dtype=float32) on tcnn.Encoding(dtype=float32)'s batch with the two parts of the vector.
    The grid's gradient equals what the encoding alone gives for the same dL/dy.  Both sum the same products with atomics, in no fixed
    order: each is within gamma(k) A of the exact sum (the grid tests' bound; A = sum |dL/dy w|, at most k <= 8 n products per
    entry), so they are within 2 gamma(8 n) A of each other.  A comes from the encoding's backward pass on |dL/dy| (the
    interpolation weights are not negative), itself within (1 + gamma) of exact."""
    import torch

    n, width = 256, 64
    model = tcnn.NetworkWithInputEncoding(6, 3, COMPOSITE, _net(width, 2), dtype=torch.float32)
    enc = tcnn.Encoding(6, COMPOSITE, dtype=torch.float32)
    n_enc = enc.params.numel()
    assert enc.n_output_dims == 17
    net = tcnn.Network(32, 3, _net(width, 2), dtype=torch.float32)
    n_net = net.params.numel()
    assert model.params.numel() == n_net + n_enc and n_net == 32 * width + width * width + 16 * width
    rs = np.random.RandomState(9)
    with torch.no_grad():
        model.params[n_net:] = _t(rs.uniform(-1, 1, n_enc).astype(np.float32))
        enc.params.copy_(model.params[n_net:])
        net.params.copy_(model.params[:n_net])
    x = rs.uniform(0, 1, (n, 6)).astype(np.float32)
    dy = _t(rs.uniform(-1, 1, (n, 3)).astype(np.float32))
    xt = _t(x, True)
    out = model(xt)
    dx, dp = torch.autograd.grad(out, (xt, model.params), dy, create_graph=True)
    (ddy_probe,) = torch.autograd.grad(dx.sum(), model.params, allow_unused=True, retain_graph=True)
    for t in (out, dx, dp, ddy_probe):
        assert t is not None and t.dtype == torch.float32 and torch.isfinite(t).all()
    # by hand: encoding, padded with ones to 32, network.  The last nested encoding absorbs the padding and SphericalHarmonics puts
    # its padding columns first (spherical_harmonics.h:58-64): [grid 8][ones 15][SH 9]
    e = enc(_t(x))
    e_pad = torch.cat([e[:, :8], torch.ones(n, 32 - e.shape[1], device="cuda"), e[:, 8:]], dim=1).requires_grad_(True)
    out_hand = net(e_pad)
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(out_hand.detach().cpu().numpy()))
    (de,) = torch.autograd.grad(out_hand, e_pad, dy)
    e2 = enc(_t(x))
    de = torch.cat([de[:, :8], de[:, 23:]], dim=1).contiguous()  # dL/d(the encoding's own 17 columns)
    (g_enc,) = torch.autograd.grad(e2, enc.params, de, retain_graph=True)
    (A,) = torch.autograd.grad(e2, enc.params, de.abs())
    gamma = 8 * n * U / (1 - 8 * n * U)
    diff = (dp[n_net:].detach() - g_enc).abs().double()
    assert (diff <= 2 * gamma * (1 + gamma) * A.double() + 1e-45).all(), float((diff - 2 * gamma * A.double()).max())
    assert g_enc.abs().max() > 0


@gpu
def test_eikonal_loop_with_torch_adam(tcnn):
    """3 -> HashGrid fp32 -> CutlassMLP 64 x 2 Softplus -> 1 trained on | |grad f| - 1 | with torch.optim.Adam: 50 steps, every loss
    finite, the mean eikonal error below where it started"""
    import torch

    torch.manual_seed(0)
    model = tcnn.NetworkWithInputEncoding(3, 1, HASHGRID, _net(64, 2, "Softplus"), dtype=torch.float32)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    x = torch.rand(512, 3, device="cuda")
    losses = []
    for _ in range(50):
        xs = x.clone().requires_grad_(True)
        f = model(xs)
        (grad,) = torch.autograd.grad(f.sum(), xs, create_graph=True)
        loss = ((grad.norm(dim=1) - 1) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-5:]) < losses[0], (losses[0], losses[-5:])


@gpu
def test_python_surface_of_fp32_modules(tcnn):
    import torch

    x = torch.rand(300, 32, device="cuda")
    half = tcnn.Network(32, 3, _net(64, 2))
    before = half(x).detach().clone()
    model = tcnn.Network(32, 3, _net(80, 2, "Tanh"), dtype=torch.float32)
    assert model.params.dtype == torch.float32 and model.dtype == torch.float32 and model.loss_scale == 1.0
    out = model(x)
    assert out.dtype == torch.float32 and out.shape == (300, 3)
    assert tcnn.Network(32, 3, _net(64, 2), dtype=torch.float16).dtype == torch.float16
    clone = pickle.loads(pickle.dumps(model))
    assert clone.dtype == torch.float32 and clone.native_tcnn_module.param_precision() == FP32
    assert torch.equal(clone(x), out)
    with pytest.raises(TypeError, match="use torch.optim for it"):
        tcnn.optimizers.Optimizer(model, {"otype": "Adam"})
    with pytest.raises(RuntimeError, match="FullyFusedMLP can only be used if the network precision is set to __half."):
        tcnn.Network(32, 3, _net(64, 2, otype="FullyFusedMLP"), dtype=torch.float32)
    # a half module made in the same process afterwards gives the bits it gave before
    assert torch.equal(tcnn.Network(32, 3, _net(64, 2))(x), before) and torch.equal(half(x), before)
