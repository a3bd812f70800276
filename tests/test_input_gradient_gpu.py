"""input_gradient (object.h:342-366) on the GPU: d output[dim] / d input at inference.

The two-pass route defines the result: forward(prepare_input_gradients) and backward(GradientMode::Ignore) on a dL/doutput that holds
(output precision)backprop_scale in column dim and +0 elsewhere, times the float 1.0f / backprop_scale.  Every case here first asserts the
route tcnn_module_input_gradient took, by name, then compares d_dinput and the output BIT FOR BIT with that sequence made by hand through
tcnn_module_forward / tcnn_module_backward: the fused kernel keeps the halves k_mlp_fwd stores and issues k_mlp_fwd's and k_mlp_bwd's
matrix instructions in their order, so there is no tolerance.  So that both routes cannot be wrong together: a linear network gives every
row the same vector, one ReLU network goes against the CPU oracle, and two backprop scales agree.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HASH = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 4, "per_level_scale": 2.0}
SCALE = 128.0


def _net(width, hidden, act="ReLU", out_act="None", otype="FullyFusedMLP"):
    return {"otype": otype, "activation": act, "output_activation": out_act, "n_neurons": width, "n_hidden_layers": hidden}


def _x(n, n_in, seed=7):
    import torch

    return torch.rand((n, n_in), generator=torch.Generator().manual_seed(seed), dtype=torch.float32).cuda().contiguous()


def _params(native, seed=11, gain=1.0):
    """the native initialisation in the module's parameter precision; gain != 1: other parameters"""
    from tinycudann.modules import _torch_precision

    return (native.initial_params(seed) * gain).to(_torch_precision(native.param_precision())).contiguous()


def _two_pass(native, x, params, dim, scale):
    """the defining sequence, by hand through the C ABI -> (d_dinput, output)"""
    import torch
    from tinycudann import _C
    from tinycudann.modules import _ptr, _stream, _torch_precision

    n, pw = x.shape[0], native.n_output_dims()
    dt = _torch_precision(native.output_precision())
    dy = torch.zeros((n, pw), dtype=dt, device="cuda")
    dy[:, dim] = scale  # (output precision)backprop_scale
    out = torch.empty((n, pw), dtype=dt, device="cuda")
    dx = torch.empty((n, x.shape[1]), dtype=torch.float32, device="cuda")
    h = C.c_void_p()
    _C.check(_C.lib.tcnn_module_forward(native._h, _stream(), n, _ptr(x), _ptr(out), _ptr(params), 1, C.byref(h)))
    try:
        _C.check(_C.lib.tcnn_module_backward(native._h, _stream(), h, n, _ptr(dx), _ptr(dy), None, _ptr(x), _ptr(out), _ptr(params)))
    finally:
        _C.lib.tcnn_context_destroy(h)
    mult = np.float32(1.0) / np.float32(scale)  # formed once in float
    return dx * float(mult), out


def _same_bits(a, b):
    import torch

    assert a.dtype == b.dtype and a.shape == b.shape
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))


def _check(native, x, params, dim, route, scale=SCALE):
    """route asserted first, then d_dinput and output against the hand-made two passes, bit for bit; returns d_dinput"""
    before = params.clone()
    got, out = native.input_gradient(x, params, dim, scale, want_output=True)
    assert native.last_input_gradient_route() == route, (native.last_input_gradient_route(), route)
    want, want_out = _two_pass(native, x, params, dim, scale)
    assert _same_bits(got, want), float((got - want).abs().max())
    assert _same_bits(out, want_out)
    got_no_out, none = native.input_gradient(x, params, dim, scale)  # output == NULL
    assert none is None and _same_bits(got_no_out, want)
    assert _same_bits(params, before)  # parameters are read only
    return got


def _fused_name(width, hidden, act):
    nb = 4 if width < 128 else 2
    return "k_mlp_input_grad<%d,%d,%d>/%s" % (width, nb, hidden, "relu" if act == "ReLU" else "act")


def _create_network(tcnn, n_in, n_out, net, precision=None):
    from tinycudann import _C
    from tinycudann.modules import _create

    return _create(_C.lib.tcnn_create_network_precision, n_in, n_out, _C.to_json_bytes(net), _C.Precision.Fp16 if precision is None else precision)


def _create_nwie(tcnn, n_in, n_out, enc, net, precision=None):
    from tinycudann import _C
    from tinycudann.modules import _create

    return _create(_C.lib.tcnn_create_network_with_input_encoding_precision, n_in, n_out, _C.to_json_bytes(enc), _C.to_json_bytes(net),
                   _C.Precision.Fp16 if precision is None else precision)


# ------------------------------------------------------------------------------------------------------------ fused: bare networks
@pytest.mark.parametrize("hidden", [1, 2, 4])
@pytest.mark.parametrize("width", [16, 32, 64, 128])
def test_network_fused_equals_two_pass(tcnn, width, hidden):
    """tcnn.Network shapes: ReLU and Softplus x output activation None and Sigmoid x 1, 3, 16, 17 outputs, n = 256 and 768; dim = first,
    last real column and, for 17 outputs (32 padded), the padded column 20"""
    n_in = 5  # the fused Identity input: 5 coordinates, padded with ones to 16
    xs = {n: _x(n, n_in) for n in (256, 768)}
    for act in ("ReLU", "Softplus"):
        for out_act in ("None", "Sigmoid"):
            for n_out in (1, 3, 16, 17):
                native = _create_network(tcnn, n_in, n_out, _net(width, hidden, act, out_act))
                params = _params(native)
                assert native.last_input_gradient_route() == "none"
                dims = sorted({0, n_out - 1} | ({20} if n_out == 17 else set()))
                for n in (256, 768):
                    for dim in dims:
                        got = _check(native, xs[n], params, dim, _fused_name(width, hidden, act))
                        assert bool(got.isfinite().all())
                        if dim < n_out:
                            assert bool((got != 0).any())


# ------------------------------------------------------------------------------------------------------------ fused: behind a grid
def _grid_params(native, width, hidden, gain=1000.0):
    """grid tables are initialised within 1e-4: scaled up, so that the encoding's derivative is no rounding residue.  The network's
    parameters come first: 16 encoded inputs (8 or 16 features, padded), `hidden` layers of `width`, 16 padded outputs."""
    n_net = 16 * width + (hidden - 1) * width * width + width * 16
    params = _params(native).clone()
    assert 0 < n_net < native.n_params()
    params[n_net:] *= gain
    return params


@pytest.mark.parametrize("features,width,hidden", [(2, 64, 2), (4, 32, 1)], ids=["F2_64x2", "F4_planes_32x1"])
def test_grid_network_fused_equals_two_pass(tcnn, features, width, hidden):
    """HashGrid 3-D (L 4, T 2^10) in front: the encoding's forward pass with dy_dx, the fused kernel writing dL/d(encoding) in the form
    the encoding's backward route asks for (level planes of F features), the encoding's backward pass"""
    enc = {**HASH, "n_features_per_level": features}
    native = _create_nwie(tcnn, 3, 3, enc, _net(width, hidden))
    params = _grid_params(native, width, hidden)
    for n in (256, 768):
        x = _x(n, 3)
        for dim in (0, 2):
            got = _check(native, x, params, dim, _fused_name(width, hidden, "ReLU"))
            assert bool((got != 0).any()) and bool(got.isfinite().all())


def test_max_level_applies_as_in_a_forward_pass(tcnn):
    native = _create_nwie(tcnn, 3, 1, HASH, _net(64, 2))
    params = _grid_params(native, 64, 2)
    x = _x(256, 3)
    full = _check(native, x, params, 0, _fused_name(64, 2, "ReLU"))
    native.set_max_level(0.5)
    cut = _check(native, x, params, 0, _fused_name(64, 2, "ReLU"))
    assert not _same_bits(full, cut)


# ------------------------------------------------------------------------------------------------------------ the two-pass cases
TWO_PASS_CASES = [
    ("sine", "network", {"n_in": 5, "net": _net(64, 2, "Sine", otype="CutlassMLP")}),
    ("width48", "network", {"n_in": 5, "net": _net(48, 2, otype="CutlassMLP")}),
    ("no_hidden", "network", {"n_in": 5, "net": _net(64, 0, otype="CutlassMLP")}),
    ("fp32", "network", {"n_in": 5, "net": _net(64, 2, otype="CutlassMLP"), "fp32": True}),
    ("depth6", "network", {"n_in": 5, "net": _net(64, 6)}),
    ("oneblob", "nwie", {"n_in": 2, "enc": {"otype": "OneBlob", "n_bins": 32}, "net": _net(64, 2)}),
    ("grid_encoding", "encoding", {"n_in": 3, "enc": HASH}),
    ("frequency_encoding", "encoding", {"n_in": 3, "enc": {"otype": "Frequency", "n_frequencies": 4}}),
]


@pytest.mark.parametrize("case", TWO_PASS_CASES, ids=[c[0] for c in TWO_PASS_CASES])
def test_two_pass_cases(tcnn, case):
    from tinycudann import _C
    from tinycudann.modules import _create

    _, kind, c = case
    precision = _C.Precision.Fp32 if c.get("fp32") else _C.Precision.Fp16
    if kind == "network":
        native = _create_network(tcnn, c["n_in"], 3, c["net"], precision)
    elif kind == "nwie":
        native = _create_nwie(tcnn, c["n_in"], 3, c["enc"], c["net"], precision)
    else:
        native = _create(_C.lib.tcnn_create_encoding, c["n_in"], _C.to_json_bytes(c["enc"]), precision)
    params = _params(native)
    if kind == "encoding" and native.n_params():
        params = params * 1000
    for n in (256, 768):
        got = _check(native, _x(n, c["n_in"]), params, 1, "two-pass", scale=1.0 if c.get("fp32") else SCALE)
        assert bool((got != 0).any())


def test_errors_leave_the_route_alone(tcnn):
    from tinycudann import _C
    from tinycudann.modules import _ptr, _stream

    native = _create_network(tcnn, 5, 17, _net(64, 2))
    params = _params(native)
    x = _x(256, 5)
    with pytest.raises(RuntimeError, match="Invalid dimension to compute the input gradient for."):
        native.input_gradient(x, params, 32, SCALE)
    assert native.last_input_gradient_route() == "none"
    with pytest.raises(RuntimeError, match="BATCH_SIZE_GRANULARITY"):
        native.input_gradient(_x(300, 5), params, 0, SCALE)
    dx = _x(256, 5)
    assert _C.lib.tcnn_module_input_gradient(None, _stream(), 256, 0, _ptr(x), _ptr(dx), None, _ptr(params), SCALE) == 1 and _C.lib.tcnn_last_error()


# ------------------------------------------------------------------------------------------------------------ independent anchors
@pytest.mark.parametrize("width,hidden", [(32, 1), (64, 2), (128, 4)])
def test_linear_network_gives_every_row_the_same_vector(tcnn, width, hidden):
    """activation None: the network is one matrix, so d output[dim] / d input does not depend on the sample -- whatever the routes do"""
    native = _create_network(tcnn, 5, 3, _net(width, hidden, "None"))
    params = _params(native)
    x = _x(768, 5)
    rows = []
    for dim in (0, 1, 2):
        got = _check(native, x, params, dim, _fused_name(width, hidden, "None"))
        assert bool((got != 0).any())
        assert _same_bits(got, got[:1].expand_as(got).contiguous())
        rows.append(got[0].clone())
    assert not _same_bits(rows[0], rows[1]) and not _same_bits(rows[1], rows[2])


def test_relu_network_against_the_oracle(tcnn, oracle):
    """64 x 2 ReLU behind an Identity encoding against the CPU oracle's backward pass from the same one-hot dL/dy, with the bar
    test_training_step_matrix.py applies to dL/dinput where bit equality is not to be had (rel_err < 2e-3); and backprop scales 128 and 1
    agree within the same bar"""
    from test_training_step_matrix import _cfg, _t, rel_err

    n, n_in, n_out, dim = 768, 3, 3, 1
    cfg = _cfg({"otype": "Identity"}, 64, 2)
    ref = oracle.Trainer(n_in, n_out, cfg, seed=1337)
    x = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in)
    dy32 = np.zeros((n, ref.model.padded_output_width), dtype=np.float32)
    dy32[:, dim] = SCALE
    want = ref.training_step(x, None, run_optimizer=False, want_dL_dx=True, external_dL_dy=oracle.half_bits(dy32))["dL_dinput"] / np.float32(SCALE)
    native = _create_nwie(tcnn, n_in, n_out, cfg["encoding"], cfg["network"])
    params = _t(np.asarray(ref.params).view(np.float16))
    got = _check(native, _t(x.astype(np.float32)), params, dim, _fused_name(64, 2, "ReLU")).cpu().numpy()
    err = rel_err(got, want)
    print("input_gradient vs oracle: rel_err %.3g" % err)
    assert np.any(want != 0) and err < 2e-3
    unscaled = _check(native, _t(x.astype(np.float32)), params, dim, _fused_name(64, 2, "ReLU"), scale=1.0).cpu().numpy()
    err1 = rel_err(unscaled, got)
    print("backprop_scale 1 vs 128: rel_err %.3g" % err1)
    assert err1 < 2e-3


def test_other_parameters_are_used(tcnn):
    native = _create_network(tcnn, 5, 3, _net(64, 2))
    x = _x(256, 5)
    a = _check(native, x, _params(native, seed=11), 0, _fused_name(64, 2, "ReLU"))
    b = _check(native, x, _params(native, seed=12), 0, _fused_name(64, 2, "ReLU"))
    assert not _same_bits(a, b)


# ------------------------------------------------------------------------------------------------------------ Python surfaces
def test_module_input_gradient_pads_rows_and_stays_outside_autograd(tcnn):
    import torch

    module = tcnn.NetworkWithInputEncoding(3, 3, HASH, _net(64, 2))
    with torch.no_grad():
        module.params[16 * 64 + 64 * 64 + 64 * 16:] *= 1000
    x = _x(300, 3)
    before = module.params.detach().clone()
    got, out = module.input_gradient(x, dim=2, return_output=True)
    native = module.native_tcnn_module
    assert native.last_input_gradient_route() == _fused_name(64, 2, "ReLU")
    assert got.shape == (300, 3) and got.dtype == torch.float32 and not got.requires_grad and out.shape == (300, 3)
    rows = torch.zeros((512, 3), dtype=torch.float32, device="cuda")
    rows[:300] = x
    want, want_out = native.input_gradient(rows, module.params.detach().half().contiguous(), 2, module.loss_scale, want_output=True)
    assert _same_bits(got, want[:300].contiguous()) and _same_bits(out.contiguous(), want_out[:300, :3].contiguous())
    assert _same_bits(module.input_gradient(x, dim=2), got)
    assert module.params.grad is None and _same_bits(module.params.detach(), before)
    for cls, args in ((tcnn.Network, (5, 3, _net(64, 2))), (tcnn.Encoding, (3, HASH))):
        m = cls(*args)
        g = m.input_gradient(_x(300, args[0]), dim=1)
        assert g.shape == (300, args[0]) and m.native_tcnn_module.last_input_gradient_route() == (_fused_name(64, 2, "ReLU") if cls is tcnn.Network else "two-pass")


def test_trainer_input_gradient_equals_the_modules(tcnn):
    import torch

    cfg = {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2}, "encoding": HASH, "network": _net(64, 2)}
    trainer = tcnn.Trainer(3, 3, cfg, seed=1337)
    x = _x(768, 3)
    target = _x(768, 3, seed=5)
    for _ in range(3):  # (so that the parameters are not the initial ones)
        trainer.training_step(x, target)
    params, grads = trainer.params().clone(), trainer.param_gradients().clone()
    got = trainer.input_gradient(x, dim=1)
    assert _same_bits(trainer.params(), params) and _same_bits(trainer.param_gradients(), grads)
    native = _create_nwie(tcnn, 3, 3, cfg["encoding"], cfg["network"])
    want = _check(native, x, params.contiguous(), 1, _fused_name(64, 2, "ReLU"), scale=trainer.default_loss_scale)
    assert _same_bits(got, want) and bool((got != 0).any())
