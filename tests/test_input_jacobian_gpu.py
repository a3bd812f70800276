"""input_jacobian on the GPU: d output[d_k] / d input for K output columns from ONE forward pass, float32 [n][K][n_input_dims].

input_gradient is the specification: every case here first asserts the route tcnn_module_input_jacobian took, by name, then compares rows
[:, k, :] BIT FOR BIT with native.input_gradient(dim = d_k) on the same input, parameters, backprop_scale and max_level state, and the output
with that call's output -- whichever route either call takes, so there is no tolerance anywhere.  (The reference of a (module, batch, scale)
is computed once per column and shared by every dims list.)  The rule for the route, mlp_input_jacobian_plan's: the fused kernel
k_mlp_input_jacobian<W,NB,NH>/relu|act for half-precision networks 16 / 32 / 64 / 128 wide with 1 to 4 hidden layers, created without
TCNN_AMD_MLP_LAYERWISE=1, for n a multiple of 16 NB (NB = 2 at 128 wide, else 4) -- except, by measurement, a run-time activation with more
than 256 workgroups (n / (64 NB)) and more dims than its class's limit (64 wide x 2: 2 dims), and ReLU 128 x 2 from 2^20 rows and 9 dims on
(tests/test_input_jacobian_plan.py has the whole rule); "two-pass" (one forward pass, K backward passes) for those, for everything else
and behind a OneBlob encoding.  So that input_gradient and input_jacobian cannot be wrong together:
a linear network's Jacobian is the product of its weight matrices, and two backprop scales agree.
"""
import numpy as np
import pytest

from test_input_gradient_gpu import HASH, SCALE, _create_network, _create_nwie, _grid_params, _net, _params, _same_bits, _x

pytestmark = pytest.mark.gpu


def _fused_name(width, hidden, act):
    nb = 4 if width < 128 else 2
    return "k_mlp_input_jacobian<%d,%d,%d>/%s" % (width, nb, hidden, "relu" if act == "ReLU" else "act")


class _Reference:
    """K calls of input_gradient, one per distinct column, made once per (module, input, parameters, scale) and left unchanged"""

    def __init__(self, native, x, params, scale=SCALE):
        self.native, self.x, self.params, self.scale = native, x, params, scale
        self.columns, self.output = {}, None

    def column(self, dim):
        if dim not in self.columns:
            self.columns[dim], out = self.native.input_gradient(self.x, self.params, dim, self.scale, want_output=True)
            if self.output is None:
                self.output = out
            assert _same_bits(out, self.output)  # input_gradient's output does not depend on dim
        return self.columns[dim]


def _check(ref, dims, route):
    """route asserted first, then every [:, k, :] and the output against input_gradient, bit for bit; returns the Jacobian"""
    import torch

    native = ref.native
    before = ref.params.clone()
    got, out = native.input_jacobian(ref.x, ref.params, dims, ref.scale, want_output=True)
    assert native.last_input_jacobian_route() == route, (native.last_input_jacobian_route(), route)
    assert got.shape == (ref.x.shape[0], len(dims), ref.x.shape[1]) and got.dtype == torch.float32
    for k, dim in enumerate(dims):
        want = ref.column(dim)
        assert _same_bits(got[:, k, :].contiguous(), want), (k, dim, float((got[:, k, :] - want).abs().max()))
    assert _same_bits(out, ref.output)
    got_no_out, none = native.input_jacobian(ref.x, ref.params, dims, ref.scale)  # output == NULL
    assert none is None and _same_bits(got_no_out, got)
    assert _same_bits(ref.params, before)  # parameters are read only
    return got


def _dims_lists(n_out, padded):
    """all real outputs (17 of them: a second launch); one list with a padded column, where there is one; a permuted list with a repeat"""
    lists = [list(range(n_out))]
    if padded > n_out:
        lists.append([0, padded - 1])
    lists.append([n_out - 1, 0, n_out - 1] + list(range(n_out // 2, 0, -1)))
    return lists


# ------------------------------------------------------------------------------------------------------------ fused: bare networks
@pytest.mark.parametrize("hidden", [1, 2, 4])
@pytest.mark.parametrize("width", [16, 32, 64, 128])
def test_network_fused_equals_input_gradient(tcnn, width, hidden):
    """tcnn.Network shapes (5 inputs through the fused Identity load): ReLU and Softplus x output activation None and Sigmoid x 1, 3, 16, 17
    outputs (17: 32 padded columns, seeds in both output tiles, and 17 dims are two launches), n = 256 and 768"""
    n_in = 5
    xs = {n: _x(n, n_in) for n in (256, 768)}
    for act in ("ReLU", "Softplus"):
        for out_act in ("None", "Sigmoid"):
            for n_out in (1, 3, 16, 17):
                native = _create_network(tcnn, n_in, n_out, _net(width, hidden, act, out_act))
                params = _params(native)
                assert native.last_input_jacobian_route() == "none"
                for n in (256, 768):
                    ref = _Reference(native, xs[n], params)
                    for dims in _dims_lists(n_out, native.n_output_dims()):
                        got = _check(ref, dims, _fused_name(width, hidden, act))
                        assert bool(got.isfinite().all()) and bool((got[:, 0, :] != 0).any())


def test_run_time_form_takes_the_two_passes_above_its_limit(tcnn):
    """Softplus 64 x 2, limit 2 dims once there are more workgroups than CUs: 2^17 rows are 512 workgroups, 2^16 rows 256"""
    native = _create_network(tcnn, 5, 3, _net(64, 2, "Softplus"))
    params = _params(native)
    above, at = _Reference(native, _x(1 << 17, 5), params), _Reference(native, _x(1 << 16, 5), params)
    _check(above, [0, 1], _fused_name(64, 2, "Softplus"))
    _check(above, [2, 0, 1], "two-pass")
    _check(at, [2, 0, 1], _fused_name(64, 2, "Softplus"))


# ------------------------------------------------------------------------------------------------------------ fused: behind a grid
def _per_sample_levels(n):
    import torch

    return torch.rand(n, generator=torch.Generator().manual_seed(3), dtype=torch.float32).cuda().contiguous()


@pytest.mark.parametrize("features,width,hidden", [(2, 64, 2), (4, 32, 1)], ids=["F2_64x2", "F4_planes_32x1"])
def test_grid_network_fused_equals_input_gradient(tcnn, features, width, hidden):
    """HashGrid 3-D (L 4, T 2^10) in front, K = 3: the encoding's forward pass with dy_dx once, the fused kernel's three buffers, the
    encoding's backward pass into each strided slice -- with every level, under set_max_level(0.5) and under a per-sample max_level"""
    enc = {**HASH, "n_features_per_level": features}
    native = _create_nwie(tcnn, 3, 3, enc, _net(width, hidden))
    params = _grid_params(native, width, hidden)
    route = _fused_name(width, hidden, "ReLU")
    for n in (256, 768):
        x = _x(n, 3)
        native.set_max_level_gpu(None)
        native.set_max_level(1000.0)
        full = _check(_Reference(native, x, params), [0, 1, 2], route)
        assert bool((full != 0).any()) and bool(full.isfinite().all())
        native.set_max_level(0.5)
        cut = _check(_Reference(native, x, params), [2, 0, 1], route)
        assert not _same_bits(full[:, 0, :].contiguous(), cut[:, 1, :].contiguous())
        native.set_max_level(1000.0)
        native.set_max_level_gpu(_per_sample_levels(n))
        per_sample = _check(_Reference(native, x, params), [0, 1, 2], route)
        assert not _same_bits(full, per_sample)
    native.set_max_level_gpu(None)


def test_more_buffers_than_fit_are_taken_in_groups(tcnn):
    """the K dL/d(network input) buffers are temporaries of at most 256 MB at a time: at 2^20 rows a 16-wide encoding's buffer is 32 MB, so
    9 dims are a group of 8 and a group of 1 -- the second group runs the network again, the encoding's forward pass never; and the two-pass
    network route with the same groups (48 wide)"""
    from tinycudann import _C
    from tinycudann.modules import _create

    x = _x(1 << 20, 3)
    dims = [16, 0, 3, 3, 31, 2, 1, 8, 4]
    n_grid = _create(_C.lib.tcnn_create_encoding, 3, _C.to_json_bytes(HASH), _C.Precision.Fp16).n_params()
    for net, route in ((_net(64, 2), _fused_name(64, 2, "ReLU")), (_net(48, 2, otype="CutlassMLP"), "two-pass")):
        native = _create_nwie(tcnn, 3, 17, HASH, net)
        params = _params(native).clone()
        params[native.n_params() - n_grid:] *= 1000  # the grid's table lies behind the network's parameters, initialised within 1e-4
        got = _check(_Reference(native, x, params), dims, route)
        assert bool((got[:, -1, :] != 0).any()) and bool(got.isfinite().all())


# ------------------------------------------------------------------------------------------------------------ the two-pass cases
COMPOSITE = {"otype": "Composite", "nested": [{**HASH, "n_dims_to_encode": 3}, {"otype": "SphericalHarmonics", "degree": 4}]}
TWO_PASS_CASES = [
    ("fp32", "network", {"n_in": 5, "net": _net(64, 2, otype="CutlassMLP"), "fp32": True}),
    ("sine", "network", {"n_in": 5, "net": _net(64, 2, "Sine", otype="CutlassMLP")}),
    ("width48", "network", {"n_in": 5, "net": _net(48, 2, otype="CutlassMLP")}),
    ("width256", "network", {"n_in": 5, "net": _net(256, 2, otype="CutlassMLP")}),
    ("no_hidden", "network", {"n_in": 5, "net": _net(64, 0, otype="CutlassMLP")}),
    ("oneblob", "nwie", {"n_in": 2, "enc": {"otype": "OneBlob", "n_bins": 32}, "net": _net(64, 2)}),
    ("grid_encoding", "encoding", {"n_in": 3, "enc": HASH}),
    ("frequency_encoding", "encoding", {"n_in": 3, "enc": {"otype": "Frequency", "n_frequencies": 4}}),
    ("layerwise_env", "network", {"n_in": 5, "net": _net(64, 2), "env": {"TCNN_AMD_MLP_LAYERWISE": "1"}}),
    # the network's plan decides behind every encoding but OneBlob, as for input_gradient: the Composite's own passes (one forward pass,
    # a backward pass per dim through both nested encodings) run around the fused kernel
    ("composite_64x2", "nwie", {"n_in": 6, "enc": COMPOSITE, "net": _net(64, 2), "route": _fused_name(64, 2, "ReLU"), "grid_gain": True}),
    ("composite_48x2", "nwie", {"n_in": 6, "enc": COMPOSITE, "net": _net(48, 2, otype="CutlassMLP"), "grid_gain": True}),
]


@pytest.mark.parametrize("case", TWO_PASS_CASES, ids=[c[0] for c in TWO_PASS_CASES])
def test_two_pass_cases(tcnn, monkeypatch, case):
    from tinycudann import _C
    from tinycudann.modules import _create

    _, kind, c = case
    precision = _C.Precision.Fp32 if c.get("fp32") else _C.Precision.Fp16
    with monkeypatch.context() as m:
        for key, value in c.get("env", {}).items():
            m.setenv(key, value)  # (the switches are read when the module is made)
        if kind == "network":
            native = _create_network(tcnn, c["n_in"], 3, c["net"], precision)
        elif kind == "nwie":
            native = _create_nwie(tcnn, c["n_in"], 3, c["enc"], c["net"], precision)
        else:
            native = _create(_C.lib.tcnn_create_encoding, c["n_in"], _C.to_json_bytes(c["enc"]), precision)
    params = _params(native)
    if kind == "encoding" and native.n_params():
        params = params * 1000
    if c.get("grid_gain"):  # the encoding's parameters (the grid's table, initialised within 1e-4) lie behind the network's
        params = params.clone()
        params[native.n_params() - _create(_C.lib.tcnn_create_encoding, c["n_in"], _C.to_json_bytes(c["enc"]), precision).n_params():] *= 1000
    padded = native.n_output_dims()
    for n in (256, 768):
        ref = _Reference(native, _x(n, c["n_in"]), params, scale=1.0 if c.get("fp32") else SCALE)
        for dims in ([0, 1, 2], [padded - 1, 1, 1, 0]):
            got = _check(ref, dims, c.get("route", "two-pass"))
            assert bool((got != 0).any()) and bool(got.isfinite().all())


# ------------------------------------------------------------------------------------------------------------ failure paths
def test_errors_leave_both_routes_alone(tcnn):
    native = _create_network(tcnn, 5, 17, _net(64, 2))
    params = _params(native)
    x = _x(256, 5)
    with pytest.raises(RuntimeError, match="Invalid dimension to compute the input gradient for."):
        native.input_jacobian(x, params, [0, 32], SCALE)
    with pytest.raises(RuntimeError, match="n_dims"):
        native.input_jacobian(x, params, [], SCALE)
    with pytest.raises(RuntimeError, match="n_dims"):
        native.input_jacobian(x, params, [0] * 33, SCALE)
    with pytest.raises(RuntimeError, match="BATCH_SIZE_GRANULARITY"):
        native.input_jacobian(_x(300, 5), params, [0], SCALE)
    assert native.last_input_jacobian_route() == "none" and native.last_input_gradient_route() == "none"
    native.input_jacobian(x, params, [0, 1], SCALE)
    assert native.last_input_jacobian_route() == _fused_name(64, 2, "ReLU") and native.last_input_gradient_route() == "none"
    with pytest.raises(RuntimeError, match="Invalid dimension"):
        native.input_jacobian(x, params, [32], SCALE)
    assert native.last_input_jacobian_route() == _fused_name(64, 2, "ReLU")
    native.input_gradient(x, params, 0, SCALE)
    gradient_route = native.last_input_gradient_route()
    assert gradient_route.startswith("k_mlp_input_grad<") and native.last_input_jacobian_route() == _fused_name(64, 2, "ReLU")
    with pytest.raises(RuntimeError, match="Invalid dimension"):
        native.input_gradient(x, params, 32, SCALE)
    assert native.last_input_gradient_route() == gradient_route and native.last_input_jacobian_route() == _fused_name(64, 2, "ReLU")


# ------------------------------------------------------------------------------------------------------------ independent anchors
def rel_err(a, b):
    """the existing oracle tests' measure: max |a - b| / max |b|"""
    from test_gpu_parity import rel_err as measure

    return measure(a, b)


@pytest.mark.parametrize("width,hidden", [(32, 1), (64, 2), (128, 4)])
def test_linear_network_jacobian_is_the_weight_product(tcnn, width, hidden):
    """activation None: the network is one matrix, so every sample's [K][n_in] block is the same matrix -- whatever the routes do -- and it
    equals the product of the half weight matrices, computed in float64, within the existing oracle test's bar (rel_err < 2e-3; the
    kernel rounds every layer's result to half, 2^-11 relative each)"""
    n_in, n_out = 5, 3
    native = _create_network(tcnn, n_in, n_out, _net(width, hidden, "None"))
    params = _params(native)
    dims = [0, 1, 2, 15]
    got = _check(_Reference(native, _x(768, n_in), params), dims, _fused_name(width, hidden, "None"))
    assert _same_bits(got, got[:1].expand_as(got).contiguous())
    # row-major [fan_out][fan_in] matrices one behind the other: 16 padded inputs, `hidden` layers of `width`, 16 padded outputs
    w = params.cpu().numpy().astype(np.float64)
    shapes = [(width, 16)] + [(width, width)] * (hidden - 1) + [(16, width)]
    product, at = np.eye(16), 0
    for rows, cols in shapes:
        product = w[at:at + rows * cols].reshape(rows, cols) @ product
        at += rows * cols
    assert at == native.n_params()
    want = product[dims, :n_in]
    err = rel_err(got[0].cpu().numpy().astype(np.float64), want)
    print("linear %d x %d: Jacobian vs the float64 weight product: rel_err %.3g" % (width, hidden, err))
    assert np.any(want[:3] != 0) and err < 2e-3


def test_backprop_scales_agree(tcnn):
    """64 x 2 ReLU behind a grid: backprop_scale 1 against 128, within the same bar"""
    native = _create_nwie(tcnn, 3, 3, HASH, _net(64, 2))
    params = _grid_params(native, 64, 2)
    x = _x(768, 3)
    scaled = _check(_Reference(native, x, params, scale=SCALE), [0, 1, 2], _fused_name(64, 2, "ReLU")).cpu().numpy()
    unscaled = _check(_Reference(native, x, params, scale=1.0), [0, 1, 2], _fused_name(64, 2, "ReLU")).cpu().numpy()
    err = rel_err(unscaled, scaled)
    print("backprop_scale 1 vs 128: rel_err %.3g" % err)
    assert np.any(scaled != 0) and err < 2e-3


# ------------------------------------------------------------------------------------------------------------ Python surfaces
def test_module_input_jacobian_pads_rows_and_stays_outside_autograd(tcnn):
    import torch

    module = tcnn.NetworkWithInputEncoding(3, 3, HASH, _net(64, 2))
    with torch.no_grad():
        module.params[16 * 64 + 64 * 64 + 64 * 16:] *= 1000
    x = _x(300, 3).requires_grad_(True)
    before = module.params.detach().clone()
    got, out = module.input_jacobian(x, return_output=True)  # dims=None: range(n_output_dims)
    native = module.native_tcnn_module
    assert native.last_input_jacobian_route() == _fused_name(64, 2, "ReLU")
    assert got.shape == (300, 3, 3) and got.dtype == torch.float32 and out.shape == (300, 3)
    assert got.grad_fn is None and not got.requires_grad and out.grad_fn is None and not out.requires_grad
    for k in range(3):
        want, want_out = module.input_gradient(x, dim=k, return_output=True)
        assert _same_bits(got[:, k, :].contiguous(), want) and _same_bits(out.contiguous(), want_out.contiguous())
    permuted = module.input_jacobian(x, dims=[2, 5, 2])
    assert permuted.shape == (300, 3, 3) and _same_bits(permuted[:, 0, :].contiguous(), got[:, 2, :].contiguous())
    assert _same_bits(permuted[:, 2, :].contiguous(), got[:, 2, :].contiguous())
    assert module.params.grad is None and x.grad is None and _same_bits(module.params.detach(), before)
    for cls, args in ((tcnn.Network, (5, 3, _net(64, 2))), (tcnn.Encoding, (3, HASH))):
        m = cls(*args)
        xm = _x(300, args[0])
        j = m.input_jacobian(xm, dims=[1, 0])
        assert j.shape == (300, 2, args[0]) and m.native_tcnn_module.last_input_jacobian_route() == (_fused_name(64, 2, "ReLU") if cls is tcnn.Network else "two-pass")
        for k, dim in enumerate((1, 0)):
            assert _same_bits(j[:, k, :].contiguous(), m.input_gradient(xm, dim=dim))


def test_trainer_input_jacobian_equals_the_modules(tcnn):
    cfg = {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2}, "encoding": HASH, "network": _net(64, 2)}
    trainer = tcnn.Trainer(3, 3, cfg, seed=1337)
    x = _x(768, 3)
    target = _x(768, 3, seed=5)
    for _ in range(3):  # (so that the parameters are not the initial ones)
        trainer.training_step(x, target)
    params, grads = trainer.params().clone(), trainer.param_gradients().clone()
    dims = [1, 0, 2, 1]
    got = trainer.input_jacobian(x, dims)
    assert _same_bits(trainer.params(), params) and _same_bits(trainer.param_gradients(), grads)
    native = _create_nwie(tcnn, 3, 3, cfg["encoding"], cfg["network"])
    want = _check(_Reference(native, x, params.contiguous(), scale=trainer.default_loss_scale), dims, _fused_name(64, 2, "ReLU"))
    assert _same_bits(got, want) and bool((got != 0).any())
    for k, dim in enumerate(dims):
        assert _same_bits(got[:, k, :].contiguous(), trainer.input_gradient(x, dim=dim))
