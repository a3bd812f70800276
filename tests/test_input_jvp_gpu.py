"""input_jvp on the GPU: jvp[:, t, :] = J(x) tangents[:, t, :] for every output column, in the module's output precision.

1. The "two-pass" route against the code it is made of: for every module with a second-order pass the result is BIT FOR BIT the
   dL_ddLdoutput of forward(prepare_input_gradients=1) + bwd_bwd_input(dL_ddLdinput = tangents[:, t, :]) -- for any dL_doutput, the
   tangent does not depend on it -- and the output is inference's.
2. The fused kernel k_mlp_input_jvp, where mlp_input_jvp_plan selects it (_route below restates the rule; tests/test_input_jvp_plan.py
   has all of it): the output is inference's bit for bit; per tangent ||jvp - R64|| <= 2 ||Rh - R64||, the project's second-order
   criterion (tests/test_network_second_order.py: R64 the recipe in float64 on the half parameters, Rh in fp32 with a rounding to half
   where the kernel rounds: z, h and u per layer), after ||Rh - R64|| <= 0.05 ||R64|| so that the bar cannot hide a wrong result; two
   runs give the same bits; a sample's rows do not depend on where in the batch it sits; a linear network anchors scale and layout.
   Shapes the plan keeps on the two passes run the same checks on that route.
3. FullyFusedMLP takes the routes of a CutlassMLP of its shape (same bits) and still has no second-order pass.
4. OneBlob: half(v k') with k' from the oracle's OneBlob backward pass, bit for bit; behind a network the route is "two-pass".
5. Trainer.input_jvp is the module's call on the trainer's parameters.  6. PPNG1 / PPNG2 are refused and leave the module usable.

Measured on the CPU for the seeds below (||Rh - R64|| / ||R64||, the restatement alone, worst tangent): ReLU 16 x 1 3.0e-4, 64 x 2 1.8e-2,
128 x 4 3.4e-2, 32 x 4 4.4e-2, LeakyReLU 64 x 2 1.5e-2, Softplus shapes 3.0e-4 .. 6.8e-4 -- all under 0.05; every GPU case prints its
own ratios (measured: ||ours - R64|| / ||Rh - R64|| = 1.000 in every case, fused and two-pass: the kernels round where Rh rounds).
"""
import numpy as np
import pytest

from test_input_gradient_gpu import HASH, _create_network, _create_nwie, _net, _params, _same_bits, _x
from test_network_second_order import _acts, _restate

pytestmark = pytest.mark.gpu

NOT_IMPLEMENTED = "not implemented"


def _tangents(n, n_tangents, n_in, seed=23):
    import torch

    return (torch.rand((n, n_tangents, n_in), generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * 2 - 1).cuda().contiguous()


def _route(width, hidden, act, n, n_tangents):
    """mlp_input_jvp_plan for a half-precision fused-shape network created without TCNN_AMD_MLP_LAYERWISE"""
    from test_input_jvp_plan import expected

    answer = expected("FullyFusedMLP", "fp16", width, hidden, act, n, n_tangents, False)
    return answer if answer == "two-pass" else answer.split()[1]


def _second_order_tangent(native, x, params, v, dy_seed=5):
    """the yardstick: dL_ddLdoutput of forward(prepare_input_gradients=1) + bwd_bwd_input(dL_ddLdinput = v) for a random dL_doutput"""
    import torch

    ctx, out = native.fwd(x.clone().requires_grad_(True), params)
    dy = (torch.rand(out.shape, generator=torch.Generator().manual_seed(dy_seed)) * 2 - 1).to(out.dtype).cuda().requires_grad_(True)
    return native.bwd_bwd_input(ctx, x, params, v.contiguous(), dy)[0]


def _check_two_pass(native, x, params, n_in, tangent_counts=(1, 3)):
    import torch

    n = x.shape[0]
    before = params.clone()
    inference = native.fwd(x, params)[1]
    nonzero = False
    for T in tangent_counts:
        v = _tangents(n, T, n_in, seed=23 + T)
        jvp, out = native.input_jvp(x, params, v, want_output=True)
        assert native.last_input_jvp_route() == "two-pass", native.last_input_jvp_route()
        assert jvp.shape == (n, T, native.n_output_dims()) and jvp.dtype == inference.dtype
        assert _same_bits(out, inference)
        for t in range(T):
            want = _second_order_tangent(native, x, params, v[:, t, :])
            assert _same_bits(jvp[:, t, :].contiguous(), want), (T, t, float((jvp[:, t, :].float() - want.float()).abs().max()))
        no_out, none = native.input_jvp(x, params, v)  # output == NULL
        assert none is None and _same_bits(no_out, jvp)
        nonzero = nonzero or bool((jvp.float() != 0).any())
        assert bool(jvp.float().isfinite().all())
    assert nonzero and _same_bits(params, before)  # parameters are read only


# ------------------------------------------------------------------------------------------------------------ 1. two-pass == second order
GRID5 = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 3, "per_level_scale": 2.0}
SH16 = {"otype": "SphericalHarmonics", "degree": 4}


def _composite(reduction):
    grid = {**HASH, "n_features_per_level": 4, "n_dims_to_encode": 3}  # 16 columns, as degree-4 spherical harmonics: a Product needs equal widths
    return {"otype": "Composite", "reduction": reduction, "nested": [grid, {**SH16, "n_dims_to_encode": 3}]}


TWO_PASS_MODULES = [
    ("leaky_48x3", "network", {"n_in": 5, "n_out": 3, "net": _net(48, 3, "LeakyReLU", otype="CutlassMLP")}),
    ("tanh_144x1_20_outputs", "network", {"n_in": 5, "n_out": 20, "net": _net(144, 1, "Tanh", otype="CutlassMLP")}),
    ("sine_64x2", "network", {"n_in": 5, "n_out": 3, "net": _net(64, 2, "Sine", otype="CutlassMLP")}),
    ("no_hidden", "network", {"n_in": 5, "n_out": 3, "net": _net(64, 0, otype="CutlassMLP")}),
    ("leaky_48x3_fp32", "network", {"n_in": 5, "n_out": 3, "net": _net(48, 3, "LeakyReLU", otype="CutlassMLP"), "fp32": True}),
    ("grid_2d_linear", "encoding", {"n_in": 2, "enc": HASH}),
    ("grid_3d_linear", "encoding", {"n_in": 3, "enc": HASH}),
    ("grid_2d_smoothstep", "encoding", {"n_in": 2, "enc": {**HASH, "interpolation": "Smoothstep"}}),
    ("grid_3d_smoothstep", "encoding", {"n_in": 3, "enc": {**HASH, "interpolation": "Smoothstep"}}),
    ("grid_5d", "encoding", {"n_in": 5, "enc": GRID5}),
    ("frequency", "encoding", {"n_in": 3, "enc": {"otype": "Frequency", "n_frequencies": 4}}),
    ("spherical_harmonics", "encoding", {"n_in": 3, "enc": SH16}),
    ("composite_concatenation", "encoding", {"n_in": 6, "enc": _composite("Concatenation")}),
    ("composite_product", "encoding", {"n_in": 6, "enc": _composite("Product")}),
    ("grid_3d_48x2", "nwie", {"n_in": 3, "n_out": 3, "enc": HASH, "net": _net(48, 2, otype="CutlassMLP")}),
    ("grid_3d_48x2_max_level", "nwie", {"n_in": 3, "n_out": 3, "enc": HASH, "net": _net(48, 2, otype="CutlassMLP"), "max_level": 0.5}),
]


def _make(tcnn, kind, c):
    from tinycudann import _C
    from tinycudann.modules import _create

    precision = _C.Precision.Fp32 if c.get("fp32") else _C.Precision.Fp16
    if kind == "network":
        return _create_network(tcnn, c["n_in"], c["n_out"], c["net"], precision)
    if kind == "nwie":
        return _create_nwie(tcnn, c["n_in"], c["n_out"], c["enc"], c["net"], precision)
    return _create(_C.lib.tcnn_create_encoding, c["n_in"], _C.to_json_bytes(c["enc"]), precision)


def _gained_params(tcnn, native, kind, c):
    """grid tables are initialised within 1e-4: scaled up, so that the encoding's derivative is no rounding residue"""
    from tinycudann import _C
    from tinycudann.modules import _create

    params = _params(native).clone()
    if kind == "network" or not native.n_params():
        return params
    n_enc = _create(_C.lib.tcnn_create_encoding, c["n_in"], _C.to_json_bytes(c["enc"]), _C.Precision.Fp16).n_params()
    params[native.n_params() - n_enc:] *= 1000  # (the encoding's parameters lie behind the network's)
    return params.contiguous()


@pytest.mark.parametrize("case", TWO_PASS_MODULES, ids=[c[0] for c in TWO_PASS_MODULES])
def test_two_pass_is_the_second_order_pass_bit_for_bit(tcnn, case):
    _, kind, c = case
    native = _make(tcnn, kind, c)
    assert native.last_input_jvp_route() == "none"
    params = _gained_params(tcnn, native, kind, c)
    if "max_level" in c:
        native.set_max_level(1000.0)
        full = native.input_jvp(_x(256, c["n_in"]), params, _tangents(256, 1, c["n_in"]))[0]
        native.set_max_level(c["max_level"])
        cut = native.input_jvp(_x(256, c["n_in"]), params, _tangents(256, 1, c["n_in"]))[0]
        assert not _same_bits(full, cut)  # the setting applies
    for n in (256, 512):
        _check_two_pass(native, _x(n, c["n_in"]), params, c["n_in"])


# ------------------------------------------------------------------------------------------------------------ 2. the fused kernel's contract
def _half_network(n_in_padded, width, hidden, pad_out, seed):
    """half weight matrices [rows][cols], Xavier-uniform, one behind the other as the module's parameters"""
    import torch

    g = torch.Generator().manual_seed(seed)
    dims = [n_in_padded] + [width] * hidden + [pad_out]
    Ws = []
    for cols, rows in zip(dims[:-1], dims[1:]):
        s = (6.0 / (cols + rows)) ** 0.5
        Ws.append(((torch.rand(rows, cols, generator=g) * 2 - 1) * s).half())
    return Ws


def _restated(Ws, acts, x, v, n_in_padded):
    """(R64, Rh) of the tangent for half-representable x [n][n_in] and v [n][n_in] behind the Identity encoding: the input padded with
    ones, the tangent with zeros"""
    import torch

    n, n_in = x.shape
    xp = torch.cat([x, torch.ones(n, n_in_padded - n_in)], dim=1)
    vp = torch.cat([v, torch.zeros(n, n_in_padded - n_in)], dim=1)
    dy = torch.zeros(n, Ws[-1].shape[0])
    return _restate(Ws, acts, xp, dy, vp, half=False)[0], _restate(Ws, acts, xp, dy, vp, half=True)[0].double()


def _criterion(name, ours, r64, rh):
    import torch

    e_ours, e_h, norm = float(torch.linalg.norm(ours - r64)), float(torch.linalg.norm(rh - r64)), float(torch.linalg.norm(r64))
    print(f"{name}: |ours-R64|/|R64| {e_ours / norm:.3e}  |Rh-R64|/|R64| {e_h / norm:.3e}  ratio {e_ours / max(e_h, 1e-300):.3f}")
    assert norm > 0 and e_h <= 0.05 * norm, (name, e_h / norm)  # the restatement alone: the bar cannot hide a wrong result
    assert e_ours <= 2 * e_h, (name, e_ours, e_h)


# (id, inputs, width, hidden, outputs, activation)
FUSED_SHAPES = [
    ("relu_16x1_1_output", 3, 16, 1, 1, "ReLU"),
    ("relu_64x2_16_outputs", 3, 64, 2, 16, "ReLU"),
    ("relu_128x4_20_outputs_32_inputs", 32, 128, 4, 20, "ReLU"),
    ("relu_32x4_20_outputs", 3, 32, 4, 20, "ReLU"),
    ("softplus_16x1_16_outputs_32_inputs", 32, 16, 1, 16, "Softplus"),
    ("softplus_64x2_20_outputs", 3, 64, 2, 20, "Softplus"),
    ("softplus_128x4_1_output", 3, 128, 4, 1, "Softplus"),
    ("softplus_32x4_16_outputs", 3, 32, 4, 16, "Softplus"),
    ("leaky_64x2_3_outputs", 3, 64, 2, 3, "LeakyReLU"),
]


@pytest.mark.parametrize("case", FUSED_SHAPES, ids=[c[0] for c in FUSED_SHAPES])
def test_fused_shapes_meet_the_contract(tcnn, case):
    import torch

    name, n_in, width, hidden, n_out, act = case
    n_in_padded, pad_out = -(-n_in // 16) * 16, -(-n_out // 16) * 16
    Ws = _half_network(n_in_padded, width, hidden, pad_out, seed=3)
    acts = _acts(hidden, act, "None")
    native = _create_network(tcnn, n_in, n_out, _net(width, hidden, act))
    params = torch.cat([W.reshape(-1) for W in Ws]).cuda().contiguous()
    assert native.n_params() == params.numel() and native.n_output_dims() == pad_out
    g = torch.Generator().manual_seed(17)
    n = 512
    x = (torch.rand(n, n_in, generator=g) * 2 - 1).half().float()
    inference = native.fwd(x.cuda(), params)[1]
    for T in (1, 3, 4):  # one launch of each form, and TT + 1: a second launch
        v = (torch.rand(n, T, n_in, generator=g) * 2 - 1).half().float()
        route = _route(width, hidden, act, n, T)
        jvp, out = native.input_jvp(x.cuda(), params, v.cuda().contiguous(), want_output=True)
        assert native.last_input_jvp_route() == route, (native.last_input_jvp_route(), route)
        assert _same_bits(out, inference)
        assert jvp.shape == (n, T, pad_out) and jvp.dtype == torch.half
        for t in range(T):
            r64, rh = _restated(Ws, acts, x, v[:, t, :], n_in_padded)
            _criterion(f"{name} {route} T={T} t={t}", jvp[:, t, :].cpu().double(), r64, rh)
        again = native.input_jvp(x.cuda(), params, v.cuda().contiguous())[0]
        assert _same_bits(again, jvp)  # two runs, the same bits
        # rows 0 .. 255 moved to rows 256 .. 511 of another call, behind other rows
        moved_x = torch.cat([(torch.rand(256, n_in, generator=g) * 2 - 1), x[:256]]).cuda().contiguous()
        moved_v = torch.cat([(torch.rand(256, T, n_in, generator=g) * 2 - 1), v[:256]]).cuda().contiguous()
        moved = native.input_jvp(moved_x, params, moved_v)[0]
        assert _same_bits(moved[256:].contiguous(), jvp[:256].contiguous())
        small = native.input_jvp(x[:256].cuda().contiguous(), params, v[:256].cuda().contiguous())[0]  # and in a batch of another size
        assert native.last_input_jvp_route() == _route(width, hidden, act, 256, T)
        if _route(width, hidden, act, 256, T) == route:
            assert _same_bits(small, jvp[:256].contiguous())


@pytest.mark.parametrize("n_in,width,hidden", [(3, 32, 1), (32, 64, 2), (3, 128, 4)])
def test_linear_network_jvp_is_the_weight_product(tcnn, n_in, width, hidden):
    """activation None: jvp = (product of the half weight matrices, in float64) half(v), within the bar test_input_jacobian_gpu.py uses
    for the same anchor (rel_err < 2e-3: every layer's result is rounded to half, 2^-11 relative each)"""
    import torch

    from test_gpu_parity import rel_err

    n_in_padded = -(-n_in // 16) * 16
    Ws = _half_network(n_in_padded, width, hidden, 16, seed=4)
    native = _create_network(tcnn, n_in, 3, _net(width, hidden, "None"))
    params = torch.cat([W.reshape(-1) for W in Ws]).cuda().contiguous()
    product = np.eye(n_in_padded)
    for W in Ws:
        product = W.numpy().astype(np.float64) @ product
    n, T = 512, 3
    v = _tangents(n, T, n_in)
    jvp = native.input_jvp(_x(n, n_in), params, v)[0]
    assert native.last_input_jvp_route() == _route(width, hidden, "None", n, T)
    want = np.einsum("ok,ntk->nto", product[:, :n_in], v.cpu().half().numpy().astype(np.float64))
    err = rel_err(jvp.cpu().numpy().astype(np.float64), want)
    print("linear %d x %d, %d inputs: jvp vs the float64 weight product: rel_err %.3g" % (width, hidden, n_in, err))
    assert np.any(want != 0) and err < 2e-3


# ------------------------------------------------------------------------------------------------------------ 3. FullyFusedMLP
def test_fully_fused_mlp_takes_the_cutlass_routes_and_keeps_no_second_order_pass(tcnn):
    import torch

    n, n_in = 512, 5
    x = _x(n, n_in)
    fused = _create_network(tcnn, n_in, 3, _net(64, 2, "Softplus"))
    cutlass = _create_network(tcnn, n_in, 3, _net(64, 2, "Softplus", otype="CutlassMLP"))
    params = _params(fused)
    for T in (1, 3):
        v = _tangents(n, T, n_in)
        a, out_a = fused.input_jvp(x, params, v, want_output=True)
        b, out_b = cutlass.input_jvp(x, params, v, want_output=True)
        assert fused.last_input_jvp_route() == cutlass.last_input_jvp_route() == _route(64, 2, "Softplus", n, T)
        assert _same_bits(a, b) and _same_bits(out_a, out_b) and bool((a.float() != 0).any())
        assert _same_bits(out_a, fused.fwd(x, params)[1])
    ctx, out = fused.fwd(x.clone().requires_grad_(True), params)
    with pytest.raises(RuntimeError, match=NOT_IMPLEMENTED):
        fused.bwd_bwd_input(ctx, x, params, _tangents(n, 1, n_in)[:, 0, :].contiguous(), torch.rand_like(out).requires_grad_(True))
    again = fused.input_jvp(x, params, _tangents(n, 3, n_in))[0]
    assert _same_bits(again, a)


# ------------------------------------------------------------------------------------------------------------ 4. OneBlob
@pytest.mark.parametrize("n_bins", [16, 64])
def test_oneblob_tangent_is_v_times_the_backward_kernels_derivative(tcnn, oracle, n_bins):
    """k' of every (sample, column) from the oracle's OneBlob backward pass with a one-hot dL_dy per column (its sum has one nonzero term:
    1.0 k'); expected half(v k') in numpy float32, one rounding; bits equal"""
    from tinycudann import _C
    from tinycudann.modules import _create

    n, n_in = 256, 2
    cfg = {"otype": "OneBlob", "n_bins": n_bins}
    native = _create(_C.lib.tcnn_create_encoding, n_in, _C.to_json_bytes(cfg), _C.Precision.Fp16)
    ref = oracle.create_encoding(n_in, cfg, alignment=0)
    width = ref.padded_output_width
    assert width == n_in * n_bins == native.n_output_dims()
    x = oracle.Pcg32(42).uniform_strided(n * n_in).reshape(n, n_in).astype(np.float32)
    k = np.zeros((n, width), dtype=np.float32)
    for col in range(width):
        dy = np.zeros((n, width), dtype=np.float32)
        dy[:, col] = 1.0
        k[:, col] = ref.backward(x, {}, oracle.half_bits(dy), want_dL_dx=True)[:, col // n_bins]
    assert np.count_nonzero(k) > 0
    import torch

    xt = torch.from_numpy(x).cuda().contiguous()
    params = _params(native)
    inference = native.fwd(xt, params)[1]
    for T in (1, 3):
        v = _tangents(n, T, n_in)
        jvp, out = native.input_jvp(xt, params, v, want_output=True)
        assert native.last_input_jvp_route() == "two-pass" and _same_bits(out, inference)
        vn = v.cpu().numpy()
        want = (np.repeat(vn, n_bins, axis=2) * k[:, None, :]).astype(np.float16)
        got = jvp.cpu().numpy()
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), float(np.abs(got.astype(np.float32) - want.astype(np.float32)).max())
        assert np.count_nonzero(want) > 0


def test_oneblob_behind_a_network_takes_the_two_passes(tcnn):
    """NetworkWithInputEncoding(OneBlob 32 bins, 64 x 2): the route, and the accuracy criterion with the network's input and tangent taken
    from the encoding's own forward pass and tangent (tested above)"""
    import torch

    from tinycudann import _C
    from tinycudann.modules import _create

    n, n_in, n_bins = 512, 2, 32
    cfg = {"otype": "OneBlob", "n_bins": n_bins}
    native = _create_nwie(tcnn, n_in, 3, cfg, _net(64, 2))
    encoding = _create(_C.lib.tcnn_create_encoding, n_in, _C.to_json_bytes(cfg), _C.Precision.Fp16)
    Ws = _half_network(n_in * n_bins, 64, 2, 16, seed=6)
    params = torch.cat([W.reshape(-1) for W in Ws]).cuda().contiguous()
    assert native.n_params() == params.numel()
    x = _x(n, n_in)
    no_params = torch.zeros(0, dtype=torch.half, device="cuda")
    e = encoding.fwd(x, no_params)[1].cpu().float()
    for T in (1, 3):
        v = _tangents(n, T, n_in)
        jvp = native.input_jvp(x, params, v)[0]
        assert native.last_input_jvp_route() == "two-pass"
        t_enc = encoding.input_jvp(x, no_params, v)[0].cpu().float()
        for t in range(T):
            r64, rh = _restated(Ws, _acts(2, "ReLU", "None"), e, t_enc[:, t, :], n_in * n_bins)
            _criterion(f"oneblob + relu_64x2 T={T} t={t}", jvp[:, t, :].cpu().double(), r64, rh)


# ------------------------------------------------------------------------------------------------------------ 5. Trainer, Python surfaces
def test_trainer_input_jvp_equals_the_modules(tcnn):
    cfg = {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2}, "encoding": HASH, "network": _net(64, 2)}
    trainer = tcnn.Trainer(3, 3, cfg, seed=1337)
    x = _x(512, 3)
    target = _x(512, 3, seed=5)
    for _ in range(3):  # (so that the parameters are not the initial ones)
        trainer.training_step(x, target)
    params, grads = trainer.params().clone(), trainer.param_gradients().clone()
    v = _tangents(512, 3, 3)
    got = trainer.input_jvp(x, v)
    assert _same_bits(trainer.params(), params) and _same_bits(trainer.param_gradients(), grads)
    native = _create_nwie(tcnn, 3, 3, cfg["encoding"], cfg["network"])
    want = native.input_jvp(x, params.contiguous(), v)[0]
    assert native.last_input_jvp_route() == _route(64, 2, "ReLU", 512, 3)
    assert _same_bits(got, want) and bool((got.float() != 0).any())


def test_module_input_jvp_pads_rows_and_stays_outside_autograd(tcnn):
    import torch

    module = tcnn.NetworkWithInputEncoding(3, 3, HASH, _net(48, 2, otype="CutlassMLP"))
    x = _x(300, 3).requires_grad_(True)
    v = _tangents(300, 3, 3).requires_grad_(True)
    before = module.params.detach().clone()
    jvp, out = module.input_jvp(x, v, return_output=True)
    assert module.native_tcnn_module.last_input_jvp_route() == "two-pass"
    assert jvp.shape == (300, 3, 3) and jvp.dtype == module.dtype and out.shape == (300, 3)
    assert jvp.grad_fn is None and not jvp.requires_grad and out.grad_fn is None
    with torch.no_grad():
        assert _same_bits(out.contiguous(), module(x).contiguous())
    flat = module.input_jvp(x, v[:, 1, :])  # 2-D tangents: T = 1, a 2-D result
    assert flat.shape == (300, 3) and _same_bits(flat.contiguous(), jvp[:, 1, :].contiguous())
    assert module.params.grad is None and x.grad is None and v.grad is None and _same_bits(module.params.detach(), before)
    with pytest.raises(ValueError, match="tangents"):
        module.input_jvp(x, v[:100])
    for cls, args in ((tcnn.Network, (5, 3, _net(48, 2, otype="CutlassMLP"))), (tcnn.Encoding, (3, HASH))):
        m = cls(*args)
        j = m.input_jvp(_x(300, args[0]), _tangents(300, 2, args[0]))
        assert j.shape == (300, 2, m.n_output_dims) and m.native_tcnn_module.last_input_jvp_route() == "two-pass"


# ------------------------------------------------------------------------------------------------------------ 6. refusals
PPNG = {"n_frequencies": 2, "n_quants": 8, "n_features": 2, "rank": 2}


@pytest.mark.parametrize("n_in,enc,name", [
    (3, dict(PPNG, otype="PPNG1"), "PPNG1"),
    (3, dict(PPNG, otype="PPNG2"), "PPNG2"),
    (5, {"otype": "Composite", "nested": [{"otype": "OneBlob", "n_bins": 16, "n_dims_to_encode": 2}, dict(PPNG, otype="PPNG1", n_dims_to_encode=3)]}, "Composite"),
], ids=["ppng1", "ppng2", "composite_oneblob_ppng1"])
def test_modules_without_a_tangent_are_refused_and_stay_usable(tcnn, n_in, enc, name):
    from tinycudann import _C
    from tinycudann.modules import _create

    native = _create(_C.lib.tcnn_create_encoding, n_in, _C.to_json_bytes(enc), _C.Precision.Fp16)
    params = _params(native)
    x = _x(256, n_in)
    before = native.fwd(x, params)[1]
    with pytest.raises(RuntimeError, match="input_jvp: not implemented for " + name):
        native.input_jvp(x, params, _tangents(256, 2, n_in))
    assert native.last_input_jvp_route() == "none" and native.last_input_gradient_route() == "none" and native.last_input_jacobian_route() == "none"
    assert _same_bits(native.fwd(x, params)[1], before)  # the next valid call is right
    # and a Composite of encodings that all have a tangent, a OneBlob among them, is not refused
    if name == "Composite":
        ok = {"otype": "Composite", "nested": [{"otype": "OneBlob", "n_bins": 16, "n_dims_to_encode": 2}, {"otype": "Frequency", "n_frequencies": 2, "n_dims_to_encode": 3}]}
        both = _create(_C.lib.tcnn_create_encoding, n_in, _C.to_json_bytes(ok), _C.Precision.Fp16)
        v = _tangents(256, 2, n_in)
        jvp = both.input_jvp(x, _params(both), v)[0]
        assert both.last_input_jvp_route() == "two-pass"
        parts = [_create(_C.lib.tcnn_create_encoding, 2, _C.to_json_bytes(ok["nested"][0]), _C.Precision.Fp16),
                 _create(_C.lib.tcnn_create_encoding, 3, _C.to_json_bytes(ok["nested"][1]), _C.Precision.Fp16)]
        a = parts[0].input_jvp(x[:, :2].contiguous(), _params(parts[0]), v[:, :, :2].contiguous())[0]
        b = parts[1].input_jvp(x[:, 2:].contiguous(), _params(parts[1]), v[:, :, 2:].contiguous())[0]
        assert _same_bits(jvp[:, :, : a.shape[2]].contiguous(), a) and _same_bits(jvp[:, :, a.shape[2]: a.shape[2] + b.shape[2]].contiguous(), b)
