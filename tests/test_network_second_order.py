"""Second-order input gradients through CutlassMLP networks: tcnn.Network and tcnn.NetworkWithInputEncoding under
backward_backward_input (Network::second_order_begin / _finish, NetworkWithInputEncoding::backward_backward_input, the
second-order epilogues of k_mlp_layers.hip).

The network is checked against two restatements of the recipe in torch on the CPU:
  R64  fp64 throughout, on the half parameters;
  Rh   fp32 with a round-to-half wherever the kernels store a half matrix.
For every result the kernels must be as close to R64 as Rh is, up to a factor 2: they round at the same points as Rh, so their
error is another realisation of the same rounding noise; two realisations may differ by sqrt(2) in norm, 2 is that rounded up.
The recipe itself is checked against torch.autograd's double backward in fp64 (CPU).  The composition with an encoding is checked
against the same pipeline assembled by hand from tcnn.Encoding and tcnn.Network."""
import ctypes

import pytest

gpu = pytest.mark.gpu
K_ACT = 10.0
LOSS_SCALE = 128.0


# ---------------------------------------------------------------------------------------------------- the recipe, restated
def _act(name, z):
    import torch

    if name == "None":
        return z
    if name == "ReLU":
        return torch.relu(z)
    if name == "LeakyReLU":
        return torch.where(z > 0, z, z * 0.01)
    if name == "Exponential":
        return torch.exp(z)
    if name == "Sine":
        return torch.sin(z)
    if name == "Sigmoid":
        return torch.sigmoid(z)
    if name == "Squareplus":
        y = z * K_ACT
        return 0.5 * (y + torch.sqrt(y * y + 4)) / K_ACT
    if name == "Softplus":
        return torch.nn.functional.softplus(z * K_ACT) / K_ACT
    if name == "Tanh":
        return torch.tanh(z)
    raise ValueError(name)


def _d1(name, x):
    """a'(z); x is z, or for ReLU / LeakyReLU anything with the sign of z"""
    import torch

    one = torch.ones_like(x)
    if name == "None":
        return one
    if name == "ReLU":
        return torch.where(x > 0, one, 0 * one)
    if name == "LeakyReLU":
        return torch.where(x > 0, one, 0.01 * one)
    if name == "Exponential":
        return torch.exp(x)
    if name == "Sine":
        return torch.cos(x)
    if name == "Sigmoid":
        s = torch.sigmoid(x)
        return s * (1 - s)
    if name == "Squareplus":
        y = x * K_ACT
        return 0.5 * (1 + y / torch.sqrt(y * y + 4))
    if name == "Softplus":
        return torch.sigmoid(x * K_ACT)
    if name == "Tanh":
        return 1 - torch.tanh(x) ** 2
    raise ValueError(name)


def _d2(name, x):
    import torch

    if name in ("None", "ReLU", "LeakyReLU"):
        return torch.zeros_like(x)
    if name == "Exponential":
        return torch.exp(x)
    if name == "Sine":
        return -torch.sin(x)
    if name == "Sigmoid":
        s = torch.sigmoid(x)
        return s * (1 - s) * (1 - 2 * s)
    if name == "Squareplus":
        q = (x * K_ACT) ** 2 + 4
        return 2 * K_ACT / (q * torch.sqrt(q))
    if name == "Softplus":
        s = torch.sigmoid(x * K_ACT)
        return K_ACT * s * (1 - s)
    if name == "Tanh":
        t = torch.tanh(x)
        return -2 * t * (1 - t * t)
    raise ValueError(name)


def _curved(name):
    return name not in ("None", "ReLU", "LeakyReLU")


def _restate(Ws, acts, x, dy, v, half):
    """The recipe of Network::second_order_* on CPU tensors.  Ws: the weight matrices [rows][cols]; acts: one activation name per
    layer.  half=False: fp64, nothing rounded (R64).  half=True: fp32, rounded to half wherever the kernels store a half matrix:
    z, h, g, d, u, r, p and the results (Rh).  Returns dL_ddLdoutput, the weight gradients per layer, dS/dinput."""
    import torch

    dt = torch.float32 if half else torch.float64
    rh = (lambda t: t.half().to(dt)) if half else (lambda t: t)
    Ws = [W.to(dt) for W in Ws]
    K = len(Ws)
    h, z = [rh(x.to(dt))], []
    for W, a in zip(Ws, acts):
        z.append(rh(h[-1] @ W.T))
        h.append(rh(_act(a, z[-1])))
    aux = [z[k] if _curved(acts[k]) else h[k + 1] for k in range(K)]  # what the derivatives are taken from
    g, d = [None] * K, [None] * K
    g[K - 1] = dy.to(dt)
    for k in range(K - 1, -1, -1):
        d[k] = g[k] if acts[k] == "None" and k == K - 1 else rh(g[k] * _d1(acts[k], aux[k]))
        if k > 0:
            g[k - 1] = rh(d[k] @ Ws[k])
    u, r = [rh(v.to(dt))], [None] * K
    for k in range(K):
        zdot = u[-1] @ Ws[k].T  # never stored: not rounded
        u.append(rh(_d1(acts[k], aux[k]) * zdot))
        if _curved(acts[k]):
            r[k] = rh(_d2(acts[k], aux[k]) * g[k] * zdot)
    dW = [rh(d[k].T @ u[k]) for k in range(K)]
    dx = torch.zeros_like(h[0])
    curved = [k for k in range(K) if _curved(acts[k])]
    if curved:
        top = curved[-1]
        p = [None] * K
        p[top] = r[top]
        for k in range(top, 0, -1):
            back = _d1(acts[k - 1], aux[k - 1]) * (p[k] @ Ws[k])
            p[k - 1] = rh((r[k - 1] if r[k - 1] is not None else 0) + back)
        for k in range(top + 1):
            dW[k] = rh(dW[k] + p[k].T @ h[k])
        dx = rh(p[0] @ Ws[0])
    return u[-1], dW, dx


def _case_tensors(n, n_in, width, hidden, n_out, act, seed):
    """half-representable weights, input, tangent and dL_doutput (at loss scale) of one network"""
    import torch

    g = torch.Generator().manual_seed(seed)
    pad_out = -(-n_out // 16) * 16
    dims = [n_in] + [width] * hidden + [pad_out]
    Ws = []
    for cols, rows in zip(dims[:-1], dims[1:]):
        s = (6.0 / (cols + rows)) ** 0.5
        Ws.append(((torch.rand(rows, cols, generator=g) * 2 - 1) * s).half())
    x = (torch.rand(n, n_in, generator=g) * 2 - 1).half()
    v = (torch.rand(n, n_in, generator=g) * 2 - 1).half()
    dy = ((torch.rand(n, pad_out, generator=g) * 2 - 1) * (LOSS_SCALE / n)).half()
    return Ws, x, v, dy


def _net_cfg(width, hidden, act, out_act="None", otype="CutlassMLP"):
    return {"otype": otype, "activation": act, "output_activation": out_act, "n_neurons": width, "n_hidden_layers": hidden}


# (id, n_in, width, hidden, n_out, activation, output activation)
NETWORK_CASES = [
    ("relu_64x2", 32, 64, 2, 16, "ReLU", "None"),  # first-order passes of this shape run the fused kernels
    ("leaky_48x3", 16, 48, 3, 3, "LeakyReLU", "None"),
    ("softplus_128x4", 32, 128, 4, 16, "Softplus", "None"),
    ("tanh_96x2_sigmoid", 32, 96, 2, 3, "Tanh", "Sigmoid"),
    ("sine_208x2", 16, 208, 2, 16, "Sine", "None"),
    ("exp_out_64x0", 32, 64, 0, 3, "ReLU", "Exponential"),
    ("squareplus_512x1", 32, 512, 1, 16, "Squareplus", "None"),
    ("sigmoid_32x2_relu_out", 16, 32, 2, 3, "Sigmoid", "ReLU"),
    ("exp_16x1_tanh_out", 16, 16, 1, 3, "Exponential", "Tanh"),
]


def _acts(hidden, act, out_act):
    return [act] * hidden + [out_act]


# ---------------------------------------------------------------------------------------------------- CPU: the recipe is right
@pytest.mark.parametrize("act,out_act", [("ReLU", "Sigmoid"), ("Softplus", "None"), ("Sine", "Sigmoid"), ("Tanh", "Exponential"), ("Squareplus", "Tanh"),
                                         ("Sigmoid", "Softplus"), ("LeakyReLU", "None"), ("Exponential", "Squareplus")])
def test_recipe_matches_autograd_double_backward(act, out_act):
    """R64 against torch.autograd in fp64: S = <v, dL/dx> differentiated with respect to dL/dy, every weight matrix and x"""
    import torch

    Ws, x, v, dy = _case_tensors(64, 16, 32, 2, 3, act, seed=5)
    acts = _acts(2, act, out_act)
    want_ddy, want_dW, want_dx = _restate(Ws, acts, x, dy, v, half=False)

    Wp = [W.double().requires_grad_(True) for W in Ws]
    xp = x.double().requires_grad_(True)
    dyp = dy.double().requires_grad_(True)
    h = xp
    for W, a in zip(Wp, acts):
        h = _act(a, h @ W.T)
    (gx,) = torch.autograd.grad(h, xp, grad_outputs=dyp, create_graph=True)
    got = torch.autograd.grad((gx * v.double()).sum(), [dyp, xp] + Wp, allow_unused=True)
    assert torch.allclose(got[0], want_ddy, rtol=1e-10, atol=1e-14)
    got_dx = torch.zeros_like(xp) if got[1] is None else got[1]
    assert torch.allclose(got_dx, want_dx, rtol=1e-10, atol=1e-14)
    for a, b in zip(got[2:], want_dW):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-14)


def test_restatements_agree_and_piecewise_linear_has_no_input_term():
    """Rh is R64 up to half rounding, and its dS/dinput is exactly zero where no activation has curvature"""
    import torch

    for act, bound in (("Softplus", 5e-3), ("ReLU", 1e-1)):
        Ws, x, v, dy = _case_tensors(1024, 32, 64, 2, 16, act, seed=1)
        acts = _acts(2, act, "None")
        a, b = _restate(Ws, acts, x, dy, v, half=False), _restate(Ws, acts, x, dy, v, half=True)
        for p, q in zip([a[0]] + a[1], [b[0]] + b[1]):
            assert float(torch.linalg.norm(q.double() - p)) <= bound * float(torch.linalg.norm(p))
        if act == "ReLU":
            assert not a[2].any() and not b[2].any()
        else:
            assert float(torch.linalg.norm(b[2].double() - a[2])) <= bound * float(torch.linalg.norm(a[2]))


# ---------------------------------------------------------------------------------------------------- GPU helpers
def _flat_params(Ws):
    import torch

    return torch.cat([W.reshape(-1) for W in Ws]).cuda()


def _run_network(tcnn, case, n, seed=11, params_grad=True):
    """(module, tensors, (dL_ddLdoutput, dL_dparams, dL_dinput)) of one bwd_bwd_input call through the C ABI"""
    _, n_in, width, hidden, n_out, act, out_act = case
    Ws, x, v, dy = _case_tensors(n, n_in, width, hidden, n_out, act, seed)
    net = tcnn.Network(n_in, n_out, _net_cfg(width, hidden, act, out_act))
    native = net.native_tcnn_module
    assert native.n_params() == sum(W.numel() for W in Ws)
    xt = x.float().cuda().requires_grad_(True)
    pt = _flat_params(Ws).requires_grad_(params_grad)
    dyt = dy.cuda().requires_grad_(True)
    ctx, _ = native.fwd(xt, pt)
    return net, (Ws, x, v, dy, xt, pt, dyt, ctx), native.bwd_bwd_input(ctx, xt, pt, v.float().cuda(), dyt)


def _check_against_restatements(case, tensors, results, report=None):
    """||ours - R64|| <= 2 ||Rh - R64|| for dL_ddLdoutput, every layer's weight gradient and dL_dinput; exact zeros where R64 has them"""
    import torch

    name, _, _, hidden, _, act, out_act = case
    Ws, x, v, dy = tensors[:4]
    acts = _acts(hidden, act, out_act)
    r64 = _restate(Ws, acts, x, dy, v, half=False)
    rh = _restate(Ws, acts, x, dy, v, half=True)
    ddy, dparams, dx = results
    ours_dW, off = [], 0
    for W in Ws:
        ours_dW.append(dparams[off:off + W.numel()].reshape(W.shape).cpu().double())
        off += W.numel()
    triples = [("dL_ddLdoutput", ddy.cpu().double(), rh[0].double(), r64[0])]
    triples += [(f"dL_dparams[{k}]", ours_dW[k], rh[1][k].double(), r64[1][k]) for k in range(len(Ws))]
    triples.append(("dL_dinput", dx.cpu().double(), rh[2].double(), r64[2]))
    failures = []
    for what, ours, h, ref in triples:
        e_ours, e_h, norm = float(torch.linalg.norm(ours - ref)), float(torch.linalg.norm(h - ref)), float(torch.linalg.norm(ref))
        ratio = e_ours / e_h if e_h > 0 else (0.0 if e_ours == 0 else float("inf"))
        print(f"{name:24s} {what:16s} |ours-R64|/|R64| {e_ours / max(norm, 1e-300):.3e}  |Rh-R64|/|R64| {e_h / max(norm, 1e-300):.3e}  ratio {ratio:.3f}")
        if report is not None:
            report.append((name, what, e_ours / max(norm, 1e-300), e_h / max(norm, 1e-300), ratio))
        if not e_ours <= 2 * e_h:
            failures.append((what, e_ours, e_h))
        if not bool((ours[ref == 0] == 0).all()):
            failures.append((what, "nonzero where R64 is exactly zero"))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------- 1. network against the restatements
@gpu
@pytest.mark.parametrize("case", NETWORK_CASES, ids=[c[0] for c in NETWORK_CASES])
def test_network_second_order_matches_restatement(tcnn, case):
    import torch

    n = 4096
    net, tensors, results = _run_network(tcnn, case, n)
    ddy, dparams, dx = results
    _check_against_restatements(case, tensors, results)

    _, _, _, hidden, _, act, out_act = case
    if not any(_curved(a) for a in _acts(hidden, act, out_act)):
        assert not dx.view(torch.int32).any()  # all bits zero: the curvature pass is not launched

    Ws, x, v, dy, xt, pt, dyt, ctx = tensors
    native = net.native_tcnn_module
    # two runs give the same bits (no atomics anywhere in the network's passes)
    ddy2, dparams2, dx2 = native.bwd_bwd_input(ctx, xt, pt, v.float().cuda(), dyt)
    assert torch.equal(ddy2.view(torch.int16), ddy.view(torch.int16)) and torch.equal(dparams2.view(torch.int16), dparams.view(torch.int16))
    assert torch.equal(dx2.view(torch.int32), dx.view(torch.int32))
    # only what is asked for is computed
    ddy3, dparams3, dx3 = native.bwd_bwd_input(ctx, xt, pt.detach(), v.float().cuda(), dyt)
    assert dparams3 is None
    assert torch.equal(ddy3.view(torch.int16), ddy.view(torch.int16)) and torch.equal(dx3.view(torch.int32), dx.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 2. composition
GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5, "interpolation": "Smoothstep"}
PPNG3 = {"otype": "PPNG3", "n_frequencies": 2, "n_quants": 8, "n_features_per_level": 2, "log2_min_freq": 0, "log2_max_freq": 2}


def _composed_by_hand(tcnn, enc_cfg, net_cfg, n_in, n_out, x, v, dy, p_net, p_enc):
    """The four steps of NetworkWithInputEncoding::backward_backward_input from separate modules: tcnn.Encoding (which does not pad)
    and tcnn.Network on the encoded batch, padded by hand to the network's input width as the encoding pads inside the model (the
    grid: with zeros), with a zero tangent in the padding"""
    import torch

    enc = tcnn.Encoding(n_in, enc_cfg)
    e_nat = enc.native_tcnn_module
    w = enc.n_output_dims
    pw = -(-w // 16) * 16
    net = tcnn.Network(pw, n_out, net_cfg)
    n_nat = net.native_tcnn_module
    assert e_nat.n_params() == p_enc.numel() and n_nat.n_params() == p_net.numel()

    def padded(t):
        return torch.cat([t.float(), torch.zeros(t.shape[0], pw - w, device="cuda")], dim=1).contiguous()

    xe = x.clone().requires_grad_(True)
    pe = p_enc.clone().requires_grad_(True)
    pn = p_net.clone().requires_grad_(True)
    ectx, e = e_nat.fwd(xe, pe)
    ef = padded(e).requires_grad_(True)
    nctx, y = n_nat.fwd(ef, pn)
    g_e, _ = n_nat.bwd(nctx, ef, pn, y, dy)                                                              # 1. dL/de
    g_e = g_e[:, :w].half().contiguous()
    t, ge_params, dx_a = e_nat.bwd_bwd_input(ectx, xe, pe, v, g_e.requires_grad_(True))                  # 2. t = J v, Hessian terms
    ddy, gn_params, q = n_nat.bwd_bwd_input(nctx, ef, pn, padded(t), dy.clone().requires_grad_(True))    # 3. the network
    dx_b, ge_more = e_nat.bwd(ectx, xe, pe, e, q[:, :w].half().contiguous())                             # 4. q through the encoding
    untouched = (ge_params == 0) & (ge_more == 0)  # (a zero of the sum elsewhere is two terms that cancel, not an untouched parameter)
    return ddy, gn_params, ge_params.float() + ge_more.float(), untouched, dx_a + dx_b, bool(q.any())


@gpu
@pytest.mark.parametrize("enc_cfg,act", [(GRID, "Softplus"), (GRID, "ReLU"), (PPNG3, "Softplus")], ids=["grid_softplus", "grid_relu", "ppng3_softplus"])
def test_composition_matches_hand_assembled_pipeline(tcnn, enc_cfg, act):
    import torch

    torch.manual_seed(3)
    n, n_in, n_out = 1024, 3, 1
    net_cfg = _net_cfg(64, 2, act)
    model = tcnn.NetworkWithInputEncoding(n_in, n_out, enc_cfg, net_cfg)
    native = model.native_tcnn_module
    n_net = 16 * 64 + 64 * 64 + 64 * 16
    n_enc = native.n_params() - n_net
    p_net = ((torch.rand(n_net, device="cuda") * 2 - 1) * 0.25).half()
    p_enc = ((torch.rand(n_enc, device="cuda") * 2 - 1) * (1.0 if enc_cfg is GRID else 0.1)).half()
    x = torch.rand(n, n_in, device="cuda") * 0.96 + 0.02
    v = torch.rand(n, n_in, device="cuda") * 2 - 1
    dy = ((torch.rand(n, 16, device="cuda") * 2 - 1) * (LOSS_SCALE / n)).half()

    xt = x.clone().requires_grad_(True)
    pt = torch.cat([p_net, p_enc]).requires_grad_(True)
    ctx, _ = native.fwd(xt, pt)
    ddy, dparams, dx = native.bwd_bwd_input(ctx, xt, pt, v, dy.clone().requires_grad_(True))

    want_ddy, want_net, want_enc, untouched, want_dx, curved = _composed_by_hand(tcnn, enc_cfg, net_cfg, n_in, n_out, x, v, dy, p_net, p_enc)
    assert curved == (act == "Softplus")
    assert torch.equal(ddy.view(torch.int16), want_ddy.view(torch.int16))
    assert torch.equal(dx.view(torch.int32), want_dx.view(torch.int32))
    assert torch.equal(dparams[:n_net].view(torch.int16), want_net.view(torch.int16))
    got_enc = dparams[n_net:].float()
    err, norm = float(torch.linalg.norm(got_enc - want_enc)), float(torch.linalg.norm(want_enc))
    print(f"encoding slice: |ours - composed| / |composed| = {err / norm:.3e}")
    assert norm > 0 and err <= 2e-2 * norm  # the bound of test_native_second_order_matches_oracle (packed-fp16 atomics)
    print(f"parameters no sample touches: {int(untouched.sum())} of {untouched.numel()}; nonzero there: {int((got_enc[untouched] != 0).sum())}; "
          f"composed terms cancel exactly: {int(((want_enc == 0) & ~untouched).sum())}")
    assert bool((got_enc[untouched] == 0).all())  # zeros sit where the composed one has zeros
    assert float(dx.abs().sum()) > 0 and float(ddy.float().abs().sum()) > 0


@gpu
def test_identity_network_against_hand_padded_tangent(tcnn):
    """tcnn.Network on 24 inputs (an Identity encoding that pads to 32 with ones): the padding columns carry a zero tangent and
    the results are those of the restatement on the padded input"""
    import torch

    n, n_in, width, hidden, n_out, act = 1024, 24, 64, 2, 3, "Softplus"
    Ws, x, v, dy = _case_tensors(n, 32, width, hidden, n_out, act, seed=21)
    x[:, n_in:] = 1.0  # what the encoding pads with
    v[:, n_in:] = 0.0  # ... whose derivative is zero
    net = tcnn.Network(n_in, n_out, _net_cfg(width, hidden, act))
    native = net.native_tcnn_module
    xt = x[:, :n_in].float().contiguous().cuda().requires_grad_(True)
    pt = _flat_params(Ws).requires_grad_(True)
    ctx, _ = native.fwd(xt, pt)
    ddy, dparams, dx = native.bwd_bwd_input(ctx, xt, pt, v[:, :n_in].float().contiguous().cuda(), dy.cuda().requires_grad_(True))
    padded_dx = torch.zeros(n, 32)
    padded_dx[:, :n_in] = dx.cpu()
    want = _restate(Ws, _acts(hidden, act, "None"), x, dy, v, half=False)
    padded_dx[:, n_in:] = want[2][:, n_in:].float()  # the model has no input there: nothing to compare
    _check_against_restatements(("identity_24", 32, width, hidden, n_out, act, "None"), (Ws, x, v, dy), (ddy, dparams, padded_dx))


# ---------------------------------------------------------------------------------------------------- 3. gradient modes through the C ABI
def _bbi_mode(tcnn, native, ctx, x, params, v, dy, grads, mode):
    import torch

    from tinycudann import _C

    n = x.shape[0]
    ddy = torch.zeros((n, native.n_output_dims()), dtype=torch.half, device="cuda")
    dx = torch.zeros_like(x)
    _C.check(_C.lib.tcnn_module_backward_backward_input_mode(native._h, torch.cuda.current_stream().cuda_stream, ctx._h, n, v.data_ptr(), x.data_ptr(), dy.data_ptr(),
                                                             grads.data_ptr(), ddy.data_ptr(), dx.data_ptr(), params.data_ptr(), ctypes.c_int(mode)))
    torch.cuda.synchronize()
    return ddy, dx


@gpu
@pytest.mark.parametrize("act", ["Softplus", "ReLU"])
def test_gradient_modes_through_c_abi(tcnn, act):
    """Overwrite ignores what the gradient buffer holds; Accumulate twice doubles the gradient within half rounding -- for the whole
    parameter vector of a model with a grid in front"""
    import torch

    from tinycudann.native import GRADIENT_ACCUMULATE, GRADIENT_OVERWRITE

    torch.manual_seed(7)
    n = 1024
    model = tcnn.NetworkWithInputEncoding(3, 1, GRID, _net_cfg(64, 2, act))
    native = model.native_tcnn_module
    params = ((torch.rand(native.n_params(), device="cuda") * 2 - 1) * 0.25).half()
    x = (torch.rand(n, 3, device="cuda") * 0.96 + 0.02).requires_grad_(True)
    v = torch.rand(n, 3, device="cuda") * 2 - 1
    dy = ((torch.rand(n, 16, device="cuda") * 2 - 1) * (LOSS_SCALE / n)).half()
    ctx, _ = native.fwd(x, params.clone().requires_grad_(True))

    clean = torch.zeros_like(params)
    ddy, dx = _bbi_mode(tcnn, native, ctx, x, params, v, dy, clean, GRADIENT_OVERWRITE)
    poisoned = torch.full_like(params, 777.0)
    ddy2, dx2 = _bbi_mode(tcnn, native, ctx, x, params, v, dy, poisoned, GRADIENT_OVERWRITE)
    n_net = 16 * 64 + 64 * 64 + 64 * 16
    assert torch.equal(poisoned[:n_net].view(torch.int16), clean[:n_net].view(torch.int16))  # the network's slice: no atomics
    err = float(torch.linalg.norm(poisoned.float() - clean.float()))
    assert err <= 2e-2 * float(torch.linalg.norm(clean.float())) and float(poisoned.float().abs().max()) < 700
    assert torch.equal(ddy2, ddy) and torch.equal(dx2, dx)

    twice = torch.zeros_like(params)
    _bbi_mode(tcnn, native, ctx, x, params, v, dy, twice, GRADIENT_ACCUMULATE)
    once = twice.clone()
    _bbi_mode(tcnn, native, ctx, x, params, v, dy, twice, GRADIENT_ACCUMULATE)
    assert float(torch.linalg.norm(once.float() - clean.float())) <= 2e-2 * float(torch.linalg.norm(clean.float()))
    # doubling is exact in half; what is left is one rounding per addition (2^-11 relative) and the grid's atomics (2e-2 in norm)
    assert float(torch.linalg.norm(twice[:n_net].float() - 2 * clean[:n_net].float())) <= 2.0 ** -9 * float(torch.linalg.norm(2 * clean[:n_net].float()))
    assert float(torch.linalg.norm(twice.float() - 2 * clean.float())) <= 2e-2 * float(torch.linalg.norm(2 * clean.float()))


# ---------------------------------------------------------------------------------------------------- 4. through PyTorch
@gpu
def test_network_double_backward_through_torch(tcnn):
    """The eikonal pattern on tcnn.Network(32 -> 1, CutlassMLP 64 x 3 Softplus) against torch.nn MLPs with the same half-rounded
    weights in fp32 (autograd; R64's role) and the restated recipe rounding to half where the kernels store (Rh's role).  Gradients
    of the eikonal loss with respect to x and every weight matrix: ||ours - ref|| <= 2 ||Rh - ref||."""
    import torch

    torch.manual_seed(0)
    n, n_in, width, hidden = 1024, 32, 64, 3
    net = tcnn.Network(n_in, 1, _net_cfg(width, hidden, "Softplus"))
    Ws, x0, _, _ = _case_tensors(n, n_in, width, hidden, 1, "Softplus", seed=31)
    with torch.no_grad():
        net.params.copy_(_flat_params(Ws).float())
    acts = _acts(hidden, "Softplus", "None")

    x = x0.float().cuda().requires_grad_(True)
    y = net(x)
    (g,) = torch.autograd.grad(y.float().sum(), x, create_graph=True)
    loss = ((g.norm(dim=1) - 1) ** 2).mean()
    loss.backward()
    got_x = x.grad.cpu().double()
    got_W, off = [], 0
    for W in Ws:
        got_W.append(net.params.grad[off:off + W.numel()].reshape(W.shape).cpu().double())
        off += W.numel()

    # the reference: a torch.nn fp32 MLP with the same half-rounded weights, differentiated by autograd
    layers = [torch.nn.Linear(W.shape[1], W.shape[0], bias=False) for W in Ws]
    with torch.no_grad():
        for layer, W in zip(layers, Ws):
            layer.weight.copy_(W.float())
    xr = x0.float().requires_grad_(True)
    hr = xr
    for layer, a in zip(layers, acts):
        hr = _act(a, layer(hr))
    (gr,) = torch.autograd.grad(hr[:, 0].sum(), xr, create_graph=True)
    ((gr.norm(dim=1) - 1) ** 2).mean().backward()
    ref_x, ref_W = xr.grad.double(), [layer.weight.grad.double() for layer in layers]

    def eikonal_rounded():
        # Rh's role: the same computation from the restated recipe in fp32, rounded to half where the kernels store.  dL/dy is the
        # loss scale (what the binding hands to the kernels), v = d loss / d g
        dt = torch.float32
        dy = torch.zeros(n, 16, dtype=dt)
        dy[:, 0] = LOSS_SCALE
        Wd = [W.to(dt) for W in Ws]
        rh = lambda t: t.half().to(dt)  # noqa: E731
        h, zs = [x0.to(dt)], []
        for W, a in zip(Wd, acts):
            zs.append(rh(h[-1] @ W.T))
            h.append(rh(_act(a, zs[-1])))
        d = dy
        for k in range(len(Wd) - 1, -1, -1):
            gk = d if k == len(Wd) - 1 else rh(d @ Wd[k + 1])
            d = gk if acts[k] == "None" else rh(gk * _d1(acts[k], zs[k]))
        grad_x = rh(d @ Wd[0]) / LOSS_SCALE  # the first-order result, as the binding returns it
        norm = grad_x.norm(dim=1, keepdim=True)
        v = 2 * (norm - 1) / n * grad_x / norm
        _, dW, dx = _restate(Ws, acts, x0, dy.half(), v.half(), True)
        return dx.double() / LOSS_SCALE, [w.double() / LOSS_SCALE for w in dW]

    rh_x, rh_W = eikonal_rounded()
    failures = []
    for what, ours, h, ref in [("x", got_x, rh_x, ref_x)] + [(f"W{k}", got_W[k], rh_W[k], ref_W[k]) for k in range(len(Ws))]:
        e_ours, e_h = float(torch.linalg.norm(ours - ref)), float(torch.linalg.norm(h - ref))
        print(f"eikonal through torch: d loss / d {what}: |ours-ref|/|ref| {e_ours / float(torch.linalg.norm(ref)):.3e}  |Rh-ref|/|ref| {e_h / float(torch.linalg.norm(ref)):.3e}")
        if not e_ours <= 2 * e_h:
            failures.append((what, e_ours, e_h))
    assert not failures, failures


@gpu
def test_sdf_fit_with_eikonal_term(tcnn):
    """HashGrid -> CutlassMLP 64 x 2 Softplus fitted to a sphere's signed distance plus an eikonal term with Adam: every loss finite,
    and | |grad f| - 1 | over a fixed probe set lower at the end than at the start (a sanity condition, not a measurement)"""
    import torch

    torch.manual_seed(0)
    enc = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 4, "per_level_scale": 1.5, "interpolation": "Smoothstep"}
    model = tcnn.NetworkWithInputEncoding(3, 1, enc, _net_cfg(64, 2, "Softplus"))
    opt = torch.optim.Adam(model.parameters(), lr=2e-3, eps=1e-15)
    probe = torch.rand(4096, 3, device="cuda") * 0.9 + 0.05

    def eikonal_error(points):
        p = points.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(model(p).float().sum(), p, create_graph=True)
        return g, (g.norm(dim=1) - 1).abs().mean().detach()

    before = float(eikonal_error(probe)[1])
    for step in range(300):
        pts = torch.rand(4096, 3, device="cuda") * 0.9 + 0.05
        sdf = (pts - 0.5).norm(dim=1) - 0.3
        p = pts.clone().requires_grad_(True)
        f = model(p).float()[:, 0]
        (g,) = torch.autograd.grad(f.sum(), p, create_graph=True)
        loss = ((f - sdf) ** 2).mean() + 0.1 * ((g.norm(dim=1) - 1) ** 2).mean()
        assert bool(torch.isfinite(loss)), (step, float(loss))
        opt.zero_grad()
        loss.backward()
        opt.step()
    after = float(eikonal_error(probe)[1])
    print(f"mean | |grad f| - 1 | over the probe set: {before:.4f} before, {after:.4f} after 300 steps")
    assert after < before


# ---------------------------------------------------------------------------------------------------- 5. boundaries
@gpu
def test_unsupported_modules_still_raise_and_leave_the_module_usable(tcnn):
    import torch

    x3 = (torch.rand(256, 3, device="cuda") * 0.9 + 0.05).requires_grad_(True)
    for enc_cfg, net_cfg in ((GRID, _net_cfg(64, 2, "ReLU", otype="FullyFusedMLP")), ({"otype": "OneBlob", "n_bins": 16}, _net_cfg(64, 2, "Softplus"))):
        model = tcnn.NetworkWithInputEncoding(3, 1, enc_cfg, net_cfg)
        native = model.native_tcnn_module
        p = model.params.detach().half().requires_grad_(True)
        ctx, out = native.fwd(x3, p)
        with pytest.raises(RuntimeError, match="backward_backward_input_impl: not implemented error"):
            native.bwd_bwd_input(ctx, x3, p, torch.rand_like(x3), torch.rand_like(out).requires_grad_(True))

    # a rejected call (a context made without input gradients) leaves the module as it was: the next valid call is right
    case = NETWORK_CASES[2]
    n = 4096
    _, n_in, width, hidden, n_out, act, out_act = case
    Ws, x, v, dy = _case_tensors(n, n_in, width, hidden, n_out, act, 11)
    net = tcnn.Network(n_in, n_out, _net_cfg(width, hidden, act, out_act))
    native = net.native_tcnn_module
    xt = x.float().cuda()
    pt = _flat_params(Ws).requires_grad_(True)
    dyt = dy.cuda().requires_grad_(True)
    ctx_no_input, _ = native.fwd(xt, pt)  # the input does not require a gradient: no input gradients prepared
    with pytest.raises(RuntimeError, match="input gradients were not prepared"):
        native.bwd_bwd_input(ctx_no_input, xt.clone().requires_grad_(True), pt, v.float().cuda(), dyt)
    xg = xt.clone().requires_grad_(True)
    ctx, _ = native.fwd(xg, pt)
    _check_against_restatements(case, (Ws, x, v, dy), native.bwd_bwd_input(ctx, xg, pt, v.float().cuda(), dyt))
