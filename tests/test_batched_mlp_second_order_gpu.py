"""BatchedMLP's second-order pass and tangent on the GPU (k_bmlp_tangent, k_bmlp_bwd2 in tiny-cuda-nn_amd/csrc/k_mlp_batched.hip) through the
C ABI: every network on its own rows against the restatements of tests/test_network_second_order.py (R64 in fp64, Rh in fp32 rounded to half
where the kernels store a matrix) under that file's bar, ||ours - R64|| <= 2 ||Rh - R64||; the bit-level contracts of the first-order pass
(a one-network module on the segment alone, two runs, Accumulate, empty networks, rows nobody owns); input_jvp against the second-order
call's dL_ddLdoutput; and an eikonal-style loss through tcnn.Network and autograd."""
import ctypes as C

import pytest

from test_batched_mlp_gpu import _bits, _module
from test_network_second_order import _acts, _case_tensors, _curved, _restate

pytestmark = pytest.mark.gpu

# name, K, n_in, width, n_out, hidden layers, activation, output activation, n, segment lengths (None: the equal split, no offsets)
CASES = [
    ("relu_empty_and_ragged", 3, 3, 16, 1, 1, "ReLU", "None", 256, (37, 0, 219)),
    ("leaky_five_uneven", 5, 32, 64, 16, 3, "LeakyReLU", "None", 512, (16, 1, 255, 64, 176)),
    ("softplus_sigmoid_padded_io_equal_split", 2, 20, 32, 17, 2, "Softplus", "Sigmoid", 512, None),
    ("tanh_rows_nobody_owns", 4, 8, 32, 4, 1, "Tanh", "None", 512, (100, 50, 0, 150)),  # the last layer has no curvature: p starts one below
    ("relu_exponential_out", 2, 3, 64, 1, 2, "ReLU", "Exponential", 256, (70, 186)),  # p passes through layers without curvature
    ("softplus_several_chunks_per_network", 2, 16, 16, 16, 1, "Softplus", "None", 8192, None),  # 8 chunks each: k_bmlp_reduce
]


def _second_order(native, x, v, dy, params, offsets, sentinel=None):
    """(dL_ddLdoutput, dL_dinput, gradients under Overwrite, gradients after Accumulate on top) of one forward and three second-order
    calls: Overwrite, Overwrite again (the same bits), Accumulate.  sentinel = (slice, value): written before the Accumulate call"""
    import torch
    from tinycudann import _C, modules

    L, n = _C.lib, x.shape[0]
    native.set_network_offsets(offsets)
    out = torch.empty((n, native.n_output_dims()), dtype=torch.half, device="cuda")
    h = C.c_void_p()
    _C.check(L.tcnn_module_forward(native._h, None, n, x.data_ptr(), out.data_ptr(), params.data_ptr(), 1, C.byref(h)))
    ctx = modules.NativeContext(h)
    runs = []
    for mode in (1, 1, 2):  # TCNN_GRADIENT_OVERWRITE twice, then TCNN_GRADIENT_ACCUMULATE onto the second
        if mode == 1:
            ddy, dx, grads = torch.full_like(dy, float("nan")), torch.full_like(x, float("nan")), torch.full_like(params, float("nan"))
        elif sentinel:
            grads[sentinel[0]] = sentinel[1]
        _C.check(L.tcnn_module_backward_backward_input_mode(native._h, None, ctx._h, n, v.data_ptr(), x.data_ptr(), dy.data_ptr(), grads.data_ptr(), ddy.data_ptr(), dx.data_ptr(),
                                                            params.data_ptr(), mode))
        runs.append((ddy.clone(), dx.clone(), grads.clone()))
    torch.cuda.synchronize()
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(_bits(a), _bits(b))  # no atomics: two runs, the same bits
    assert torch.equal(_bits(runs[2][0]), _bits(runs[0][0])) and torch.equal(_bits(runs[2][1]), _bits(runs[0][1]))
    return runs[0][0], runs[0][1], runs[0][2], runs[2][2]


@pytest.mark.parametrize("name,K,n_in,width,n_out,hidden,act,oact,n,lengths", CASES, ids=[c[0] for c in CASES])
def test_every_network_on_its_rows(tcnn, name, K, n_in, width, n_out, hidden, act, oact, n, lengths):
    import numpy as np
    import torch

    native, single = _module(K, n_in, width, n_out, hidden, act, oact), _module(1, n_in, width, n_out, hidden, act, oact)
    P, in_w, out_w = single.n_params(), -(-n_in // 16) * 16, native.n_output_dims()
    bounds = np.concatenate([[0], np.cumsum(lengths)]) if lengths else np.arange(K + 1) * (n // K)
    offsets = torch.tensor(bounds, dtype=torch.int32, device="cuda") if lengths else None
    acts = _acts(hidden, act, oact)
    curved = any(_curved(a) for a in acts)

    # network k's tensors come from the restatements' own generator, on the padded width: x gets ones and v zeros in the padding
    per_net = [_case_tensors(max(int(bounds[k + 1] - bounds[k]), 1), in_w, width, hidden, n_out, act, seed=100 + k) for k in range(K)]
    x, v, dy = torch.rand(n, n_in) * 2 - 1, torch.rand(n, n_in) * 2 - 1, (torch.rand(n, out_w) / 8).half()  # (rows nobody owns: anything)
    for k, (Ws, xk, vk, dyk) in enumerate(per_net):
        b, e = int(bounds[k]), int(bounds[k + 1])
        xk[:, n_in:], vk[:, n_in:] = 1.0, 0.0
        x[b:e], v[b:e], dy[b:e] = xk[:e - b, :n_in].float(), vk[:e - b, :n_in].float(), dyk[:e - b]
    params = torch.cat([W.reshape(-1) for Ws, *_ in per_net for W in Ws]).cuda()
    assert params.numel() == K * P
    xd, vd, dyd = x.cuda(), v.cuda(), dy.cuda()
    empty = [k for k in range(K) if bounds[k] == bounds[k + 1]]
    sentinel = (slice(empty[0] * P, (empty[0] + 1) * P), 3.0) if empty else None
    ddy, dx, first, second = _second_order(native, xd, vd, dyd, params, offsets, sentinel)

    assert not _bits(ddy[bounds[-1]:]).any() and not _bits(dx[bounds[-1]:]).any()  # rows that nobody owns: +0
    if not curved:
        assert not _bits(dx).any()  # all bits zero: no curvature chain
    failures = []
    for k, (Ws, xk, vk, dyk) in enumerate(per_net):
        b, e = int(bounds[k]), int(bounds[k + 1])
        g1, g2 = first[k * P:(k + 1) * P], second[k * P:(k + 1) * P]
        if b == e:  # +0 under Overwrite, untouched under Accumulate
            assert not _bits(g1).any() and torch.all(g2 == 3.0)
            continue
        r64, rh = (_restate(Ws, acts, xk[:e - b], dyk[:e - b], vk[:e - b], half=half) for half in (False, True))
        ours_dW, off = [], 0
        for W in Ws:
            ours_dW.append(g1[off:off + W.numel()].reshape(W.shape))
            off += W.numel()
        triples = [("dL_ddLdoutput", ddy[b:e], rh[0], r64[0]), ("dL_dinput", dx[b:e], rh[2][:, :n_in], r64[2][:, :n_in])]
        triples += [(f"dL_dparams[{i}]", ours_dW[i], rh[1][i], r64[1][i]) for i in range(len(Ws))]
        for what, ours, h, ref in triples:
            ours, h = ours.cpu().double(), h.double()
            e_ours, e_h = float(torch.linalg.norm(ours - ref)), float(torch.linalg.norm(h - ref))
            print(f"{name} network {k} {what:16s} |ours-R64| {e_ours:.3e}  |Rh-R64| {e_h:.3e}  ratio {e_ours / e_h if e_h > 0 else 0.0:.3f}")
            if not e_ours <= 2 * e_h or not bool((ours[ref == 0] == 0).all()):
                failures.append((k, what, e_ours, e_h))
        # Accumulate on top of Overwrite: (half)(first + sum) with first = (half)sum, so within one half step of twice the first
        twice = 2.0 * g1.double().cpu().numpy()
        assert np.all(np.abs(g2.double().cpu().numpy() - twice) <= np.spacing(np.abs(twice).astype(np.float16)).astype(np.float64))
        # the same bits as one network alone on this segment
        n1 = -(-(e - b) // 256) * 256
        x1, v1, dy1 = torch.zeros((n1, n_in), device="cuda"), torch.zeros((n1, n_in), device="cuda"), torch.zeros((n1, out_w), dtype=torch.half, device="cuda")
        x1[:e - b], v1[:e - b], dy1[:e - b] = xd[b:e], vd[b:e], dyd[b:e]
        ddy1, dx1, grads1, _ = _second_order(single, x1, v1, dy1, params[k * P:(k + 1) * P].clone(), torch.tensor([0, e - b], dtype=torch.int32, device="cuda"))
        assert torch.equal(_bits(ddy1[:e - b]), _bits(ddy[b:e])) and torch.equal(_bits(dx1[:e - b]), _bits(dx[b:e])) and torch.equal(_bits(grads1), _bits(g1))
    assert not failures, failures


@pytest.mark.parametrize("T", [1, 3, 4])
def test_input_jvp_is_the_second_order_call_per_direction(tcnn, T):
    import torch

    K, n_in, n = 3, 3, 512
    native = _module(K, n_in, 32, 17, 2, "Softplus", "Sigmoid")
    native.set_network_offsets(torch.tensor([0, 100, 100, 400], dtype=torch.int32, device="cuda"))
    g = torch.Generator().manual_seed(T)
    x, tangents = (torch.rand(n, n_in, generator=g) * 2 - 1).cuda(), (torch.rand(n, T, n_in, generator=g) * 2 - 1).cuda()
    params = native.initial_params(5).half()
    dy = torch.zeros((n, native.n_output_dims()), dtype=torch.half, device="cuda").requires_grad_(True)
    jvp, output = native.input_jvp(x, params, tangents, True)
    assert native.last_input_jvp_route() == "k_bmlp_tangent"
    assert torch.equal(_bits(output), _bits(native.fwd(x, params)[1]))  # inference()'s bits
    ctx, _ = native.fwd(x.clone().requires_grad_(True), params)
    for t in range(T):
        ddy, _, _ = native.bwd_bwd_input(ctx, x, params, tangents[:, t].contiguous(), dy)
        assert torch.equal(_bits(jvp[:, t]), _bits(ddy))
    assert jvp[:400].float().abs().sum() > 0 and not _bits(jvp[400:]).any()


def test_eikonal_loss_through_tcnn_network(tcnn):
    import torch

    K, n_in, n = 3, 3, 300
    net = {"otype": "BatchedMLP", "n_networks": K, "n_neurons": 32, "n_hidden_layers": 2, "activation": "Softplus", "output_activation": "None"}
    module = tcnn.Network(n_in, 1, net, seed=3)
    offsets = torch.tensor([0, 100, 100, 300], dtype=torch.int32, device="cuda")
    module.set_network_offsets(offsets)
    x = (torch.rand((n, n_in), device="cuda") * 2 - 1).requires_grad_(True)
    y = module(x)
    (gx,) = torch.autograd.grad(y.float().sum(), x, create_graph=True)
    loss = ((gx.norm(dim=1) - 1) ** 2).sum()
    (v,) = torch.autograd.grad(loss, gx, retain_graph=True)
    loss.backward()

    native, scale = module.native_tcnn_module, module.loss_scale
    native.set_network_offsets(offsets)
    xp, vp, dyp = torch.zeros((512, n_in), device="cuda"), torch.zeros((512, n_in), device="cuda"), torch.zeros((512, 16), dtype=torch.half, device="cuda")
    xp[:n], vp[:n], dyp[:n, 0] = x.detach(), v, scale
    xp, params = xp.requires_grad_(True), module.params.detach().half().requires_grad_(True)
    ctx, _ = native.fwd(xp, params)
    _, dparams, dx = native.bwd_bwd_input(ctx, xp, params, vp, dyp)
    assert torch.allclose(x.grad, dx[:n] / scale, rtol=0, atol=2.0 ** -24) and x.grad.abs().sum() > 0
    assert torch.allclose(module.params.grad, dparams.float() / scale, rtol=0, atol=2.0 ** -24)
    assert not module.params.grad.view(K, -1)[1].any() and module.params.grad.view(K, -1)[0].any()

    module.zero_grad()
    x2 = x.detach().clone().requires_grad_(True)
    jvp = module.input_jvp(x2, torch.rand((n, 2, n_in), device="cuda"), differentiable=True)
    jvp.float().sum().backward()
    assert x2.grad.abs().sum() > 0 and module.params.grad.view(K, -1)[2].any() and not module.params.grad.view(K, -1)[1].any()
