"""BatchedMLP on the GPU (tiny-cuda-nn_amd/csrc/k_mlp_batched.hip) through the C ABI: every network against grad_checks.float64_step on its own
rows and weights, bit for bit against a one-network module on that segment alone, Accumulate after Overwrite, rows that nobody owns; then
the same through tcnn.Network and autograd.  Bars: the suite's own (outputs and dL/dinput |a - b| <= 1e-2 |b| + 1e-3 max|b|; weight
gradients assert_weight_grads_close(rtol=3e-2, half_stored=True))."""
import ctypes as C

import numpy as np
import pytest

import grad_checks as gc

pytestmark = pytest.mark.gpu

# name, K, n_in, width, n_out, hidden layers, activation, output activation, n, segment lengths (None: the equal split, no offsets)
CASES = [
    ("empty_and_ragged", 3, 3, 16, 1, 1, "ReLU", "None", 256, (37, 0, 219)),
    ("five_uneven", 5, 32, 64, 16, 3, "LeakyReLU", "None", 512, (16, 1, 255, 64, 176)),
    ("padded_io_equal_split", 2, 20, 32, 17, 2, "None", "Sigmoid", 512, None),
    ("rows_nobody_owns", 4, 8, 32, 4, 1, "ReLU", "None", 512, (100, 50, 0, 150)),
    ("several_chunks_per_network", 2, 16, 16, 16, 1, "ReLU", "None", 8192, None),  # 8 chunks each: S = 8 workgroups and k_bmlp_reduce
]


def _module(K, n_in, width, n_out, hidden, act, oact):
    from tinycudann import _C, modules

    net = {"otype": "BatchedMLP", "n_networks": K, "n_neurons": width, "n_hidden_layers": hidden, "activation": act, "output_activation": oact}
    return modules._create(_C.lib.tcnn_create_network, n_in, n_out, _C.to_json_bytes(net))


def _passes(native, x, params, dy, offsets, sentinel=None):
    """(output, dL/dinput, gradients under Overwrite, gradients after Accumulate on top) of one forward and two backward calls;
    sentinel = (slice, value): written into the Overwrite result before the Accumulate call"""
    import torch
    from tinycudann import _C, modules

    L, n = _C.lib, x.shape[0]
    native.set_network_offsets(offsets)
    out, inferred = (torch.full((n, native.n_output_dims()), float("nan"), dtype=torch.half, device="cuda") for _ in range(2))
    h = C.c_void_p()
    _C.check(L.tcnn_module_forward(native._h, None, n, x.data_ptr(), out.data_ptr(), params.data_ptr(), 1, C.byref(h)))
    ctx = modules.NativeContext(h)
    _C.check(L.tcnn_module_inference(native._h, None, n, x.data_ptr(), inferred.data_ptr(), params.data_ptr()))
    dx = torch.full((n, native.n_input_dims()), float("nan"), device="cuda")
    grads = torch.full_like(params, float("nan"))
    args = (native._h, None, ctx._h, n, dx.data_ptr(), dy.data_ptr(), grads.data_ptr(), x.data_ptr(), out.data_ptr(), params.data_ptr())
    _C.check(L.tcnn_module_backward_mode(*args, 1))
    first = grads.clone()
    if sentinel:
        grads[sentinel[0]] = sentinel[1]
    _C.check(L.tcnn_module_backward_mode(*args, 2))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), inferred.view(torch.int16))
    return out, dx, first, grads


def _bits(t):
    import torch

    return t.contiguous().view(torch.int16 if t.dtype == torch.half else torch.int32)


def _close(got, want, what):
    bound = 1e-2 * np.abs(want) + 1e-3 * np.max(np.abs(want))
    assert np.all(np.abs(got - want) <= bound), f"{what}: worst {np.max(np.abs(got - want) - bound):.3g} over the bar"


@pytest.mark.parametrize("name,K,n_in,width,n_out,hidden,act,oact,n,lengths", CASES, ids=[c[0] for c in CASES])
def test_every_network_on_its_rows(tcnn, name, K, n_in, width, n_out, hidden, act, oact, n, lengths):
    import torch

    native = _module(K, n_in, width, n_out, hidden, act, oact)
    single = _module(1, n_in, width, n_out, hidden, act, oact)
    P, in_w, out_w = single.n_params(), -(-n_in // 16) * 16, native.n_output_dims()
    sizes = [(width, in_w)] + [(width, width)] * (hidden - 1) + [(out_w, width)]
    slices, off = [], 0
    for r, c in sizes:
        slices.append((off, r, c))
        off += r * c
    assert off == P and native.n_params() == K * P
    bounds = np.concatenate([[0], np.cumsum(lengths)]) if lengths else np.arange(K + 1) * (n // K)
    offsets = torch.tensor(bounds, dtype=torch.int32, device="cuda") if lengths else None

    rng = np.random.default_rng(7)
    w = np.concatenate([rng.uniform(-1, 1, r * c) * np.sqrt(6.0 / (r + c)) for _ in range(K) for r, c in sizes]).astype(np.float16)
    x = rng.uniform(-1, 1, (n, n_in)).astype(np.float16).astype(np.float32)
    dy = (rng.uniform(-1, 1, (n, out_w)) / 8).astype(np.float16)
    params, xd, dyd = torch.tensor(w, device="cuda"), torch.tensor(x, device="cuda"), torch.tensor(dy, device="cuda")
    empty = [k for k in range(K) if bounds[k] == bounds[k + 1]]
    sentinel = (slice(empty[0] * P, (empty[0] + 1) * P), 3.0) if empty else None
    out, dx, first, second = _passes(native, xd, params, dyd, offsets, sentinel)

    # rows that nobody owns: +0 in the output and in dL/dinput
    assert not _bits(out[bounds[-1]:]).any() and not _bits(dx[bounds[-1]:]).any()
    for k in range(K):
        b, e = int(bounds[k]), int(bounds[k + 1])
        g1, g2 = first[k * P:(k + 1) * P], second[k * P:(k + 1) * P]
        if b == e:  # +0 under Overwrite, untouched under Accumulate
            assert not _bits(g1).any() and torch.all(g2 == 3.0)
            continue
        wk = w[k * P:(k + 1) * P]
        xp = np.ones((e - b, in_w))
        xp[:, :n_in] = x[b:e]
        ref = gc.float64_step(xp, wk, slices, act, oact, external_dL_dy=dy[b:e].astype(np.float64))
        _close(out[b:e].double().cpu().numpy(), ref["out"], f"{name}: output of network {k}")
        _close(dx[b:e].double().cpu().numpy(), ref["douts"][0] @ wk[:width * in_w].reshape(width, in_w).astype(np.float64)[:, :n_in], f"{name}: dL/dinput of network {k}")
        gc.assert_weight_grads_close(g1.cpu().numpy(), ref["grads"], slices, rtol=3e-2, half_stored=True, what=f"{name}: network {k}")
        gc.assert_structural_zeros(g1.cpu().numpy().view(np.uint16), ref["grads"], slices, what=f"{name}: network {k}")
        # Accumulate on top of Overwrite: (half)(first + sum) with first = (half)sum, so within one half step of twice the first
        twice = 2.0 * g1.double().cpu().numpy()
        assert np.all(np.abs(g2.double().cpu().numpy() - twice) <= np.spacing(np.abs(twice).astype(np.float16)).astype(np.float64))
        # the same bits as one network alone on this segment
        n1 = -(-(e - b) // 256) * 256
        x1, dy1 = torch.zeros((n1, n_in), device="cuda"), torch.zeros((n1, out_w), dtype=torch.half, device="cuda")
        x1[:e - b], dy1[:e - b] = xd[b:e], dyd[b:e]
        out1, dx1, grads1, _ = _passes(single, x1, params[k * P:(k + 1) * P].clone(), dy1, torch.tensor([0, e - b], dtype=torch.int32, device="cuda"))
        assert torch.equal(_bits(out1[:e - b]), _bits(out[b:e])) and torch.equal(_bits(dx1[:e - b]), _bits(dx[b:e])) and torch.equal(_bits(grads1), _bits(g1))


def test_initial_params_are_one_stream_of_cutlass_networks(tcnn):
    from tinycudann import _C, modules
    import torch

    one = modules._create(_C.lib.tcnn_create_network, 32, 16, _C.to_json_bytes({"otype": "CutlassMLP", "n_neurons": 64, "n_hidden_layers": 2}))
    assert torch.equal(_module(1, 20, 64, 16, 2, "ReLU", "None").initial_params(11), one.initial_params(11))
    three = _module(3, 20, 64, 16, 2, "ReLU", "None").initial_params(11)
    assert torch.equal(three[: one.n_params()], one.initial_params(11)) and not torch.equal(three[one.n_params(): 2 * one.n_params()], one.initial_params(11))


def test_autograd_through_tcnn_network(tcnn):
    import torch

    K, n_in, n_out, n = 3, 5, 3, 300
    net = {"otype": "BatchedMLP", "n_networks": K, "n_neurons": 32, "n_hidden_layers": 2, "activation": "ReLU", "output_activation": "None"}
    module = tcnn.Network(n_in, n_out, net, seed=3)
    offsets = torch.tensor([0, 100, 100, 300], dtype=torch.int32, device="cuda")
    module.set_network_offsets(offsets)
    x = (torch.rand((n, n_in), device="cuda") * 2 - 1).requires_grad_(True)
    weight = torch.rand((n, n_out), device="cuda") - 0.5
    y = module(x)
    (y.float() * weight).sum().backward()
    assert module.params.view(K, -1).shape[0] == K and y.shape == (n, n_out)

    xp, dyp = torch.zeros((512, n_in), device="cuda"), torch.zeros((512, 16), dtype=torch.half, device="cuda")
    xp[:n], dyp[:n, :n_out] = x.detach(), (weight * module.loss_scale).half()
    out, dx, grads, _ = _passes(module.native_tcnn_module, xp, module.params.detach().half(), dyp, offsets)
    assert torch.equal(y.detach(), out[:n, :n_out])
    assert torch.allclose(x.grad, dx[:n] / module.loss_scale, rtol=0, atol=2.0 ** -24)
    assert torch.allclose(module.params.grad, grads.float() / module.loss_scale, rtol=0, atol=2.0 ** -24)
    assert not module.params.grad.view(K, -1)[1].any() and module.params.grad.view(K, -1)[0].any()
