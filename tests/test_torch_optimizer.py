"""tcnn.optimizers.Optimizer: the library's optimizers as a torch.optim.Optimizer on the PyTorch modules."""
import numpy as np
import pytest

from test_optimizers import NESTED
from test_standalone_optimizer import ADAM, LOSS_SCALE

pytestmark = pytest.mark.gpu


def _model(tcnn, seed=1337):
    from test_gpu_parity import CONFIG_C3B

    return tcnn.NetworkWithInputEncoding(2, 3, CONFIG_C3B["encoding"], CONFIG_C3B["network"], seed=seed)


def _bits32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _half_exact_gradient(oracle, n, n_net, step):
    """fp32 gradients that are a half times 2^-7 (what a module's backward pass yields at loss scale 128), and the half itself"""
    import torch

    g = oracle.Pcg32(11 + step).uniform_strided(n, -4.0, 4.0)
    g[n_net + step::3] = 0.0
    g_h = torch.from_numpy(oracle.half_bits(g).view(np.float16)).cuda()
    return g_h.float() / LOSS_SCALE, g_h


def test_module_steps_equal_the_trainers_and_install_the_working_copy(tcnn, oracle):
    import torch
    from tinycudann import _C

    from test_gpu_parity import CONFIG_C3B, _bits

    model = _model(tcnn)
    layers = tcnn.optimizers.module_layer_sizes(model)
    ref_model = oracle.Trainer(2, 3, CONFIG_C3B, seed=1337).model
    assert layers == [tuple(ls) for ls in ref_model.network.layer_sizes()]
    n, n_net = model.params.numel(), sum(r * c for r, c in layers)
    assert n == ref_model.n_params
    assert model.reuse_working_copy is False
    opt = tcnn.optimizers.Optimizer(model, ADAM)
    assert model.reuse_working_copy is True and len(opt.param_groups) == 1 and abs(opt.param_groups[0]["lr"] - 1e-2) < 1e-9
    tr = tcnn.Trainer(2, 3, {**CONFIG_C3B, "optimizer": ADAM}, seed=1337)
    tr.set_params_full_precision(model.params.detach())
    p0 = _bits32(model.params).copy()
    for step in range(3):
        g, g_h = _half_exact_gradient(oracle, n, n_net, step)
        model.params.grad = g
        version = model.params._version
        opt.step()
        assert model.params._version == version + 1  # as an in-place torch update
        _C.memcpy_dtod(_C.lib.tcnn_trainer_param_gradients(tr._h), g_h.data_ptr(), n * 2)
        tr.optimizer_step(LOSS_SCALE)
    got = _bits32(model.params)
    assert np.array_equal(got, _bits32(tr.params_full_precision())) and not np.array_equal(got, p0)
    assert opt.native(model).step_count() == 3
    # the working copy: the half weights the step wrote, equal to the trainer's and to params.half(); the tensor the next forward reads
    working = model._working_copy
    assert working is opt._half[0] and working.dtype == torch.half
    assert np.array_equal(_bits(working), _bits(tr.params())) and torch.equal(working, model.params.detach().half())
    seen = []
    native_fwd = model.native_tcnn_module.fwd
    model.native_tcnn_module.fwd = lambda input, params: (seen.append(params.data_ptr()), native_fwd(input, params))[1]
    x = torch.rand(256, 2, device="cuda")
    y = model(x)
    assert seen == [working.data_ptr()] and model._working_copy is working, "the forward pass cast the parameters again"
    # and it is what a cast of the parameters gives
    model.invalidate_working_copy()
    assert torch.equal(model(x), y) and seen[1] != seen[0]


def test_training_converges_and_leaves_untouched_entries_alone(tcnn, oracle):
    """L2 on oracle.synthetic_batch through the module and its own loss.  Grid entries no sample ever touched (zero gradient in
    every step) keep their initial bits.  torch.optim.Adam keeps those too -- their moments are zero -- so the difference in
    semantics is shown where it exists: entries that had a gradient in the step before and none in this one stay where they are
    under the library's Adam (adam.h:76-84) and are moved by their momentum under torch.optim.Adam, fed the same gradients."""
    import torch

    model = _model(tcnn)
    n_net = sum(r * c for r, c in tcnn.optimizers.module_layer_sizes(model))
    opt = tcnn.optimizers.Optimizer(model, ADAM)
    twin = torch.nn.Parameter(model.params.detach().clone())
    twin_opt = torch.optim.Adam([twin], lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    initial = _bits32(model.params).copy()
    batches = [tuple(torch.from_numpy(a).cuda() for a in oracle.synthetic_batch(1024, 2, 3, seed=100 + s)) for s in range(8)]
    hit = torch.zeros_like(model.params, dtype=torch.bool)
    losses, steps = [], 200
    for step in range(steps):
        x, t = batches[step % len(batches)]
        loss = (model(x).float() - t).square().mean()
        opt.zero_grad()
        loss.backward()
        g = model.params.grad
        nonzero = g != 0
        if step == steps - 1:
            before, twin_before = model.params.detach().clone(), twin.detach().clone()
            stale = ~nonzero & previous
            stale[:n_net] = False
        hit |= nonzero
        previous = nonzero
        twin.grad = g.clone()
        opt.step()
        twin_opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)), losses
    print(f"loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] < losses[0]
    never = ~hit
    never[:n_net] = False
    assert int(never.sum()) > 1000 and int(stale.sum()) > 1000, (int(never.sum()), int(stale.sum()))
    never, stale = never.cpu().numpy(), stale.cpu().numpy()
    final = _bits32(model.params)
    print(f"never hit: {never.sum()}, stale: {stale.sum()}, moved by torch.optim.Adam among the stale: {np.count_nonzero(_bits32(twin)[stale] != _bits32(twin_before)[stale])}")  # measured: 251444, 72055, 72054
    assert np.array_equal(final[never], initial[never])
    assert np.array_equal(_bits32(twin)[never], initial[never])  # zero moments: torch.optim.Adam does not move them either
    assert np.array_equal(final[stale], _bits32(before)[stale])
    # torch.optim.Adam's step for an entry is lr m^ / (sqrt(v^) + eps) whatever its gradient: it shows wherever it is at least one
    # spacing of the fp32 weight (a smaller one may round away)
    state = twin_opt.state[twin]
    t = float(state["step"])
    update = 1e-2 * (state["exp_avg"] / (1 - 0.9 ** t)) / ((state["exp_avg_sq"] / (1 - 0.99 ** t)).sqrt() + 1e-15)
    must_move = stale & (np.abs(update.cpu().numpy()) >= np.spacing(np.abs(twin_before.cpu().numpy())))
    assert must_move.sum() > 1000
    assert np.all(_bits32(twin)[must_move] != _bits32(twin_before)[must_move])


def test_checkpoint_resumes_bitwise(tcnn, oracle):
    import torch

    from test_gpu_parity import _bits

    model = _model(tcnn)
    n = model.params.numel()
    n_net = sum(r * c for r, c in tcnn.optimizers.module_layer_sizes(model))
    opt = tcnn.optimizers.Optimizer(model, NESTED)
    for step in range(3):
        model.params.grad = _half_exact_gradient(oracle, n, n_net, step)[0]
        opt.step()
    state, weights = opt.state_dict(), {k: v.clone() for k, v in model.state_dict().items()}
    assert state["native_state"][0].dtype == torch.uint8 and len(state["param_groups"]) == 1
    other = _model(tcnn, seed=7)
    other_opt = tcnn.optimizers.Optimizer(other, NESTED)
    other.load_state_dict(weights)
    other_opt.load_state_dict(state)
    assert other_opt.native(0).step_count() == 3
    assert np.array_equal(_bits(other_opt.inference_params(other)), _bits(opt.inference_params(model)))
    for step in (3, 4):
        for m, o in ((model, opt), (other, other_opt)):
            m.params.grad = _half_exact_gradient(oracle, n, n_net, step)[0]
            o.step()
    assert np.array_equal(_bits32(other.params), _bits32(model.params))
    assert np.array_equal(_bits(other._working_copy), _bits(model._working_copy))
    assert np.array_equal(_bits(other_opt.inference_params(other)), _bits(opt.inference_params(model)))
    assert other_opt.native(0).learning_rate() == opt.native(0).learning_rate()  # the decayed rate (ExponentialDecay), not reset by the restore


def test_lr_scheduler_reaches_the_native_optimizer(tcnn):
    import torch

    model = _model(tcnn)
    opt = tcnn.optimizers.Optimizer(model, ADAM)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    before = model.params.detach().clone()
    model.params.grad = torch.ones_like(model.params)
    opt.step()
    first = (model.params.detach() - before).abs().max().item()
    sched.step()
    assert abs(opt.param_groups[0]["lr"] - 5e-3) < 1e-9
    before = model.params.detach().clone()
    opt.step()
    second = (model.params.detach() - before).abs().max().item()
    assert abs(opt.native(0).learning_rate() - 5e-3) < 1e-9
    # Adam's steps on a constant gradient have the size of the learning rate
    assert abs(first - 1e-2) < 1e-4 and abs(second - 5e-3) < 1e-4, (first, second)


def test_missing_and_half_gradients(tcnn, oracle):
    import torch

    a, b = _model(tcnn, seed=1), _model(tcnn, seed=2)
    opt = tcnn.optimizers.Optimizer([a, b], [ADAM, {"otype": "SGD", "learning_rate": 1e-1, "l2_reg": 0.0}])
    assert [g["lr"] for g in opt.param_groups] == [pytest.approx(1e-2), pytest.approx(1e-1)]
    n = a.params.numel()
    n_net = sum(r * c for r, c in tcnn.optimizers.module_layer_sizes(a))
    g, g_h = _half_exact_gradient(oracle, n, n_net, 0)
    a0, b0 = a.params.detach().clone(), b.params.detach().clone()
    b.params.grad_dtype = torch.float16
    b.params.grad = g_h / LOSS_SCALE  # a half gradient (exact: a power of two), module a has none
    opt.step()
    assert torch.equal(a.params.detach(), a0) and opt.native(a).step_count() == 0 and a._working_copy is None
    assert opt.native(b).step_count() == 1
    assert torch.equal(b.params.detach(), b0 - 0.1 * (g_h / LOSS_SCALE).float())  # SGD, sgd.h:44-72: one rounding per operation
    # a non-contiguous fp32 gradient is made contiguous
    wide = torch.zeros(n, 2, device="cuda")
    wide[:, 0] = g
    a.params.grad = wide[:, 0]
    assert not a.params.grad.is_contiguous()
    opt.step()
    assert opt.native(a).step_count() == 1 and not torch.equal(a.params.detach(), a0)


def test_writes_by_other_means_invalidate_the_working_copy(tcnn, oracle):
    import torch

    from test_gpu_parity import _bits

    model = _model(tcnn)
    n = model.params.numel()
    n_net = sum(r * c for r, c in tcnn.optimizers.module_layer_sizes(model))
    opt = tcnn.optimizers.Optimizer(model, NESTED)
    model.params.grad = _half_exact_gradient(oracle, n, n_net, 0)[0]
    opt.step()
    stale = model._working_copy
    x = torch.rand(256, 2, device="cuda")
    y_old = model(x)
    fresh = _model(tcnn, seed=99)
    model.load_state_dict(fresh.state_dict())
    y_new = model(x)
    assert model._working_copy is not stale and torch.equal(model._working_copy, fresh.params.detach().half())
    assert torch.equal(y_new, fresh(x)) and not torch.equal(y_new, y_old)
    # the next step starts from the loaded weights, in fp32 and in half
    model.params.grad = torch.zeros_like(model.params)
    opt.step()
    assert torch.equal(model.params.detach()[n_net:], fresh.params.detach()[n_net:])  # zero gradient: grid entries stay
    assert np.array_equal(_bits(model._working_copy)[n_net:], _bits(fresh.params.detach().half())[n_net:])
    assert model._working_copy is opt._half[0]


def test_rejections(tcnn):
    import torch

    enc = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 4, "per_level_scale": 2.0}
    with pytest.raises(TypeError, match="torch.optim"):
        tcnn.optimizers.Optimizer(tcnn.Encoding(2, enc, dtype=torch.float32), ADAM)
    with pytest.raises(TypeError, match="not Linear"):
        tcnn.optimizers.Optimizer(torch.nn.Linear(4, 4), ADAM)
    with pytest.raises(RuntimeError, match="Invalid optimizer type: Shampoo"):
        tcnn.optimizers.Optimizer(tcnn.Encoding(2, enc), {"otype": "Shampoo"})
    half = tcnn.Encoding(2, enc)
    opt = tcnn.optimizers.Optimizer(half, ADAM)  # an encoding alone: no matrix weights
    assert tcnn.optimizers.module_layer_sizes(half) == [] and opt.inference_params(half) is None


def test_write_through_data_and_invalidate_reaches_the_optimizer(tcnn, oracle):
    """A write through `params.data` shows in no version counter; the documented remedy, `invalidate_working_copy()`, must also make
    the optimizer take its half weights from the parameter again: its step stores half weights for updated parameters only, so
    grid entries without a gradient would otherwise keep their value from before the write, in the copy the next forward reads."""
    import torch

    from test_gpu_parity import _bits
    from test_optimizers import _composite

    model = _model(tcnn)
    n = model.params.numel()
    n_net = sum(r * c for r, c in tcnn.optimizers.module_layer_sizes(model))
    opt = tcnn.optimizers.Optimizer(model, _composite(n_net, n - n_net))  # SGD on the network, Ema -> Adam on the grid: custom weights assembled from both
    x = torch.rand(256, 2, device="cuda")
    grad = torch.zeros(n, device="cuda")
    grad[:n_net] = 1.0  # the grid part: zero gradient, nothing stored for it by the step
    for seed, forward_in_between in ((99, False), (98, True)):
        model.params.grad = _half_exact_gradient(oracle, n, n_net, 0)[0]
        opt.step()
        model(x)
        assert model._working_copy is opt._half[0]
        fresh = _model(tcnn, seed=seed)
        model.params.data.copy_(fresh.params.data)
        model.invalidate_working_copy()
        if forward_in_between:  # the module then has a copy of its own
            assert torch.equal(model(x), fresh(x))
        model.params.grad = grad.clone()
        opt.step()
        working = model._working_copy
        assert working is opt._half[0]
        assert torch.equal(model.params.detach()[n_net:], fresh.params.detach()[n_net:])
        assert np.array_equal(_bits(working), _bits(model.params.detach().half()))
        assert not torch.equal(model.params.detach()[:n_net], fresh.params.detach()[:n_net])
        custom = opt.inference_params(model)  # rebuilt from the new weights where the nested optimizer keeps none of its own
        assert np.array_equal(_bits(custom)[:n_net], _bits(working)[:n_net])


def test_backward_of_a_graph_from_before_the_step_raises(tcnn):
    """The step overwrites the half weights a forward pass saved for its backward pass: like after torch's own in-place updates, a
    later backward through that graph is an error, not a gradient at the new weights."""
    import torch

    model = _model(tcnn)
    opt = tcnn.optimizers.Optimizer(model, ADAM)
    x = torch.rand(256, 2, device="cuda")
    for _ in range(2):  # the second round: the graph saved the optimizer's own buffer
        opt.zero_grad()
        loss = model(x).float().square().mean()
        loss.backward(retain_graph=True)
        opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
