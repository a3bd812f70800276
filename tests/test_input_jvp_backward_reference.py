"""The yardstick of tests/test_input_jvp_backward_gpu.py, pinned on the CPU: the fp64 restatement R64 of the reverse of a tangent pass
(input_jvp_backward_reference.recipe) equals torch.autograd through torch.func.jvp on an fp64 MLP -- every layer's weight gradient, dL/dx and
dL/dv -- to 1e-10 relative; the composed route's order of passes (input_jvp_backward_reference.composed) is the same quantity; and its
half-rounded form Rh stays within the guard the GPU criterion needs."""
import pytest

from input_jvp_backward_reference import composed, pass_terms, recipe
from test_network_second_order import _act, _acts, _case_tensors


def _cotangents(n, n_tangents, n_out, seed, scale=1.0):
    import torch

    g = torch.Generator().manual_seed(seed)
    ubar = ((torch.rand(n, n_tangents, n_out, generator=g) * 2 - 1) * scale).half()
    obar = ((torch.rand(n, n_out, generator=g) * 2 - 1) * scale).half()
    return ubar, obar


def _tensors(n, n_in, width, hidden, n_out, act, n_tangents, seed):
    import torch

    Ws, x, _, _ = _case_tensors(n, n_in, width, hidden, n_out, act, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    vs = (torch.rand(n, n_tangents, n_in, generator=g) * 2 - 1).half()
    ubar, obar = _cotangents(n, n_tangents, Ws[-1].shape[0], seed + 2000)
    return Ws, x, vs, ubar, obar


def _relative(a, b):
    import torch

    return float(torch.linalg.norm(a.double() - b.double())) / max(float(torch.linalg.norm(b.double())), 1e-300)


@pytest.mark.parametrize("with_output", [True, False])
@pytest.mark.parametrize("act,out_act", [("Softplus", "Sigmoid"), ("Tanh", "Softplus"), ("ReLU", "Tanh"), ("Softplus", "None")])
def test_recipe_matches_autograd_through_func_jvp(act, out_act, with_output):
    import torch

    n_tangents = 3
    Ws, x, vs, ubar, obar = _tensors(64, 16, 32, 2, 3, act, n_tangents, seed=5)
    acts = _acts(2, act, out_act)
    if not with_output:
        obar = None
    dW, dx, dv = recipe(Ws, acts, x, vs, ubar, obar)

    Wp = [W.double().requires_grad_(True) for W in Ws]
    xp = x.double().requires_grad_(True)
    vp = vs.double().requires_grad_(True)

    def f(inp):
        h = inp
        for W, a in zip(Wp, acts):
            h = _act(a, h @ W.T)
        return h

    loss = 0
    for t in range(n_tangents):
        out, jv = torch.func.jvp(f, (xp,), (vp[:, t],))
        loss = loss + (jv * ubar[:, t].double()).sum()
    if obar is not None:
        loss = loss + (out * obar.double()).sum()
    got = torch.autograd.grad(loss, [xp, vp] + Wp)
    assert _relative(dx, got[0]) <= 1e-10
    assert _relative(dv, got[1]) <= 1e-10
    for k in range(len(Ws)):
        assert _relative(dW[k], got[2 + k]) <= 1e-10, k
    if act == "ReLU" and out_act == "None":
        assert not dx.any()


@pytest.mark.parametrize("act,out_act", [("Softplus", "Sigmoid"), ("Tanh", "None"), ("ReLU", "None"), ("LeakyReLU", "Exponential")])
def test_composed_order_is_the_recipe(act, out_act):
    """the first-order pass of dL_doutput, then per tangent the second-order pass and a first-order pass: the same sums in fp64"""
    Ws, x, vs, ubar, obar = _tensors(64, 16, 32, 2, 3, act, 4, seed=7)
    acts = _acts(2, act, out_act)
    want = recipe(Ws, acts, x, vs, ubar, obar)
    got = composed(Ws, acts, x, vs, ubar, obar, half=False)
    terms = pass_terms(Ws, acts, x, vs, ubar, obar)
    assert len(terms) == 1 + 4 * (2 if act in ("Softplus", "Tanh") or out_act != "None" else 1)
    for k in range(len(Ws)):
        assert _relative(got[0][k], want[0][k]) <= 1e-10, k
        assert _relative(sum(term[k] for term in terms), want[0][k]) <= 1e-10, k  # the passes' terms add up to the whole
    assert _relative(got[1], want[1]) <= 1e-10 or (not want[1].any() and not got[1].any())
    assert _relative(got[2], want[2]) <= 1e-10


def test_piecewise_linear_networks_have_no_input_gradient_from_the_tangents():
    Ws, x, vs, ubar, _ = _tensors(64, 16, 32, 2, 3, "ReLU", 3, seed=9)
    for act in ("ReLU", "LeakyReLU", "None"):
        acts = _acts(2, act, "None")
        assert not recipe(Ws, acts, x, vs, ubar, None)[1].any()
        assert not composed(Ws, acts, x, vs, ubar, None, half=True)[1].any()


def test_half_restatement_is_the_fp64_one_up_to_half_rounding():
    """the guard of the GPU criterion, ||Rh - R64|| <= 0.05 ||R64||, on a representative shape"""
    Ws, x, vs, ubar, obar = _tensors(512, 32, 64, 2, 16, "Softplus", 3, seed=1)
    acts = _acts(2, "Softplus", "None")
    r64 = recipe(Ws, acts, x, vs, ubar, obar)
    rh = composed(Ws, acts, x, vs, ubar, obar, half=True)
    for k in range(len(Ws)):
        assert _relative(rh[0][k], r64[0][k]) <= 0.05, k
    assert _relative(rh[1], r64[1]) <= 0.05
    assert _relative(rh[2], r64[2]) <= 0.05
