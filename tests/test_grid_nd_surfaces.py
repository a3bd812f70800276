"""A 5-dimensional grid encoding (and its 1-, 6- and 7-dimensional siblings) on every surface above the kernels: the C ABI and the C++
header in a stand-alone program, NetworkWithInputEncoding against its parts chained by hand, Trainer.inference against the module,
a Composite under each reduction, input_jacobian against input_gradient, max_level per sample, a snapshot round trip, and a short
training run.  The kernels themselves are held to the numpy restatement by tests/test_grid_nd_gpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

from grid_nd_reference import GridND
from grid_reference import edge_x, to_device
from test_grid_nd_host import build_api_program

pytestmark = pytest.mark.gpu

GRID5 = {"otype": "HashGrid", "n_levels": 5, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 2, "per_level_scale": 1.5}
NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
CONFIG5 = {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6},
           "encoding": GRID5, "network": NETWORK}


def _x(n, D, seed=3):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.uniform(0, 1, (n - 256, D)), edge_x(256, D)]).astype(np.float32)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("D", [5, 1, 7])
def test_c_abi_and_header_api_run_a_grid(tcnn, tmp_path, D):
    """tests/cpp/grid_nd_api.cpp creates the encoding through tcnn_create_encoding and through tcnn::cpp::create_encoding, runs inference
    with each and destroys both: the restatement's bits from either"""
    program = build_api_program(str(tmp_path))
    n = 512
    ref = GridND(D, GRID5)
    x = _x(n, D)
    params = np.random.RandomState(1).uniform(-1, 1, ref.n_params).astype(np.float16)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint32(n).tobytes() + x.tobytes() + params.tobytes())
    r = subprocess.run([program, str(D), json.dumps(GRID5), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gpu checks ok" in r.stdout, r.stdout + r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    width = int(np.frombuffer(raw[:4], dtype=np.uint32)[0])
    got = np.frombuffer(raw[4:], dtype=np.uint16).reshape(2, n, width)
    want, _ = ref.forward(x, params)
    assert width == ref.n_output_dims
    assert np.array_equal(got[0], want.view(np.uint16)) and np.array_equal(got[1], want.view(np.uint16))


def test_network_with_input_encoding_equals_its_parts(tcnn):
    """NetworkWithInputEncoding(5 -> 3): the encoded batch (10 features, padded with zeros to the network's 16) through the network, by hand"""
    import torch

    n = 512
    model = tcnn.NetworkWithInputEncoding(5, 3, GRID5, NETWORK).native_tcnn_module
    enc = tcnn.Encoding(5, GRID5).native_tcnn_module
    net = tcnn.Network(16, 3, NETWORK).native_tcnn_module
    assert model.n_params() == net.n_params() + enc.n_params()
    torch.manual_seed(0)
    params = ((torch.rand(model.n_params(), device="cuda") * 2 - 1) * 0.5).half()
    x = to_device(_x(n, 5))
    _, whole = model.fwd(x, params)
    _, encoded = enc.fwd(x, params[net.n_params():].contiguous())  # network weights first, then the encoding's parameters
    padded = torch.zeros(n, 16, device="cuda")
    padded[:, :10] = encoded.float()
    _, by_hand = net.fwd(padded, params[:net.n_params()].contiguous())
    assert whole.shape == by_hand.shape and np.array_equal(_bits(whole), _bits(by_hand)) and bool(torch.any(whole != 0))


def test_trainer_inference_equals_the_module(tcnn):
    import torch

    n = 512
    tr = tcnn.Trainer(5, 3, CONFIG5, seed=1337)
    model = tcnn.NetworkWithInputEncoding(5, 3, GRID5, NETWORK).native_tcnn_module
    assert tr.n_params == model.n_params()
    params = ((torch.rand(tr.n_params, device="cuda") * 2 - 1) * 0.5).half()
    tr.set_params(params)
    x = to_device(_x(n, 5))
    _, out = model.fwd(x, params)
    got = tr.inference(x)
    assert got.dtype == torch.float32 and torch.equal(got, out.float()[:, :3]) and bool(torch.any(got != 0))
    assert np.array_equal(_bits(tr.inference_half(x)), _bits(out))
    # the same rows as [dims][n] (TCNN_LAYOUT_SOA): the grid reads coordinates n floats apart
    from tinycudann.native import LAYOUT_SOA

    assert torch.equal(tr.inference(x.t().contiguous(), input_layout=LAYOUT_SOA), got)


def test_composite_of_a_grid_and_spherical_harmonics_equals_its_parts(tcnn):
    """position (5) + direction (3): the grid's ten columns, then the spherical harmonics', each bit for bit its own module's"""
    n = 512
    cfg = {"otype": "Composite", "nested": [dict(GRID5, n_dims_to_encode=5), {"otype": "SphericalHarmonics", "degree": 3}]}
    both = tcnn.Encoding(8, cfg).native_tcnn_module
    grid = tcnn.Encoding(5, GRID5).native_tcnn_module
    sh = tcnn.Encoding(3, {"otype": "SphericalHarmonics", "degree": 3})
    assert both.n_params() == grid.n_params() and both.n_output_dims() == 19
    x = np.concatenate([_x(n, 5), np.random.RandomState(2).uniform(0, 1, (n, 3)).astype(np.float32)], axis=1)
    params = to_device(np.random.RandomState(1).uniform(-1, 1, grid.n_params()).astype(np.float16))
    _, out = both.fwd(to_device(x), params)
    _, g = grid.fwd(to_device(x[:, :5]), params)
    s = sh(to_device(x[:, 5:]))
    assert np.array_equal(_bits(out[:, :10].contiguous()), _bits(g))
    assert np.array_equal(_bits(out[:, -9:].contiguous()), _bits(s[:, -9:].contiguous()))
    want, _ = GridND(5, GRID5).forward(x[:, :5], params.cpu().numpy())
    assert np.array_equal(_bits(g), want.view(np.uint16))


@pytest.mark.parametrize("reduction", ["Sum", "Product"])
def test_composite_reductions_over_grids_of_new_dimensions(tcnn, reduction):
    """a 5-D grid, a 7-D grid and a 1-D grid of equal width combined in fp32 in nesting order and rounded once (composite.h:47-133)"""
    import torch

    n = 512
    nested = [dict(GRID5, n_dims_to_encode=5, dims_to_encode_begin=0), dict(GRID5, n_dims_to_encode=7, dims_to_encode_begin=0, log2_hashmap_size=11),
              dict(GRID5, n_dims_to_encode=1, dims_to_encode_begin=6, base_resolution=4)]
    whole = tcnn.Encoding(7, {"otype": "Composite", "reduction": reduction, "nested": nested}).native_tcnn_module
    parts = [tcnn.Encoding(c["n_dims_to_encode"], {k: v for k, v in c.items() if not k.startswith(("n_dims", "dims_to"))}).native_tcnn_module for c in nested]
    assert whole.n_params() == sum(p.n_params() for p in parts) and whole.n_output_dims() == 10
    x = _x(n, 7)
    lo, hi = (-1.0, 1.0) if reduction == "Sum" else (0.5, 1.5)
    params = to_device(np.random.RandomState(1).uniform(lo, hi, whole.n_params()).astype(np.float16))
    _, out = whole.fwd(to_device(x), params)
    acc, at = None, 0
    for p, c in zip(parts, nested):
        b = c["dims_to_encode_begin"]
        _, y = p.fwd(to_device(x[:, b:b + c["n_dims_to_encode"]]), params[at:at + p.n_params()].contiguous())
        at += p.n_params()
        acc = y.float() if acc is None else (acc + y.float() if reduction == "Sum" else acc * y.float())
    assert np.array_equal(_bits(out), _bits(acc.half())) and bool(torch.any(out != 0))


def test_input_jacobian_rows_equal_input_gradient(tcnn):
    import torch

    n = 256
    model = tcnn.NetworkWithInputEncoding(5, 3, GRID5, NETWORK)
    enc = tcnn.Encoding(7, dict(GRID5, log2_hashmap_size=11, interpolation="Smoothstep"))
    for m, D, dims in ((model, 5, [0, 1, 2]), (enc, 7, [0, 3, 9])):
        with torch.no_grad():
            m.params.copy_((torch.rand_like(m.params) * 2 - 1) * 0.5)
        x = to_device(_x(n, D))
        jac = m.input_jacobian(x, dims=dims)
        assert tuple(jac.shape) == (n, len(dims), D) and bool(torch.any(jac != 0))
        for k, dim in enumerate(dims):
            assert torch.equal(jac[:, k, :], m.input_gradient(x, dim=dim)), (D, dim)


def test_max_level_per_sample(tcnn):
    """set_max_level_gpu: row i keeps the levels l < max_level_i * n_levels + 1e-3 (grid.h:67-75), the others read zero"""
    import torch

    n = 512
    ref = GridND(5, GRID5)
    x = _x(n, 5)
    params = np.random.RandomState(1).uniform(-1, 1, ref.n_params).astype(np.float16)
    native = tcnn.Encoding(5, GRID5).native_tcnn_module
    levels_on = np.random.RandomState(4).randint(0, 6, n)
    per_sample = to_device((levels_on.astype(np.float32) + 0.25) / 5.0 - 0.02)  # between two level boundaries: m = levels_on + 0.15
    native.set_max_level_gpu(per_sample)
    _, out = native.fwd(to_device(x), to_device(params))
    want, _ = ref.forward(x, params)
    want = want.copy()
    for i in range(n):
        m = np.float32(np.float32(per_sample[i].item()) * np.float32(10.0)) / np.float32(2.0)
        want[i, 2 * int(np.ceil(m + np.float32(1e-3))):] = 0
    assert np.array_equal(_bits(out), want.view(np.uint16))
    native.set_max_level_gpu(None)
    native.set_max_level(0.5)  # m = 2.5: levels 0, 1, 2
    _, out = native.fwd(to_device(x), to_device(params))
    full, _ = ref.forward(x, params)
    full = full.copy()
    full[:, 6:] = 0
    assert np.array_equal(_bits(out), full.view(np.uint16))


def test_snapshot_round_trip(tcnn):
    import torch

    a = tcnn.Trainer(5, 3, CONFIG5, seed=1337)
    x = to_device(_x(1024, 5))
    t = torch.rand(1024, 3, device="cuda")
    for _ in range(3):
        a.training_step(x, t)
    blob = a.serialize(serialize_optimizer=True)
    b = tcnn.Trainer(5, 3, CONFIG5, seed=7)
    assert not torch.equal(a.params(), b.params())
    b.deserialize(blob)
    assert torch.equal(a.params(), b.params()) and b.optimizer_step_count() == 3
    assert torch.equal(a.inference(x), b.inference(x))
    a.deserialize(blob)
    a.training_step(x, t)
    b.training_step(x, t)
    assert torch.equal(a.params_full_precision(), b.params_full_precision())


def _target(x):
    import torch

    # smooth and separable: a sum over the dimensions of one-dimensional waves, three phases
    return torch.stack([torch.sin(2 * np.pi * x + k).mean(dim=1) for k in range(3)], dim=1) * 0.5 + 0.5


@pytest.mark.parametrize("D,dtype", [(5, "half"), (5, "float32"), (1, "half"), (7, "half")])
def test_trainer_learns_a_smooth_separable_target(tcnn, D, dtype):
    """a D-dimensional grid in front of a 64 x 2 network, 200 steps of 1024 samples: every loss finite, the last ten below the first ten"""
    import torch

    cfg = dict(CONFIG5, encoding=dict(GRID5, n_levels=6, log2_hashmap_size=14, base_resolution=4))
    if dtype == "float32":
        cfg = dict(cfg, network=dict(NETWORK, otype="CutlassMLP"))
    tr = tcnn.Trainer(D, 3, cfg, seed=1337, dtype=torch.float32 if dtype == "float32" else None)
    torch.manual_seed(0)
    losses = []
    for _ in range(200):
        x = torch.rand(1024, D, device="cuda")
        ctx = tr.training_step(x, _target(x))
        losses.append(tr.loss(ctx))
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print(f"{D}-D grid + 64x2 ({dtype}): mean loss of the first ten steps {first:.5f}, of the last ten {last:.5f}; kernel {tr.last_step_kernel()}")
    assert np.all(np.isfinite(losses)) and last < first
    # the step runs whatever a 4-D grid of the same shape runs
    four = tcnn.Trainer(4, 3, cfg, seed=1337, dtype=torch.float32 if dtype == "float32" else None)
    x4 = torch.rand(1024, 4, device="cuda")
    four.training_step(x4, _target(x4))
    assert tr.last_step_kernel() == four.last_step_kernel()
    assert tr.list_scatters() == 0
