"""BatchedMLP ("otype": "BatchedMLP", tiny-cuda-nn_amd/csrc/k_mlp_batched.hip) through the C ABI, without a device: what the constructor
refuses and says, and what a module reports.  (initial_params goes through device memory: tests/test_batched_mlp_gpu.py checks it.)"""
import ctypes as C
import os

import pytest

from conftest import ROOT

FP32, FP16 = 0, 1


def _net(**over):
    net = {"otype": "BatchedMLP", "n_networks": 4, "n_neurons": 32, "n_hidden_layers": 2, "activation": "ReLU", "output_activation": "None"}
    net.update(over)
    return net


def _create(n_in, n_out, net, precision=FP16, enc=None):
    from tinycudann import _C, modules

    if enc is None:
        return modules._create(_C.lib.tcnn_create_network_precision, n_in, n_out, _C.to_json_bytes(net), precision)
    return modules._create(_C.lib.tcnn_create_network_with_input_encoding_precision, n_in, n_out, _C.to_json_bytes(enc), _C.to_json_bytes(net), precision)


def _layer_sizes(native):
    from tinycudann import _C

    n = C.c_size_t()
    _C.check(_C.lib.tcnn_module_layer_sizes(native._h, None, 0, C.byref(n)))
    flat = (C.c_uint32 * (2 * n.value))()
    _C.check(_C.lib.tcnn_module_layer_sizes(native._h, flat, n.value, C.byref(n)))
    return [(int(flat[2 * i]), int(flat[2 * i + 1])) for i in range(n.value)]


REFUSALS = [
    ("fp32", 3, 3, _net(), FP32, None, "BatchedMLP can only be used if the network precision is set to __half."),
    ("sine", 3, 3, _net(activation="Sine"), FP16, None, "BatchedMLP: Sine activation is not supported in the fused kernels"),
    ("width_48", 3, 3, _net(n_neurons=48), FP16, None, "BatchedMLP only supports 16, 32, and 64 neurons, but got 48."),
    ("no_networks", 3, 3, _net(n_networks=0), FP16, None, "BatchedMLP: n_networks must be at least 1."),
    ("no_hidden_layer", 3, 3, _net(n_hidden_layers=0), FP16, None, "BatchedMLP requires at least 1 hidden layer"),
    ("input_80", 80, 3, _net(), FP16, None, "the input width must be between 1 and 64, but got 80."),
    ("output_65", 3, 65, _net(), FP16, None, "the output width must be between 1 and 64, but got 65."),
    # 64 -> 64 x 6 -> 64: 7 matrices of 4096 weights: 2 * 7 * 64 * 72 + 36864 + 4 * 28672 = 216064 bytes
    ("lds", 64, 64, _net(n_neurons=64, n_hidden_layers=6), FP16, None, r"needs 216064 bytes of LDS in the backward kernel .* the limit is 147456 bytes."),
    ("encoding", 3, 3, _net(), FP16, {"otype": "Frequency", "n_frequencies": 4}, "takes no other input encoding, but got Frequency"),
]


@pytest.mark.parametrize("name,n_in,n_out,net,precision,enc,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_constructor_refuses(tcnn, name, n_in, n_out, net, precision, enc, message):
    with pytest.raises(RuntimeError, match=message):
        _create(n_in, n_out, net, precision, enc)


def test_trainer_refuses(tcnn):
    from tinycudann import _C

    h = C.c_void_p()
    config = {"network": _net(), "encoding": {"otype": "Identity"}, "loss": {"otype": "L2"}, "optimizer": {"otype": "Adam"}}
    assert _C.lib.tcnn_create_from_config(3, 3, _C.to_json_bytes(config), C.byref(h)) != 0
    assert "a trainer has no way to say which rows go to which network" in _C.lib.tcnn_last_error().decode()
    # and an unknown otype says what it said
    with pytest.raises(RuntimeError, match="Invalid network type: BatchedMLPs"):
        _create(3, 3, _net(otype="BatchedMLPs"))


def test_what_a_module_reports(tcnn):
    from tinycudann import _C

    batched = _create(20, 17, _net(n_networks=5, n_neurons=64, n_hidden_layers=3))
    single = _create(32, 17, {"otype": "CutlassMLP", "n_neurons": 64, "n_hidden_layers": 3})
    assert batched.n_networks() == 5 and single.n_networks() == 0
    assert batched.n_params() == 5 * single.n_params() == 5 * (64 * 32 + 2 * 64 * 64 + 32 * 64)
    assert _layer_sizes(batched) == 5 * _layer_sizes(single) == 5 * [(64, 32), (64, 64), (64, 64), (32, 64)]
    assert (batched.n_input_dims(), batched.n_output_dims(), batched.param_precision(), batched.output_precision()) == (20, 32, FP16, FP16)
    assert batched.hyperparams() == {"otype": "BatchedMLP", "n_networks": 5, "n_neurons": 64, "n_hidden_layers": 3, "activation": "ReLU", "output_activation": "None"}
    assert batched.name() == "BatchedMLP"
    # the offsets are a BatchedMLP's alone (NULL: the equal split; nothing is read here)
    batched.set_network_offsets(None)
    with pytest.raises(RuntimeError, match="is no BatchedMLP"):
        single.set_network_offsets(None)
    header = open(os.path.join(ROOT, "include", "tcnn_amd.h")).read()
    for name in ("tcnn_module_set_network_offsets", "tcnn_module_n_networks", "tcnn_module_backward_mode"):
        assert name + "(" in header and name in _C._SIGNATURES
