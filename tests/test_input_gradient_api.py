"""input_gradient (object.h:342-366) through the C ABI and the C++ headers, without a GPU: the header methods compile with a plain C++14
compiler and link, NULL handles report an error with a message, and a dimension past the padded output width -- or a batch size off the
granularity -- is refused with the reference's text before anything is allocated or launched (modules are made without a device).  What the
routes compute is tests/test_input_gradient_gpu.py's."""
import ctypes as C
import json
import os
import subprocess

import pytest

from conftest import ROOT
from test_grid_max_level_api import _hip_libdir

LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "input_gradient_api.cpp")
GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 4, "per_level_scale": 2.0}
TCNN_ERROR = 1  # tcnn_amd.h: what every int-returning function returns with a message in tcnn_last_error()
NET = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}


@pytest.fixture(scope="module")
def lib(tcnn):
    from tinycudann import _C

    return _C


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "input_gradient_api")
    hip = _hip_libdir()
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", f"-I{os.path.join(ROOT, 'include')}", SRC, f"-L{LIBDIR}", "-ltcnn_amd",
           f"-Wl,-rpath,{LIBDIR}", f"-Wl,-rpath,{hip}", f"-Wl,-rpath-link,{hip}", "-o", out]
    subprocess.check_call(cmd)
    return out


def test_header_methods_compile_link_and_refuse_bad_calls(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host checks ok" in r.stdout


def _modules(lib):
    L = lib.lib
    made = []
    for n_out in (1, 17):
        h = C.c_void_p()
        lib.check(L.tcnn_create_network_with_input_encoding(3, n_out, json.dumps(GRID).encode(), json.dumps(NET).encode(), C.byref(h)))
        made.append(h)
    h = C.c_void_p()
    lib.check(L.tcnn_create_network(5, 3, json.dumps(NET).encode(), C.byref(h)))
    made.append(h)
    h = C.c_void_p()
    lib.check(L.tcnn_create_encoding(3, json.dumps(GRID).encode(), 1, C.byref(h)))
    made.append(h)
    return made


def test_dimension_and_batch_size_are_checked_before_anything_runs(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)  # never read: both errors come first
    for h in _modules(lib):
        try:
            assert L.tcnn_module_last_input_gradient_route(h) == b"none"
            padded = L.tcnn_module_n_output_dims(h)
            for dim in (padded, padded + 1, 0xFFFFFFFF):
                assert L.tcnn_module_input_gradient(h, None, 256, dim, fake, fake, None, fake, 128.0) == TCNN_ERROR
                assert L.tcnn_last_error() == b"Invalid dimension to compute the input gradient for."
            assert L.tcnn_module_input_gradient(h, None, 300, padded - 1, fake, fake, None, fake, 128.0) == TCNN_ERROR
            assert b"BATCH_SIZE_GRANULARITY" in L.tcnn_last_error()
            assert L.tcnn_module_input_gradient(h, None, 0, padded - 1, None, None, None, None, 128.0) == 0  # an empty batch is no work
            assert L.tcnn_module_last_input_gradient_route(h) == b"none"
        finally:
            L.tcnn_module_destroy(h)


def test_null_handles_report_an_error(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)
    assert L.tcnn_module_input_gradient(None, None, 256, 0, fake, fake, None, fake, 128.0) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_trainer_input_gradient(None, None, 256, 0, fake, fake, 128.0) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_module_last_input_gradient_route(None) is None and b"null module" in L.tcnn_last_error()


def test_python_surfaces_exist(tcnn):
    from tinycudann.modules import Module, NativeModule

    assert callable(NativeModule.input_gradient) and callable(NativeModule.last_input_gradient_route)
    assert callable(Module.input_gradient) and callable(tcnn.Trainer.input_gradient)
    for cls in (tcnn.Encoding, tcnn.Network, tcnn.NetworkWithInputEncoding):
        assert cls.input_gradient is Module.input_gradient
