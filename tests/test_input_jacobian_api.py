"""input_jacobian (input_gradient for several output columns from one forward pass) through the C ABI and the C++ headers, without a GPU:
the header methods compile with a plain C++14 compiler and link, NULL handles report an error with a message, and every bad argument -- a
dim past the padded output width, n_dims of 0 or past the padded width, NULL dims, a batch size off the granularity -- is refused before
anything is allocated or launched (modules are made without a device, the pointers are fake and never read).  What the routes compute is
tests/test_input_jacobian_gpu.py's."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from test_grid_max_level_api import _hip_libdir
from test_input_gradient_api import LIBDIR, TCNN_ERROR, _modules

SRC = os.path.join(ROOT, "tests", "cpp", "input_jacobian_api.cpp")
INVALID_DIM = b"Invalid dimension to compute the input gradient for."


@pytest.fixture(scope="module")
def lib(tcnn):
    from tinycudann import _C

    return _C


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "input_jacobian_api")
    hip = _hip_libdir()
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", f"-I{os.path.join(ROOT, 'include')}", SRC, f"-L{LIBDIR}", "-ltcnn_amd",
           f"-Wl,-rpath,{LIBDIR}", f"-Wl,-rpath,{hip}", f"-Wl,-rpath-link,{hip}", "-o", out]
    subprocess.check_call(cmd)
    return out


def test_header_methods_compile_link_and_refuse_bad_calls(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host checks ok" in r.stdout


def _dims(*values):
    return (C.c_uint32 * len(values))(*values)


def test_arguments_are_checked_before_anything_runs(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)  # never read: every error comes first
    for h in _modules(lib):
        try:
            assert L.tcnn_module_last_input_jacobian_route(h) == b"none"
            padded = L.tcnn_module_n_output_dims(h)
            for dim in (padded, padded + 1, 0xFFFFFFFF):
                for dims in (_dims(dim), _dims(0, dim), _dims(dim, 0)):
                    if len(dims) > padded:
                        continue
                    assert L.tcnn_module_input_jacobian(h, None, 256, dims, len(dims), fake, fake, None, fake, 128.0) == TCNN_ERROR
                    assert L.tcnn_last_error() == INVALID_DIM
            too_many = _dims(*([0] * (padded + 1)))
            for dims, n_dims in ((_dims(0), 0), (too_many, padded + 1), (None, 1), (None, 0)):
                assert L.tcnn_module_input_jacobian(h, None, 256, dims, n_dims, fake, fake, None, fake, 128.0) == TCNN_ERROR
                assert b"n_dims" in L.tcnn_last_error() and L.tcnn_last_error() != INVALID_DIM
            assert L.tcnn_module_input_jacobian(h, None, 300, _dims(padded - 1), 1, fake, fake, None, fake, 128.0) == TCNN_ERROR
            assert b"BATCH_SIZE_GRANULARITY" in L.tcnn_last_error()
            assert L.tcnn_module_input_jacobian(h, None, 0, _dims(padded - 1, 0), min(2, padded), None, None, None, None, 128.0) == 0  # an empty batch is no work
            assert L.tcnn_module_last_input_jacobian_route(h) == b"none"
            assert L.tcnn_module_last_input_gradient_route(h) == b"none"
        finally:
            L.tcnn_module_destroy(h)


def test_null_handles_report_an_error(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)
    assert L.tcnn_module_input_jacobian(None, None, 256, _dims(0), 1, fake, fake, None, fake, 128.0) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_trainer_input_jacobian(None, None, 256, _dims(0), 1, fake, fake, 128.0) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_module_last_input_jacobian_route(None) is None and b"null module" in L.tcnn_last_error()


def test_python_surfaces_exist(tcnn):
    from tinycudann.modules import Module, NativeModule

    assert callable(NativeModule.input_jacobian) and callable(NativeModule.last_input_jacobian_route)
    assert callable(Module.input_jacobian) and callable(tcnn.Trainer.input_jacobian)
    for cls in (tcnn.Encoding, tcnn.Network, tcnn.NetworkWithInputEncoding):
        assert cls.input_jacobian is Module.input_jacobian
