"""input_jvp (every output's derivative along given input directions, forward mode) through the C ABI and the C++ headers, without a GPU:
the symbols exist with their signatures, the header methods compile with a plain C++14 compiler and link, NULL handles report an error with
a message, and every bad argument -- NULL tangents or jvp, n_tangents of 0, a batch size off the granularity, a module without a tangent
(PPNG1, PPNG2, a Composite holding one) -- is refused before anything is allocated or launched (modules are made without a device, the
pointers are fake and never read) and leaves the three route strings alone.  What the routes compute is tests/test_input_jvp_gpu.py's."""
import ctypes as C
import json
import os
import subprocess

import pytest

from conftest import ROOT
from test_grid_max_level_api import _hip_libdir
from test_input_gradient_api import LIBDIR, TCNN_ERROR, _modules

SRC = os.path.join(ROOT, "tests", "cpp", "input_jvp_api.cpp")
PPNG = {"n_frequencies": 2, "n_quants": 8, "n_features": 2, "rank": 2}
NO_TANGENT = [  # (input dims, encoding, the module's name)
    (3, dict(PPNG, otype="PPNG1"), b"PPNG1"),
    (3, dict(PPNG, otype="PPNG2"), b"PPNG2"),
    (5, {"otype": "Composite", "nested": [{"otype": "OneBlob", "n_bins": 16, "n_dims_to_encode": 2}, dict(PPNG, otype="PPNG1", n_dims_to_encode=3)]}, b"Composite"),
]


@pytest.fixture(scope="module")
def lib(tcnn):
    from tinycudann import _C

    return _C


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "input_jvp_api")
    hip = _hip_libdir()
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", f"-I{os.path.join(ROOT, 'include')}", SRC, f"-L{LIBDIR}", "-ltcnn_amd",
           f"-Wl,-rpath,{LIBDIR}", f"-Wl,-rpath,{hip}", f"-Wl,-rpath-link,{hip}", "-o", out]
    subprocess.check_call(cmd)
    return out


def test_header_methods_compile_link_and_refuse_bad_calls(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host checks ok" in r.stdout


def test_symbols_and_signatures(lib):
    u32, vp = C.c_uint32, C.c_void_p
    f = lib.lib.tcnn_module_input_jvp  # (m, stream, n_elements, n_tangents, input, tangents, jvp, output, params)
    assert f.restype is C.c_int and list(f.argtypes) == [vp, vp, u32, u32, vp, vp, vp, vp, vp]
    f = lib.lib.tcnn_trainer_input_jvp  # (t, stream, n_elements, n_tangents, input, tangents, jvp)
    assert f.restype is C.c_int and list(f.argtypes) == [vp, vp, u32, u32, vp, vp, vp]
    f = lib.lib.tcnn_module_last_input_jvp_route
    assert f.restype is C.c_char_p and list(f.argtypes) == [vp]
    header = open(os.path.join(ROOT, "include", "tcnn_amd.h")).read()
    for name in ("tcnn_module_input_jvp", "tcnn_trainer_input_jvp", "tcnn_module_last_input_jvp_route"):
        assert name + "(" in header


def _routes(L, h):
    return L.tcnn_module_last_input_jvp_route(h), L.tcnn_module_last_input_gradient_route(h), L.tcnn_module_last_input_jacobian_route(h)


def test_arguments_are_checked_before_anything_runs(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)  # never read: every error comes first
    for h in _modules(lib):
        try:
            assert L.tcnn_module_last_input_jvp_route(h) == b"none"
            assert L.tcnn_module_input_jvp(h, None, 256, 1, fake, None, fake, None, fake) == TCNN_ERROR
            assert b"tangents" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp(h, None, 256, 1, fake, fake, None, None, fake) == TCNN_ERROR
            assert b"jvp" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp(h, None, 256, 0, fake, fake, fake, None, fake) == TCNN_ERROR
            assert b"n_tangents" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp(h, None, 300, 2, fake, fake, fake, None, fake) == TCNN_ERROR
            assert b"BATCH_SIZE_GRANULARITY" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp(h, None, 0, 2, None, fake, fake, None, None) == 0  # an empty batch is no work
            assert _routes(L, h) == (b"none", b"none", b"none")
        finally:
            L.tcnn_module_destroy(h)


def test_modules_without_a_tangent_are_refused(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)
    for n_in, encoding, name in NO_TANGENT:
        made = []
        h = C.c_void_p()
        lib.check(L.tcnn_create_encoding(n_in, json.dumps(encoding).encode(), 1, C.byref(h)))
        made.append(h)
        h = C.c_void_p()
        net = {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
        lib.check(L.tcnn_create_network_with_input_encoding(n_in, 3, json.dumps(encoding).encode(), json.dumps(net).encode(), C.byref(h)))
        made.append(h)
        for h, who in zip(made, (name, b"NetworkWithInputEncoding")):
            try:
                assert L.tcnn_module_input_jvp(h, None, 256, 2, fake, fake, fake, None, fake) == TCNN_ERROR
                assert L.tcnn_last_error() == b"input_jvp: not implemented for " + who
                assert _routes(L, h) == (b"none", b"none", b"none")
            finally:
                L.tcnn_module_destroy(h)


def test_null_handles_report_an_error(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)
    assert L.tcnn_module_input_jvp(None, None, 256, 1, fake, fake, fake, None, fake) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_trainer_input_jvp(None, None, 256, 1, fake, fake, fake) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_module_last_input_jvp_route(None) is None and b"null module" in L.tcnn_last_error()


def test_python_surfaces_exist(tcnn):
    from tinycudann.modules import Module, NativeModule

    assert callable(NativeModule.input_jvp) and callable(NativeModule.last_input_jvp_route)
    assert callable(Module.input_jvp) and callable(tcnn.Trainer.input_jvp)
    for cls in (tcnn.Encoding, tcnn.Network, tcnn.NetworkWithInputEncoding):
        assert cls.input_jvp is Module.input_jvp
