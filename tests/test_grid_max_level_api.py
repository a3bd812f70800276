"""max_level of the grid encodings (the reference's GridEncoding::set_max_level / max_level / set_max_level_gpu, grid_interface.h:101-123)
through the C ABI and the C++ header API.  Module construction does not touch the GPU: none of this needs one (trainers initialise
their parameters on the device -- their round trips are in test_grid_max_level.py)."""
import ctypes as C
import json
import math
import os
import subprocess

import pytest

from conftest import CONFIG_C3A, ROOT

LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "max_level_api.cpp")

GRID = CONFIG_C3A["encoding"]
NET = CONFIG_C3A["network"]
COMPOSITE = {"otype": "Composite", "nested": [dict(GRID, n_dims_to_encode=3), {"otype": "SphericalHarmonics", "degree": 4, "n_dims_to_encode": 3}]}


@pytest.fixture(scope="module")
def lib(tcnn):
    from tinycudann import _C

    return _C


def _encoding(lib, n_dims, cfg):
    h = C.c_void_p()
    lib.check(lib.lib.tcnn_create_encoding(n_dims, json.dumps(cfg).encode(), 1, C.byref(h)))
    return h


def _nwie(lib, n_dims, enc, net=NET):
    h = C.c_void_p()
    lib.check(lib.lib.tcnn_create_network_with_input_encoding(n_dims, 16, json.dumps(enc).encode(), json.dumps(net).encode(), C.byref(h)))
    return h


@pytest.mark.parametrize("kind", ["encoding", "network_with_input_encoding"])
def test_module_round_trip(lib, kind):
    L = lib.lib
    h = _encoding(lib, 2, GRID) if kind == "encoding" else _nwie(lib, 2, GRID)
    try:
        assert L.tcnn_module_max_level(h) == 1000.0  # grid_interface.h:118
        for v in (0.5, 0.0, 0.4999375, 1.0, 1000.0, 7.25):
            assert L.tcnn_module_set_max_level(h, v) == 0
            assert L.tcnn_module_max_level(h) == C.c_float(v).value
        assert L.tcnn_module_set_max_level(h, float("nan")) == 0
        assert math.isnan(L.tcnn_module_max_level(h)) and L.tcnn_last_error() == b""  # a NaN that was set is no error
        # the per-sample pointer is stored, not read: setting and clearing it needs no device
        assert L.tcnn_module_set_max_level_gpu(h, C.c_void_p(0x1000)) == 0
        assert L.tcnn_module_set_max_level_gpu(h, None) == 0
    finally:
        L.tcnn_module_destroy(h)


@pytest.mark.parametrize("enc", [{"otype": "OneBlob", "n_bins": 32}, {"otype": "Identity"}])
def test_modules_without_a_grid_report_an_error(lib, enc):
    L = lib.lib
    for h in (_encoding(lib, 2, enc), _nwie(lib, 2, enc)):
        try:
            assert L.tcnn_module_set_max_level(h, 0.5) != 0
            msg = L.tcnn_last_error().decode()
            assert "max_level" in msg and "no grid encoding" in msg, msg
            assert L.tcnn_module_set_max_level_gpu(h, None) != 0
            assert "no grid encoding" in L.tcnn_last_error().decode()
            assert math.isnan(L.tcnn_module_max_level(h))
            assert "no grid encoding" in L.tcnn_last_error().decode()
        finally:
            L.tcnn_module_destroy(h)


def test_composite_with_a_grid_accepts(lib):
    L = lib.lib
    for h in (_encoding(lib, 6, COMPOSITE), _nwie(lib, 6, COMPOSITE)):
        try:
            assert L.tcnn_module_set_max_level(h, 0.25) == 0, L.tcnn_last_error()
            assert L.tcnn_module_max_level(h) == 0.25
            assert L.tcnn_module_set_max_level_gpu(h, None) == 0
        finally:
            L.tcnn_module_destroy(h)


def test_hyperparams_do_not_carry_the_setting(lib):
    L = lib.lib
    for make in (lambda: _encoding(lib, 2, GRID), lambda: _nwie(lib, 2, GRID), lambda: _encoding(lib, 6, COMPOSITE)):
        plain, cut = make(), make()
        try:
            assert L.tcnn_module_set_max_level(cut, 0.5) == 0
            assert L.tcnn_module_hyperparams(cut) == L.tcnn_module_hyperparams(plain)
        finally:
            L.tcnn_module_destroy(plain)
            L.tcnn_module_destroy(cut)


def test_python_native_module_round_trip(tcnn, lib):
    from tinycudann.modules import NativeModule, _create

    m = _create(lib.lib.tcnn_create_encoding, 2, lib.to_json_bytes(GRID), 1)
    assert isinstance(m, NativeModule) and m.max_level() == 1000.0
    m.set_max_level(0.375)
    assert m.max_level() == 0.375
    bad = _create(lib.lib.tcnn_create_encoding, 2, lib.to_json_bytes({"otype": "OneBlob", "n_bins": 16}), 1)
    with pytest.raises(RuntimeError, match="no grid encoding"):
        bad.set_max_level(0.5)
    with pytest.raises(RuntimeError, match="no grid encoding"):
        bad.max_level()


def _hip_libdir():
    if os.path.exists("/opt/rocm/lib/libamdhip64.so"):
        return "/opt/rocm/lib"
    import torch

    return os.path.join(os.path.dirname(torch.__file__), "lib")


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "max_level_api")
    hip = _hip_libdir()
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", f"-I{os.path.join(ROOT, 'include')}", SRC, f"-L{LIBDIR}", "-ltcnn_amd",
           f"-Wl,-rpath,{LIBDIR}", f"-Wl,-rpath,{hip}", f"-Wl,-rpath-link,{hip}", "-o", out]
    subprocess.check_call(cmd)
    return out


def test_header_api_holds_the_value_before_binding(binary):
    r = subprocess.run([binary, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host checks ok" in r.stdout


@pytest.mark.gpu
def test_header_api_applies_the_value_at_binding(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu checks ok" in r.stdout
