"""tcnn::Loss<T>::evaluate of the C++ header surface (include/tiny-cuda-nn/tcnn_api.h): a caller with its own matrices, compiled with
plain g++ against the headers and linked with libtcnn_amd.so (tests/cpp/loss_api.cpp)."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_cpp_api import LIBDIR, _hip_libdir

SRC = os.path.join(ROOT, "tests", "cpp", "loss_api.cpp")


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "loss_api")
    hip = _hip_libdir()
    # -ffp-contract=off: the host restates the device's float expressions operation by operation (the library is built the same way)
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}", SRC, f"-L{LIBDIR}", "-ltcnn_amd",
           f"-Wl,-rpath,{LIBDIR}", f"-Wl,-rpath,{hip}", f"-Wl,-rpath-link,{hip}", "-o", out]
    subprocess.check_call(cmd)
    return out


def test_loss_header_compiles_and_host_checks_pass(binary):
    r = subprocess.run([binary, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host checks ok" in r.stdout


@pytest.mark.gpu
def test_loss_header_evaluates_like_the_host_expressions(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu checks ok" in r.stdout
