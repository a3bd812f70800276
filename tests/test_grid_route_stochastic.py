"""The grid encoding's routes with stochastic_interpolation set (tests/cpp/grid_route_stochastic.cpp): over the argument ranges of the route
table, a Linear or Smoothstep grid never records hit lists, never takes the list-fed gradient kernel, the scatter records or the MLP
kernel's list-order tail, and otherwise keeps the plain grid's forward kernel and gradient family; a Nearest grid routes exactly like a
plain one.  No GPU: both routes are pure host code, and constructing a GridEncoding touches no device."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "grid_route_stochastic.cpp")
LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "grid_route_stochastic")
    # the internal headers are HIP headers: host-only compilation with hipcc
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", "-o", out])
    return out


def test_stochastic_routes(binary):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TCNN_AMD_")}  # the program sets each switch set itself
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.rstrip().endswith("ok")
