"""How a grid encoding's batch is produced and how its parameter gradients are accumulated: grid_forward_route's and grid_backward_route's
answers for every case of tests/cpp/grid_route_table.cpp, under every switch set it lists, equal the recorded table (no GPU: both routes are
pure host code, and constructing a GridEncoding touches no device).

tests/golden/grid_route_table.txt was recorded on the commit before the two routes existed, by a program with the same cases that asked that
commit's public predicates in that commit's order: fused_encode's / GridEncoding::forward's choice of kernel (forward_plane_features,
grid_rows_planes, grid_planes_to_rows_supported), what forward / forward_planes record (lds_scatter_usable, hit_lists_usable),
fused_mlp_and_scatter's level_plane_features and its `records` expression (no hit lists recorded, no padding, scatter_records_usable), the
branch order of GridEncoding::backward and backward_all_levels (scratch32, lds_scatter_usable && n % 64 == 0, lists recorded and current,
m_any_binned, else the atomic kernel) with every CHECK_THROW on the way as "none", take_prologue's conditions on the encoding (an offer of
the fused step, not passed on under a scalar cut-off, no binned level) and list_gradient_tail apart from the item map.  A fused step whose
batch is no multiple of 256 is "none" there too (Model::check_batch); that program found no other case that threw."""
import difflib
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "grid_route_table.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "grid_route_table.txt")
LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "grid_route_table")
    # the internal headers are HIP headers: host-only compilation with hipcc
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", "-o", out])
    return out


def test_routes_reproduce_the_recorded_table(binary):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TCNN_AMD_")}  # the program sets each switch set itself
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout
    with open(GOLDEN) as f:
        want = f.read()
    if got != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.splitlines(), "recorded", "routes", lineterm="", n=1))
        pytest.fail("the routes differ from the recorded table in %d lines:\n%s" % (len(diff), "\n".join(diff[:60])))
    # the table is not trivial: every gradient kernel, every dL/dy form, every forward kernel and recording occurs
    answers = set(got.replace("=", " ").split())
    kernels = {a.split("/")[3] for a in answers if a.count("/") >= 3}
    forms = {a.split("/")[2].rstrip("0123456789") for a in answers if a.count("/") >= 3}
    assert got.count("\nS ") + got.startswith("S ") == 8
    assert kernels == {"-", "atomic", "scratch32", "bitplanes", "bitplanes+binned", "lists"} and forms == {"rows", "planes", "records"}
    assert {a.split("/")[0] for a in answers if a.count("/") >= 3} == {"rows", "planes", "p2r"} and {a.split("/")[1] for a in answers if a.count("/") >= 3} == {"-", "bits", "lists"}
    assert "none" in answers and any(a.endswith("/tail/prologue") for a in answers)
