"""Which fused MLP training kernel runs, and over how many workgroups: mlp_train_plan's choice for every case of
tests/cpp/mlp_train_plan_table.cpp, under every switch set it lists, equals the recorded table (no GPU: the plan is pure host code).

tests/golden/mlp_train_plan_table.txt was recorded on the commit before mlp_train_plan existed, by a program with the same cases that
asked that commit's functions in that commit's order: NetworkWithInputEncoding::fused_mlp_and_scatter's slab sizing
(mlp_train_regs_supported && mlp_train_r32_applies ? mlp_train_r32_grid : mlp_train_fused_grid), then mlp_train_fused's chain
(mlp_train_r32ob_applies, mlp_train_r32w_applies, mlp_train_regs_supported && slabs, pick_config) and mlp_train_regs's
(mlp_train_r32_applies), with every CHECK_THROW on the way as "none".  The number recorded is the grid as launched; that program found no
case with weight gradients where the slabs as sized differed from it."""
import difflib
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "mlp_train_plan_table.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_train_plan_table.txt")
LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "mlp_train_plan_table")
    # the internal headers are HIP headers: host-only compilation with hipcc
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", "-o", out])
    return out


def test_plan_reproduces_the_recorded_table(binary):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TCNN_AMD_")}  # the program sets each switch set itself
    r = subprocess.run([binary], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout
    with open(GOLDEN) as f:
        want = f.read()
    if got != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.splitlines(), "recorded", "mlp_train_plan", lineterm="", n=1))
        pytest.fail("the plan differs from the recorded table in %d lines:\n%s" % (len(diff), "\n".join(diff[:60])))
    assert got.count("\nS ") == 14 and all(k in got for k in ("none:0", "r32ob", "r32w", "r32a", "regs", "train", "noob"))  # (the table is not empty)
