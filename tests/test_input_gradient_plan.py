"""Which route input_gradient takes for a network: mlp_input_gradient_plan's answer for every case of
tests/cpp/input_gradient_plan_table.cpp (no GPU: the plan is pure host code) against the rule, written out here on its own:

  fused      a half-precision network the fused kernels run (FullyFusedMLP or CutlassMLP; 16, 32, 64 or 128 wide; 1 to 4 hidden layers; any
             activation but Sine), created without TCNN_AMD_MLP_LAYERWISE=1, for n a multiple of 16 NB -- NB = 4 column blocks of 16 samples
             per wave below 128 wide, 2 at 128; workgroups of 4 waves, one trip per wave up to 2048 of them
             -- except 128 wide x (3 | 4) hidden layers in the compiled ReLU form on a full machine (2048 workgroups: 2^18 rows and up),
             where the fused kernel measured no faster than the two passes (DESIGN.md "input_gradient")
  two-pass   that class, and everything else that can be made: fp32, Sine, zero hidden layers, other widths (48; 256: only one hidden layer would fit in
             registers, so it is not instantiated), more than 4 hidden layers, TCNN_AMD_MLP_LAYERWISE=1
  invalid    what the network's constructor refuses (FullyFusedMLP: fp32, widths other than 16 / 32 / 64 / 128, no hidden layer, Sine)
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "input_gradient_plan_table.cpp")
LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")
LINE = re.compile(r"^(\w+) (fp16|fp32) w(\d+) h(\d+) (\w+) n(\d+) layerwise_env([01]) -> (.*)$")


@pytest.fixture(scope="module")
def table(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "input_gradient_plan_table")
    # the internal headers are HIP headers: host-only compilation with hipcc
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", "-o", out])
    env = {k: v for k, v in os.environ.items() if not k.startswith("TCNN_AMD_")}  # the program sets the switch itself
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def expected(otype, precision, width, hidden, activation, n, layerwise_env):
    fully_fused = otype == "FullyFusedMLP"
    if fully_fused and (precision == "fp32" or width not in (16, 32, 64, 128) or hidden == 0 or activation == "Sine"):
        return "invalid"
    layer_by_layer = precision == "fp32" or activation == "Sine" or hidden == 0 or width not in (16, 32, 64, 128, 256) or layerwise_env
    if layer_by_layer or width == 256 or hidden > 4:
        return "two-pass"
    nb = 4 if width < 128 else 2
    if n % (16 * nb):
        return "two-pass"
    workgroups = -(-(n // (16 * nb)) // 4)
    if width == 128 and activation == "ReLU" and hidden >= 3 and workgroups >= 2048:
        return "two-pass"  # measured: no faster than the two passes on a full machine
    grid = min(workgroups, 2048)
    return "fused k_mlp_input_grad<%d,%d,%d>/%s nb%d grid%d" % (width, nb, hidden, "relu" if activation == "ReLU" else "act", nb, grid)


def test_plan_follows_the_rule(table):
    assert table[-1] == "%d cases" % (2 * 2 * 2 * 6 * 7 * 9 * 3)
    answers = set()
    wrong = []
    for line in table[:-1]:
        m = LINE.match(line)
        assert m, line
        otype, precision, width, hidden, activation, n, env, got = m.groups()
        want = expected(otype, precision, int(width), int(hidden), activation, int(n), env == "1")
        answers.add(got.split()[0])
        if got != want:
            wrong.append("%s   (rule: %s)" % (line, want))
    assert not wrong, "%d cases differ from the rule:\n%s" % (len(wrong), "\n".join(wrong[:40]))
    assert answers == {"fused", "two-pass", "invalid"}
