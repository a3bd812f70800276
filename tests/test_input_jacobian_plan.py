"""Which route input_jacobian takes for a network: mlp_input_jacobian_plan's answer for every case of
tests/cpp/input_jacobian_plan_table.cpp (no GPU: the plan is pure host code) -- test_input_gradient_plan.py's table (and 2^20 rows) x n_dims in
{1, 3, 16, 17} -- against the rule, written out here on its own:

  fused      a half-precision network the fused kernels run (FullyFusedMLP or CutlassMLP; 16, 32, 64 or 128 wide; 1 to 4 hidden layers; any
             activation but Sine), created without TCNN_AMD_MLP_LAYERWISE=1, for n a multiple of 16 NB -- NB = 4 column blocks of 16 samples
             per wave below 128 wide, 2 at 128; workgroups of 4 waves, one trip per wave up to 2048 of them (more than 16 dims are further
             launches of the same kernel) -- except the classes in which the fused kernel measured no faster than the Jacobian's own two
             passes by more than 3 %, the spread between boxes (DESIGN.md "input_jacobian"):
               - any activation but ReLU (the run-time form), more than 256 workgroups, and n_dims above the class's limit: 16 wide -- no
                 limit with 1 to 3 hidden layers, never fused with 4; 32 wide -- no limit with 1 or 2, 1 dim with 3, never with 4;
                 64 wide -- 3 dims with 1 hidden layer, else 2; 128 wide -- 2 dims with 1 hidden layer, else 1
               - ReLU, 128 wide, 2 hidden layers, 2^20 rows and up, more than 8 dims
             mlp_input_gradient_plan's measured exception (128 wide x (3 | 4) hidden layers, ReLU, full machine) is NOT part of this rule:
             it was measured on a kernel that does not share its forward chain
  two-pass   those classes, and everything else that can be made: fp32, Sine, zero hidden layers, other widths (48; 256: not instantiated),
             more than 4 hidden layers, TCNN_AMD_MLP_LAYERWISE=1
  invalid    what the network's constructor refuses (FullyFusedMLP: fp32, widths other than 16 / 32 / 64 / 128, no hidden layer, Sine)
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "input_jacobian_plan_table.cpp")
LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")
LINE = re.compile(r"^(\w+) (fp16|fp32) w(\d+) h(\d+) (\w+) n(\d+) k(\d+) layerwise_env([01]) -> (.*)$")


@pytest.fixture(scope="module")
def table(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "input_jacobian_plan_table")
    # the internal headers are HIP headers: host-only compilation with hipcc
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", "-o", out])
    env = {k: v for k, v in os.environ.items() if not k.startswith("TCNN_AMD_")}  # the program sets the switch itself
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def expected(otype, precision, width, hidden, activation, n, n_dims, layerwise_env):
    fully_fused = otype == "FullyFusedMLP"
    if fully_fused and (precision == "fp32" or width not in (16, 32, 64, 128) or hidden == 0 or activation == "Sine"):
        return "invalid"
    layer_by_layer = precision == "fp32" or activation == "Sine" or hidden == 0 or width not in (16, 32, 64, 128, 256) or layerwise_env
    if layer_by_layer or width == 256 or hidden > 4 or n_dims < 1:
        return "two-pass"
    nb = 4 if width < 128 else 2
    if n % (16 * nb):
        return "two-pass"
    workgroups = -(-(n // (16 * nb)) // 4)
    if activation != "ReLU" and workgroups > 256:
        limit = {16: (None, None, None, 0), 32: (None, None, 1, 0), 64: (3, 2, 2, 2), 128: (2, 1, 1, 1)}[width][hidden - 1]
        if limit is not None and n_dims > limit:
            return "two-pass"  # measured: the run-time form's backward chain loses to k_mlp_bwd from this many dims on
    if activation == "ReLU" and width == 128 and hidden == 2 and n >= 2 ** 20 and n_dims > 8:
        return "two-pass"  # measured: 1.011 and 1.033 at 16 dims
    grid = min(workgroups, 2048)
    return "fused k_mlp_input_jacobian<%d,%d,%d>/%s nb%d grid%d" % (width, nb, hidden, "relu" if activation == "ReLU" else "act", nb, grid)


def test_plan_follows_the_rule(table):
    assert table[-1] == "%d cases" % (2 * 2 * 2 * 6 * 7 * 9 * 4 * 4)
    answers = set()
    wrong = []
    for line in table[:-1]:
        m = LINE.match(line)
        assert m, line
        otype, precision, width, hidden, activation, n, k, env, got = m.groups()
        want = expected(otype, precision, int(width), int(hidden), activation, int(n), int(k), env == "1")
        answers.add(got.split()[0])
        if got != want:
            wrong.append("%s   (rule: %s)" % (line, want))
    assert not wrong, "%d cases differ from the rule:\n%s" % (len(wrong), "\n".join(wrong[:40]))
    assert answers == {"fused", "two-pass", "invalid"}
