"""Which route input_jvp takes for a network: mlp_input_jvp_plan's answer for every case of tests/cpp/input_jvp_plan_table.cpp (no GPU:
the plan is pure host code, and the program asks every case twice) -- test_input_jacobian_plan.py's table x n_tangents in {1, 2, 3, 4} --
against the rule, written out here on its own:

  two-pass   everything that runs layer by layer: fp32, Sine, zero hidden layers, widths other than 16 / 32 / 64 / 128 (48; 256: not
             instantiated), more than 4 hidden layers, TCNN_AMD_MLP_LAYERWISE=1; n that is no multiple of 16 NB; and every class of the
             fused shapes in which tools/bench_input_jvp.py did not measure the kernel faster than the call's own two passes by more than
             3 %, the spread between boxes (FUSED below; DESIGN.md "input_jvp / The plan rule", profiles/input_jvp_bench.txt)
  fused      k_mlp_input_jvp<W,NB,NH,TT>/relu|act for the classes in FUSED: TT = 1 tangent chain per launch for one tangent, else 3 (two
             tangents: the third chain runs on zeros; four: a second launch); NB column blocks of 16 samples per wave as the input-gradient
             kernels have them (4 below 128 wide, 2 at 128), halved for TT = 3 at 64 and 128 wide; workgroups of 4 waves, up to 2048
  invalid    what the network's constructor refuses (FullyFusedMLP: fp32, widths other than 16 / 32 / 64 / 128, no hidden layer, Sine)

(A OneBlob encoding in front of the network keeps the two passes whatever the plan says: that is the model's decision, as for
input_gradient, and tests/test_input_jvp_gpu.py asserts it.)  Every fused name the plan returns must be an instantiation in the library
that build.py built: the kernels' host stubs are looked up by their template arguments.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "input_jvp_plan_table.cpp")
LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")
LINE = re.compile(r"^(\w+) (fp16|fp32) w(\d+) h(\d+) (\w+) n(\d+) t(\d+) layerwise_env([01]) -> (.*)$")
RELU_ENUM = 1  # Activation::ReLU, the compiled form's template argument; -1: the activation chosen at run time


def fused_class(width, hidden, relu, workgroups, n_tangents):
    """FUSED: the measured rule.  profiles/input_jvp_bench.txt section 2 has every instantiated class at 2^18 and 2^14 rows: the two
    passes take 1.31 to 9.85 times the kernel's time, so there is no exception"""
    return True


@pytest.fixture(scope="module")
def table(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "input_jvp_plan_table")
    # the internal headers are HIP headers: host-only compilation with hipcc
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", "-o", out])
    env = {k: v for k, v in os.environ.items() if not k.startswith("TCNN_AMD_")}  # the program sets the switch itself
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def expected(otype, precision, width, hidden, activation, n, n_tangents, layerwise_env):
    fully_fused = otype == "FullyFusedMLP"
    if fully_fused and (precision == "fp32" or width not in (16, 32, 64, 128) or hidden == 0 or activation == "Sine"):
        return "invalid"
    layer_by_layer = precision == "fp32" or activation == "Sine" or hidden == 0 or width not in (16, 32, 64, 128, 256) or layerwise_env
    if layer_by_layer or width == 256 or hidden > 4 or n_tangents < 1:
        return "two-pass"
    tt = 1 if n_tangents == 1 else 3
    nb = 4 if width < 128 else 2
    if tt == 3 and width >= 64:
        nb //= 2
    if n % (16 * nb):
        return "two-pass"
    workgroups = -(-(n // (16 * nb)) // 4)
    if not fused_class(width, hidden, activation == "ReLU", workgroups, n_tangents):
        return "two-pass"
    grid = min(workgroups, 2048)
    return "fused k_mlp_input_jvp<%d,%d,%d,%d>/%s nb%d tt%d grid%d" % (width, nb, hidden, tt, "relu" if activation == "ReLU" else "act", nb, tt, grid)


def test_plan_follows_the_rule(table):
    assert table[-1] == "%d cases" % (2 * 2 * 2 * 6 * 7 * 9 * 4 * 4)
    answers = set()
    wrong = []
    for line in table[:-1]:
        m = LINE.match(line)
        assert m, line
        otype, precision, width, hidden, activation, n, t, env, got = m.groups()
        want = expected(otype, precision, int(width), int(hidden), activation, int(n), int(t), env == "1")
        answers.add(got.split()[0])
        if got != want:
            wrong.append("%s   (rule: %s)" % (line, want))
        if precision == "fp32" or env == "1" or activation == "Sine" or int(hidden) == 0 or int(width) in (48, 256):
            assert got in ("two-pass", "invalid"), line  # layer-by-layer and fp32 descriptors: two-pass at every n and T
    assert not wrong, "%d cases differ from the rule:\n%s" % (len(wrong), "\n".join(wrong[:40]))
    assert {"two-pass", "invalid"} <= answers <= {"fused", "two-pass", "invalid"}


def test_every_fused_name_is_an_instantiation_of_the_built_library(table):
    """the names the plan can return against the kernels in libtcnn_amd.so (k_mlp_input_jvp.hip is one of build.py's SOURCES)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("tcnn_build", os.path.join(LIBDIR, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    names = {line.split(" -> ")[1].split()[1] for line in table[:-1] if " -> fused " in line}
    if not names:  # the measured rule keeps every class on the two passes: then the kernel is not shipped either
        assert "k_mlp_input_jvp.hip" not in build.SOURCES
        return
    assert "k_mlp_input_jvp.hip" in build.SOURCES
    symbols = subprocess.run(["nm", "-C", os.path.join(LIBDIR, "libtcnn_amd.so")], capture_output=True, text=True, check=True).stdout
    built = set(re.findall(r"k_mlp_input_jvp<(-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+)>", symbols))
    assert built
    for name in sorted(names):
        m = re.fullmatch(r"k_mlp_input_jvp<(\d+),(\d+),(\d+),(\d+)>/(relu|act)", name)
        assert m, name
        w, nb, nh, tt, form = m.groups()
        assert (w, nb, str(RELU_ENUM if form == "relu" else -1), nh, tt) in built, name
