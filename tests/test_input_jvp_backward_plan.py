"""Which route input_jvp_backward takes for a network: mlp_input_jvp_backward_plan's answer for every case of
tests/cpp/input_jvp_backward_plan_table.cpp (no GPU: the plan is pure host code, and the program asks every case twice) -- the table of
test_input_jvp_plan.py -- against the committed golden tests/golden/input_jvp_backward_plan_table.txt, and against the rule:

  two-pass   everything that runs layer by layer (fp32, Sine, zero hidden layers, widths and depths without an instantiation,
             TCNN_AMD_MLP_LAYERWISE=1), n that is no multiple of 16 NB, and every class of the fused shapes in which no fused kernel was
             measured faster than the call's composed route by more than 3 %
  fused      k_mlp_input_jvp_bwd<W,NB,NH,TT>/relu|act for the measured classes.  No such kernel is built: the set is empty, and a name the
             plan returned would have to be an instantiation in the library
  invalid    what the network's constructor refuses (FullyFusedMLP: fp32, widths other than 16 / 32 / 64 / 128, no hidden layer, Sine)
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "input_jvp_backward_plan_table.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "input_jvp_backward_plan_table.txt")
LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")
LINE = re.compile(r"^(\w+) (fp16|fp32) w(\d+) h(\d+) ([\w,*]+) layerwise_env([01]) -> (.*)$")
ACTIVATIONS = ("None", "ReLU", "LeakyReLU", "Exponential", "Sine", "Sigmoid", "Squareplus", "Softplus", "Tanh")
ANSWER = re.compile(r"two-pass|fused k_mlp_input_jvp_bwd<(16|32|64|128),\d+,[1-4],(1|3)>/(relu|act) nb\d+ tt(1|3) grid\d+")
BATCHES, N_TANGENTS = (256, 768, 1 << 18, 1 << 20), (1, 2, 3, 4)


def answers_of(text):
    """{(n, n_tangents): answer} of a line's right-hand side ("all <answer>", or one entry per batch size and number of tangents)"""
    if text.startswith("all "):
        return {(n, t): text[4:] for n in BATCHES for t in N_TANGENTS}
    found = {}
    for entry in text.split("; "):
        n, t, answer = re.fullmatch(r"n(\d+) t(\d+) (.*)", entry).groups()
        found[(int(n), int(t))] = answer
    return found


@pytest.fixture(scope="module")
def table(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "input_jvp_backward_plan_table")
    # the internal headers are HIP headers: host-only compilation with hipcc
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", "-o", out])
    env = {k: v for k, v in os.environ.items() if not k.startswith("TCNN_AMD_")}  # the program sets the switch itself
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def test_table_is_the_committed_golden(table):
    golden = open(GOLDEN).read().splitlines()
    assert len(table) == len(golden)
    wrong = [(got, want) for got, want in zip(table, golden) if got != want]
    assert not wrong, "%d lines differ from the golden, first: %r" % (len(wrong), wrong[:5])


def test_plan_follows_the_rule(table):
    assert table[-1] == "%d cases" % (2 * 2 * 2 * 6 * 7 * 9 * 4 * 4)
    kinds, networks = set(), 0
    named = {}  # (otype, precision, width, hidden, env) -> the activations that lines other than the shape's "*" line name
    for grouped in table[:-1]:
        m = LINE.match(grouped)
        assert m, grouped
        otype, precision, width, hidden, activations, env, got = m.groups()
        if activations != "*":
            named.setdefault((otype, precision, width, hidden, env), set()).update(activations.split(","))
    for grouped in table[:-1]:
        otype, precision, width, hidden, activations, env, got = LINE.match(grouped).groups()
        others = named.get((otype, precision, width, hidden, env), set())
        activations = [a for a in ACTIVATIONS if a not in others] if activations == "*" else activations.split(",")
        networks += len(activations)
        for activation in activations:
            assert activation in ACTIVATIONS, grouped
            kinds |= _check_network(grouped, otype, precision, width, hidden, activation, env, got)
    assert networks == 2 * 2 * 2 * 6 * 7 * 9  # every network is on exactly one line
    assert {"two-pass", "invalid"} <= kinds <= {"fused", "two-pass", "invalid"}


def _check_network(line, otype, precision, width, hidden, activation, env, got):
    """one network of a line against the rule; returns the kinds of answers it got"""
    fully_fused = otype == "FullyFusedMLP"
    invalid = fully_fused and (precision == "fp32" or int(width) not in (16, 32, 64, 128) or int(hidden) == 0 or activation == "Sine")
    assert (got == "invalid") == invalid, line
    if invalid:
        return {"invalid"}
    answers = answers_of(got)
    assert set(answers) == {(n, t) for n in BATCHES for t in N_TANGENTS}, line
    for answer in answers.values():
        assert ANSWER.fullmatch(answer), line
    if precision == "fp32" or env == "1" or activation == "Sine" or int(hidden) == 0 or int(width) in (48, 256) or int(hidden) > 4:
        assert got == "all two-pass", line  # layer-by-layer, fp32 and uninstantiated descriptors: two-pass at every n and T
    return {answer.split()[0] for answer in answers.values()}


def test_every_fused_name_is_an_instantiation_of_the_built_library(table):
    names = set(re.findall(r"fused (\S+) nb", "\n".join(table[:-1])))
    symbols = subprocess.run(["nm", "-C", os.path.join(LIBDIR, "libtcnn_amd.so")], capture_output=True, text=True, check=True).stdout
    built = set(re.findall(r"k_mlp_input_jvp_bwd<(-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+)>", symbols))
    if not names:  # no class is fused: then no such kernel is shipped either
        assert not built
        return
    for name in sorted(names):
        w, nb, nh, tt, form = re.fullmatch(r"k_mlp_input_jvp_bwd<(\d+),(\d+),(\d+),(\d+)>/(relu|act)", name).groups()
        assert (w, nb, "1" if form == "relu" else "-1", nh, tt) in built, name
