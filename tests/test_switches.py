"""The switches have one reader.  switches_reload() (capi.cpp) is the only place of the product library that looks at the environment:
tests/cpp/switches_table.cpp prints every field of Switches for each environment below (no GPU: host code), and the lines expected are
written out here -- the defaults, and per environment the fields that differ from them.  The second test holds the source to the rule: under
tiny-cuda-nn_amd/csrc the token getenv followed by ( stands in capi.cpp and in the definition of lab_env (tcnn_common.h; compiled
only with -DTCNN_AMD_DEV) and nowhere else, comments included."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "switches_table.cpp")
LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")
CSRC = os.path.join(LIBDIR, "csrc")

# every field of Switches, in the order the program prints them, with its default
DEFAULTS = {
    "grid_planes": 1, "grid_rows_planes": 1, "grid_scatter_lds": 1, "scatter_records": 1, "scatter_tune": 1, "scatter_lists": -1, "scatter_wide": 0, "fused_step": 1, "side_jobs": 1,
    "live_image": 1, "adam_steps32": 0, "adam_in_reduce": 1, "adam_prologue": 1, "adam_prologue_refused": 0, "mlp_r32": 1, "mlp_r32a": -1, "mlp_regs": 1, "mlp_fast": 1, "mlp_prio": 1,
    "listgrad_in_mlp": 1, "mlp_layerwise": 0, "mlp_regw": 1, "mlp_variant_forced": 0, "mlp_variant": "0,0,0", "wgrad_rows": 1, "mlp_fwd_lds": 1, "fuse_oneblob": 1,
}
# switches that are on unless the variable begins with 0, and switches that are off unless it begins with 1: (variable, field)
OFF_WITH_0 = [("GRID_PLANES", "grid_planes"), ("GRID_ROWS_PLANES", "grid_rows_planes"), ("SCATTER_RECORDS", "scatter_records"), ("SCATTER_TUNE", "scatter_tune"), ("FUSED_STEP", "fused_step"),
              ("SIDE_JOBS", "side_jobs"), ("LIVE_IMAGE", "live_image"), ("ADAM_IN_REDUCE", "adam_in_reduce"), ("MLP_R32", "mlp_r32"), ("MLP_REGS", "mlp_regs"), ("MLP_FAST", "mlp_fast"),
              ("LISTGRAD_IN_MLP", "listgrad_in_mlp"), ("MLP_REGW", "mlp_regw"), ("WGRAD_ROWS", "wgrad_rows"), ("MLP_FWD_LDS", "mlp_fwd_lds"), ("FUSE_ONEBLOB", "fuse_oneblob")]
ON_WITH_1 = [("SCATTER_WIDE", "scatter_wide"), ("ADAM_STEPS32", "adam_steps32"), ("MLP_LAYERWISE", "mlp_layerwise")]
# (environment, the fields that differ from the defaults)
ENVIRONMENTS = (
    [("-", {})]
    + [e for var, field in OFF_WITH_0 for e in ((f"TCNN_AMD_{var}=0", {field: 0}), (f"TCNN_AMD_{var}=1", {}))]
    + [e for var, field in ON_WITH_1 for e in ((f"TCNN_AMD_{var}=1", {field: 1}), (f"TCNN_AMD_{var}=0", {}))]
    + [
        ("TCNN_AMD_SCATTER_LISTS=0", {"scatter_lists": 0}), ("TCNN_AMD_SCATTER_LISTS=1", {"scatter_lists": 1}), ("TCNN_AMD_SCATTER_LISTS=2", {}),
        ("TCNN_AMD_MLP_R32A=0", {"mlp_r32a": 0}), ("TCNN_AMD_MLP_R32A=1", {"mlp_r32a": 1}), ("TCNN_AMD_MLP_R32A=x", {}),
        ("TCNN_AMD_MLP_PRIO=0", {"mlp_prio": 0}), ("TCNN_AMD_MLP_PRIO=1", {}), ("TCNN_AMD_MLP_PRIO=2", {"mlp_prio": 2}), ("TCNN_AMD_MLP_PRIO=3", {"mlp_prio": 3}),
        ("TCNN_AMD_ADAM_PROLOGUE=0", {"adam_prologue": 0}), ("TCNN_AMD_ADAM_PROLOGUE=refuse", {"adam_prologue_refused": 1}),
        ("TCNN_AMD_GRID_SCATTER=atomic", {"grid_scatter_lds": 0}), ("TCNN_AMD_GRID_SCATTER=lds", {}), ("TCNN_AMD_GRID_SCATTER=atomics", {}),
        # forced only when all three numbers parse (what follows them is not looked at), whatever they are
        ("TCNN_AMD_MLP_VARIANT=1,8,8", {"mlp_variant_forced": 1, "mlp_variant": "1,8,8"}), ("TCNN_AMD_MLP_VARIANT=2,4,16", {"mlp_variant_forced": 1, "mlp_variant": "2,4,16"}),
        ("TCNN_AMD_MLP_VARIANT=0,0,0", {"mlp_variant_forced": 1}), ("TCNN_AMD_MLP_VARIANT=1,8,8,9", {"mlp_variant_forced": 1, "mlp_variant": "1,8,8"}),
        ("TCNN_AMD_MLP_VARIANT=1,8", {}), ("TCNN_AMD_MLP_VARIANT=1,8,", {}), ("TCNN_AMD_MLP_VARIANT=1 8 8", {}), ("TCNN_AMD_MLP_VARIANT=x", {}), ("TCNN_AMD_MLP_VARIANT=", {}),
        # removed with the form it selected; laboratory knobs are no switches
        ("TCNN_AMD_MLP_PW=1", {}), ("TCNN_AMD_SCATTER_LEVELS=0,3", {}), ("TCNN_AMD_MLP_IMAGE_LDS=0", {}),
    ]
)


def _line(env, changed):
    assert set(changed) <= set(DEFAULTS)
    return env + ": " + " ".join(f"{k}={changed.get(k, v)}" for k, v in DEFAULTS.items())


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "switches_table")
    # the internal headers are HIP headers: host-only compilation with hipcc
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", "-o", out])
    return out


def test_switches_reload_reads_every_switch(binary):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TCNN_AMD_")}  # the program sets each environment itself
    r = subprocess.run([binary] + [e for e, _ in ENVIRONMENTS], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    want = [_line(e, changed) for e, changed in ENVIRONMENTS]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    assert {k for _, changed in ENVIRONMENTS for k in changed} == set(DEFAULTS)  # every field is moved by some environment


def test_the_environment_has_one_reader():
    sites = []
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), errors="replace") as f:
            for i, line in enumerate(f, 1):
                if re.search(r"\bgetenv\s*\(", line):
                    sites.append((name, i, line.strip()))
    elsewhere = [s for s in sites if s[0] != "capi.cpp" and s[2] != "inline const char* lab_env(const char* name) { return getenv(name); }"]
    assert not elsewhere, "the environment is read outside switches_reload() and lab_env():\n" + "\n".join("%s:%d: %s" % s for s in elsewhere)
    assert any(s[0] == "capi.cpp" for s in sites) and any(s[0] == "tcnn_common.h" for s in sites)  # (the search finds what it looks for)
