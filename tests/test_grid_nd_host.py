"""Grid encodings of 1, 5, 6 and 7 input dimensions on the host (no GPU: constructing an encoding touches no device).
  * tests/cpp/grid_nd_api.cpp builds them through the C++ header API: n_params and the padded output width equal the numpy restatement's
    (tests/grid_nd_reference.py), in both precisions; 0 and 8 dimensions are refused with the reference's message.
  * tests/cpp/grid_nd_levels.cpp prints the level table -- offset, size, scale, hashed, stride[] -- which equals the restatement's: dense
    levels, levels whose stride loop exits early, hashed levels, levels capped at 2^31 - 1 entries and strides that wrap in uint32.
  * the routes of the shapes tests/test_grid_nd_gpu.py runs, and the recorded route table of tests/cpp/grid_route_table_nd.cpp."""
import difflib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from grid_nd_reference import DIMS_MESSAGE, GridND
from test_cpp_api import _hip_libdir

LIBDIR = os.path.join(ROOT, "tiny-cuda-nn_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "grid_route_table_nd.txt")


def _hipcc_host(name, directory):
    out = os.path.join(directory, name)
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", "-o", out])
    return out


def build_api_program(directory):
    """tests/cpp/grid_nd_api.cpp with plain g++ against the public headers (also used by tests/test_grid_nd_surfaces.py)"""
    out = os.path.join(directory, "grid_nd_api")
    hip = _hip_libdir()
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-O1", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "cpp", "grid_nd_api.cpp"),
                           f"-L{LIBDIR}", "-ltcnn_amd", f"-Wl,-rpath,{LIBDIR}", f"-Wl,-rpath,{hip}", f"-Wl,-rpath-link,{hip}", "-o", out])
    return out


@pytest.fixture(scope="module")
def programs(tcnn, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cpp"))
    return {"levels": _hipcc_host("grid_nd_levels", d), "routes": _hipcc_host("grid_route_table_nd", d), "api": build_api_program(d)}


def _run(cmd):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TCNN_AMD_")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


# the shapes of tests/test_grid_nd_gpu.py, then shapes whose level sizes reach the cap and whose strides wrap in uint32
def _cfg(otype, levels, F, log2_t, base, scale, **extra):
    return dict({"otype": otype, "n_levels": levels, "n_features_per_level": F, "log2_hashmap_size": log2_t, "base_resolution": base, "per_level_scale": scale}, **extra)


TABLE_CASES = [
    (1, _cfg("HashGrid", 6, 2, 8, 4, 2.5)), (5, _cfg("HashGrid", 5, 2, 10, 2, 1.5)), (6, _cfg("HashGrid", 4, 4, 10, 2, 1.5)), (7, _cfg("HashGrid", 4, 2, 11, 2, 2.0)),
    (5, _cfg("DenseGrid", 5, 2, 10, 2, 1.5)), (7, _cfg("TiledGrid", 4, 8, 11, 2, 2.0)), (1, _cfg("DenseGrid", 4, 1, 19, 16, 2.0)),
    (5, _cfg("HashGrid", 16, 2, 19, 16, 2.0)), (6, _cfg("HashGrid", 16, 4, 22, 16, 2.0)), (7, _cfg("HashGrid", 16, 2, 24, 16, 2.0)),  # hashed from level 0 or 1 on
    (7, _cfg("DenseGrid", 8, 1, 19, 16, 2.0)), (5, _cfg("DenseGrid", 10, 2, 19, 16, 2.0)), (6, _cfg("DenseGrid", 8, 2, 19, 8, 1.7)),  # capped sizes, wrapping strides
    (7, _cfg("TiledGrid", 6, 2, 19, 20, 1.5)), (5, _cfg("TiledGrid", 8, 4, 19, 90, 1.3)),  # base^D wraps in uint32
    (1, _cfg("HashGrid", 16, 2, 19, 16, 2.0)),
]


@pytest.mark.parametrize("n_in,cfg", TABLE_CASES, ids=lambda v: v if isinstance(v, int) else f"{v['otype'][:-4]}-L{v['n_levels']}-F{v['n_features_per_level']}-T{v['log2_hashmap_size']}-b{v['base_resolution']}")
def test_level_table_equals_the_restatement(programs, n_in, cfg):
    nd = GridND(n_in, cfg)
    lines = _run([programs["levels"], str(n_in), "0", json.dumps(cfg)]).splitlines()
    head = lines[0].split()
    assert head[0] == "n_params" and int(head[1]) == nd.n_params and int(head[3]) == nd.n_output_dims
    levels = [l.split() for l in lines if l.startswith("level ")]
    assert len(levels) == nd.n_levels
    kinds = set()
    for l, words in enumerate(levels):
        assert int(words[1]) == l
        assert int(words[3]) == int(nd.offsets[l]), f"level {l} offset"
        assert int(words[5]) == nd.sizes[l], f"level {l} size"
        assert int(words[7], 16) == int(np.float32(nd.scales[l]).view(np.uint32)), f"level {l} scale"
        assert int(words[9]) == int(nd.hashed[l]), f"level {l} hashed"
        assert [int(w) for w in words[11:18]] == nd.strides[l] + [0] * (7 - n_in), f"level {l} strides"
        kinds.add("hashed" if nd.hashed[l] else ("early" if n_in > 1 and nd.strides[l][-1] == 0 else "dense"))
    print(n_in, cfg["otype"], sorted(kinds))


def test_the_table_cases_reach_every_kind_of_level():
    seen = set()
    for n_in, cfg in TABLE_CASES:
        nd = GridND(n_in, cfg)
        for l in range(nd.n_levels):
            seen.add("hashed" if nd.hashed[l] else ("early-exit" if n_in > 1 and nd.strides[l][-1] == 0 else "dense"))
            if nd.sizes[l] == next_multiple_8(0xFFFFFFFF // 2):
                seen.add("capped")
            if n_in > 1 and any(nd.strides[l][d] != 0 and nd.strides[l][d] != nd.resolutions[l] ** d for d in range(n_in)):
                seen.add("wrapped")
    assert {"hashed", "early-exit", "dense", "capped", "wrapped"} <= seen, seen
    gpu = GridND(5, _cfg("HashGrid", 5, 2, 10, 2, 1.5))  # the 5-D shape of the GPU tests: a dense level, an early exit, hashed levels
    assert not gpu.hashed[0] and gpu.hashed[2] and gpu.strides[2][4] != 0 and gpu.hashed[3] and gpu.strides[3][4] == 0
    gpu7 = GridND(7, _cfg("HashGrid", 4, 2, 11, 2, 2.0))
    assert gpu7.sizes[0] == 128 and not gpu7.hashed[0] and gpu7.hashed[1]


def next_multiple_8(v):
    return (v + 7) // 8 * 8


def test_header_api_builds_one_to_seven_dimensions(programs):
    cfg = _cfg("HashGrid", 5, 2, 10, 2, 1.5)
    out = _run([programs["api"], "--no-gpu", json.dumps(cfg)])
    assert "host checks ok" in out
    rows = [l.split(None, 3) for l in out.splitlines() if l.startswith("dims ")]
    assert len(rows) == 18
    for _, dims, precision, rest in rows:
        dims = int(dims)
        if dims in (0, 8):
            assert rest == "error " + DIMS_MESSAGE, rest
        else:
            nd = GridND(dims, cfg)
            assert rest == f"n_params {nd.n_params} width {nd.n_output_dims}", (dims, precision, rest)


def test_zero_and_eight_dimensions_keep_the_message(programs):
    for dims in (0, 8):
        assert _run([programs["levels"], str(dims), "0", json.dumps(_cfg("HashGrid", 4, 2, 10, 2, 1.5))]).strip() == "error " + DIMS_MESSAGE


# (n_in, config, expected route of a module's forward + backward at 256 / 512 / 1024 rows, any_binned): what tests/test_grid_nd_gpu.py relies on
GPU_ROUTES = [
    (5, _cfg("HashGrid", 5, 2, 10, 2, 1.5), "rows/bits/bitplanes", 0),        # every level fits one scatter chunk
    (5, _cfg("HashGrid", 4, 2, 15, 8, 2.0), "rows/bits/bitplanes", 0),        # hashed levels of 4 chunks
    (5, _cfg("HashGrid", 4, 2, 18, 8, 2.0), "rows/bits/bitplanes+binned", 1), # levels of 32 chunks: binned, as a 4-D grid of this shape
    (4, _cfg("HashGrid", 4, 2, 18, 8, 2.0), "rows/bits/bitplanes+binned", 1),
    (7, _cfg("HashGrid", 4, 4, 11, 2, 2.0), "rows/bits/bitplanes", 0),
    (1, _cfg("HashGrid", 6, 2, 8, 4, 2.5), "rows/bits/bitplanes", 0),
    (5, _cfg("HashGrid", 5, 1, 10, 2, 1.5), "rows/-/scratch32", 0),
]


@pytest.mark.parametrize("n_in,cfg,want,binned", GPU_ROUTES, ids=lambda v: str(v) if not isinstance(v, dict) else f"F{v['n_features_per_level']}-T{v['log2_hashmap_size']}")
def test_routes_of_the_gpu_shapes(programs, n_in, cfg, want, binned):
    lines = _run([programs["levels"], str(n_in), "0", json.dumps(cfg)]).splitlines()
    assert int(lines[0].split()[5]) == binned
    assert [l.split()[2] for l in lines if l.startswith("route ")] == [want] * 3
    atomic = "rows/-/scratch32" if cfg["n_features_per_level"] == 1 else "rows/-/atomic"
    assert [l.split()[2] for l in lines if l.startswith("route-atomic ")] == [atomic] * 3
    fp32 = _run([programs["levels"], str(n_in), "1", json.dumps(cfg)]).splitlines()
    assert [l.split()[2] for l in fp32 if l.startswith("route ")] == ["rows/-/atomic"] * 3


def test_routes_reproduce_the_recorded_table(programs):
    got = _run([programs["routes"]])
    with open(GOLDEN) as f:
        want = f.read()
    if got != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.splitlines(), "recorded", "routes", lineterm="", n=1))
        pytest.fail("the routes differ from the recorded table in %d lines:\n%s" % (len(diff), "\n".join(diff[:60])))
    answers = {a for a in got.replace("=", " ").split() if a.count("/") >= 3}
    # hit lists and level planes stay with 2 and 3 dimensions; everything else a 4-D grid takes occurs
    assert {a.split("/")[0] for a in answers} == {"rows"} and {a.split("/")[1] for a in answers} == {"-", "bits"}
    assert {a.split("/")[3] for a in answers} == {"-", "atomic", "scratch32", "bitplanes", "bitplanes+binned"}
    assert not any(a.split("/")[2].startswith("records") for a in answers) and not any("/tail" in a for a in answers)
