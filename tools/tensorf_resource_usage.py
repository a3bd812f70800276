"""Registers, scratch, LDS and occupancy of every k_tensorf_* instantiation, as hipcc reports them (-Rpass-analysis=kernel-resource-usage)
when it compiles k_tensorf.hip for gfx950 with the library's flags.  No GPU needed.

    python tools/tensorf_resource_usage.py    # compiles, writes profiles/tensorf_resource_usage.txt, exits 1 if a kernel uses scratch or static LDS
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_nd_resource_usage as usage  # noqa: E402

SOURCE = "k_tensorf.hip"
OUT = os.path.join(usage.ROOT, "profiles", "tensorf_resource_usage.txt")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        found = list(usage.kernels(usage.compile_log(SOURCE, tmp)))
    names = subprocess.run([usage.demangler()], input="\n".join(r["name"].replace("DF16_", "Dh") for r in found), capture_output=True, text=True, check=True).stdout.splitlines()
    rows = sorted((re.sub(r"^void |\(.*$", "", re.sub(r"tcnn_amd::\(anonymous namespace\)::", "", name)), r) for r, name in zip(found, names))
    lines = ["# every kernel of k_tensorf.hip (<T, CP, D, F> / <CP, D, F>; CP false: the vector-matrix form): hipcc --offload-arch=gfx950, the library's flags, -Rpass-analysis=kernel-resource-usage",
             "# (tools/tensorf_resource_usage.py).  scratch: bytes per lane; occupancy: waves per SIMD; lds: static bytes per workgroup (k_tensorf_bwd asks for its",
             "# accumulators dynamically: at most 64 KB, 8 bytes per entry and component of the chunk's planes and line segments)",
             f"{'kernel':44s} {'VGPR':>5s} {'AGPR':>5s} {'scratch':>8s} {'occupancy':>10s} {'lds':>6s}"]
    lines += [f"{name:44s} {r['vgpr']:5d} {r['agpr']:5d} {r['scratch']:8d} {r['occupancy']:10d} {r['lds']:6d}" for name, r in rows]
    bad = [name for name, r in rows if r["scratch"] != 0 or r["lds"] != 0]
    lines.append(f"# {len(rows)} kernels, {len(bad)} with scratch or static LDS")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
