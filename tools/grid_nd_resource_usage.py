"""Registers, scratch and occupancy of every grid kernel instantiated for 1, 5, 6 and 7 input dimensions, as hipcc reports them
(-Rpass-analysis=kernel-resource-usage) when it compiles the library's grid sources for gfx950 with the library's flags.  No GPU needed.

    python tools/grid_nd_resource_usage.py            # compiles, writes profiles/grid_nd_resource_usage.txt, exits 1 if a kernel uses scratch
    python tools/grid_nd_resource_usage.py --logs DIR # reads DIR/<source>.log instead of compiling (a remark log per source)
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
import build as lib_build  # noqa: E402

SOURCES = ["k_grid_nd.hip", "k_grid.hip", "k_grid_scatter.hip", "k_grid_bin.hip", "k_grid_bwdbwd.hip"]
OUT = os.path.join(ROOT, "profiles", "grid_nd_resource_usage.txt")
FIELDS = {"vgpr": r"VGPRs", "agpr": r"AGPRs", "scratch": r"ScratchSize \[bytes/lane\]", "occupancy": r"Occupancy \[waves/SIMD\]", "lds": r"LDS Size \[bytes/block\]"}


def compile_log(src, directory):
    log = os.path.join(directory, src + ".log")
    cmd = ["hipcc"] + lib_build.FLAGS + lib_build.EXTRA_FLAGS.get(src, []) + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", os.path.join(lib_build.CSRC, src), "-o", os.path.join(directory, src + ".o")]
    with open(log, "w") as f:
        subprocess.check_call(cmd, stdout=f, stderr=subprocess.STDOUT)
    return log


def kernels(log):
    text = open(log).read()
    for block in re.split(r"remark: [^\n]*Function Name: ", text)[1:]:
        mangled = block.split()[0]
        row = {"name": mangled}
        for key, pattern in FIELDS.items():
            m = re.search(pattern + r": (\d+)", block)
            row[key] = int(m.group(1)) if m else -1
        yield row


def demangler():
    """llvm-cxxfilt beside hipcc's clang, else c++filt (_Float16's mangling DF16_ is handed to either as the older Dh)"""
    hipcc = shutil.which("hipcc")
    if hipcc:
        for rel in ("../llvm/bin/llvm-cxxfilt", "../lib/llvm/bin/llvm-cxxfilt"):
            path = os.path.join(os.path.dirname(os.path.realpath(hipcc)), rel)
            if os.path.exists(path):
                return path
    return shutil.which("llvm-cxxfilt") or "c++filt"


def new_dimension(name):
    """the kernel's D where it is one of the dimensions this table is about: the template arguments hold it as <..., D, ...>"""
    m = re.search(r"<(.*)>", name)
    if not m:
        return None
    if "k_grid_nd_" in name:
        args = [a.strip() for a in m.group(1).split(",")]
        dims = [int(a) for a in args if a in ("5", "6", "7")]
        return dims[0] if dims else None
    args = [a.strip() for a in m.group(1).split(",")]
    ints = [a for a in args if re.fullmatch(r"\d+", a)]
    # k_grid_fwd<T, D, F>, k_grid_bwd<T, GT, D, F, S>, k_grid_bwd_input<T, D>, k_grid_scatter<D, F, R, S>, k_bin_*<D, ...>, k_grid_bwdbwd_*<.., D, ..>: D is the first integer
    if not ints or "k_bin_accum" in name or "k_grid_mask" in name:
        return None
    d = int(ints[0])
    return d if d in (1, 5, 6, 7) else None


def main():
    logs = None
    if "--logs" in sys.argv:
        logs = sys.argv[sys.argv.index("--logs") + 1]
    with tempfile.TemporaryDirectory() as tmp:
        if logs is None:
            with ThreadPoolExecutor(max_workers=4) as ex:
                paths = list(ex.map(lambda s: compile_log(s, tmp), SOURCES))
        else:
            paths = [os.path.join(logs, s + ".log") for s in SOURCES]
        rows = []
        for src, path in zip(SOURCES, paths):
            found = list(kernels(path))
            names = subprocess.run([demangler()], input="\n".join(r["name"].replace("DF16_", "Dh") for r in found), capture_output=True, text=True, check=True).stdout.splitlines()
            for r, name in zip(found, names):
                name = re.sub(r"tcnn_amd::\(anonymous namespace\)::", "", name)
                name = re.sub(r"^void |\(.*$", "", name)
                d = new_dimension(name)
                if d is not None:
                    rows.append((src, name, r))
    rows.sort(key=lambda t: (SOURCES.index(t[0]), t[1]))
    lines = ["# grid kernels instantiated for 1, 5, 6 and 7 input dimensions: hipcc --offload-arch=gfx950, the library's flags, -Rpass-analysis=kernel-resource-usage",
             "# (tools/grid_nd_resource_usage.py).  scratch: bytes per lane; occupancy: waves per SIMD; lds: static bytes per workgroup",
             f"{'source':22s} {'kernel':66s} {'VGPR':>5s} {'AGPR':>5s} {'scratch':>8s} {'occupancy':>10s} {'lds':>6s}"]
    for src, name, r in rows:
        lines.append(f"{src:22s} {name:66s} {r['vgpr']:5d} {r['agpr']:5d} {r['scratch']:8d} {r['occupancy']:10d} {r['lds']:6d}")
    spilling = [name for _, name, r in rows if r["scratch"] != 0]
    lines.append(f"# {len(rows)} kernels, {len(spilling)} with scratch")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-1:]))
    for name in spilling:
        print("scratch:", name)
    return 1 if spilling else 0


if __name__ == "__main__":
    sys.exit(main())
