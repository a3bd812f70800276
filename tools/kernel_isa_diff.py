"""Compare the device code of kernel files between two source trees, instruction by instruction.

    python tools/kernel_isa_diff.py <parent tree> <branch tree> [csrc files ...] [--keep DIR] [--jobs N]

For a refactoring of hand-scheduled kernels: the claim "nothing changed" is checked on what the compiler emits, not on the source.  Each
file of each tree is compiled to gfx950 assembly with that tree's own build.py flags (FLAGS + EXTRA_FLAGS[file]; `-x hip
--cuda-device-only -S`: no GPU, no linking), once as the product and once with -DTCNN_AMD_DEV.  Comments, .file / .ident / .loc lines and the
per-compilation __hip_cuid_* symbol are dropped, and so is the function's index in the module from its local labels (.LBB<index>_<block>,
.Lfunc_begin<index>, .Lfunc_end<index>: removing a kernel from a file renumbers those of every kernel behind it and changes no
instruction); then the two texts are compared:

  * per file: is the whole remaining assembly identical (then the code object is the parent's);
  * per kernel symbol: are the instruction stream and the resource metadata (vgpr / agpr / sgpr counts, LDS and scratch bytes) identical;
    if not, how many lines differ (a unified diff's + and - lines) and which metadata fields moved.

It only diffs; it looks for no particular instruction.  Exit status 0: every file identical in both builds, 1 otherwise.
"""
import argparse
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

DEFAULT_FILES = ["k_train_r32.hip", "k_train_r32a.hip", "k_train_r32w.hip", "k_train_r32ob.hip", "k_train_regs.hip", "k_train.hip"]
LOCAL_LABEL = re.compile(r"\.L(BB|func_begin|func_end)\d+")  # the block number behind it (_<block>) stays
META_KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"]


def load_build(tree):
    path = os.path.join(tree, "tiny-cuda-nn_amd", "build.py")
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_to_asm(tree, build, src, dev, out):
    cmd = (["hipcc"] + list(build.FLAGS) + (["-DTCNN_AMD_DEV"] if dev else []) + list(build.EXTRA_FLAGS.get(src, []))
           + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(tree, "tiny-cuda-nn_amd", "csrc", src), "-o", out])
    subprocess.check_call(cmd)
    with open(out) as f:
        return f.read()


def strip(text):
    lines = []
    for line in text.splitlines():
        s = line.strip()
        if not s.startswith((".asciz", ".ascii", ".string")):
            s = s.split(";", 1)[0].rstrip()
        if not s or s.startswith((".file", ".ident", ".loc")) or "__hip_cuid_" in s:
            continue
        s = LOCAL_LABEL.sub(r".L\1", s)
        lines.append(s)
    return lines


def kernels(lines):
    """{symbol: (instruction lines, {metadata key: value})} of the .amdhsa_kernel symbols"""
    names = [l.split()[1] for l in lines if l.startswith(".amdhsa_kernel ")]
    meta = {n: {} for n in names}
    # the code-object metadata: one list item per kernel.  Stripped lines have lost their indentation: the fields wanted are told apart by
    # name (a kernel's .name follows its arguments' and is the last one before .wavefront_size -- fields are sorted by name)
    item = {}
    for l in lines:
        m = re.match(r"^(?:- )?(\.[a-z_]+):\s*(.*)$", l)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key in META_KEYS or key == ".name":
            item[key] = val
        if key == ".wavefront_size":  # the last field of a kernel's item
            if item.get(".name") in meta:
                meta[item[".name"]] = {k: item.get(k) for k in META_KEYS}
            item = {}
    body = {}
    for n in names:
        try:
            start = lines.index(n + ":")
        except ValueError:
            body[n] = []
            continue
        end = start
        while end < len(lines) and not lines[end].startswith(".size\t" + n) and not lines[end].startswith(".size " + n):
            end += 1
        body[n] = lines[start:end]
    return {n: (body[n], meta[n]) for n in names}


def n_diff(a, b):
    return sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))


def compare(src, dev, pa, br, report):
    tag = "%s [%s]" % (src, "dev" if dev else "product")
    if pa == br:
        nk = len(kernels(br))
        report.append("%-36s identical (%d stripped lines, %d kernels)" % (tag, len(br), nk))
        return True
    report.append("%-36s DIFFERS: %d of %d stripped lines" % (tag, n_diff(pa, br), len(pa)))
    kp, kb = kernels(pa), kernels(br)
    if list(kp) != list(kb):
        report.append("    kernel symbols or their order differ: %d in the parent, %d in the branch" % (len(kp), len(kb)))
    for n in kb:
        if n not in kp:
            report.append("    %s: new" % n)
            continue
        (ip, mp), (ib, mb) = kp[n], kb[n]
        moved = ["%s %s -> %s" % (k, mp.get(k), mb.get(k)) for k in META_KEYS if mp.get(k) != mb.get(k)]
        stream = "stream identical" if ip == ib else "stream differs in %d of %d lines" % (n_diff(ip, ib), len(ip))
        report.append("    %s: %s; metadata %s" % (n, stream, "identical" if not moved else ", ".join(moved)))
    return False


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("files", nargs="*", default=DEFAULT_FILES)
    ap.add_argument("--keep", help="keep the assembly files in this directory")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--product-only", action="store_true", help="skip the -DTCNN_AMD_DEV build (quick look while working)")
    args = ap.parse_args()
    trees = {"parent": os.path.abspath(args.parent), "branch": os.path.abspath(args.branch)}
    builds = {k: load_build(t) for k, t in trees.items()}
    tmp = args.keep or tempfile.mkdtemp(prefix="isa_diff_")
    os.makedirs(tmp, exist_ok=True)
    jobs = [(which, src, dev) for src in args.files for dev in ([False] if args.product_only else [False, True]) for which in ("parent", "branch")]

    def run(job):
        which, src, dev = job
        out = os.path.join(tmp, "%s.%s%s.s" % (os.path.splitext(src)[0], which, ".dev" if dev else ""))
        return job, strip(compile_to_asm(trees[which], builds[which], src, dev, out))

    with ThreadPoolExecutor(max_workers=args.jobs) as ex:
        asm = dict(ex.map(run, jobs))
    report = []
    same = True
    for src in args.files:
        for dev in ([False] if args.product_only else [False, True]):
            same &= compare(src, dev, asm[("parent", src, dev)], asm[("branch", src, dev)], report)
    print("\n".join(report))
    print("all identical" if same else "NOT all identical")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
