"""How far the device's expf, logf, sinf, cosf and tanhf are from correctly rounded, in float steps: the K_f of tests/activation_sweep_f32.py --
and its powf(beta, t), the one libm call of Adam's debiasing factor: the K_POWF of tests/adam_reference.py.

    python tools/libm_f32_ulp.py arguments ARGS.f32 POW_ARGS.f32       # the arguments: the sweep, what the expressions of mlp_device.h pass, and (beta, t)
    tools/ubench/libm_f32 ARGS.f32 RESULTS.f32 POW_ARGS.f32 POW.f32    # on the GPU (tools/ubench/libm_f32.hip)
    python tools/libm_f32_ulp.py report RESULTS.f32 POW.f32 [PROFILE]  # largest distance and a histogram per function -> profiles/libm_f32_ulp.txt

The yardstick is the float64 value rounded once to float32 (activation_sweep._rounded; adam_reference.pow_rounded); no kernel of the project
takes part.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import activation_sweep as sw  # noqa: E402
import adam_reference as ar  # noqa: E402
import activation_sweep_f32 as s32  # noqa: E402

F = np.float32
FUNCTIONS = [("expf", np.exp), ("logf", np.log), ("sinf", np.sin), ("cosf", np.cos), ("tanhf", np.tanh)]


def segments():
    """[(name, float32 array, the functions whose expressions pass it)]"""
    x = s32.sweep_x().ravel()
    with np.errstate(all="ignore"):
        x10 = x * s32.K_ACT
        y = s32.activation_fwd(s32.ONE_CANDIDATE, "Softplus", x[None])[0]
        e = sw._rounded(np.exp)(x10)
        one_plus = np.concatenate([s32.moved(e, j) + F(1) for j in range(-s32.MAX_K, s32.MAX_K + 1)])
    return [
        ("x", x, ("expf", "logf", "sinf", "cosf", "tanhf")),  # the sweep itself: every function (logf: the bare function only)
        ("-x", -x, ("expf",)),                                # logistic, expf_near_zero in Sigmoid' and ''
        ("10 x", x10, ("expf",)),                             # Softplus
        ("-10 x", -x10, ("expf",)),                           # logistic(10 x): Softplus' and ''
        ("-10 y", -y * s32.K_ACT, ("expf",)),                 # activation_bwd's Softplus, y its forward output (expf from 2^-6 on)
        ("1 + expf(10 x)", one_plus, ("logf",)),              # Softplus; expf(10 x) within MAX_K steps of correctly rounded
    ]


def write_arguments(path, pow_path):
    a = np.concatenate([s[1] for s in segments()]).astype(F)
    a.tofile(path)
    print(f"{a.size} arguments -> {path}")
    p = ar.pow_arguments()
    p.tofile(pow_path)
    print(f"{p.shape[0]} (beta, t) pairs -> {pow_path}")


def pow_report(pow_results_path):
    """(K_POWF, the table's rows): powf(beta, t) for every beta of tests/adam_reference.py, t = 1 .. 64"""
    args = ar.pow_arguments()
    got = np.fromfile(pow_results_path, dtype=F)
    assert got.size == args.shape[0], (got.size, args.shape[0])
    unlike_all = ~np.isfinite(got) | (got <= 0)
    d_all = ar.float_steps(np.where(unlike_all, F(1), got), ar.pow_rounded(args))
    rows = []
    for beta in ar.BETAS:
        sel = args[:, 0] == F(beta)
        d, unlike = d_all[sel], unlike_all[sel]
        d_like = d[~unlike]
        worst = int(d_like.max()) if d_like.size else 0
        hist = np.bincount(np.minimum(d_like, 9), minlength=10)
        where = f"t = {int(args[sel][int(np.argmax(np.where(unlike, 0, d))), 1])}" if worst else ""
        rows.append(f"{'powf':<6} {f'({beta!r}, 1 .. {ar.POW_STEPS[-1]})':<16} {'yes':<5} {int(sel.sum()):>8} {worst:>6} {int(unlike.sum()):>7}  " + " ".join(f"{int(h):>7}" for h in hist) + f"  {where}")
    k = (1 << 30) if unlike_all.any() else int(d_all.max())
    return k, rows


def distances(fn, args, got):
    with np.errstate(all="ignore"):
        want = sw._rounded(fn)(args)
    d = np.abs(s32.ordered(got) - s32.ordered(want))
    both_nan = np.isnan(got) & np.isnan(want)
    same_inf = np.isinf(got) & (got == want)
    unlike = (np.isfinite(got) != np.isfinite(want)) | (np.isnan(got) != np.isnan(want))
    d[both_nan | same_inf] = 0
    return d, unlike


def report(results_path, pow_results_path, profile_path):
    segs = segments()
    n = sum(s[1].size for s in segs)
    res = np.fromfile(results_path, dtype=F)
    assert res.size == 5 * n, (res.size, n)
    res = res.reshape(5, n)
    lines = ["The device's libm against the correctly rounded value (float64, rounded once), in float steps, on an MI355X: tools/ubench/libm_f32.hip,",
             "compiled with build.py's FLAGS, over the sweep of tests/activation_sweep_f32.py (x) and over the arguments the expressions of mlp_device.h",
             "pass (tools/libm_f32_ulp.py).  K_f: the largest distance over the sweep and the arguments the function is called with; the other rows are",
             "for the record.  unlike: results that are finite on one side only (or NaN on one side only), none of which a distance describes.",
             "powf: powf(beta, t) as Adam's debiasing factor calls it (adam_debias, k_misc.hip), for every beta of tests/adam_reference.py and t = 1 .. 64:",
             "K_POWF is the tolerance constant of that file.",
             ""]
    ks = {}
    table = []
    for i, (name, fn) in enumerate(FUNCTIONS):
        at = 0
        for seg, args, users in segs:
            got = res[i, at:at + args.size]
            at += args.size
            d, unlike = distances(fn, args, got)
            d_like = d[~unlike]
            worst = int(d_like.max()) if d_like.size else 0
            hist = np.bincount(np.minimum(d_like, 9), minlength=10)
            used = name in users
            if used:
                ks[name] = max(ks.get(name, 0), worst)
                if unlike.any():
                    ks[name] = max(ks[name], 1 << 30)
            where = ""
            if worst:
                j = int(np.argmax(np.where(unlike, 0, d)))
                where = f"{float(args[j])!r}"
            table.append(f"{name:<6} {seg:<16} {'yes' if used else 'no':<5} {args.size:>8} {worst:>6} {int(unlike.sum()):>7}  " + " ".join(f"{int(h):>7}" for h in hist) + f"  {where}")
    ks["powf"], pow_rows = pow_report(pow_results_path)
    table += pow_rows
    for name in [f[0] for f in FUNCTIONS] + ["powf"]:
        lines.append(f"K_{name.upper():<6} = {ks[name]}")
    lines += ["", f"{'libm':<6} {'arguments':<16} {'K_f?':<5} {'count':>8} {'worst':>6} {'unlike':>7}  " + " ".join(f"{'=' + str(k):>7}" for k in range(9)) + f" {'>=9':>7}  worst at"]
    lines += table
    text = "\n".join(lines) + "\n"
    print(text)
    if profile_path:
        with open(profile_path, "w") as f:
            f.write(text)
    return ks


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "arguments":
        write_arguments(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 4 and sys.argv[1] == "report":
        report(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "libm_f32_ulp.txt"))
    else:
        sys.exit(__doc__)
