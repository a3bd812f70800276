"""Time tcnn.Encoding TensoRF (half; one level) at 2^18 rows: VM at F = 16 and 32 and CP at D = 3 and 4 (F = 16), each at R = 128 and 300, beside
KPlanes/Sum at D = 3 (its defaults) and HashGrid (L = 16, F = 2, T = 2^19): the forward pass alone and forward + backward (parameter
gradients).  tools/bench_kplanes.py's protocol: one process; every repetition times each encoding once, in turn, with device events around a
warmed-up loop; median and range over the repetitions.  The encodings are different functions of different widths: the table says what each
costs per call.  Writes profiles/tensorf_bench.txt / .json (or --out-dir) and prints the JSON.  A GPU is required: there is no fallback.
usage (GPU box): python tools/bench_tensorf.py [--reps 7] [--iters 20] [--warmup 5] [--log2-batch 18]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))

import torch  # noqa: E402

import tinycudann as tcnn  # noqa: E402


def tensorf(decomposition, F, R):
    return {"otype": "TensoRF", "decomposition": decomposition, "n_components": F, "n_levels": 1, "base_resolution": R}


# name -> (D, config)
KINDS = {f"TensoRF/VM F{F} R{R}": (3, tensorf("VM", F, R)) for F in (16, 32) for R in (128, 300)}
KINDS.update({f"TensoRF/CP {D}-D F16 R{R}": (D, tensorf("CP", 16, R)) for D in (3, 4) for R in (128, 300)})
KINDS["KPlanes/Sum"] = (3, {"otype": "KPlanes", "reduction": "Sum"})
KINDS["HashGrid"] = (3, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0})


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log2-batch", type=int, default=18)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tensorf.py needs a GPU"
    n = 1 << args.log2_batch
    gen = torch.Generator(device="cuda").manual_seed(42)
    inputs = {D: torch.rand(n, D, device="cuda", generator=gen) for D in (3, 4)}
    runs, shapes = {}, {}
    for kind, (D, config) in KINDS.items():
        enc, x = tcnn.Encoding(D, config), inputs[D]
        shapes[kind] = {"n_input_dims": D, "n_output_dims": enc.n_output_dims, "n_params": enc.params.numel()}
        w = torch.randn(enc.n_output_dims, device="cuda", dtype=torch.float16) * 1e-3

        def forward(enc=enc, x=x):
            with torch.no_grad():
                enc(x)

        def forward_backward(enc=enc, x=x, w=w):
            enc.params.grad = None
            (enc(x) * w).sum().backward()

        runs[kind] = {"forward": forward, "forward_backward": forward_backward}
        for fn in runs[kind].values():  # warm up every shape the timed window uses
            for _ in range(args.warmup):
                fn()
    torch.cuda.synchronize()
    samples = {kind: {k: [] for k in passes} for kind, passes in runs.items()}
    for _ in range(args.reps):  # alternating: each repetition visits every encoding and both passes
        for kind, passes in runs.items():
            for k, fn in passes.items():
                samples[kind][k].append(timed(fn, args.iters))
    result = {"metric": "tcnn.Encoding TensoRF (one level) beside KPlanes/Sum (defaults) and HashGrid (L16 F2 T2^19), half: forward and forward+backward per call", "unit": "ms", "rows": n,
              "reps": args.reps, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "encodings": {}}
    for kind in KINDS:
        row = dict(shapes[kind])
        for k, v in samples[kind].items():
            row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        result["encodings"][kind] = row
    print(json.dumps(result), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "tensorf_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    lines = [f"# {result['metric']}; {n} rows, {args.reps} alternating repetitions of {args.iters} calls, device events ({result['device']})",
             f"{'encoding':>24s} {'D':>2s} {'columns':>7s} {'parameters':>10s} {'forward ms (median, min .. max)':>34s} {'fwd+bwd ms (median, min .. max)':>34s}"]
    for kind, r in result["encodings"].items():
        f_, b_ = r["forward"], r["forward_backward"]
        lines.append(f"{kind:>24s} {r['n_input_dims']:2d} {r['n_output_dims']:7d} {r['n_params']:10d} {f_['median_ms']:12.4f} {f_['min_ms']:9.4f} .. {f_['max_ms']:8.4f} "
                     f"{b_['median_ms']:12.4f} {b_['min_ms']:9.4f} .. {b_['max_ms']:8.4f}")
    with open(os.path.join(args.out_dir, "tensorf_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
