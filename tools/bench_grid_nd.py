"""Time tcnn.Encoding (HashGrid, L = 16, F = 2, T = 2^19, half) at 2^18 rows for D = 1, 4, 5, 6 and 7 input dimensions: the forward pass
alone and forward + backward (parameter gradients).  One process; every repetition times each D once, in turn, with device events around
a warmed-up loop; median and range over the repetitions.  Beside the times: the gathers the forward pass issues (rows x levels x 2^D,
4 bytes each -- counted from the shapes, not measured) and the rate per gather, to be read against the 4-D figure of the same run.
Writes profiles/grid_nd_bench.txt / .json (or --out-dir) and prints the JSON.  A GPU is required: there is no fallback.
usage (GPU box): python tools/bench_grid_nd.py [--reps 7] [--iters 20] [--warmup 5] [--log2-batch 18] [--only D]   (--only: one D, for a profiler run)"""
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

ENCODING = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
DIMS = (1, 4, 5, 6, 7)


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
    ap.add_argument("--only", type=int, choices=DIMS)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_grid_nd.py needs a GPU"
    n = 1 << args.log2_batch
    dims = (args.only,) if args.only else DIMS
    gen = torch.Generator(device="cuda").manual_seed(42)
    runs = {}
    for D in dims:
        enc = tcnn.Encoding(D, ENCODING)
        x = torch.rand(n, D, device="cuda", generator=gen)
        w = torch.randn(enc.n_output_dims, device="cuda", dtype=torch.float16) * 1e-3

        def forward(enc=enc, x=x):
            with torch.no_grad():
                enc(x)

        def forward_backward(enc=enc, x=x, w=w):
            enc.params.grad = None
            (enc(x) * w).sum().backward()

        runs[D] = {"forward": forward, "forward_backward": forward_backward}
        for fn in runs[D].values():  # warm up every shape the timed window uses
            for _ in range(args.warmup):
                fn()
    torch.cuda.synchronize()
    samples = {D: {k: [] for k in runs[D]} for D in dims}
    for _ in range(args.reps):  # alternating: each repetition visits every D and both passes
        for D in dims:
            for k, fn in runs[D].items():
                samples[D][k].append(timed(fn, args.iters))
    result = {"metric": "tcnn.Encoding HashGrid L16 F2 T2^19 half: forward and forward+backward per call", "unit": "ms", "rows": n, "reps": args.reps, "iters": args.iters,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "dims": {}}
    for D in dims:
        gathers = n * ENCODING["n_levels"] * (1 << D)
        row = {"forward_gathers": gathers}
        for k, v in samples[D].items():
            row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        row["forward_gathers_per_s"] = round(gathers / (row["forward"]["median_ms"] * 1e-3), 0)
        result["dims"][str(D)] = row
    if "4" in result["dims"]:
        base = result["dims"]["4"]["forward_gathers_per_s"]
        for row in result["dims"].values():
            row["gather_rate_vs_4d"] = round(row["forward_gathers_per_s"] / base, 3)
    print(json.dumps(result), flush=True)
    if args.only:
        return
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "grid_nd_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    lines = [f"# {result['metric']}; {n} rows, {args.reps} alternating repetitions of {args.iters} calls, device events ({result['device']})",
             f"# gathers: rows x 16 levels x 2^D (counted); rate = gathers / forward median", f"{'D':>2s} {'forward ms (median, min .. max)':>34s} {'fwd+bwd ms (median, min .. max)':>34s} {'gathers':>12s} {'Ggathers/s':>11s} {'vs 4-D':>7s}"]
    for D in dims:
        r = result["dims"][str(D)]
        f_, b_ = r["forward"], r["forward_backward"]
        lines.append(f"{D:2d} {f_['median_ms']:12.4f} {f_['min_ms']:9.4f} .. {f_['max_ms']:8.4f} {b_['median_ms']:12.4f} {b_['min_ms']:9.4f} .. {b_['max_ms']:8.4f} {r['forward_gathers']:12d} "
                     f"{r['forward_gathers_per_s'] / 1e9:11.2f} {r.get('gather_rate_vs_4d', float('nan')):7.3f}")
    with open(os.path.join(args.out_dir, "grid_nd_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
