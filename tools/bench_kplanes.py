"""Time tcnn.Encoding KPlanes (its defaults: L = 4, F = 2, base_resolution 64, per_level_scale 2; Product and Sum, half) beside HashGrid and
PermutoGrid of the same D (L = 16, F = 2, T = 2^19) at 2^18 rows for D = 3 and 4: the forward pass alone and forward + backward (parameter
gradients).  One process; every repetition times each (D, encoding) once, in turn, with device events around a warmed-up loop; median and
range over the repetitions.  Beside the times: the gathers a forward pass issues (rows x levels x gathers per level, counted from the shapes,
not measured) and the rate per gather.  The three encodings are different functions with different widths (8 columns against 32): the table
says what each costs per call, not which fits a field better.
Writes profiles/kplanes_bench.txt / .json (or --out-dir) and prints the JSON.  A GPU is required: there is no fallback.
--second-order: the same protocol for the second-order pass, through the native module (half): the tangent alone (backward_backward_input
asked for dL_ddLdy only), the full call (tangent, dL/dx and the parameter gradient) and input_jvp with 3 tangents behind a 64 x 2 CutlassMLP,
for KPlanes and for HashGrid; writes profiles/kplanes_second_order_bench.txt / .json instead.
usage (GPU box): python tools/bench_kplanes.py [--second-order] [--reps 7] [--iters 20] [--warmup 5] [--log2-batch 18]"""
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

HASHED = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
DIMS = (3, 4)
# name -> (config, levels, gathers per (row, level))
KINDS = {"KPlanes/Product": lambda D: ({"otype": "KPlanes", "reduction": "Product"}, 4, 2 * D * (D - 1)),
         "KPlanes/Sum": lambda D: ({"otype": "KPlanes", "reduction": "Sum"}, 4, 2 * D * (D - 1)),
         "HashGrid": lambda D: (dict(HASHED, otype="HashGrid"), 16, 1 << D),
         "PermutoGrid": lambda D: (dict(HASHED, otype="PermutoGrid"), 16, D + 1)}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


MLP = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
SECOND_ORDER_KINDS = ("KPlanes/Product", "KPlanes/Sum", "HashGrid")


def second_order_runs(D, config, n, gen):
    """the three timed calls of one (D, encoding): closures over device tensors made once"""
    x, v = torch.rand(n, D, device="cuda", generator=gen), torch.rand(n, 3, D, device="cuda", generator=gen) * 2 - 1
    enc, model = tcnn.Encoding(D, config), tcnn.NetworkWithInputEncoding(D, 16, config, MLP)
    native, params = enc.native_tcnn_module, enc.params.detach().half()
    dy = (torch.randn(n, native.n_output_dims(), device="cuda") * 1e-3).half()
    ctx = native.fwd(x.requires_grad_(True), params)[0]
    v0, frozen, model_params = v[:, 0].contiguous(), x.detach(), model.params.detach().half()

    def full():
        native.bwd_bwd_input(ctx, x, params.requires_grad_(True), v0, dy.requires_grad_(True))

    return {"tangent": lambda: native.bwd_bwd_input(ctx, frozen, params.detach(), v0, dy.requires_grad_(True)), "second_order": full,
            "input_jvp_3_mlp": lambda: model.native_tcnn_module.input_jvp(frozen, model_params, v)}


def second_order(args):
    n, gen = 1 << args.log2_batch, torch.Generator(device="cuda").manual_seed(42)
    runs = {(D, kind): second_order_runs(D, KINDS[kind](D)[0], n, gen) for D in DIMS for kind in SECOND_ORDER_KINDS}
    for passes in runs.values():
        for fn in passes.values():
            for _ in range(args.warmup):
                fn()
    torch.cuda.synchronize()
    samples = {key: {k: [] for k in passes} for key, passes in runs.items()}
    for _ in range(args.reps):
        for key, passes in runs.items():
            for k, fn in passes.items():
                samples[key][k].append(timed(fn, args.iters))
    result = {"metric": "native second-order pass of KPlanes (defaults) beside HashGrid (L16 F2 T2^19), half: tangent alone, full call, input_jvp (3 tangents) behind a 64x2 CutlassMLP", "unit": "ms",
              "rows": n, "reps": args.reps, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "dims": {str(D): {kind: {k: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for k, t in samples[D, kind].items()}
                                for kind in SECOND_ORDER_KINDS} for D in DIMS}}
    print(json.dumps(result), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "kplanes_second_order_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    lines = [f"# {result['metric']}; {n} rows, {args.reps} alternating repetitions of {args.iters} calls, device events ({result['device']})",
             f"{'D':>2s} {'encoding':>16s} " + " ".join(f"{k + ' ms (median, min .. max)':>40s}" for k in ("tangent", "second_order", "input_jvp_3_mlp"))]
    for D in DIMS:
        for kind in SECOND_ORDER_KINDS:
            r = result["dims"][str(D)][kind]
            lines.append(f"{D:2d} {kind:>16s} " + " ".join(f"{t['median_ms']:18.4f} {t['min_ms']:9.4f} .. {t['max_ms']:8.4f}" for t in r.values()))
    with open(os.path.join(args.out_dir, "kplanes_second_order_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--second-order", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log2-batch", type=int, default=18)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kplanes.py needs a GPU"
    if args.second_order:
        return second_order(args)
    n = 1 << args.log2_batch
    gen = torch.Generator(device="cuda").manual_seed(42)
    runs, shapes = {}, {}
    for D in DIMS:
        x = torch.rand(n, D, device="cuda", generator=gen)
        for kind, make in KINDS.items():
            config, levels, per_level = make(D)
            enc = tcnn.Encoding(D, config)
            shapes[D, kind] = {"n_output_dims": enc.n_output_dims, "n_params": enc.params.numel(), "forward_gathers": n * levels * per_level}
            w = torch.randn(enc.n_output_dims, device="cuda", dtype=torch.float16) * 1e-3

            def forward(enc=enc, x=x):
                with torch.no_grad():
                    enc(x)

            def forward_backward(enc=enc, x=x, w=w):
                enc.params.grad = None
                (enc(x) * w).sum().backward()

            runs[D, kind] = {"forward": forward, "forward_backward": forward_backward}
            for fn in runs[D, kind].values():  # warm up every shape the timed window uses
                for _ in range(args.warmup):
                    fn()
    torch.cuda.synchronize()
    samples = {key: {k: [] for k in passes} for key, passes in runs.items()}
    for _ in range(args.reps):  # alternating: each repetition visits every D, every encoding and both passes
        for key, passes in runs.items():
            for k, fn in passes.items():
                samples[key][k].append(timed(fn, args.iters))
    result = {"metric": "tcnn.Encoding KPlanes (defaults) beside HashGrid and PermutoGrid (L16 F2 T2^19), half: forward and forward+backward per call", "unit": "ms", "rows": n,
              "reps": args.reps, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "dims": {}}
    for D in DIMS:
        per_d = {}
        for kind in KINDS:
            row = dict(shapes[D, kind])
            for k, v in samples[D, kind].items():
                row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            row["forward_gathers_per_s"] = round(row["forward_gathers"] / (row["forward"]["median_ms"] * 1e-3), 0)
            per_d[kind] = row
        result["dims"][str(D)] = per_d
    print(json.dumps(result), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "kplanes_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    lines = [f"# {result['metric']}; {n} rows, {args.reps} alternating repetitions of {args.iters} calls, device events ({result['device']})",
             "# gathers: rows x levels x (4 C(D, 2) | 2^D | D + 1), counted; rate = gathers / forward median",
             f"{'D':>2s} {'encoding':>16s} {'columns':>7s} {'parameters':>10s} {'forward ms (median, min .. max)':>34s} {'fwd+bwd ms (median, min .. max)':>34s} {'gathers':>12s} {'Ggathers/s':>11s}"]
    for D in DIMS:
        for kind in KINDS:
            r = result["dims"][str(D)][kind]
            f_, b_ = r["forward"], r["forward_backward"]
            lines.append(f"{D:2d} {kind:>16s} {r['n_output_dims']:7d} {r['n_params']:10d} {f_['median_ms']:12.4f} {f_['min_ms']:9.4f} .. {f_['max_ms']:8.4f} {b_['median_ms']:12.4f} {b_['min_ms']:9.4f} .. "
                         f"{b_['max_ms']:8.4f} {r['forward_gathers']:12d} {r['forward_gathers_per_s'] / 1e9:11.2f}")
    with open(os.path.join(args.out_dir, "kplanes_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
