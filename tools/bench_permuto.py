"""Time tcnn.Encoding PermutoGrid beside HashGrid of the same D (L = 16, F = 2, T = 2^19, half) at 2^18 rows for D = 3 .. 7: the forward
pass alone and forward + backward (parameter gradients).  One process; every repetition times each (D, encoding) once, in turn, with device
events around a warmed-up loop; median and range over the repetitions.  Beside the times: the gathers a forward pass issues (rows x levels x
(D + 1) on the lattice, x 2^D on the grid, 4 bytes each -- counted from the shapes, not measured), the rate per gather, and the lattice's time
as a fraction of the grid's next to the fraction of the gathers, (D + 1) / 2^D.
Writes profiles/permuto_bench.txt / .json (or --out-dir) and prints the JSON.  A GPU is required: there is no fallback.
--second-order: the same protocol for the second-order pass ("second_order": true), D = 3, 5, 7, through the native module (half): the
encoding's forward call; the tangent alone (backward_backward_input asked for dL_ddLdy only: one k_permuto_tangent launch for one direction);
that call three times over (three tangent() calls); the full call (tangent, zeros for dL/dx, the parameter gradient); and input_jvp with 1 and
with 3 tangents behind a 64 x 2 CutlassMLP -- the one caller of Encoding::tangents(), which serves all directions of a group in ONE launch.
No entry point runs tangents() alone: input_jvp_3 - input_jvp_1 is two more directions in that launch PLUS two more in the network.  HashGrid
(a tangent() call per direction) runs beside it as context.  Writes profiles/permuto_second_order_bench.txt / .json instead.
usage (GPU box): python tools/bench_permuto.py [--second-order] [--reps 7] [--iters 20] [--warmup 5] [--log2-batch 18]"""
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

SHAPE = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
DIMS = (3, 4, 5, 6, 7)
KINDS = {"PermutoGrid": lambda D: D + 1, "HashGrid": lambda D: 1 << D}  # gathers per (row, level)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


MLP = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
SECOND_ORDER_DIMS = (3, 5, 7)
SECOND_ORDER_PASSES = ("forward", "tangent", "three_tangent_calls", "second_order", "input_jvp_1_mlp", "input_jvp_3_mlp")


def second_order_runs(D, config, n, gen):
    """the timed calls of one (D, encoding): closures over device tensors made once"""
    x, v = torch.rand(n, D, device="cuda", generator=gen), torch.rand(n, 3, D, device="cuda", generator=gen) * 2 - 1
    enc, model = tcnn.Encoding(D, config), tcnn.NetworkWithInputEncoding(D, 16, config, MLP)
    native, params = enc.native_tcnn_module, enc.params.detach().half()
    dy = (torch.randn(n, native.n_output_dims(), device="cuda") * 1e-3).half()
    ctx = native.fwd(x.requires_grad_(True), params)[0]
    v0, v1, frozen, model_params = v[:, 0].contiguous(), v[:, :1].contiguous(), x.detach(), model.params.detach().half()

    def tangent():
        native.bwd_bwd_input(ctx, frozen, params.detach(), v0, dy.requires_grad_(True))

    def three_tangent_calls():
        for _ in range(3):
            tangent()

    return {"forward": lambda: native.fwd(frozen, params), "tangent": tangent, "three_tangent_calls": three_tangent_calls,
            "second_order": lambda: native.bwd_bwd_input(ctx, x, params.requires_grad_(True), v0, dy.requires_grad_(True)),
            "input_jvp_1_mlp": lambda: model.native_tcnn_module.input_jvp(frozen, model_params, v1),
            "input_jvp_3_mlp": lambda: model.native_tcnn_module.input_jvp(frozen, model_params, v)}


def second_order(args):
    n, gen = 1 << args.log2_batch, torch.Generator(device="cuda").manual_seed(42)
    configs = {"PermutoGrid": dict(SHAPE, otype="PermutoGrid", second_order=True), "HashGrid": dict(SHAPE, otype="HashGrid")}
    runs = {(D, kind): second_order_runs(D, config, n, gen) for D in SECOND_ORDER_DIMS for kind, config in configs.items()}
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
    result = {"metric": "native second-order pass of PermutoGrid (second_order) beside HashGrid, L16 F2 T2^19 half: forward, tangent alone, three tangent calls, full call, input_jvp (1 and 3 tangents) behind a 64x2 CutlassMLP",
              "unit": "ms", "rows": n, "reps": args.reps, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "dims": {str(D): {kind: {k: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for k, t in samples[D, kind].items()}
                                for kind in configs} for D in SECOND_ORDER_DIMS}}
    print(json.dumps(result), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "permuto_second_order_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    lines = [f"# {result['metric']}; {n} rows, {args.reps} alternating repetitions of {args.iters} calls, device events ({result['device']})",
             f"{'D':>2s} {'encoding':>11s} {'pass':>20s} {'ms (median, min .. max)':>34s}"]
    for D in SECOND_ORDER_DIMS:
        for kind in configs:
            for k, t in result["dims"][str(D)][kind].items():
                lines.append(f"{D:2d} {kind:>11s} {k:>20s} {t['median_ms']:12.4f} {t['min_ms']:9.4f} .. {t['max_ms']:8.4f}")
    with open(os.path.join(args.out_dir, "permuto_second_order_bench.txt"), "w") as f:
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
    assert torch.cuda.is_available(), "bench_permuto.py needs a GPU"
    if args.second_order:
        return second_order(args)
    n = 1 << args.log2_batch
    gen = torch.Generator(device="cuda").manual_seed(42)
    runs = {}
    for D in DIMS:
        x = torch.rand(n, D, device="cuda", generator=gen)
        for kind in KINDS:
            enc = tcnn.Encoding(D, dict(SHAPE, otype=kind))
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
    for _ in range(args.reps):  # alternating: each repetition visits every D, both encodings and both passes
        for key, passes in runs.items():
            for k, fn in passes.items():
                samples[key][k].append(timed(fn, args.iters))
    result = {"metric": "tcnn.Encoding PermutoGrid and HashGrid, L16 F2 T2^19 half: forward and forward+backward per call", "unit": "ms", "rows": n, "reps": args.reps,
              "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "dims": {}}
    for D in DIMS:
        per_d = {}
        for kind, per_level in KINDS.items():
            gathers = n * SHAPE["n_levels"] * per_level(D)
            row = {"forward_gathers": gathers}
            for k, v in samples[D, kind].items():
                row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            row["forward_gathers_per_s"] = round(gathers / (row["forward"]["median_ms"] * 1e-3), 0)
            per_d[kind] = row
        per_d["gather_fraction"] = round((D + 1) / (1 << D), 4)
        for k in ("forward", "forward_backward"):
            per_d[k + "_time_fraction"] = round(per_d["PermutoGrid"][k]["median_ms"] / per_d["HashGrid"][k]["median_ms"], 4)
        result["dims"][str(D)] = per_d
    print(json.dumps(result), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "permuto_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    lines = [f"# {result['metric']}; {n} rows, {args.reps} alternating repetitions of {args.iters} calls, device events ({result['device']})",
             "# gathers: rows x 16 levels x (D + 1 | 2^D), counted; rate = gathers / forward median; fractions: PermutoGrid / HashGrid of the same D",
             f"{'D':>2s} {'encoding':>11s} {'forward ms (median, min .. max)':>34s} {'fwd+bwd ms (median, min .. max)':>34s} {'gathers':>12s} {'Ggathers/s':>11s}"]
    for D in DIMS:
        per_d = result["dims"][str(D)]
        for kind in KINDS:
            r = per_d[kind]
            f_, b_ = r["forward"], r["forward_backward"]
            lines.append(f"{D:2d} {kind:>11s} {f_['median_ms']:12.4f} {f_['min_ms']:9.4f} .. {f_['max_ms']:8.4f} {b_['median_ms']:12.4f} {b_['min_ms']:9.4f} .. {b_['max_ms']:8.4f} "
                         f"{r['forward_gathers']:12d} {r['forward_gathers_per_s'] / 1e9:11.2f}")
        lines.append(f"{D:2d}   fractions: gathers {per_d['gather_fraction']:.4f}, forward time {per_d['forward_time_fraction']:.4f}, forward+backward time {per_d['forward_backward_time_fraction']:.4f}")
    with open(os.path.join(args.out_dir, "permuto_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
