"""Time tcnn.Encoding TensoRF (half; one level) at 2^18 rows: VM at F = 16 and 32 and CP at D = 3 and 4 (F = 16), each at R = 128 and 300, beside
KPlanes/Sum at D = 3 (its defaults) and HashGrid (L = 16, F = 2, T = 2^19): the forward pass alone and forward + backward (parameter
gradients).  tools/bench_kplanes.py's protocol: one process; every repetition times each encoding once, in turn, with device events around a
warmed-up loop; median and range over the repetitions.  The encodings are different functions of different widths: the table says what each
costs per call.  Writes profiles/tensorf_bench.txt / .json (or --out-dir) and prints the JSON.  A GPU is required: there is no fallback.
--second-order: the same protocol for the second-order pass ("second_order": true) of VM F = 16 and CP 4-D F = 16 at R = 128, through the
native module (half): the forward call; the first-order backward call (dL/dx and dL/dparams); the tangent alone (backward_backward_input asked
for dL_ddLdy only: one k_tensorf_tangent launch for one direction); that call three times over; the full call (tangent, dQ/dx, dQ/dparams);
and input_jvp with 1 and with 3 tangents behind a 64 x 2 CutlassMLP -- the one caller of Encoding::tangents(), which serves all directions of
a group in ONE launch.  No entry point runs tangents() alone: input_jvp_3 - input_jvp_1 is two more directions in that launch PLUS two more
in the network.  Writes profiles/tensorf_second_order_bench.txt / .json instead.
usage (GPU box): python tools/bench_tensorf.py [--second-order] [--reps 7] [--iters 20] [--warmup 5] [--log2-batch 18]"""
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


MLP = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
SECOND_ORDER_KINDS = {"TensoRF/VM F16 R128": (3, tensorf("VM", 16, 128)), "TensoRF/CP 4-D F16 R128": (4, tensorf("CP", 16, 128))}


def second_order_runs(D, config, n, gen):
    """the timed calls of one encoding: closures over device tensors made once"""
    x, v = torch.rand(n, D, device="cuda", generator=gen), torch.rand(n, 3, D, device="cuda", generator=gen) * 2 - 1
    enc, model = tcnn.Encoding(D, config), tcnn.NetworkWithInputEncoding(D, 16, config, MLP)
    native, params = enc.native_tcnn_module, enc.params.detach().half()
    dy = (torch.randn(n, native.n_output_dims(), device="cuda") * 1e-3).half()
    ctx, out = native.fwd(x.requires_grad_(True), params.requires_grad_(True))
    v0, v1, frozen, model_params = v[:, 0].contiguous(), v[:, :1].contiguous(), x.detach(), model.params.detach().half()

    def tangent():
        native.bwd_bwd_input(ctx, frozen, params.detach(), v0, dy.requires_grad_(True))

    def three_tangent_calls():
        for _ in range(3):
            tangent()

    return {"forward": lambda: native.fwd(frozen, params.detach()), "first_order_backward": lambda: native.bwd(ctx, x, params, out, dy), "tangent": tangent,
            "three_tangent_calls": three_tangent_calls, "second_order": lambda: native.bwd_bwd_input(ctx, x, params, v0, dy.requires_grad_(True)),
            "input_jvp_1_mlp": lambda: model.native_tcnn_module.input_jvp(frozen, model_params, v1),
            "input_jvp_3_mlp": lambda: model.native_tcnn_module.input_jvp(frozen, model_params, v)}


def second_order(args):
    n, gen = 1 << args.log2_batch, torch.Generator(device="cuda").manual_seed(42)
    runs = {kind: second_order_runs(D, dict(config, second_order=True), n, gen) for kind, (D, config) in SECOND_ORDER_KINDS.items()}
    for passes in runs.values():
        for fn in passes.values():
            for _ in range(args.warmup):
                fn()
    torch.cuda.synchronize()
    samples = {kind: {k: [] for k in passes} for kind, passes in runs.items()}
    for _ in range(args.reps):  # alternating: each repetition visits both encodings and every pass
        for kind, passes in runs.items():
            for k, fn in passes.items():
                samples[kind][k].append(timed(fn, args.iters))
    result = {"metric": "native second-order pass of TensoRF (second_order, one level, half): forward, first-order backward, tangent alone, three tangent calls, full call, input_jvp (1 and 3 tangents) behind a 64x2 CutlassMLP",
              "unit": "ms", "rows": n, "reps": args.reps, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "encodings": {kind: {k: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for k, t in samples[kind].items()} for kind in runs}}
    print(json.dumps(result), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "tensorf_second_order_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    lines = [f"# {result['metric']}; {n} rows, {args.reps} alternating repetitions of {args.iters} calls, device events ({result['device']})",
             f"{'encoding':>24s} {'pass':>22s} {'ms (median, min .. max)':>34s}"]
    lines += [f"{kind:>24s} {k:>22s} {t['median_ms']:12.4f} {t['min_ms']:9.4f} .. {t['max_ms']:8.4f}" for kind, passes in result["encodings"].items() for k, t in passes.items()]
    with open(os.path.join(args.out_dir, "tensorf_second_order_bench.txt"), "w") as f:
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
    assert torch.cuda.is_available(), "bench_tensorf.py needs a GPU"
    if args.second_order:
        return second_order(args)
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
