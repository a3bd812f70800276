"""Full-precision networks (k_mlp_layers.hip; weight gradients: k_mlp_layers_f32.hip): forward + backward time of tcnn.Network(dtype=torch.float32) at 2^18 rows beside what a
user had before it existed -- a torch.nn.Sequential of bias-free Linear layers in fp32 -- and beside the half tcnn.Network, for scale.

    python tools/bench_fp32_network.py [--reps 7] [--steps 20] [--txt out.txt] [--json out.json] [--only-tcnn-fp32]

The arms alternate in one process: `reps` repetitions of `steps` steps between device events each; median and range are reported.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool with --only-tcnn-fp32 (one arm, so that the
trace holds nothing else); the forward GEMM's share of the fp32 matrix peak is worked out from those."""
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

BATCH = 1 << 18
PEAK_F32_MATRIX = 157.3e12  # FLOP/s, v_mfma_f32_* with f32 operands (MI355X spec)
SHAPES = {"64x2": (32, 64, 2, 16), "256x4": (32, 256, 4, 16)}  # n_in, width, hidden layers, n_out


def net(width, hidden):
    return {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}


def torch_mlp(n_in, width, hidden, n_out):
    dims = [n_in] + [width] * hidden
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [torch.nn.Linear(a, b, bias=False), torch.nn.ReLU()]
    mods.append(torch.nn.Linear(dims[-1], n_out, bias=False))
    return torch.nn.Sequential(*mods).cuda()


def step_of(model, x, dy):
    def step():
        model.zero_grad(set_to_none=True)
        out = model(x)
        out.backward(dy.to(out.dtype))
    return step


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def flops_fwd(n_in, width, hidden, n_out):
    dims = [n_in] + [width] * hidden + [n_out]
    return sum(2.0 * BATCH * a * b for a, b in zip(dims[:-1], dims[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--txt", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-tcnn-fp32", action="store_true")
    a = ap.parse_args()
    results, lines = [], []
    for name, (n_in, width, hidden, n_out) in SHAPES.items():
        x = torch.rand(BATCH, n_in, device="cuda", requires_grad=True)  # dL/dinput is part of the backward pass in every arm
        dy = torch.rand(BATCH, n_out, device="cuda")
        arms = {"tcnn_fp32": step_of(tcnn.Network(n_in, n_out, net(width, hidden), dtype=torch.float32), x, dy)}
        if not a.only_tcnn_fp32:
            arms = {"torch_linear_fp32": step_of(torch_mlp(n_in, width, hidden, n_out), x, dy), **arms,
                    "tcnn_half": step_of(tcnn.Network(n_in, n_out, net(width, hidden)), x, dy)}
        for fn in arms.values():  # warm-up: allocations, code objects
            timed(fn, 3)
        times = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                times[k].append(timed(fn, a.steps))
        r = {"shape": name, "batch": BATCH, "n_in": n_in, "width": width, "hidden": hidden, "n_out": n_out, "steps": a.steps, "reps": a.reps,
             "forward_gflop": flops_fwd(n_in, width, hidden, n_out) / 1e9, "arms": {}}
        for k, ts in times.items():
            r["arms"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "all_ms": ts}
            # forward + data backward + weight gradients = three products per layer (the input layer's data product included here)
            tf = 3 * flops_fwd(n_in, width, hidden, n_out) / (statistics.median(ts) * 1e-3)
            lines.append(f"{name} {k}: forward+backward median {statistics.median(ts):.3f} ms (range {min(ts):.3f} .. {max(ts):.3f}), "
                         f"{tf / 1e12:.1f} TFLOP/s over the three products = {100 * tf / PEAK_F32_MATRIX:.1f} % of the fp32 matrix peak")
            print(lines[-1], flush=True)
        if "torch_linear_fp32" in r["arms"]:
            ratio = r["arms"]["tcnn_fp32"]["median_ms"] / r["arms"]["torch_linear_fp32"]["median_ms"]
            r["tcnn_fp32_over_torch"] = ratio
            lines.append(f"{name}: tcnn fp32 / torch Linear fp32 = {ratio:.3f}")
            print(lines[-1], flush=True)
        results.append(r)
    if a.txt:
        with open(a.txt, "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
