"""Full-precision training: (1) the bandwidth of Adam with fp32 weights (k_adam<..., float, float>: one weight vector, 30 B/param with narrow step
counts) beside the half-weight k_adam on the same fp32 gradients (32 B/param) at 2^24 parameters with dense gradients, and (2) the time of a
native fp32 training step -- tcnn.native.Trainer(dtype=torch.float32) -- beside the only way to train an fp32 model without it:
tcnn.NetworkWithInputEncoding(dtype=torch.float32) + a torch MSE + torch.optim.Adam.

    python tools/bench_fp32_training.py [--reps 7] [--steps 20] [--txt out.txt] [--json out.json] [--only native_fp32]

The arms alternate in one process: `reps` repetitions of `steps` steps between device events each; median and range are reported.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool with --only native_fp32 (one arm per run, no
counters collected)."""
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

N_ADAM = 1 << 24
BATCH = 1 << 18
HBM_PEAK = 8.0e12  # B/s (MI355X spec)
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}
# Bytes per parameter and step with uint16 step counts.  The count the design uses: gradient 4 + weights 8 (one float vector, read and
# stored) + moments 16 + step count 2 = 30; the half-weight form on the same fp32 gradients stores a half copy besides: 32.  Counting the
# step count both ways (read 2, written 2) they are 32 and 34; both figures are reported.
ADAM_BYTES = {"adam_fp32_weights": 30, "adam_half_weights": 32}
ADAM_BYTES_BOTH_WAYS = {"adam_fp32_weights": 32, "adam_half_weights": 34}
HASHGRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}
STEP_SHAPES = {
    "hashgrid_32x1": (3, 1, HASHGRID, {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 1}),
    "identity32_256x4": (32, 16, {"otype": "Identity"}, {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 256, "n_hidden_layers": 4}),
}


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(arms, reps, steps):
    for fn in arms.values():  # warm-up: allocations, code objects
        timed(fn, 3)
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            times[k].append(timed(fn, steps))
    return {k: {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "all_ms": ts} for k, ts in times.items()}


def adam_arms():
    n = N_ADAM
    layers = [(1024, 1024)]  # 2^20 matrix weights in front, the rest non-matrix; dense gradients: no quad is skipped
    g = torch.rand(n, device="cuda") - 0.5
    g[g == 0] = 0.25
    w32, w16_fp = torch.rand(n, device="cuda") - 0.5, torch.rand(n, device="cuda") - 0.5
    w16 = w16_fp.half()
    full = tcnn.optimizers.NativeOptimizer(ADAM, n, layers, weight_dtype=torch.float32)
    half = tcnn.optimizers.NativeOptimizer(ADAM, n, layers)
    return {"adam_fp32_weights": lambda: full.step_unchecked(w32, None, g, 1.0), "adam_half_weights": lambda: half.step_unchecked(w16_fp, w16, g, 1.0)}


def step_arms(n_in, n_out, enc, net, only):
    x = torch.rand(BATCH, n_in, device="cuda")
    t = torch.rand(BATCH, n_out, device="cuda")
    arms = {}
    if only in (None, "native_fp32"):
        tr = tcnn.native.Trainer(n_in, n_out, {"loss": {"otype": "L2"}, "optimizer": ADAM, "encoding": enc, "network": net}, dtype=torch.float32)
        arms["native_fp32"] = lambda: tr.training_step(x, t)
    if only in (None, "torch_fp32"):
        model = tcnn.NetworkWithInputEncoding(n_in, n_out, enc, net, dtype=torch.float32)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.99), eps=1e-15)

        def torch_step():
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.mse_loss(model(x), t).backward()
            opt.step()
        arms["torch_fp32"] = torch_step
    if only in (None, "native_half"):
        th = tcnn.native.Trainer(n_in, n_out, {"loss": {"otype": "L2"}, "optimizer": ADAM, "encoding": enc, "network": net})
        arms["native_half"] = lambda: th.training_step(x, t)
    return arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--txt", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="one arm of the training step alone (for a kernel trace): native_fp32, torch_fp32 or native_half")
    a = ap.parse_args()
    results, lines = {"reps": a.reps, "steps": a.steps}, []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    if a.only is None:
        r = alternate(adam_arms(), a.reps, a.steps)
        for k, v in r.items():
            v["bytes_per_param"] = ADAM_BYTES[k]
            v["bytes_per_s"] = N_ADAM * ADAM_BYTES[k] / (v["median_ms"] * 1e-3)
            v["bytes_per_s_counting_step_counts_both_ways"] = N_ADAM * ADAM_BYTES_BOTH_WAYS[k] / (v["median_ms"] * 1e-3)
            say(f"adam 2^24 {k}: median {1e3 * v['median_ms']:.1f} us (range {1e3 * v['min_ms']:.1f} .. {1e3 * v['max_ms']:.1f}), {ADAM_BYTES[k]} B/param, "
                f"{v['bytes_per_s'] / 1e12:.3f} TB/s = {v['bytes_per_s'] / HBM_PEAK:.3f} of the HBM peak "
                f"({ADAM_BYTES_BOTH_WAYS[k]} B/param with the step counts counted both ways: {v['bytes_per_s_counting_step_counts_both_ways'] / 1e12:.3f} TB/s)")
        ratio = r["adam_fp32_weights"]["bytes_per_s"] / r["adam_half_weights"]["bytes_per_s"]
        say(f"adam 2^24: bytes/s of the fp32-weight form / the half-weight form = {ratio:.3f}")
        results["adam"] = {"n_params": N_ADAM, "arms": r, "fp32_over_half_bytes_per_s": ratio}
    results["training_step"] = {}
    for name, (n_in, n_out, enc, net) in STEP_SHAPES.items():
        r = alternate(step_arms(n_in, n_out, enc, net, a.only), a.reps, a.steps)
        for k, v in r.items():
            say(f"step 2^18 {name} {k}: median {v['median_ms']:.3f} ms (range {v['min_ms']:.3f} .. {v['max_ms']:.3f})")
        entry = {"batch": BATCH, "arms": r}
        if "native_fp32" in r and "torch_fp32" in r:
            entry["native_over_torch"] = r["native_fp32"]["median_ms"] / r["torch_fp32"]["median_ms"]
            say(f"step 2^18 {name}: native fp32 / torch fp32 = {entry['native_over_torch']:.3f}")
        results["training_step"][name] = entry
    if a.txt:
        with open(a.txt, "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
