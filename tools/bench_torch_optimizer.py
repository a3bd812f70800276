"""A full training step of a PyTorch module with its own loss -- forward, MSE, backward, optimizer -- under three optimizers
(DESIGN.md "Native optimizers for the PyTorch modules"):

    python tools/bench_torch_optimizer.py [--log2-batch 18] [--steps K] [--warmup W] [--reps R] [--only ARM] [--trainer-reference] [--json out.json]

  torch_adam        torch.optim.Adam(eps=1e-15) in its default form          (what a caller had before tcnn.optimizers)
  torch_adam_fused  the same with fused=True, where this torch build has it
  tcnn              tcnn.optimizers.Optimizer with the C3a Adam configuration (k_adam on the fp32 .grad, half weights written in the same pass)
on C3a's NetworkWithInputEncoding (HashGrid L16 F2 T 2^19, 64 x 2), one model per arm, the same inputs, alternating repetition by
repetition in one process.  Times are device events around K steps; R repetitions, median and range.  Two numbers per arm: the full
step, and the optimizer call alone on a .grad left by a real backward pass.  --log2-batch 14 is the sparse row: most grid quads have
no gradient there.
--trainer-reference: after the timed part, K optimizer steps of a tcnn.Trainer on the same parameter vector with the same gradients
in half (k_adam's half-gradient form) -- the reference point for a `rocprofv3 --kernel-trace --stats` run of this tool."""
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

GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}


def make_optimizer(arm, model):
    if arm == "tcnn":
        return tcnn.optimizers.Optimizer(model, ADAM)
    extra = {"fused": True} if arm == "torch_adam_fused" else {}
    return torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.99), eps=1e-15, **extra)


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def summary(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-batch", type=int, default=18)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["torch_adam", "torch_adam_fused", "tcnn"], default=None)
    ap.add_argument("--trainer-reference", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_torch_optimizer.py needs a GPU")
    torch.manual_seed(0)
    n = 1 << a.log2_batch
    x = torch.rand(n, 2, device="cuda")
    target = torch.stack([torch.sin(8 * x[:, 0]), torch.cos(8 * x[:, 1]), x[:, 0] * x[:, 1]], dim=1)

    arms, skipped = {}, {}
    for arm in ("torch_adam", "torch_adam_fused", "tcnn"):
        if a.only not in (None, arm):
            continue
        model = tcnn.NetworkWithInputEncoding(2, 3, GRID, NETWORK)
        try:
            opt = make_optimizer(arm, model)
        except (RuntimeError, TypeError, ValueError) as e:  # fused=True is not offered by every torch build
            skipped[arm] = str(e).splitlines()[0]
            print(f"{arm}: not available in this torch build ({skipped[arm]})", flush=True)
            continue

        def full(model=model, opt=opt):
            opt.zero_grad()
            loss = (model(x).float() - target).square().mean()
            loss.backward()
            opt.step()
            return loss

        arms[arm] = {"model": model, "opt": opt, "full": full, "opt_only": opt.step}
    for arm in arms.values():
        for _ in range(a.warmup):
            loss = arm["full"]()
        assert bool(torch.isfinite(loss))
    torch.cuda.synchronize()
    times = {name: {"full": [], "opt_only": []} for name in arms}
    for _ in range(a.reps):  # alternating: every arm sees the same clocks and the same neighbours
        for name, arm in arms.items():
            times[name]["full"].append(timed(arm["full"], a.steps))
        for name, arm in arms.items():  # .grad is what the last full step's backward pass left
            times[name]["opt_only"].append(timed(arm["opt_only"], a.steps))
    n_params = next(iter(arms.values()))["model"].params.numel()
    grad = next(iter(arms.values()))["model"].params.grad
    n_matrix = sum(r * c for r, c in tcnn.optimizers.module_layer_sizes(next(iter(arms.values()))["model"]))
    quads = grad[n_matrix:][: (n_params - n_matrix) // 4 * 4].view(-1, 4)
    live_quads = float((quads != 0).any(dim=1).float().mean())
    result = {"batch": n, "steps": a.steps, "reps": a.reps, "n_params": n_params, "live_grid_quads": live_quads, "torch": torch.__version__, "skipped": skipped,
              "encoding": GRID, "network": NETWORK, "optimizer": ADAM}
    print(f"2^{a.log2_batch} rows, {n_params} parameters, {100 * live_quads:.1f} % of the grid's quads have a gradient; {a.reps} x {a.steps} steps, median (min - max) ms", flush=True)
    for name, t in times.items():
        result[name] = {k: summary(v) for k, v in t.items()}
        f, o = result[name]["full"], result[name]["opt_only"]
        print(f"{name:17s} full step {f['median_ms']:.3f} ({f['min_ms']:.3f} - {f['max_ms']:.3f})   optimizer alone {o['median_ms']:.3f} ({o['min_ms']:.3f} - {o['max_ms']:.3f})", flush=True)
    if "tcnn" in result and any(k in result for k in ("torch_adam", "torch_adam_fused")):
        best = min((k for k in ("torch_adam", "torch_adam_fused") if k in result), key=lambda k: result[k]["opt_only"]["median_ms"])
        d_opt = result[best]["opt_only"]["median_ms"] - result["tcnn"]["opt_only"]["median_ms"]
        d_full = result[best]["full"]["median_ms"] - result["tcnn"]["full"]["median_ms"]
        result["comparison"] = {"faster_torch_arm": best, "optimizer_ms_saved": d_opt, "full_step_ms_saved": d_full, "full_step_ms_saved_beyond_optimizer": d_full - d_opt,
                                "tcnn_over_torch_optimizer": result["tcnn"]["opt_only"]["median_ms"] / result[best]["opt_only"]["median_ms"]}
        print(f"against {best}: optimizer alone {d_opt:+.3f} ms saved (ratio {result['comparison']['tcnn_over_torch_optimizer']:.3f}), full step {d_full:+.3f} ms saved, "
              f"{d_full - d_opt:+.3f} ms of it outside the optimizer call (the cast pass the installed working copy removes)", flush=True)
    if a.trainer_reference:
        config = {"loss": {"otype": "L2"}, "optimizer": ADAM, "encoding": GRID, "network": NETWORK}
        tr = tcnn.Trainer(2, 3, config)
        from tinycudann import _C

        g_half = (grad * 128.0).half().contiguous()
        _C.memcpy_dtod(_C.lib.tcnn_trainer_param_gradients(tr._h), g_half.data_ptr(), n_params * 2)
        t = [timed(lambda: tr.optimizer_step(128.0), a.steps) for _ in range(a.reps)]
        result["trainer_optimizer_step"] = summary(t)
        print(f"{'trainer (half g)':17s} optimizer alone {statistics.median(t):.3f} ({min(t):.3f} - {max(t):.3f})", flush=True)
    print(json.dumps({k: v for k, v in result.items() if k not in ("encoding", "network", "optimizer")}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
