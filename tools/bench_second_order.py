"""One eikonal training step through the second-order pass of CutlassMLP (DESIGN.md "Second-order pass through CutlassMLP"):
forward, autograd.grad(create_graph=True), loss = SDF term + eikonal term, backward.

    python tools/bench_second_order.py [--log2-batch 18] [--steps K] [--warmup W] [--reps R] [--json out.json]

Two models on the same inputs in the same run, alternating repetition by repetition:
  fused_network  tcnn.NetworkWithInputEncoding(3 -> 1, HashGrid L16 F2 T 2^19 Smoothstep, CutlassMLP 64 x 2 Softplus)
  torch_mlp      tcnn.Encoding (the same grid) + a torch.nn half MLP of the same shape: what callers had to use before the network
                 had a second-order pass (it runs without one too)
Times are device events around K steps; R repetitions, median and range reported.  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this tool with `--only fused_network`."""
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

GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 1.5, "interpolation": "Smoothstep"}
NETWORK = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}


class Softplus10(torch.nn.Module):
    """the library's Softplus: log(1 + exp(10 x)) / 10"""

    def forward(self, x):
        return torch.nn.functional.softplus(x, beta=10.0)


class EncodingPlusTorchMlp(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.encoding = tcnn.Encoding(3, GRID)
        w = self.encoding.n_output_dims
        self.mlp = torch.nn.Sequential(torch.nn.Linear(w, 64, bias=False), Softplus10(), torch.nn.Linear(64, 64, bias=False), Softplus10(), torch.nn.Linear(64, 1, bias=False)).half().cuda()

    def forward(self, x):
        return self.mlp(self.encoding(x))


def make_step(model, points, sdf):
    params = list(model.parameters())

    def step():
        p = points.detach().requires_grad_(True)
        f = model(p).float()[:, 0]
        (g,) = torch.autograd.grad(f.sum(), p, create_graph=True)
        loss = ((f - sdf) ** 2).mean() + 0.1 * ((g.norm(dim=1) - 1) ** 2).mean()
        for q in params:
            q.grad = None
        loss.backward()
        return loss

    return step


def timed(step, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-batch", type=int, default=18)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["fused_network", "torch_mlp"], default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_second_order.py needs a GPU")
    torch.manual_seed(0)
    n = 1 << a.log2_batch
    points = torch.rand(n, 3, device="cuda") * 0.9 + 0.05
    sdf = (points - 0.5).norm(dim=1) - 0.3
    models = {"fused_network": lambda: tcnn.NetworkWithInputEncoding(3, 1, GRID, NETWORK), "torch_mlp": EncodingPlusTorchMlp}
    steps = {name: make_step(make(), points, sdf) for name, make in models.items() if a.only in (None, name)}
    for step in steps.values():
        for _ in range(a.warmup):
            loss = step()
        assert bool(torch.isfinite(loss))
    torch.cuda.synchronize()
    times = {name: [] for name in steps}
    for _ in range(a.reps):  # alternating: both models see the same clocks and the same neighbours
        for name, step in steps.items():
            times[name].append(timed(step, a.steps))
    result = {"batch": n, "steps": a.steps, "reps": a.reps, "encoding": GRID, "network": NETWORK}
    for name, t in times.items():
        result[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t}
        print(f"{name:14s} eikonal step at 2^{a.log2_batch} rows: median {statistics.median(t):.3f} ms (min {min(t):.3f}, max {max(t):.3f}; {a.reps} x {a.steps} steps)", flush=True)
    if len(times) == 2:
        result["torch_mlp_over_fused_network"] = result["torch_mlp"]["median_ms"] / result["fused_network"]["median_ms"]
        print(f"torch_mlp / fused_network = {result['torch_mlp_over_fused_network']:.2f}", flush=True)
    print(json.dumps({k: v for k, v in result.items() if k not in ("encoding", "network")}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
