"""One eikonal training step through the second-order pass of a Composite input layer (DESIGN.md "Second-order pass through Composite and
the analytic encodings"): forward, autograd.grad(create_graph=True), loss = SDF term + eikonal term, backward.

    python tools/bench_composite_second_order.py [--log2-batch 18] [--steps K] [--warmup W] [--reps R] [--json out.json]

Two models on the same points in the same run, alternating repetition by repetition (the protocol of tools/bench_second_order.py):
  composite_network  tcnn.NetworkWithInputEncoding(6 -> 1, Composite[HashGrid L16 F2 T 2^19 Smoothstep, Frequency(6)], CutlassMLP 64 x 2
                     Softplus) on [p, p]
  hand_assembled     what callers had before the Composite had a second-order pass: tcnn.Encoding (the same grid) + the frequency
                     terms in torch + torch.cat + tcnn.Network (the same MLP)
Times are device events around K steps; R repetitions, median and range reported.  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this tool with `--only composite_network`."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
import torch  # noqa: E402

import tinycudann as tcnn  # noqa: E402

GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 1.5, "interpolation": "Smoothstep"}
N_FREQUENCIES = 6
COMPOSITE = {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, **GRID}, {"n_dims_to_encode": 3, "otype": "Frequency", "n_frequencies": N_FREQUENCIES}]}
NETWORK = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}


class CompositeNetwork(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.model = tcnn.NetworkWithInputEncoding(6, 1, COMPOSITE, NETWORK)

    def forward(self, p):
        return self.model(torch.cat([p, p], dim=1))


class HandAssembled(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.encoding = tcnn.Encoding(3, GRID)
        self.network = tcnn.Network(self.encoding.n_output_dims + 3 * 2 * N_FREQUENCIES, 1, NETWORK)
        self.register_buffer("scales", (2.0 ** torch.arange(N_FREQUENCIES, device="cuda")) * math.pi)

    def forward(self, p):
        arg = p[:, :, None] * self.scales
        periodic = torch.stack([torch.sin(arg), torch.cos(arg)], dim=3).reshape(p.shape[0], -1)  # [dim][frequency][sin, cos]: the encoding's column order
        return self.network(torch.cat([self.encoding(p).float(), periodic], dim=1))


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
    ap.add_argument("--only", choices=["composite_network", "hand_assembled"], default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_composite_second_order.py needs a GPU")
    torch.manual_seed(0)
    n = 1 << a.log2_batch
    points = torch.rand(n, 3, device="cuda") * 0.9 + 0.05
    sdf = (points - 0.5).norm(dim=1) - 0.3
    models = {"composite_network": CompositeNetwork, "hand_assembled": HandAssembled}
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
    result = {"batch": n, "steps": a.steps, "reps": a.reps, "encoding": COMPOSITE, "network": NETWORK}
    for name, t in times.items():
        result[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t}
        print(f"{name:18s} eikonal step at 2^{a.log2_batch} rows: median {statistics.median(t):.3f} ms (min {min(t):.3f}, max {max(t):.3f}; {a.reps} x {a.steps} steps)", flush=True)
    if len(times) == 2:
        result["composite_network_over_hand_assembled"] = result["composite_network"]["median_ms"] / result["hand_assembled"]["median_ms"]
        print(f"composite_network / hand_assembled = {result['composite_network_over_hand_assembled']:.3f} (expected: at most 1.03)", flush=True)
    print(json.dumps({k: v for k, v in result.items() if k not in ("encoding", "network")}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
