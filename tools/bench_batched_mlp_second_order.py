"""BatchedMLP's second-order pass and tangent (k_bmlp_tangent, k_bmlp_bwd2) against what callers had before, through tcnn.Network:

    python tools/bench_batched_mlp_second_order.py [--reps R] [--steps K] [--warmup W] [--out lines.txt]

Shape: 32 inputs -> 64 x 2 Softplus -> 16 outputs, equal split, K in {16, 256, 4096} networks x {64, 1024} rows each.  Timed, in ms per
call: one eikonal step (forward, autograd.grad(create_graph=True), loss = ((|grad| - 1)^2).mean(), backward) and input_jvp with 1 and 3
directions.  Device events around `steps` calls; `reps` repetitions of the three variants, interleaved; the median (min .. max) is printed.
  loop    K separate tcnn.Network CutlassMLP modules, each on its own rows (at most 64 of them timed, scaled to K -- marked "scaled")
  single  ONE CutlassMLP of the same shape on all K x rows rows: what the hardware does when every row shares one weight set (the ceiling)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
import torch  # noqa: E402

import tinycudann as tcnn  # noqa: E402

N_IN, N_OUT, LOOP_MAX = 32, 16, 64


def net(otype, **more):
    return dict({"otype": otype, "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}, **more)


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def passes(modules, xs):
    """(eikonal step, input_jvp T = 1, input_jvp T = 3) callables over module i on xs[i]"""
    vs = [torch.rand((x.shape[0], 3, N_IN), device="cuda") for x in xs]

    def eikonal():
        for m, x in zip(modules, xs):
            m.params.grad = x.grad = None
            x.requires_grad_(True)
            (g,) = torch.autograd.grad(m(x).float().sum(), x, create_graph=True)
            ((g.norm(dim=1) - 1) ** 2).mean().backward()

    def jvp(T):
        def run():
            for m, x, v in zip(modules, xs, vs):
                m.input_jvp(x, v[:, :T])
        return run

    return eikonal, jvp(1), jvp(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_batched_mlp_second_order: needs the GPU (no fallback)")
    lines = []
    for K in (16, 256, 4096):
        for rows in (64, 1024):
            x = torch.rand((K * rows, N_IN), device="cuda")
            n_loop = min(K, LOOP_MAX)
            variants = {"batched": [tcnn.Network(N_IN, N_OUT, net("BatchedMLP", n_networks=K))], "single": [tcnn.Network(N_IN, N_OUT, net("CutlassMLP"))],
                        "loop": [tcnn.Network(N_IN, N_OUT, net("CutlassMLP"), seed=i) for i in range(n_loop)]}
            fns = {}
            for name, modules in variants.items():
                for m in modules:
                    m.reuse_working_copy = True  # (no per-call cast of the parameters in any of the three)
                xs = list(x[: n_loop * rows].split(rows)) if name == "loop" else [x]
                fns[name] = passes(modules, [t.clone() for t in xs])
            for what, i in (("eikonal step", 0), ("input_jvp T=1", 1), ("input_jvp T=3", 2)):
                times = {name: [] for name in fns}
                for name in fns:
                    for _ in range(a.warmup):
                        fns[name][i]()
                torch.cuda.synchronize()
                for _ in range(a.reps):  # interleaved: every repetition times all three
                    for name in fns:
                        times[name].append(window(fns[name][i], a.steps) * (K / n_loop if name == "loop" else 1.0))
                cell = "  ".join(f"{name} {statistics.median(ts):.4f} ({min(ts):.4f} .. {max(ts):.4f})" for name, ts in times.items())
                scaled = f"  (loop: {n_loop} modules timed, scaled by {K // n_loop})" if n_loop < K else ""
                lines.append(f"K={K:5d} rows/network={rows:5d}  {what:14s} ms: {cell}{scaled}")
                print(lines[-1], flush=True)
            del variants, fns
            tcnn.free_temporary_memory()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
