"""BatchedMLP (k_mlp_batched.hip) against the two things that existed before it, through tcnn.Network and autograd:

    python tools/bench_batched_mlp.py [--steps K] [--warmup W] [--out lines.txt]

Shape: 32 inputs -> 64 x 2 hidden layers -> 16 outputs, equal split, K in {16, 256, 4096} networks x {64, 1024} rows each; forward
(no_grad) and forward + backward (parameter gradients) in ms per call, device events around `steps` calls after `warmup`.
  loop    K separate tcnn.Network CutlassMLP modules, each on its own rows (for K = 4096: 64 of them timed, times 64 -- marked "scaled")
  single  ONE CutlassMLP of the same shape on all K x rows rows: what the hardware does when every row shares one weight set (the ceiling)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
import torch  # noqa: E402

import tinycudann as tcnn  # noqa: E402

N_IN, N_OUT, LOOP_MAX = 32, 16, 64


def net(otype, **more):
    return dict({"otype": otype, "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}, **more)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def passes(modules, xs):
    """(forward, forward + backward) callables over module i on xs[i]"""
    def forward():
        with torch.no_grad():
            for m, x in zip(modules, xs):
                m(x)

    def both():
        for m, x in zip(modules, xs):
            m.params.grad = None
            m(x).float().sum().backward()

    return forward, both


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_batched_mlp: needs the GPU (no fallback)")
    lines = []
    for K in (16, 256, 4096):
        for rows in (64, 1024):
            x = torch.rand((K * rows, N_IN), device="cuda")
            batched = tcnn.Network(N_IN, N_OUT, net("BatchedMLP", n_networks=K))
            single = tcnn.Network(N_IN, N_OUT, net("CutlassMLP"))
            n_loop = min(K, LOOP_MAX)
            loop = [tcnn.Network(N_IN, N_OUT, net("CutlassMLP"), seed=i) for i in range(n_loop)]
            for m in [batched, single] + loop:
                m.reuse_working_copy = True  # (no per-call cast of the parameters in any of the three)
            t = {}
            for name, (fwd, both) in (("batched", passes([batched], [x])), ("single", passes([single], [x])), ("loop", passes(loop, list(x[: n_loop * rows].split(rows))))):
                scale = K / n_loop if name == "loop" else 1.0
                t[name] = (timed(fwd, a.steps, a.warmup) * scale, timed(both, a.steps, a.warmup) * scale)
            scaled = f" (loop: {n_loop} modules timed, scaled by {K // n_loop})" if n_loop < K else ""
            lines.append(f"K={K:5d} rows/network={rows:5d}  forward ms: batched {t['batched'][0]:.4f}  loop {t['loop'][0]:.4f}  single {t['single'][0]:.4f}   "
                         f"forward+backward ms: batched {t['batched'][1]:.4f}  loop {t['loop'][1]:.4f}  single {t['single'][1]:.4f}{scaled}")
            print(lines[-1], flush=True)
            del batched, single, loop
            tcnn.free_temporary_memory()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
