"""Time stochastic_interpolation of the grid encodings: the C3a training step at 2^18 samples and a tcnn.Encoding forward + backward
(3-D, L = 16, F = 2, T = 2^19), each with the key off and on, and with the key on also under TCNN_AMD_GRID_SCATTER=atomic (the
reference-shaped kernel: one packed-fp16 atomic per sample and level instead of 2^D).  Device events around warmed-up loops.
Prints one JSON line (milliseconds per step / per forward + backward).
usage (GPU box): python tools/bench_grid_stochastic.py [--steps 100] [--warmup 20] [--log2-batch 18] [--only off|on|on_atomic]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import tinycudann as tcnn  # noqa: E402
from conftest import CONFIG_C3A  # noqa: E402
from tinycudann.native import Trainer  # noqa: E402

ENCODING_3D = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
# (name, the key, environment while the model is created: the switches are read then)
SETTINGS = [("off", False, {}), ("on", True, {}), ("on_atomic", True, {"TCNN_AMD_GRID_SCATTER": "atomic"})]


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


def create(make, env):
    for k, v in env.items():
        os.environ[k] = v
    try:
        return make()
    finally:
        for k in env:
            del os.environ[k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--log2-batch", type=int, default=18)
    ap.add_argument("--only", choices=[s[0] for s in SETTINGS], help="time the training step under this one setting (for a profiler run)")
    args = ap.parse_args()
    n = 1 << args.log2_batch
    gen = torch.Generator(device="cuda").manual_seed(42)
    x = torch.rand(n, 2, device="cuda", generator=gen)
    y = torch.rand(n, 3, device="cuda", generator=gen)
    x3 = torch.rand(n, 3, device="cuda", generator=gen)
    result = {"metric": "stochastic_interpolation: C3a step and Encoding (3-D, L16, F2, T2^19) forward+backward", "unit": "ms", "batch": n, "steps": args.steps,
              "warmup": args.warmup, "step_ms": {}, "step_kernel": {}, "encoding_fwd_bwd_ms": {}}
    for name, key, env in SETTINGS:
        if args.only and name != args.only:
            continue
        cfg = {**CONFIG_C3A, "encoding": dict(CONFIG_C3A["encoding"], stochastic_interpolation=key)}
        tr = create(lambda: Trainer(2, 3, cfg, seed=1337), env)
        result["step_ms"][name] = round(timed(lambda: tr.training_step(x, y), args.steps, args.warmup), 4)
        result["step_kernel"][name] = tr.last_step_kernel()
        del tr
    if args.only:
        print(json.dumps(result), flush=True)
        return
    for name, key, env in SETTINGS:
        enc = create(lambda: tcnn.Encoding(3, dict(ENCODING_3D, stochastic_interpolation=key)), env)
        w = torch.randn(enc.n_output_dims, device="cuda", dtype=torch.float16) * 1e-3

        def fwd_bwd():
            enc.params.grad = None
            (enc(x3) * w).sum().backward()

        result["encoding_fwd_bwd_ms"][name] = round(timed(fwd_bwd, args.steps // 2, args.warmup), 4)
        del enc
    for group in ("step_ms", "encoding_fwd_bwd_ms"):
        base = result[group]["off"]
        result[group + "_ratio_to_off"] = {k: round(v / base, 3) for k, v in result[group].items()}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
