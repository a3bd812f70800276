"""Time the grid encodings' max_level settings (Trainer / tcnn.Encoding set_max_level, set_max_level_gpu): the C3a training step and a
tcnn.Encoding forward + backward of C3a's grid, unset and under each setting, with device events around warmed-up loops.
Prints one JSON line (milliseconds per step / per forward + backward).
usage (GPU box): python tools/bench_max_level.py [--steps 100] [--warmup 20] [--log2-batch 18]"""
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

SETTINGS = [("unset", None), ("1000", 1000.0), ("0.75", 0.75), ("0.5", 0.5), ("0.25", 0.25), ("per_sample_uniform", "uniform")]


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


def apply(obj, setting, per_sample):
    if setting is None:
        return
    if setting == "uniform":  # instant-ngp's random max level: one uniform draw in [0, 1) per sample
        obj.set_max_level_gpu(per_sample)
    else:
        obj.set_max_level(setting)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--log2-batch", type=int, default=18)
    ap.add_argument("--only", choices=[name for name, _ in SETTINGS], help="time the training step under this one setting (for a profiler run)")
    args = ap.parse_args()
    n = 1 << args.log2_batch
    gen = torch.Generator(device="cuda").manual_seed(42)
    x = torch.rand(n, 2, device="cuda", generator=gen)
    y = torch.rand(n, 3, device="cuda", generator=gen)
    per_sample = torch.rand(n, device="cuda", generator=gen)
    result = {"metric": "max_level C3a step and Encoding forward+backward", "unit": "ms", "batch": n, "steps": args.steps, "warmup": args.warmup,
              "step_ms": {}, "encoding_fwd_bwd_ms": {}}
    if args.only:
        tr = Trainer(2, 3, CONFIG_C3A, seed=1337)
        apply(tr, dict(SETTINGS)[args.only], per_sample)
        result["step_ms"][args.only] = round(timed(lambda: tr.training_step(x, y), args.steps, args.warmup), 4)
        print(json.dumps(result), flush=True)
        return
    for name, setting in SETTINGS:
        tr = Trainer(2, 3, CONFIG_C3A, seed=1337)
        apply(tr, setting, per_sample)
        result["step_ms"][name] = round(timed(lambda: tr.training_step(x, y), args.steps, args.warmup), 4)
        del tr
    for name, setting in SETTINGS:
        enc = tcnn.Encoding(2, CONFIG_C3A["encoding"])
        apply(enc, setting, per_sample)
        w = torch.randn(enc.n_output_dims, device="cuda", dtype=torch.float16) * 1e-3

        def fwd_bwd():
            enc.params.grad = None
            (enc(x) * w).sum().backward()

        result["encoding_fwd_bwd_ms"][name] = round(timed(fwd_bwd, args.steps // 2, args.warmup), 4)
        del enc
    base = result["step_ms"]["unset"]
    result["step_ratio_to_unset"] = {k: round(v / base, 3) for k, v in result["step_ms"].items()}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
