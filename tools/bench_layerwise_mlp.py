"""The layer-by-layer MLP path (k_mlp_layers.hip): training-step time and inference throughput for the shapes of DESIGN.md
"CutlassMLP layer by layer", with per-layer FLOPs and bytes computed from the shapes and the time each GEMM would take at its bound.

    python tools/bench_layerwise_mlp.py [--steps K] [--warmup W] [--only NAME ...] [--json out.json]

The "ab_*" shapes run twice, with the specialised kernels and with TCNN_AMD_MLP_LAYERWISE=1.  Per-kernel times (which share of the bound
each GEMM reaches) come from a separate `rocprofv3 --kernel-trace --stats` run of this tool; the "gemm_*" shapes exist for that: one
k_layer_gemm launch per inference (Identity input, zero hidden layers)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
import torch  # noqa: E402

import tinycudann as tcnn  # noqa: E402

PEAK_MFMA = 2.5e15  # dense fp16 MFMA, spec (MI355X)
PEAK_HBM = 8.0e12   # bytes/s, spec (6.3e12 measured by a float4 copy)
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}
C3B_GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16, "per_level_scale": 1.5}
IDENTITY = {"otype": "Identity"}


def net(width, hidden, act="ReLU", otype="CutlassMLP"):
    return {"otype": otype, "activation": act, "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}


# name: (n_in, n_out, batch, encoding, network, env, train)
SHAPES = {
    "siren512x4_2^18": (32, 3, 1 << 18, IDENTITY, net(512, 4, "Sine"), {}, True),
    "siren512x4_2^20": (32, 3, 1 << 20, IDENTITY, net(512, 4, "Sine"), {}, True),
    "c3b_grid_96x3_2^18": (2, 3, 1 << 18, C3B_GRID, net(96, 3), {}, True),
    "zero_hidden_32to16_2^20": (32, 16, 1 << 20, IDENTITY, net(64, 0, "None"), {}, True),
    "gemm_512x512_2^20": (512, 512, 1 << 20, IDENTITY, net(64, 0, "None"), {}, False),
    "ab_64x2_fused": (32, 3, 1 << 18, IDENTITY, net(64, 2, otype="FullyFusedMLP"), {}, True),
    "ab_64x2_layerwise": (32, 3, 1 << 18, IDENTITY, net(64, 2, otype="FullyFusedMLP"), {"TCNN_AMD_MLP_LAYERWISE": "1"}, True),
    "ab_128x4_fused": (32, 3, 1 << 18, IDENTITY, net(128, 4, otype="FullyFusedMLP"), {}, True),
    "ab_128x4_layerwise": (32, 3, 1 << 18, IDENTITY, net(128, 4, otype="FullyFusedMLP"), {"TCNN_AMD_MLP_LAYERWISE": "1"}, True),
}


def layers(n_in, n_out, network):
    w, h, pad = network["n_neurons"], network["n_hidden_layers"], (n_out + 15) // 16 * 16
    enc_w = (n_in + 15) // 16 * 16
    if h == 0:
        return [(pad, enc_w)]
    return [(w, enc_w)] + [(w, w)] * (h - 1) + [(pad, w)]


def gemm_rows(batch, rows, cols, sine=False):
    """forward GEMM of one layer: FLOPs, HBM bytes (input read once, output written, + the pre-activation for Sine), time at its bound"""
    flops = 2.0 * batch * rows * cols
    nbytes = 2.0 * batch * (cols + rows * (2 if sine else 1)) + 2.0 * rows * cols
    t_mfma, t_hbm = flops / PEAK_MFMA, nbytes / PEAK_HBM
    return {"rows": rows, "cols": cols, "gflop": flops / 1e9, "mbytes": nbytes / 1e6, "bound": "MFMA" if t_mfma >= t_hbm else "HBM",
            "bound_us": max(t_mfma, t_hbm) * 1e6}


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


def run(name, steps, warmup):
    n_in, n_out, batch, enc, network, env, train = SHAPES[name]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        cfg = {"loss": {"otype": "L2"}, "optimizer": ADAM, "encoding": enc, "network": network}
        tr = tcnn.Trainer(n_in, n_out, cfg, seed=1337)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    x = torch.rand((batch, n_in), device="cuda")
    t = torch.rand((batch, n_out), device="cuda") if train else None
    out = torch.empty((batch, tr.padded_output_width), dtype=torch.half, device="cuda")
    r = {"name": name, "batch": batch, "network": network, "encoding": enc["otype"], "env": env}
    if train:
        r["train_step_ms"] = timed(lambda: tr.training_step(x, t), steps, warmup)
        r["step_kernel"] = tr.last_step_kernel()
    r["inference_ms"] = timed(lambda: tr.inference_half(x, out), steps, warmup)
    r["inference_rows_per_s"] = batch / r["inference_ms"] * 1e3
    sine = network["activation"] == "Sine"
    r["layers"] = [gemm_rows(batch, rows, cols, sine and i < network["n_hidden_layers"]) for i, (rows, cols) in enumerate(layers(n_in, n_out, network))]
    r["forward_bound_us"] = sum(l["bound_us"] for l in r["layers"])
    r["inference_share_of_bound"] = r["forward_bound_us"] / (r["inference_ms"] * 1e3)  # whole inference (encoding, trims included)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    results = []
    for name in a.only or list(SHAPES):
        r = run(name, a.steps, a.warmup)
        results.append(r)
        step = f"step {r['train_step_ms']:.3f} ms ({r['step_kernel']}), " if "train_step_ms" in r else ""
        print(f"{name}: {step}inference {r['inference_ms']:.3f} ms = {r['inference_rows_per_s']:.3e} rows/s, forward GEMMs at their bound "
              f"{r['forward_bound_us']:.1f} us ({100 * r['inference_share_of_bound']:.1f} % of the inference time)", flush=True)
        for i, l in enumerate(r["layers"]):
            print(f"    layer {i}: {l['rows']} x {l['cols']}  {l['gflop']:.2f} GFLOP  {l['mbytes']:.1f} MB  {l['bound']}-bound  {l['bound_us']:.1f} us at peak", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
