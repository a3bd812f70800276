"""Time input_gradient's fused route against the two passes it replaces, in one process on one GPU.

  fused     tcnn_module_input_gradient (its route is reported: what the plan chooses is what runs)
  two-pass  the same result made by hand from the kernels of the two-pass route: a one-hot dL/dy, tcnn_module_forward with
            prepare_input_gradients, tcnn_module_backward without parameter gradients, the multiplication by 1 / backprop_scale

Shapes: HashGrid (3-D, L 16, F 2, T 2^19) + 64 x 2 with one output at 2^18 and 2^20 rows; bare networks 128 x 4 at 2^20 rows and 64 x 4 at
2^18 rows.  The two sides run interleaved (A B A B ...), each run between device events after a warm-up; the medians are reported.
Prints one JSON line per shape (milliseconds).
usage (GPU box): python tools/bench_input_gradient.py [--runs 30] [--warmup 5] [--all] [--only <shape>] [--side fused|two-pass]
(--only / --side: one shape, one side -- for a profiler run)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))

import torch  # noqa: E402

from tinycudann import _C  # noqa: E402
from tinycudann.modules import _create, _ptr, _stream  # noqa: E402

GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
SCALE = 128.0


def net(width, hidden):
    return {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}


SHAPES = {  # name: (encoding or None, network, inputs, outputs, log2 rows)
    "grid18": (GRID, net(64, 2), 3, 1, 18),
    "grid20": (GRID, net(64, 2), 3, 1, 20),
    "net128x4": (None, net(128, 4), 16, 1, 20),
    "net64x4": (None, net(64, 4), 16, 1, 18),
    # one more per class of instantiations the plan can choose (--only, or --all)
    "net128x2": (None, net(128, 2), 16, 1, 20),
    "net32x4": (None, net(32, 4), 16, 1, 18),
    "net16x4": (None, net(16, 4), 16, 1, 18),
    "net64x4_softplus": (None, dict(net(64, 4), activation="Softplus"), 16, 1, 18),
    "net128x4_softplus": (None, dict(net(128, 4), activation="Softplus"), 16, 1, 20),
    "net64x2_small": (None, net(64, 2), 16, 1, 12),
}
DEFAULT = ("grid18", "grid20", "net128x4", "net64x4")


def make(shape):
    enc, network, n_in, n_out, _ = shape
    if enc is None:
        return _create(_C.lib.tcnn_create_network, n_in, n_out, _C.to_json_bytes(network))
    return _create(_C.lib.tcnn_create_network_with_input_encoding, n_in, n_out, _C.to_json_bytes(enc), _C.to_json_bytes(network))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=list(SHAPES))
    ap.add_argument("--all", action="store_true", help="also the shapes beyond the four default ones")
    ap.add_argument("--side", choices=["fused", "two-pass"])
    args = ap.parse_args()
    assert args.runs >= 20 or args.side, "the medians are of at least 20 runs"
    for name, shape in SHAPES.items():
        if (args.only and name != args.only) or (not args.only and not args.all and name not in DEFAULT):
            continue
        native = make(shape)
        n, n_in, pw = 1 << shape[4], shape[2], native.n_output_dims()
        x = torch.rand((n, n_in), device="cuda", generator=torch.Generator(device="cuda").manual_seed(42))
        params = native.initial_params(1337).half().contiguous()
        dx_f = torch.empty((n, n_in), dtype=torch.float32, device="cuda")
        dx_t = torch.empty((n, n_in), dtype=torch.float32, device="cuda")
        dy = torch.empty((n, pw), dtype=torch.half, device="cuda")
        out = torch.empty((n, pw), dtype=torch.half, device="cuda")
        mult = 1.0 / SCALE

        def fused():
            _C.check(_C.lib.tcnn_module_input_gradient(native._h, _stream(), n, 0, _ptr(x), _ptr(dx_f), None, _ptr(params), SCALE))

        def two_pass():
            dy.zero_()
            dy[:, 0] = SCALE
            h = C.c_void_p()
            _C.check(_C.lib.tcnn_module_forward(native._h, _stream(), n, _ptr(x), _ptr(out), _ptr(params), 1, C.byref(h)))
            _C.check(_C.lib.tcnn_module_backward(native._h, _stream(), h, n, _ptr(dx_t), _ptr(dy), None, _ptr(x), _ptr(out), _ptr(params)))
            _C.lib.tcnn_context_destroy(h)
            dx_t.mul_(mult)

        sides = {"fused": fused, "two-pass": two_pass}
        if args.side:
            sides = {args.side: sides[args.side]}
        for _ in range(args.warmup):
            for f in sides.values():
                f()
        torch.cuda.synchronize()
        route = native.last_input_gradient_route()
        times = {k: [] for k in sides}
        for _ in range(args.runs):
            for k, f in sides.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        result = {"shape": name, "rows": n, "route": route, "runs": args.runs, "unit": "ms"}
        for k, v in times.items():
            result[k + "_median"] = round(statistics.median(v), 4)
            result[k + "_min"] = round(min(v), 4)
        if len(times) == 2:
            # (route "two-pass": the plan keeps the two passes for this class -- both sides then time the same kernels)
            assert torch.equal(dx_f.view(torch.int32), dx_t.view(torch.int32)), "the two sides differ"
            result["two_pass_over_fused"] = round(result["two-pass_median"] / result["fused_median"], 3)
        print(json.dumps(result), flush=True)
        del native


if __name__ == "__main__":
    main()
