"""Time input_jacobian against what it replaces and against its own two-pass route, in one process on one GPU.

  jacobian  tcnn_module_input_jacobian of K dims (its route is reported: what the plan chooses is what runs)
  k-calls   K calls of tcnn_module_input_gradient, one per dim: what a caller had to do before
  two-pass  the Jacobian's two-pass route made by hand from its kernels: ONE tcnn_module_forward with prepare_input_gradients, then per dim
            a one-hot dL/dy and tcnn_module_backward without parameter gradients, and one multiplication by 1 / backprop_scale over all
            (into K dense buffers: the strided slices of the real route cost the same stores)

Shapes: tools/bench_input_gradient.py's, with 3 outputs and K = 3; the 2^18 grid shape also at K = 16 (all 16 padded columns).  The sides run
interleaved (A B C A B C ...), each run between device events after a warm-up; the medians are reported, and the three results are compared
bit for bit.  Prints one JSON line per shape (milliseconds).
usage (GPU box): python tools/bench_input_jacobian.py [--runs 30] [--warmup 5] [--all] [--only <shape> ...] [--dims K] [--side jacobian|k-calls|two-pass]
(--only / --side: one shape, one side -- for a profiler run; --dims: another number of dims, for the plan rule's evidence)"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_input_gradient import DEFAULT, SCALE, SHAPES as GRADIENT_SHAPES, make  # noqa: E402
from tinycudann import _C  # noqa: E402
from tinycudann.modules import _ptr, _stream  # noqa: E402

# name: ((encoding or None, network, inputs, outputs, log2 rows), dims)
SHAPES = {name: ((s[0], s[1], s[2], 3, s[4]), (0, 1, 2)) for name, s in GRADIENT_SHAPES.items()}
SHAPES["grid18_k16"] = (SHAPES["grid18"][0], tuple(range(16)))


def shape_of(name):
    """a named shape, or a bare network spelled <relu|softplus><width>x<hidden>[@<log2 rows>] (16 inputs, 3 outputs, K = 3; 2^18 rows):
    the plan rule's evidence is taken over these, with --dims for other K"""
    if name in SHAPES:
        return SHAPES[name]
    m = re.fullmatch(r"(relu|softplus)(\d+)x(\d+)(?:@(\d+))?", name)
    if not m:
        raise SystemExit("unknown shape %r" % name)
    network = dict(GRADIENT_SHAPES["net64x4"][1], activation={"relu": "ReLU", "softplus": "Softplus"}[m.group(1)], n_neurons=int(m.group(2)), n_hidden_layers=int(m.group(3)))
    return (None, network, 16, 3, int(m.group(4) or 18)), (0, 1, 2)


DEFAULT = DEFAULT + ("grid18_k16",)
SIDES = ("jacobian", "k-calls", "two-pass")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", nargs="+", help="named shapes, or <relu|softplus><width>x<hidden>[@<log2 rows>]")
    ap.add_argument("--dims", type=int, help="K: the padded columns 0 .. K - 1 (1 .. 16) instead of the shape's own dims")
    ap.add_argument("--all", action="store_true", help="also the shapes beyond the default ones")
    ap.add_argument("--side", choices=SIDES)
    args = ap.parse_args()
    assert args.runs >= 20 or args.side, "the medians are of at least 20 runs"
    for name in args.only or (SHAPES if args.all else DEFAULT):
        shape, dims = shape_of(name)
        if args.dims:
            dims = tuple(range(args.dims))
        native = make(shape)
        n, n_in, pw, K = 1 << shape[4], shape[2], native.n_output_dims(), len(dims)
        x = torch.rand((n, n_in), device="cuda", generator=torch.Generator(device="cuda").manual_seed(42))
        params = native.initial_params(1337).half().contiguous()
        c_dims = (C.c_uint32 * K)(*dims)
        jac = torch.empty((n, K, n_in), dtype=torch.float32, device="cuda")
        dx_calls = torch.empty((K, n, n_in), dtype=torch.float32, device="cuda")
        dx_two = torch.empty((K, n, n_in), dtype=torch.float32, device="cuda")
        one_hot = torch.zeros((pw, pw), dtype=torch.half, device="cuda")
        one_hot.fill_diagonal_(SCALE)
        dy = torch.empty((n, pw), dtype=torch.half, device="cuda")
        out = torch.empty((n, pw), dtype=torch.half, device="cuda")
        mult = 1.0 / SCALE

        def jacobian():
            _C.check(_C.lib.tcnn_module_input_jacobian(native._h, _stream(), n, c_dims, K, _ptr(x), _ptr(jac), None, _ptr(params), SCALE))

        def k_calls():
            for k, dim in enumerate(dims):
                _C.check(_C.lib.tcnn_module_input_gradient(native._h, _stream(), n, dim, _ptr(x), _ptr(dx_calls[k]), None, _ptr(params), SCALE))

        def two_pass():
            h = C.c_void_p()
            _C.check(_C.lib.tcnn_module_forward(native._h, _stream(), n, _ptr(x), _ptr(out), _ptr(params), 1, C.byref(h)))
            for k, dim in enumerate(dims):
                dy.copy_(one_hot[dim].expand(n, pw))  # (one kernel, as k_one_hot)
                _C.check(_C.lib.tcnn_module_backward(native._h, _stream(), h, n, _ptr(dx_two[k]), _ptr(dy), None, _ptr(x), _ptr(out), _ptr(params)))
            _C.lib.tcnn_context_destroy(h)
            dx_two.mul_(mult)

        sides = {"jacobian": jacobian, "k-calls": k_calls, "two-pass": two_pass}
        if args.side:
            sides = {args.side: sides[args.side]}
        for _ in range(args.warmup):
            for f in sides.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(args.runs):
            for k, f in sides.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        result = {"shape": name, "rows": n, "dims": K, "runs": args.runs, "unit": "ms"}
        if "jacobian" in sides:
            result["route"] = native.last_input_jacobian_route()
        if "k-calls" in sides:
            result["k_calls_route"] = native.last_input_gradient_route()
        for k, v in times.items():
            result[k + "_median"] = round(statistics.median(v), 4)
            result[k + "_min"] = round(min(v), 4)
        if len(times) == 3:
            got = jac.permute(1, 0, 2).contiguous().view(torch.int32)
            assert torch.equal(got, dx_calls.view(torch.int32)), "input_jacobian and the K input_gradient calls differ"
            assert torch.equal(got, dx_two.view(torch.int32)), "input_jacobian and the hand-made two passes differ"
            result["k_calls_over_jacobian"] = round(result["k-calls_median"] / result["jacobian_median"], 3)
            result["two_pass_over_jacobian"] = round(result["two-pass_median"] / result["jacobian_median"], 3)
        print(json.dumps(result), flush=True)
        del native


if __name__ == "__main__":
    main()
