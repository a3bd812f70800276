"""Time a training step through input_jvp against what a caller had to do before, in one process on one GPU.

A step is: forward (jvp and output), a loss on both -- mean(jvp^2) + mean(output^2), its two cotangents written by one elementwise pass --
and the backward pass to the parameter gradients and dL_dinput.

  new       tcnn_module_input_jvp_forward + the loss + tcnn_module_input_jvp_backward on the module as configured (its backward route is
            reported: what the plan chooses is what runs)
  before    the only way to the same gradients until now, on the CutlassMLP form of the network (FullyFusedMLP has no second-order pass):
            tcnn_module_forward with prepare_input_gradients; per tangent tcnn_module_backward_backward_input asked for dL_ddLdoutput (J v_t);
            the loss; tcnn_module_backward for the output term; per tangent tcnn_module_backward_backward_input_mode again with
            dL_doutput = dL_djvp_t for the parameter gradients (Accumulate) and dL_dinput (added)

Section 1 (default): the grid L16 F2 T 2^19 + 64 x 2 at 2^18 rows; 64 x 4 and 128 x 4, ReLU and Softplus; a 3-output deformation head
(Softplus 64 x 3 on 3 inputs); T = 1 and 3.
Section 2 (--classes): the class table a plan rule would be read from -- ReLU | Softplus x 16 / 32 / 64 / 128 wide x 1 .. 4 hidden layers x
T = 1 | 3 at 2^18 and 2^14 rows -- new against before.  While mlp_input_jvp_backward_plan names no fused kernel, both columns run the
composed route and the table records its cost per class.

The sides run interleaved (A B A B ...), each run between device events after a warm-up; the medians are reported.  Prints one JSON line
per shape and T (milliseconds).  usage (GPU box): python tools/bench_input_jvp_backward.py [--runs 30] [--warmup 5] [--classes]
[--only <shape> ...] [--tangents T ...] [--side new|before]   (--only / --side: one shape, one side -- for a profiler run)"""
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

from bench_input_gradient import SHAPES as GRADIENT_SHAPES, make, net  # noqa: E402
from tinycudann import _C  # noqa: E402
from tinycudann.modules import _ptr, _stream  # noqa: E402

GRID = GRADIENT_SHAPES["grid18"][0]
OVERWRITE, ACCUMULATE = 1, 2


def _net(width, hidden, act):
    return dict(net(width, hidden), activation=act)


SHAPES = {  # name: (encoding or None, network, inputs, outputs, log2 rows)
    "grid18": (GRID, _net(64, 2, "ReLU"), 3, 3, 18),
    "relu64x4": (None, _net(64, 4, "ReLU"), 16, 3, 18),
    "softplus64x4": (None, _net(64, 4, "Softplus"), 16, 3, 18),
    "relu128x4": (None, _net(128, 4, "ReLU"), 16, 3, 18),
    "softplus128x4": (None, _net(128, 4, "Softplus"), 16, 3, 18),
    "deformation": (None, _net(64, 3, "Softplus"), 3, 3, 18),
}
SIDES = ("new", "before")


def shape_of(name):
    if name in SHAPES:
        return SHAPES[name]
    m = re.fullmatch(r"(relu|softplus)(\d+)x(\d+)(?:@(\d+))?", name)
    if not m:
        raise SystemExit("unknown shape %r" % name)
    return (None, _net(int(m.group(2)), int(m.group(3)), {"relu": "ReLU", "softplus": "Softplus"}[m.group(1)]), 16, 3, int(m.group(4) or 18))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", nargs="+", help="named shapes, or <relu|softplus><width>x<hidden>[@<log2 rows>]")
    ap.add_argument("--tangents", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--classes", action="store_true", help="section 2: the class table")
    ap.add_argument("--side", choices=SIDES)
    args = ap.parse_args()
    assert args.runs >= 20 or args.side, "the medians are of at least 20 runs"
    names = args.only or list(SHAPES)
    if args.classes and not args.only:
        names = ["%s%dx%d@%d" % (a, w, h, r) for r in (18, 14) for a in ("relu", "softplus") for w in (16, 32, 64, 128) for h in (1, 2, 3, 4)]
    for name in names:
        shape = shape_of(name)
        native, cutlass = make(shape), make(shape[:1] + (dict(shape[1], otype="CutlassMLP"),) + shape[2:])
        n, n_in, n_out, pw = 1 << shape[4], shape[2], shape[3], native.n_output_dims()
        gen = torch.Generator(device="cuda").manual_seed(42)
        x = torch.rand((n, n_in), device="cuda", generator=gen)
        params = native.initial_params(1337).half().contiguous()
        grads = {k: torch.empty_like(params) for k in SIDES}
        dx = {k: torch.empty((n, n_in), dtype=torch.float32, device="cuda") for k in SIDES}
        dx_more = torch.empty((n, n_in), dtype=torch.float32, device="cuda")
        out = torch.empty((n, pw), dtype=torch.half, device="cuda")
        zero_dy = torch.zeros((n, pw), dtype=torch.half, device="cuda")
        for T in args.tangents:
            # (behind the grid, whose finest level has 2^19 cells per unit, a unit tangent gives |J v| of that order, and the second-order grid
            # gradients -- that once more -- overflow half on either side: the tangents are scaled down, as a caller would)
            v = ((torch.rand((n, T, n_in), device="cuda", generator=gen) * 2 - 1) * (2.0 ** -12 if shape[0] is not None else 1.0)).contiguous()
            v_rows = v.permute(1, 0, 2).contiguous()  # [T][n][n_in]: what the second-order pass takes per call
            jvp = torch.empty((n, T, pw), dtype=torch.half, device="cuda")
            jvp_rows = torch.empty((T, n, pw), dtype=torch.half, device="cuda")
            # loss = mean(jvp[..., :n_out]^2) + mean(out[:, :n_out]^2), at a loss scale of 128: the cotangents, zero in the padding
            mask = torch.zeros(pw, dtype=torch.float32, device="cuda")
            mask[:n_out] = 1
            c_jvp, c_out = mask * (2.0 * 128 / (n * T * n_out)), mask * (2.0 * 128 / (n * n_out))

            def new():
                h = C.c_void_p()
                _C.check(_C.lib.tcnn_module_input_jvp_forward(native._h, _stream(), n, T, _ptr(x), _ptr(v), _ptr(jvp), _ptr(out), _ptr(params), C.byref(h)))
                d_jvp, d_out = (jvp * c_jvp).half(), (out * c_out).half()
                _C.check(_C.lib.tcnn_module_input_jvp_backward(native._h, _stream(), h, n, T, _ptr(x), _ptr(v), _ptr(d_jvp), _ptr(d_out), _ptr(params), _ptr(grads["new"]),
                                                               _ptr(dx["new"]), None, OVERWRITE))
                _C.lib.tcnn_context_destroy(h)

            def before():
                h = C.c_void_p()
                _C.check(_C.lib.tcnn_module_forward(cutlass._h, _stream(), n, _ptr(x), _ptr(out), _ptr(params), 1, C.byref(h)))
                for t in range(T):
                    _C.check(_C.lib.tcnn_module_backward_backward_input(cutlass._h, _stream(), h, n, _ptr(v_rows[t]), _ptr(x), _ptr(zero_dy), None, _ptr(jvp_rows[t]), None, _ptr(params)))
                d_jvp, d_out = (jvp_rows * c_jvp).half(), (out * c_out).half()
                _C.check(_C.lib.tcnn_module_backward(cutlass._h, _stream(), h, n, _ptr(dx["before"]), _ptr(d_out), _ptr(grads["before"]), _ptr(x), _ptr(out), _ptr(params)))
                for t in range(T):
                    _C.check(_C.lib.tcnn_module_backward_backward_input_mode(cutlass._h, _stream(), h, n, _ptr(v_rows[t]), _ptr(x), _ptr(d_jvp[t]), _ptr(grads["before"]), None,
                                                                             _ptr(dx_more), _ptr(params), ACCUMULATE))
                    dx["before"].add_(dx_more)
                _C.lib.tcnn_context_destroy(h)

            sides = {"new": new, "before": before}
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
            result = {"shape": name, "rows": n, "tangents": T, "runs": args.runs, "unit": "ms"}
            if "new" in sides:
                result["route"] = native.last_input_jvp_backward_route()
                result["forward_route"] = native.last_input_jvp_route()
            for k, t in times.items():
                result[k + "_median"] = round(statistics.median(t), 4)
                result[k + "_min"] = round(min(t), 4)
            if len(times) == 2:
                result["before_over_new"] = round(result["before_median"] / result["new_median"], 3)
                a, b = grads["new"].float(), grads["before"].float()
                result["gradients_finite"] = [bool(a.isfinite().all()), bool(b.isfinite().all())]  # (new, before)
                result["jvp_finite"] = [bool(jvp.float().isfinite().all()), bool(jvp_rows.float().isfinite().all())]
                result["gradients_rel_difference"] = round(float(torch.linalg.norm(a - b)) / max(float(torch.linalg.norm(b)), 1e-30), 6)
                result["dL_dinput_rel_difference"] = round(float(torch.linalg.norm(dx["new"] - dx["before"])) / max(float(torch.linalg.norm(dx["before"])), 1e-30), 6)
            print(json.dumps(result), flush=True)
        del native, cutlass


if __name__ == "__main__":
    main()
