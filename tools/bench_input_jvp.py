"""Time input_jvp against what a caller had to do before and against its own two-pass route, in one process on one GPU.

  jvp       tcnn_module_input_jvp of T tangents (its route is reported: what the plan chooses is what runs)
  before    what gave J v until now, on the CutlassMLP form of the network (FullyFusedMLP has no second-order pass): ONE tcnn_module_forward
            with prepare_input_gradients, then per tangent tcnn_module_backward_backward_input asked for dL_ddLdoutput only
  two-pass  input_jvp's own two-pass route: the same call on a module of the same shape created under TCNN_AMD_MLP_LAYERWISE=1, whose
            plan is "two-pass" by definition (the encoding pass once, the encoding's tangent per direction, the network's layer-by-layer
            forward pass once and its tangent pass per direction)

Shapes: tools/bench_input_jacobian.py's table (3 outputs), T = 1 and 3 (--tangents for others); for a 16-output head behind the grid at
T = 3 also `jacobian`: tcnn_module_input_jacobian with K = 16, which returns the same 16 x 3 Jacobian.  The sides run interleaved
(A B C A B C ...), each run between device events after a warm-up; the medians are reported.  Prints one JSON line per shape and T
(milliseconds).  usage (GPU box): python tools/bench_input_jvp.py [--runs 30] [--warmup 5] [--all] [--only <shape> ...] [--tangents T ...]
[--side jvp|before|two-pass]   (--only / --side: one shape, one side -- for a profiler run)"""
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

SHAPES = {name: (s[0], s[1], s[2], 3, s[4]) for name, s in GRADIENT_SHAPES.items()}
SHAPES["grid18_o16"] = SHAPES["grid18"][:3] + (16,) + SHAPES["grid18"][4:]
DEFAULT = DEFAULT + ("grid18_o16",)
SIDES = ("jvp", "before", "two-pass")


def shape_of(name):
    """a named shape, or a bare network spelled <relu|softplus><width>x<hidden>[@<log2 rows>] (16 inputs, 3 outputs; 2^18 rows): the plan
    rule's evidence is taken over these"""
    if name in SHAPES:
        return SHAPES[name]
    m = re.fullmatch(r"(relu|softplus)(\d+)x(\d+)(?:@(\d+))?", name)
    if not m:
        raise SystemExit("unknown shape %r" % name)
    network = dict(GRADIENT_SHAPES["net64x4"][1], activation={"relu": "ReLU", "softplus": "Softplus"}[m.group(1)], n_neurons=int(m.group(2)), n_hidden_layers=int(m.group(3)))
    return (None, network, 16, 3, int(m.group(4) or 18))


def make_sides(shape):
    """(the module as configured, its CutlassMLP form, the same shape made to run layer by layer)"""
    os.environ["TCNN_AMD_MLP_LAYERWISE"] = "1"  # (the switches are read when a module is made; this one is kept by the network made under it)
    try:
        layerwise = make(shape)
    finally:
        del os.environ["TCNN_AMD_MLP_LAYERWISE"]
    return make(shape), make(shape[:1] + (dict(shape[1], otype="CutlassMLP"),) + shape[2:]), layerwise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", nargs="+", help="named shapes, or <relu|softplus><width>x<hidden>[@<log2 rows>]")
    ap.add_argument("--tangents", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--all", action="store_true", help="also the shapes beyond the default ones")
    ap.add_argument("--side", choices=SIDES)
    args = ap.parse_args()
    assert args.runs >= 20 or args.side, "the medians are of at least 20 runs"
    for name in args.only or (SHAPES if args.all else DEFAULT):
        shape = shape_of(name)
        native, cutlass, layerwise = make_sides(shape)
        n, n_in, pw = 1 << shape[4], shape[2], native.n_output_dims()
        gen = torch.Generator(device="cuda").manual_seed(42)
        x = torch.rand((n, n_in), device="cuda", generator=gen)
        params = native.initial_params(1337).half().contiguous()
        out = torch.empty((n, pw), dtype=torch.half, device="cuda")
        dy = torch.zeros((n, pw), dtype=torch.half, device="cuda")
        for T in args.tangents:
            v = (torch.rand((n, T, n_in), device="cuda", generator=gen) * 2 - 1).contiguous()
            v_rows = v.permute(1, 0, 2).contiguous()  # [T][n][n_in]: what the second-order pass takes per call
            got, two, before = (torch.empty((n, T, pw), dtype=torch.half, device="cuda") for _ in range(3))
            before_rows = torch.empty((T, n, pw), dtype=torch.half, device="cuda")

            def jvp():
                _C.check(_C.lib.tcnn_module_input_jvp(native._h, _stream(), n, T, _ptr(x), _ptr(v), _ptr(got), None, _ptr(params)))

            def two_pass():
                _C.check(_C.lib.tcnn_module_input_jvp(layerwise._h, _stream(), n, T, _ptr(x), _ptr(v), _ptr(two), None, _ptr(params)))

            def before_calls():
                h = C.c_void_p()
                _C.check(_C.lib.tcnn_module_forward(cutlass._h, _stream(), n, _ptr(x), _ptr(out), _ptr(params), 1, C.byref(h)))
                for t in range(T):
                    _C.check(_C.lib.tcnn_module_backward_backward_input(cutlass._h, _stream(), h, n, _ptr(v_rows[t]), _ptr(x), _ptr(dy), None, _ptr(before_rows[t]), None, _ptr(params)))
                _C.lib.tcnn_context_destroy(h)

            sides = {"jvp": jvp, "before": before_calls, "two-pass": two_pass}
            K = 16
            if shape[3] == K and T == 3 and not args.side:
                dims = (C.c_uint32 * K)(*range(K))
                jac = torch.empty((n, K, n_in), dtype=torch.float32, device="cuda")

                def jacobian():
                    _C.check(_C.lib.tcnn_module_input_jacobian(native._h, _stream(), n, dims, K, _ptr(x), _ptr(jac), None, _ptr(params), SCALE))

                sides["jacobian"] = jacobian
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
            if "jvp" in sides:
                result["route"] = native.last_input_jvp_route()
            if "two-pass" in sides:
                assert layerwise.last_input_jvp_route() == "two-pass"
            for k, t in times.items():
                result[k + "_median"] = round(statistics.median(t), 4)
                result[k + "_min"] = round(min(t), 4)
            if len(times) >= 3:
                before.copy_(before_rows.permute(1, 0, 2))
                assert torch.equal(two.view(torch.int16), before.view(torch.int16)), "the two-pass route and the second-order pass differ"
                scale = float(two.float().abs().max())
                result["jvp_vs_two_pass_max_abs_over_max"] = round(float((got.float() - two.float()).abs().max()) / max(scale, 1e-30), 6)
                result["two_pass_over_jvp"] = round(result["two-pass_median"] / result["jvp_median"], 3)
                result["before_over_jvp"] = round(result["before_median"] / result["jvp_median"], 3)
                if "jacobian" in sides:
                    result["jacobian_over_jvp"] = round(result["jacobian_median"] / result["jvp_median"], 3)
            print(json.dumps(result), flush=True)
        del native, cutlass, layerwise


if __name__ == "__main__":
    main()
