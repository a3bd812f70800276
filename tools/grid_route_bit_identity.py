#!/usr/bin/env python3
"""Bit comparison of the grid encoding's forward and gradient paths under two builds of the library (a refactor's parent and the refactor).

    TCNN_AMD_LIB=<parent's libtcnn_amd.so> python tools/grid_route_bit_identity.py run parent.json
    python tools/grid_route_bit_identity.py run branch.json
    python tools/grid_route_bit_identity.py compare parent.json branch.json [summary.txt]

`run` (one process per library) takes every case below through three steps on seeded batches and records, per case, a sha256 over the raw
bits of everything the case produces -- output, loss, dL_dinput, parameter gradients, the parameters after the optimizer's steps -- plus which
launches did the work: list_scatters, list_gradient_tails, scatter_wide_fallbacks, last_step_kernel.  Cases: a Trainer's training_step
(GradientMode Overwrite, and Accumulate in its second step; with and without dL_dinput), the Trainer's forward() + backward() (the unfused
model passes, with and without input gradients, Overwrite and Accumulate), a NetworkWithInputEncoding module's and an Encoding module's
forward / backward with and without input gradients; max_level none, scalar and per sample; the grid shapes of tests/test_gpu_parity.py's
SCATTER_CASES / ROWS_CASES plus F = 1, an fp32 encoding and a grid with binned levels; batches of 4096, 2^14 and 2^16; under the default
switches and each A/B switch of SWITCH_SETS (a switch set holds from the creation of the case's model on).  Three steps, so that the scatter
tuner's re-cut plan (second filtered launch) is included."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCH_SETS = [{}, {"TCNN_AMD_GRID_PLANES": "0"}, {"TCNN_AMD_GRID_ROWS_PLANES": "0"}, {"TCNN_AMD_GRID_SCATTER": "atomic"}, {"TCNN_AMD_SCATTER_RECORDS": "0"},
               {"TCNN_AMD_SCATTER_LISTS": "0"}, {"TCNN_AMD_SCATTER_LISTS": "1"}, {"TCNN_AMD_LISTGRAD_IN_MLP": "0"}, {"TCNN_AMD_ADAM_PROLOGUE": "0"},
               {"TCNN_AMD_SIDE_JOBS": "0"}, {"TCNN_AMD_SCATTER_TUNE": "0"}]
# the switch sets under which every kind of case, the max_level states and the middle batch size are run (the others: a training step, the two
# modules' passes, no cut-off, 4096 and 2^16)
FULL_SETS = ({}, {"TCNN_AMD_SCATTER_LISTS": "1"}, {"TCNN_AMD_GRID_SCATTER": "atomic"})


def grid(levels, F, log2_t, base, scale, **more):
    return dict({"otype": "HashGrid", "n_levels": levels, "n_features_per_level": F, "log2_hashmap_size": log2_t, "base_resolution": base, "per_level_scale": scale}, **more)


ENCODINGS = [  # (name, n_in, config, fp32)
    ("2d-L16F2T19", 2, grid(16, 2, 19, 16, 2.0), False), ("2d-L16F2T15", 2, grid(16, 2, 15, 16, 1.5), False), ("3d-L8F4T16", 3, grid(8, 4, 16, 8, 2.0), False),
    ("3d-L4F8T14", 3, grid(4, 8, 14, 8, 2.0), False), ("2d-dense-L5F2", 2, {"otype": "DenseGrid", "n_levels": 5, "n_features_per_level": 2, "base_resolution": 16, "per_level_scale": 2.0}, False),
    ("2d-L8F2T14-smooth", 2, grid(8, 2, 14, 8, 1.5, interpolation="Smoothstep"), False), ("2d-L8F2T14-nearest", 2, grid(8, 2, 14, 8, 1.5, interpolation="Nearest"), False),
    ("3d-L8F2T18", 3, grid(8, 2, 18, 8, 2.0), False), ("2d-L8F4T17", 2, grid(8, 4, 17, 16, 1.5), False), ("2d-L4F8T12", 2, grid(4, 8, 12, 16, 2.0), False),
    ("3d-L6F2T18", 3, grid(6, 2, 18, 8, 2.0), False),  # 12 features: padded to 16 in front of a network
    ("2d-L8F1T15", 2, grid(8, 1, 15, 16, 1.5), False), ("3d-L8F2T18-fp32", 3, grid(8, 2, 18, 8, 2.0), True), ("3d-L8F4T19-binned", 3, grid(8, 4, 19, 16, 2.0), False),
]
NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
CONFIG = {"loss": {"otype": "RelativeL2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}, "network": NETWORK}
N_OUT = 3
STEPS = 3


def run(out_path):
    sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
    import torch

    import tinycudann as tcnn
    from tinycudann import native

    def bits(h, *tensors):
        for t in tensors:
            if t is not None:
                h.update(t.detach().contiguous().cpu().numpy().tobytes())

    def batches(n, n_in, width, half):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        xs = [torch.rand((n, n_in), device="cuda", generator=gen) for _ in range(STEPS)]
        ts = [torch.rand((n, N_OUT), device="cuda", generator=gen) for _ in range(STEPS)]
        dys = [((torch.rand((n, width), device="cuda", generator=gen) - 0.5) * 4).to(torch.half if half else torch.float32) for _ in range(STEPS)]
        level = torch.rand((n,), device="cuda", generator=gen)
        return xs, ts, dys, level

    def set_level(obj, state, level):
        if state == "scalar":
            obj.set_max_level(0.5)
        elif state == "per-sample":
            obj.set_max_level_gpu(level)

    def trainer_case(n_in, enc, n, state, kind):
        xs, ts, _, level = batches(n, n_in, 1, True)
        tr = tcnn.Trainer(n_in, N_OUT, dict(CONFIG, encoding=enc), seed=1337)
        set_level(tr, state, level)
        h = hashlib.sha256()
        for i in range(STEPS):
            dx = torch.zeros((n, n_in), device="cuda") if kind.endswith("dx") else None
            mode = native.GRADIENT_ACCUMULATE if i == 1 else native.GRADIENT_OVERWRITE
            if kind.startswith("step"):
                ctx = tr.training_step(xs[i], ts[i], dL_dinput=dx, gradient_mode=mode)
            else:  # the unfused passes of the model
                ctx = tr.forward(xs[i], ts[i], prepare_input_gradients=dx is not None)
                tr.backward(ctx, xs[i], dL_dinput=dx, gradient_mode=mode)
                tr.optimizer_step()
            bits(h, ctx.output(), dx, tr.param_gradients())
            h.update(repr(tr.loss(ctx)).encode())
        bits(h, tr.params(), tr.params_full_precision())
        return {"sha256": h.hexdigest(), "list_scatters": tr.list_scatters(), "list_gradient_tails": tr.list_gradient_tails(), "scatter_wide_fallbacks": tr.scatter_wide_fallbacks(),
                "last_step_kernel": tr.last_step_kernel()}

    def module_case(n_in, enc, fp32, n, state, kind):
        if kind.startswith("nwie"):
            module = tcnn.NetworkWithInputEncoding(n_in, N_OUT, enc, NETWORK)
        else:
            module = tcnn.Encoding(n_in, enc, dtype=torch.float32 if fp32 else None)
        nat = module.native_tcnn_module
        xs, _, dys, level = batches(n, n_in, nat.n_output_dims(), not (fp32 and kind.startswith("enc")))
        set_level(nat, state, level)
        params = module.params.detach().to(torch.float32 if fp32 and kind.startswith("enc") else torch.half).requires_grad_(True)
        h = hashlib.sha256()
        for i in range(STEPS):
            x = xs[i].requires_grad_(kind.endswith("dx"))
            ctx, out = nat.fwd(x, params)
            dx, g = nat.bwd(ctx, x, params, out, dys[i])
            bits(h, out, dx, g)
        return {"sha256": h.hexdigest(), "list_scatters": nat.list_scatters()}

    results = {}
    for sw in SWITCH_SETS:
        for k in list(os.environ):
            if k.startswith("TCNN_AMD_") and k != "TCNN_AMD_LIB":
                del os.environ[k]
        os.environ.update(sw)
        full = sw in FULL_SETS
        sw_name = ",".join(f"{k[9:]}={v}" for k, v in sw.items()) or "default"
        for name, n_in, enc, fp32 in ENCODINGS:
            for n in (4096, 1 << 14, 1 << 16) if full else (4096, 1 << 16):
                for state in ("none", "scalar", "per-sample") if full and n == 4096 else ("none",):
                    for kind in ("step", "step-dx", "model", "model-dx", "nwie", "nwie-dx", "enc", "enc-dx") if full else ("step", "nwie", "enc", "enc-dx"):
                        if fp32 and not kind.startswith("enc"):
                            continue  # (networks are half precision)
                        key = f"{sw_name} | {name} | n={n} | max_level={state} | {kind}"
                        results[key] = trainer_case(n_in, enc, n, state, kind) if kind[:4] in ("step", "mode") else module_case(n_in, enc, fp32, n, state, kind)
            print(sw_name, name, len(results), flush=True)
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(results, f, indent=0, sort_keys=True)
    print(f"{len(results)} cases -> {out_path}")


def compare(a_path, b_path, summary_path=None):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    differing = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    paths = {}
    for k, v in b.items():
        kernel = v.get("last_step_kernel", "module")
        path = ("lists" if v["list_scatters"] else "no lists") + ("+tail" if v.get("list_gradient_tails") else "") + ("+wide" if v.get("scatter_wide_fallbacks") else "")
        paths[f"{kernel}: {path}"] = paths.get(f"{kernel}: {path}", 0) + 1
    lines = [f"cases: {len(a)} parent, {len(b)} branch", "paths covered (MLP kernel of the last step or module: gradient path x cases): " + ", ".join(f"{k} x{v}" for k, v in sorted(paths.items())),
             f"differing cases: {len(differing)}"] + [f"  {k}: {a.get(k)} != {b.get(k)}" for k in differing[:40]]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if summary_path:
        with open(summary_path, "w") as f:
            f.write(text)
    return 1 if differing or len(a) != len(b) else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    else:
        sys.exit(__doc__)
