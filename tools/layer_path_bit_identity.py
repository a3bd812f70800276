#!/usr/bin/env python3
"""Bit comparison of the layer-by-layer MLP path (k_mlp_layers.hip, k_mlp_layers_f32.hip) and of the fused networks' weight-gradient panels
under two builds of the library (a refactor's parent and the refactor).

    TCNN_AMD_LIB=<parent's libtcnn_amd.so> python tools/layer_path_bit_identity.py run parent.json
    python tools/layer_path_bit_identity.py run branch.json
    python tools/layer_path_bit_identity.py compare parent.json branch.json [summary.txt]

`run` (one process per library) records, per case, a sha256 over the raw bits of everything the case produces.  A case is a tcnn.Network shape
x hidden activation x output activation x precision (fp16, fp32) x batch size (256 = BATCH_SIZE_GRANULARITY: one sample block of the 64 x 256
tiling and two of the 128 x 128 tiling; 512: two and four) x one of
    module   the module's passes on seeded tensors: inference; forward + backward with dL/dinput and parameter gradients;
             backward_backward_input with dL/d(dL/doutput), parameter gradients and dS/dinput
    trainer  the same network behind an Identity encoding in a Trainer: forward() + backward() with dL_dinput under GradientMode Overwrite, then
             Accumulate (output, loss, dL_dinput and the parameter gradients of both steps)
Shapes (SHAPES): 16 -> 48 -> 48 -> 3 (the narrow tiling; k = 16, shorter than one stage; k = 48, a partial second stage: fp32 skips the missing
k-steps, half multiplies zeros; 48 rows in a 64-row block: a skipped tile), 32 -> 144 -> 144 -> 20 (padded to 32; the 128 x 128 tiling whose second
output block holds one live tile; k = 144: four stages and a half), 32 -> 16 with no hidden layer, and a 64-wide Sine network (pre-activations
stored, cosine backward).  Hidden activations ReLU, Sine and Tanh (Tanh has curvature: the R / P products run); output activations None and
Sigmoid (mlp_layer_delta, mlp_activation_backward_output).  In half only: the fused kernels' Network::backward at width 64 and at width 256 (tiled
weight-gradient panels; 256 is two column panels), and the width-64 network once more under TCNN_AMD_MLP_LAYERWISE=1 (a switch holds from the
creation of the case's model on)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mlp(otype, act, out_act, width, hidden):
    return {"otype": otype, "activation": act, "output_activation": out_act, "n_neurons": width, "n_hidden_layers": hidden}


SHAPES = [  # (name, n_in, n_out, width, hidden layers, hidden activations)
    ("16-48-48-3", 16, 3, 48, 2, ("ReLU", "Sine", "Tanh")), ("32-144-144-20", 32, 20, 144, 2, ("ReLU", "Sine", "Tanh")),
    ("32-16-no-hidden", 32, 16, 16, 0, ("None",)), ("32-64-64-16-sine", 32, 16, 64, 2, ("Sine",)),
]
FUSED = [  # half only: (name, n_in, n_out, network, switches)
    ("fused-w64", 32, 16, mlp("FullyFusedMLP", "ReLU", "None", 64, 2), {}), ("fused-w256", 32, 16, mlp("CutlassMLP", "ReLU", "None", 256, 2), {}),
    ("fused-w64-sigmoid", 32, 16, mlp("FullyFusedMLP", "ReLU", "Sigmoid", 64, 2), {}), ("w64-layerwise", 32, 16, mlp("FullyFusedMLP", "ReLU", "None", 64, 2), {"TCNN_AMD_MLP_LAYERWISE": "1"}),
]
BATCHES = (256, 512)


def run(out_path):
    sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
    import torch

    import tinycudann as tcnn
    from tinycudann import native

    def bits(h, *tensors):
        for t in tensors:
            if t is not None:
                h.update(t.detach().contiguous().cpu().numpy().tobytes())

    def rand(gen, shape, dtype=torch.float32):
        return ((torch.rand(shape, device="cuda", generator=gen) - 0.5) * 2).to(dtype)

    def module_case(n_in, n_out, net, fp32, n, second_order):
        module = tcnn.Network(n_in, n_out, net, dtype=torch.float32 if fp32 else None)
        nat = module.native_tcnn_module
        dtype = torch.float32 if fp32 else torch.half
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        x, v, dy = rand(gen, (n, n_in)), rand(gen, (n, n_in)), rand(gen, (n, nat.n_output_dims()), dtype)
        params = module.params.detach().to(dtype)
        h = hashlib.sha256()
        bits(h, nat.fwd(x, params)[1])  # inference
        x.requires_grad_(True), params.requires_grad_(True), dy.requires_grad_(True)
        ctx, out = nat.fwd(x, params)
        bits(h, out, *nat.bwd(ctx, x, params, out, dy))
        if second_order:
            bits(h, *nat.bwd_bwd_input(ctx, x, params, v, dy))
        return {"sha256": h.hexdigest()}

    def trainer_case(n_in, n_out, net, fp32, n):
        config = {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2}, "encoding": {"otype": "Identity"}, "network": net}
        tr = tcnn.Trainer(n_in, n_out, config, seed=1337, dtype=torch.float32 if fp32 else None)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        h = hashlib.sha256()
        for mode in (native.GRADIENT_OVERWRITE, native.GRADIENT_ACCUMULATE):
            x, t = rand(gen, (n, n_in)), rand(gen, (n, n_out))
            dx = torch.zeros((n, n_in), device="cuda")
            ctx = tr.forward(x, t, prepare_input_gradients=True)
            tr.backward(ctx, x, dL_dinput=dx, gradient_mode=mode)
            bits(h, ctx.output(), dx, tr.param_gradients())
            h.update(repr(tr.loss(ctx)).encode())
        return {"sha256": h.hexdigest()}

    def set_switches(sw):
        for k in list(os.environ):
            if k.startswith("TCNN_AMD_") and k != "TCNN_AMD_LIB":
                del os.environ[k]
        os.environ.update(sw)

    results = {}
    set_switches({})
    for name, n_in, n_out, width, hidden, acts in SHAPES:
        for act in acts:
            for out_act in ("None", "Sigmoid"):
                net = mlp("CutlassMLP", act, out_act, width, hidden)
                for fp32 in (False, True):
                    for n in BATCHES:
                        key = f"{name} | {act} | {out_act} | {'fp32' if fp32 else 'fp16'} | n={n}"
                        results[key + " | module"] = module_case(n_in, n_out, net, fp32, n, True)
                        results[key + " | trainer"] = trainer_case(n_in, n_out, net, fp32, n)
        print(name, len(results), flush=True)
    for name, n_in, n_out, net, sw in FUSED:
        set_switches(sw)
        for n in BATCHES:
            results[f"{name} | fp16 | n={n} | module"] = module_case(n_in, n_out, net, False, n, net["otype"] == "CutlassMLP")
            results[f"{name} | fp16 | n={n} | trainer"] = trainer_case(n_in, n_out, net, False, n)
        print(name, len(results), flush=True)
    set_switches({})
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
    lines = [f"cases: {len(a)} parent, {len(b)} branch", f"differing cases: {len(differing)}"] + [f"  {k}: {a.get(k)} != {b.get(k)}" for k in differing[:40]]
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
