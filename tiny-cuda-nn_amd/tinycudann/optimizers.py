"""The library's optimizers for PyTorch modules: `tcnn.optimizers.Optimizer(modules, config)`.

The optimizers a `tcnn.Trainer` runs -- Adam, SGD, Novograd, Ema, ExponentialDecay, Average, Batched, Lookahead, Composite
(optimizers/*.h of the reference, nested as instant-ngp configures them) -- for callers whose loss is their own:

    model = tcnn.NetworkWithInputEncoding(3, 4, encoding, network)
    opt = tcnn.optimizers.Optimizer(model, {"otype": "Ema", "decay": 0.95, "nested": {"otype": "ExponentialDecay", ...,
                                            "nested": {"otype": "Adam", "learning_rate": 1e-2, "epsilon": 1e-15, "l2_reg": 1e-6}}})
    loss = render(model(x)).sub(target).square().mean(); loss.backward(); opt.step(); opt.zero_grad()

What differs from `torch.optim.Adam` is the reference's semantics (optimizers/adam.h): a non-matrix parameter (a hash-grid entry)
whose gradient is exactly zero is not touched -- no moment decay, no step count, no move; `l2_reg` applies to the weight matrices
only; every parameter has its own step count and debiasing; `non_matrix_learning_rate_factor` and weight clipping exist.  The same
model then trains the same way through `tcnn.Trainer` and through the modules.

One native optimizer (`_C.lib.tcnn_optimizer_*`, include/tcnn_amd.h) per module.  Its step reads `params.grad` as it is (fp32, or half),
updates the fp32 `params` in place and writes the half weights in the same pass into a buffer this object owns, which it installs as the
module's working copy: attaching an optimizer turns the module's `reuse_working_copy` on, and the next `forward` runs no cast pass.
A write to the parameter by other means (`load_state_dict`, `copy_`) shows in its version counter: the module rebuilds its copy, and
the half buffer is taken from the parameter again before the next step.  Writes through `.data` show nowhere: call
`module.invalidate_working_copy()` after them, as without an optimizer -- the optimizer notices that the module no longer holds the
copy it was handed and resynchronises too.  The half buffer's version counter is bumped with the parameter's: a backward pass through
a graph from before the step raises instead of differentiating at the new weights.
"""
import contextlib
import ctypes as C
import json

import torch

from . import _C
from .modules import Module

GRADIENT_PRECISION = {torch.float32: _C.Precision.Fp32, torch.float16: _C.Precision.Fp16}


class NativeOptimizer:
    """One tcnn_optimizer_t handle: tcnn::Optimizer<half> (optimizer.h) on caller-owned parameter and gradient vectors.
    weight_dtype=torch.float32: Optimizer<float> -- ONE float weight vector, `step(params_fp32, None, gradients_fp32)`, float custom weights."""

    def __init__(self, config, n_params, layer_sizes=(), device=None, weight_dtype=torch.half):
        """device: where the optimizer's state lives (the parameters' device); None: the current one, once the configuration is accepted"""
        if weight_dtype not in GRADIENT_PRECISION:
            raise ValueError(f"NativeOptimizer only supports fp32 or fp16 precision, but got {weight_dtype}")
        self.weight_dtype = weight_dtype
        flat = [int(v) for pair in layer_sizes for v in pair]
        sizes = (C.c_uint32 * max(len(flat), 1))(*flat)
        h = C.c_void_p()
        self._h = None
        self.device = None if device is None else torch.device(device)
        with self._on_device():
            _C.check(_C.lib.tcnn_optimizer_create_precision(_C.to_json_bytes(config), int(n_params), sizes, len(flat) // 2, GRADIENT_PRECISION[weight_dtype], C.byref(h)))
        self._h = h
        self.n_params = int(n_params)
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    def _on_device(self):
        """the state was allocated on self.device: everything that touches it runs with that device current"""
        return contextlib.nullcontext() if self.device is None else torch.cuda.device(self.device)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _C is not None and getattr(_C, "lib", None) is not None:  # modules may already be torn down at exit
            _C.lib.tcnn_optimizer_destroy(h)

    def step(self, params_fp32, params_half, gradients, loss_scale=1.0, stream=None):
        """One step on `stream` (default: the current torch stream).  gradients: float32 or float16, n_params values."""
        # (fp32 weights: ONE weight vector -- params_half is None, or params_fp32 again; the library refuses any other pointer)
        checked = ((params_fp32, torch.float32),) if self.weight_dtype == torch.float32 else ((params_fp32, torch.float32), (params_half, torch.float16))
        for t, dtype in checked:
            if not (t is not None and t.is_cuda and t.is_contiguous() and t.dtype == dtype and t.numel() == self.n_params):
                raise RuntimeError(f"tcnn: the optimizer needs contiguous device tensors of {self.n_params} values: float32 master weights and float16 working weights")
        if gradients.dtype not in GRADIENT_PRECISION:
            raise RuntimeError(f"tcnn: gradients must be float32 or float16, not {gradients.dtype}")
        if not (gradients.is_cuda and gradients.is_contiguous() and gradients.numel() == self.n_params):
            raise RuntimeError(f"tcnn: gradients must be a contiguous device tensor of {self.n_params} values")
        if not (params_fp32.device == gradients.device == self.device and (params_half is None or params_half.device == self.device)):
            raise RuntimeError(f"tcnn: the optimizer's state lives on {self.device}; weights and gradients must live there too")
        self.step_unchecked(params_fp32, params_half, gradients, loss_scale, stream)

    def step_unchecked(self, params_fp32, params_half, gradients, loss_scale=1.0, stream=None):
        """step() for callers that have made its checks themselves (the per-step host time counts: the kernel takes ~60 us on C3a)"""
        device = self.device
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        if device.index != torch.cuda.current_device():
            with torch.cuda.device(device):
                return self.step_unchecked(params_fp32, params_half, gradients, loss_scale, stream)
        if _C.lib.tcnn_optimizer_step(self._h, stream, loss_scale, params_fp32.data_ptr(), None if params_half is None else params_half.data_ptr(), gradients.data_ptr(),
                                      GRADIENT_PRECISION[gradients.dtype]):
            _C.check(1)

    def step_count(self):
        return int(_C.lib.tcnn_optimizer_step_count(self._h))

    def learning_rate(self):
        return float(_C.lib.tcnn_optimizer_learning_rate(self._h))

    def set_learning_rate(self, value):
        _C.check(_C.lib.tcnn_optimizer_set_learning_rate(self._h, float(value)))

    def update_hyperparams(self, config):
        _C.check(_C.lib.tcnn_optimizer_update_hyperparams(self._h, _C.to_json_bytes(config)))

    def hyperparams(self):
        return json.loads(_C.lib.tcnn_optimizer_hyperparams(self._h).decode())

    def serialize(self):
        """MessagePack bytes of the object a Trainer snapshot carries as its "optimizer" entry."""
        ptr, size = C.c_void_p(), C.c_size_t()
        with self._on_device():
            _C.check(_C.lib.tcnn_optimizer_serialize(self._h, C.byref(ptr), C.byref(size)))
        return C.string_at(ptr, size.value)

    def deserialize(self, data):
        data = bytes(data)
        with self._on_device():
            _C.check(_C.lib.tcnn_optimizer_deserialize(self._h, data, len(data)))

    def custom_weights(self):
        """A tensor copy (on the optimizer's device, in its weight dtype) of its inference weights (Ema, Average, Lookahead), or None."""
        ptr = _C.lib.tcnn_optimizer_custom_weights(self._h)
        if not ptr:
            return None
        with self._on_device():
            torch.cuda.synchronize()
            out = torch.empty(self.n_params, dtype=self.weight_dtype, device=self.device)
            _C.memcpy_dtod(out.data_ptr(), ptr, self.n_params * self.weight_dtype.itemsize)
        return out

    def weights_restored(self, params_half, stream=None):
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        with self._on_device():
            _C.check(_C.lib.tcnn_optimizer_weights_restored(self._h, stream, params_half.data_ptr()))


def module_layer_sizes(module):
    """[(rows, cols)] of a tcnn.Module's weight matrices in parameter order (tcnn_module_layer_sizes)."""
    h = module.native_tcnn_module._h
    n = C.c_size_t()
    _C.check(_C.lib.tcnn_module_layer_sizes(h, None, 0, C.byref(n)))
    flat = (C.c_uint32 * max(2 * n.value, 1))()
    _C.check(_C.lib.tcnn_module_layer_sizes(h, flat, n.value, C.byref(n)))
    return [(int(flat[2 * i]), int(flat[2 * i + 1])) for i in range(n.value)]


class Optimizer(torch.optim.Optimizer):
    """modules: one tcnn.Module or a list; config: the optimizer configuration a Trainer takes (nesting included), or one per module.
    Each module is one param group with one native optimizer.  `param_groups[i]["lr"]` starts as the native learning rate and is
    forwarded whenever it changed, so torch.optim.lr_scheduler works; loss scale is 1 (the modules unscale their gradients)."""

    def __init__(self, modules, config):
        modules = [modules] if isinstance(modules, torch.nn.Module) else list(modules)
        if not modules:
            raise ValueError("tcnn.optimizers.Optimizer: no modules given")
        configs = list(config) if isinstance(config, (list, tuple)) else [config] * len(modules)
        if len(configs) != len(modules):
            raise ValueError(f"tcnn.optimizers.Optimizer: {len(configs)} configurations for {len(modules)} modules")
        for m in modules:
            if not isinstance(m, Module):
                raise TypeError(f"tcnn.optimizers.Optimizer optimizes tcnn modules (Encoding, Network, NetworkWithInputEncoding), not {type(m).__name__}: "
                                "use torch.optim for other parameters")
            if m.dtype != torch.half:
                raise TypeError("tcnn.optimizers.Optimizer needs half-precision working weights; this module's parameters are used in "
                                f"{m.dtype} (Encoding(dtype=torch.float32)): use torch.optim for it")
        self._modules = modules
        self._natives = [NativeOptimizer(c, m.params.numel(), module_layer_sizes(m), m.params.device) for m, c in zip(modules, configs)]
        self._half = [None] * len(modules)  # the half weights the native step writes; the module's working copy
        self._installed = [False] * len(modules)  # the half weights have been handed to the module as its working copy
        self._seen = [None] * len(modules)  # (version, address, device) of the parameter the half weights belong to
        groups = [{"params": [m.params], "lr": n.learning_rate()} for m, n in zip(modules, self._natives)]
        super().__init__(groups, {})
        self._native_lr = [g["lr"] for g in self.param_groups]
        for m in modules:
            m.reuse_working_copy = True

    @staticmethod
    def _key(p):
        return (p._version, p.data_ptr(), p.device)

    def _current(self, i, p, module):
        """Whether the half weights of module i still are parameter p's: nobody but step() wrote p (version, address), and the module
        has not dropped or replaced the copy it was handed -- which is what `invalidate_working_copy()` after a write through
        `params.data` does, the one kind of write that shows nowhere else."""
        return self._half[i] is not None and self._seen[i] == self._key(p) and not (self._installed[i] and module._working_copy is not self._half[i])

    def _sync_half(self, i, p, force=False):
        """The half weights of module i, current for parameter p: taken from it again (and the optimizer told) when not, or when forced."""
        if force or self._half[i] is None or self._seen[i] != self._key(p):
            first = self._half[i] is None
            self._half[i] = p.detach().to(torch.half).contiguous() if first or self._half[i].device != p.device else self._half[i].copy_(p.detach())
            self._seen[i] = self._key(p)
            if not first:
                self._natives[i].weights_restored(self._half[i])
        return self._half[i]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for i, (group, module, native) in enumerate(zip(self.param_groups, self._modules, self._natives)):
            p = group["params"][0]
            if p.grad is None:
                continue
            if group["lr"] != self._native_lr[i]:
                native.set_learning_rate(group["lr"])
                self._native_lr[i] = group["lr"]
            grad = p.grad
            if grad.dtype not in GRADIENT_PRECISION:
                grad = grad.float()
            if not grad.is_contiguous():
                grad = grad.contiguous()
            if not (grad.device == p.device == native.device and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError(f"tcnn.optimizers.Optimizer: the parameter must be a contiguous float32 tensor on {native.device}, where the optimizer was made, "
                                   "with its gradient on the same device")
            half = self._half[i] if self._current(i, p, module) else self._sync_half(i, p, force=True)
            native.step_unchecked(p, half, grad, 1.0)  # (p: an fp32 contiguous device Parameter of a tcnn.Module, half: made from it)
            # what an in-place torch update does: working copies see the write to p, and the backward pass of a graph that saved the half
            # weights before this step raises torch's "modified by an inplace operation" instead of differentiating at the new weights
            torch.autograd.graph.increment_version(p)
            torch.autograd.graph.increment_version(half)
            self._seen[i] = self._key(p)
            if module.params is p:
                module._working_copy, module._working_key = half, self._seen[i]
                self._installed[i] = True
        return loss

    def inference_params(self, module):
        """A half tensor copy of the optimizer's inference weights for `module` (Ema / Average / Lookahead weights), or None.
        To evaluate with them: `module.params.data.copy_(w.float()); module.invalidate_working_copy()`."""
        i = next((k for k, m in enumerate(self._modules) if m is module), None)
        if i is None:
            raise ValueError("tcnn.optimizers.Optimizer.inference_params: not a module of this optimizer")
        return self._natives[i].custom_weights()

    def native(self, module_or_index=0):
        if isinstance(module_or_index, int):
            return self._natives[module_or_index]
        return self._natives[next(k for k, m in enumerate(self._modules) if m is module_or_index)]

    def state_dict(self):
        """torch's layout (param_groups with their "lr") plus, per group, the native state as a uint8 tensor of the bytes
        tcnn_optimizer_serialize yields: a checkpoint resumes bit-identically."""
        out = super().state_dict()
        out["native_state"] = [torch.frombuffer(bytearray(n.serialize()), dtype=torch.uint8).clone() for n in self._natives]
        out["native_lr"] = list(self._native_lr)  # the rates last forwarded (a nested ExponentialDecay moves the native one by itself)
        return out

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        native_state, native_lr = state_dict.pop("native_state", None), state_dict.pop("native_lr", None)
        if native_state is None or len(native_state) != len(self._natives):
            raise ValueError("tcnn.optimizers.Optimizer.load_state_dict: the state holds no native optimizer state for these modules")
        super().load_state_dict(state_dict)
        for i, (n, blob) in enumerate(zip(self._natives, native_state)):
            n.deserialize(blob.cpu().numpy().tobytes())
            # the half weights are taken from the parameter again: it was usually loaded along with this state
            n.weights_restored(self._sync_half(i, self.param_groups[i]["params"][0], force=True))
            self._native_lr[i] = native_lr[i] if native_lr is not None else self.param_groups[i]["lr"]
