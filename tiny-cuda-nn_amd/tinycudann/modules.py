"""PyTorch(-ROCm) surface of tcnn_amd: `Encoding`, `Network`, `NetworkWithInputEncoding`.

Same names, constructor arguments and tensor contracts as the reference's Python package
(bindings/torch/tinycudann/modules.py:162-329 and the `_C.Module` methods of bindings.cpp:75-266), so instant-ngp-style
callers can switch by changing nothing but the installed package; the implementation behind those names is this package's.  PyTorch is used for what it is here: device memory,
streams and autograd plumbing; every computation happens in libtcnn_amd.so behind the C ABI.
"""
import contextlib
import gc
import json
import warnings

import torch

from . import _C


def _torch_precision(p):
    if p == _C.Precision.Fp16:
        return torch.half
    if p == _C.Precision.Fp32:
        return torch.float
    raise ValueError(f"Unknown precision {p}")


def _require_gpu():
    if not torch.cuda.is_available():
        # modules.py:18-19 of the reference raises the same kind of error at import time
        raise EnvironmentError("tinycudann (tcnn_amd) needs a ROCm GPU (gfx950): torch.cuda.is_available() is False.")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def free_temporary_memory():
    gc.collect()
    _C.free_temporary_memory()


class NativeModule:
    """One tcnn_module_t handle; the counterpart of bindings.cpp's `Module` class."""

    def __init__(self, handle):
        self._h = handle
        self._max_level_gpu = None  # the per-sample array handed to the native module (kept alive here)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _C is not None and getattr(_C, 'lib', None) is not None:  # modules may already be torn down at exit
            _C.lib.tcnn_module_destroy(h)

    # --- max_level of the grid encoding(s) (GridEncoding::set_max_level / set_max_level_gpu, grid_interface.h:101-123; tcnn_amd.h)
    def set_max_level(self, value):
        _C.check(_C.lib.tcnn_module_set_max_level(self._h, float(value)))

    def max_level(self):
        value = float(_C.lib.tcnn_module_max_level(self._h))
        if value != value and _C.lib.tcnn_last_error():  # NaN: an error, or a NaN that was set (tcnn_last_error() is empty then)
            raise RuntimeError(_C.lib.tcnn_last_error().decode("utf-8", "replace"))
        return value

    def set_max_level_gpu(self, per_sample):
        """per_sample: a float32 device tensor with one value per row of every later call (kept alive here), or None"""
        _C.check(_C.lib.tcnn_module_set_max_level_gpu(self._h, _ptr(per_sample)))
        self._max_level_gpu = per_sample

    def max_level_gpu(self):
        return self._max_level_gpu

    # --- bindings.cpp:242-260
    def n_input_dims(self):
        return int(_C.lib.tcnn_module_n_input_dims(self._h))

    def n_output_dims(self):
        return int(_C.lib.tcnn_module_n_output_dims(self._h))

    def n_params(self):
        return int(_C.lib.tcnn_module_n_params(self._h))

    def list_scatters(self):
        """backward passes of the module's grid encoding(s) that ran the list-fed gradient kernel (tcnn_amd.h: tcnn_module_list_scatters)"""
        return int(_C.lib.tcnn_module_list_scatters(self._h))

    def param_precision(self):
        return int(_C.lib.tcnn_module_param_precision(self._h))

    def output_precision(self):
        return int(_C.lib.tcnn_module_output_precision(self._h))

    def hyperparams(self):
        return json.loads(_C.lib.tcnn_module_hyperparams(self._h).decode())

    def name(self):
        return _C.lib.tcnn_module_name(self._h).decode()

    def initial_params(self, seed):  # bindings.cpp:236-240
        out = torch.zeros(self.n_params(), dtype=torch.float32, device="cuda")
        _C.check(_C.lib.tcnn_module_initialize_params(self._h, int(seed), _ptr(out), 1.0))
        return out

    def _check_inputs(self, input, params):
        if not (input.is_cuda and input.is_contiguous() and params.is_cuda and params.is_contiguous()):
            raise RuntimeError("tcnn: input and params must be contiguous device tensors")
        if input.dtype != torch.float32 or params.dtype != _torch_precision(self.param_precision()):
            raise RuntimeError("tcnn: wrong dtype for input or params")
        if input.shape[1] != self.n_input_dims() or params.shape[0] != self.n_params():
            raise RuntimeError("tcnn: wrong shape for input or params")
        if input.device != params.device:
            raise RuntimeError("tcnn: input and params live on different devices")

    def fwd(self, input, params):  # bindings.cpp:79-110
        self._check_inputs(input, params)
        with torch.cuda.device(input.device):
            n = input.shape[0]
            output = torch.empty((n, self.n_output_dims()), dtype=_torch_precision(self.output_precision()), device=input.device)
            ctx = None
            if not input.requires_grad and not params.requires_grad:
                _C.check(_C.lib.tcnn_module_inference(self._h, _stream(), n, _ptr(input), _ptr(output), _ptr(params)))
            else:
                h = _C.C.c_void_p()
                _C.check(_C.lib.tcnn_module_forward(self._h, _stream(), n, _ptr(input), _ptr(output), _ptr(params), int(input.requires_grad), _C.C.byref(h)))
                ctx = NativeContext(h)
        return ctx, output

    def bwd(self, ctx, input, params, output, dL_doutput):  # bindings.cpp:112-174
        if ctx is None or not ctx._h:
            raise RuntimeError("Module::bwd: called with invalid context. fwd likely (mistakenly) ran in inference mode.")
        self._check_inputs(input, params)
        for t in (output, dL_doutput):
            if not (t.is_cuda and t.is_contiguous()) or t.dtype != _torch_precision(self.output_precision()):
                raise RuntimeError("tcnn: output / dL_doutput must be contiguous device tensors in output precision")
            if t.shape[0] != input.shape[0] or t.shape[1] != self.n_output_dims():
                raise RuntimeError("tcnn: wrong shape for output / dL_doutput")
        with torch.cuda.device(input.device):
            n = input.shape[0]
            dL_dinput = torch.empty((n, input.shape[1]), dtype=torch.float32, device=input.device) if input.requires_grad else None
            dL_dparams = torch.empty(self.n_params(), dtype=params.dtype, device=input.device) if params.requires_grad else None
            if input.requires_grad or params.requires_grad:
                _C.check(_C.lib.tcnn_module_backward(self._h, _stream(), ctx._h, n, _ptr(dL_dinput), _ptr(dL_doutput), _ptr(dL_dparams),
                                                     _ptr(input), _ptr(output), _ptr(params)))
        return dL_dinput, dL_dparams

    def input_gradient(self, input, params, dim, backprop_scale, want_output=False):  # object.h:342-366
        """d output[dim] / d input with `params`, float32 [n, n_input_dims] (and the forward pass's padded output if asked for):
        tcnn_amd.h tcnn_module_input_gradient.  n must be a multiple of the batch granularity."""
        self._check_inputs(input, params)
        with torch.cuda.device(input.device):
            n = input.shape[0]
            d_dinput = torch.empty((n, self.n_input_dims()), dtype=torch.float32, device=input.device)
            output = torch.empty((n, self.n_output_dims()), dtype=_torch_precision(self.output_precision()), device=input.device) if want_output else None
            _C.check(_C.lib.tcnn_module_input_gradient(self._h, _stream(), n, int(dim), _ptr(input), _ptr(d_dinput), _ptr(output), _ptr(params), float(backprop_scale)))
        return d_dinput, output

    def last_input_gradient_route(self):
        """ "none" before the first input_gradient call, then "two-pass" or the fused MLP kernel's name (tcnn_amd.h: tcnn_module_last_input_gradient_route)"""
        return _C.lib.tcnn_module_last_input_gradient_route(self._h).decode()

    def input_jacobian(self, input, params, dims, backprop_scale, want_output=False):
        """d output[dims[k]] / d input for every k from one forward pass, float32 [n, len(dims), n_input_dims] (and the forward pass's padded
        output if asked for): tcnn_amd.h tcnn_module_input_jacobian.  dims count padded columns; n must be a multiple of the batch granularity."""
        self._check_inputs(input, params)
        dims = [int(d) for d in dims]
        with torch.cuda.device(input.device):
            n = input.shape[0]
            jacobian = torch.empty((n, len(dims), self.n_input_dims()), dtype=torch.float32, device=input.device)
            output = torch.empty((n, self.n_output_dims()), dtype=_torch_precision(self.output_precision()), device=input.device) if want_output else None
            _C.check(_C.lib.tcnn_module_input_jacobian(self._h, _stream(), n, (_C.C.c_uint32 * len(dims))(*dims), len(dims), _ptr(input), _ptr(jacobian), _ptr(output), _ptr(params),
                                                       float(backprop_scale)))
        return jacobian, output

    def last_input_jacobian_route(self):
        """ "none" before the first input_jacobian call, then "two-pass" or the fused MLP kernel's name (tcnn_amd.h: tcnn_module_last_input_jacobian_route)"""
        return _C.lib.tcnn_module_last_input_jacobian_route(self._h).decode()

    def input_jvp(self, input, params, tangents, want_output=False):
        """J(x) tangents[:, t, :] for every t, [n, T, n_output_dims] in the output precision, from float32 tangents [n, T, n_input_dims] (and
        the forward pass's padded output if asked for): tcnn_amd.h tcnn_module_input_jvp.  n must be a multiple of the batch granularity."""
        self._check_inputs(input, params)
        n, n_tangents = input.shape[0], tangents.shape[1]
        assert tangents.dtype == torch.float32 and tangents.is_contiguous() and tangents.device == input.device and tuple(tangents.shape) == (n, n_tangents, self.n_input_dims())
        with torch.cuda.device(input.device):
            dtype = _torch_precision(self.output_precision())
            jvp = torch.empty((n, n_tangents, self.n_output_dims()), dtype=dtype, device=input.device)
            output = torch.empty((n, self.n_output_dims()), dtype=dtype, device=input.device) if want_output else None
            _C.check(_C.lib.tcnn_module_input_jvp(self._h, _stream(), n, n_tangents, _ptr(input), _ptr(tangents), _ptr(jvp), _ptr(output), _ptr(params)))
        return jvp, output

    def last_input_jvp_route(self):
        """ "none" before the first input_jvp call, then "two-pass" or the fused MLP kernel's name (tcnn_amd.h: tcnn_module_last_input_jvp_route)"""
        return _C.lib.tcnn_module_last_input_jvp_route(self._h).decode()

    def input_jvp_fwd(self, input, params, tangents, want_output=False):
        """input_jvp with a context for input_jvp_bwd: (context, jvp, output) -- the same bits (tcnn_amd.h: tcnn_module_input_jvp_forward)"""
        self._check_inputs(input, params)
        n, n_tangents = input.shape[0], tangents.shape[1]
        assert tangents.dtype == torch.float32 and tangents.is_contiguous() and tangents.device == input.device and tuple(tangents.shape) == (n, n_tangents, self.n_input_dims())
        with torch.cuda.device(input.device):
            dtype = _torch_precision(self.output_precision())
            jvp = torch.empty((n, n_tangents, self.n_output_dims()), dtype=dtype, device=input.device)
            output = torch.empty((n, self.n_output_dims()), dtype=dtype, device=input.device) if want_output else None
            h = _C.C.c_void_p()
            _C.check(_C.lib.tcnn_module_input_jvp_forward(self._h, _stream(), n, n_tangents, _ptr(input), _ptr(tangents), _ptr(jvp), _ptr(output), _ptr(params), _C.C.byref(h)))
        return NativeContext(h), jvp, output

    def input_jvp_bwd(self, ctx, input, params, tangents, dL_djvp, dL_doutput=None, want_params=True, want_input=True, want_tangents=True, dL_dparams=None):
        """The gradients of sum_t <dL_djvp[:, t], J v_t> + <dL_doutput, f(x)>: (dL_dparams, dL_dinput, dL_dtangents), None where not wanted
        (tcnn_amd.h: tcnn_module_input_jvp_backward).  No loss scale inside.  dL_dparams given: accumulated onto it, else a new tensor."""
        if ctx is None or not ctx._h:
            raise RuntimeError("Module::bwd: called with invalid context. fwd likely (mistakenly) ran in inference mode.")
        self._check_inputs(input, params)
        n, n_tangents = input.shape[0], tangents.shape[1]
        dtype = _torch_precision(self.output_precision())
        assert tangents.dtype == torch.float32 and tangents.is_contiguous() and tuple(tangents.shape) == (n, n_tangents, self.n_input_dims())
        assert dL_djvp.dtype == dtype and dL_djvp.is_contiguous() and tuple(dL_djvp.shape) == (n, n_tangents, self.n_output_dims())
        assert dL_doutput is None or (dL_doutput.dtype == dtype and dL_doutput.is_contiguous() and tuple(dL_doutput.shape) == (n, self.n_output_dims()))
        with torch.cuda.device(input.device):
            mode = 0  # TCNN_GRADIENT_IGNORE
            if dL_dparams is not None:
                assert dL_dparams.dtype == params.dtype and dL_dparams.is_contiguous() and dL_dparams.shape == params.shape
                mode = 2  # TCNN_GRADIENT_ACCUMULATE
            elif want_params:
                dL_dparams = torch.empty(self.n_params(), dtype=params.dtype, device=input.device)
                mode = 1  # TCNN_GRADIENT_OVERWRITE
            if self.n_params() == 0:
                mode = 0  # (nothing to write, and no buffer to name)
            dL_dinput = torch.empty((n, self.n_input_dims()), dtype=torch.float32, device=input.device) if want_input else None
            dL_dtangents = torch.empty((n, n_tangents, self.n_input_dims()), dtype=torch.float32, device=input.device) if want_tangents else None
            _C.check(_C.lib.tcnn_module_input_jvp_backward(self._h, _stream(), ctx._h, n, n_tangents, _ptr(input), _ptr(tangents), _ptr(dL_djvp), _ptr(dL_doutput), _ptr(params),
                                                           _ptr(dL_dparams), _ptr(dL_dinput), _ptr(dL_dtangents), mode))
        return dL_dparams, dL_dinput, dL_dtangents

    def last_input_jvp_backward_route(self):
        """ "none" before the first input_jvp_bwd call, then "two-pass" (tcnn_amd.h: tcnn_module_last_input_jvp_backward_route)"""
        return _C.lib.tcnn_module_last_input_jvp_backward_route(self._h).decode()

    def bwd_bwd_input(self, ctx, input, params, dL_ddLdinput, dL_doutput):  # bindings.cpp:172-245
        """from dL_ddLdinput to (dL_ddLdoutput, dL_dparams, dL_dinput); each is None unless its tensor requires grad."""
        if ctx is None or not ctx._h:
            raise RuntimeError("Module::bwd_bwd_input: called with invalid context. fwd likely (mistakenly) ran in inference mode.")
        self._check_inputs(input, params)
        if not (dL_ddLdinput.is_cuda and dL_ddLdinput.is_contiguous() and dL_ddLdinput.dtype == torch.float32 and dL_ddLdinput.shape == input.shape):
            raise RuntimeError("tcnn: dL_ddLdinput must be a contiguous float32 device tensor shaped like input")
        if not (dL_doutput.is_cuda and dL_doutput.is_contiguous()) or dL_doutput.dtype != _torch_precision(self.output_precision()):
            raise RuntimeError("tcnn: dL_doutput must be a contiguous device tensor in output precision")
        if dL_doutput.shape[0] != input.shape[0] or dL_doutput.shape[1] != self.n_output_dims():
            raise RuntimeError("tcnn: wrong shape for dL_doutput")
        with torch.cuda.device(input.device):
            n = input.shape[0]
            dL_ddLdoutput = torch.zeros((n, self.n_output_dims()), dtype=dL_doutput.dtype, device=input.device) if dL_doutput.requires_grad else None
            dL_dparams = torch.zeros(self.n_params(), dtype=params.dtype, device=input.device) if params.requires_grad else None
            dL_dinput = torch.zeros((n, input.shape[1]), dtype=torch.float32, device=input.device) if input.requires_grad else None
            # The reference only makes the native call when dL_doutput or params require grad (bindings.cpp:224), which leaves
            # dL_dinput all zero for a frozen grid; here the Hessian term is computed whenever the input asks for it.
            if dL_doutput.requires_grad or params.requires_grad or input.requires_grad:
                _C.check(_C.lib.tcnn_module_backward_backward_input(self._h, _stream(), ctx._h, n, _ptr(dL_ddLdinput), _ptr(input), _ptr(dL_doutput), _ptr(dL_dparams),
                                                                    _ptr(dL_ddLdoutput), _ptr(dL_dinput), _ptr(params)))
        return dL_ddLdoutput, dL_dparams, dL_dinput


class NativeContext:
    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _C is not None and getattr(_C, 'lib', None) is not None:  # modules may already be torn down at exit
            _C.lib.tcnn_context_destroy(h)


def _create(fn, *args):
    h = _C.C.c_void_p()
    _C.check(fn(*args, _C.C.byref(h)))
    return NativeModule(h)


# ----------------------------------------------------------------------------------------------------------------------
# autograd glue.  What has to match the reference (bindings/torch/tinycudann/modules.py:91-160) is behaviour: the native
# forward runs in inference mode when nothing requires a gradient; gradients are computed at loss_scale and divided
# afterwards; the first-order backward pass is itself differentiable with respect to dL_doutput, input and params (second-order
# INPUT gradients: eikonal / SDF losses); nothing is propagated through dL_dparams.  The construction is this package's own:
# one record per call, two Functions that only shuttle tensors in and out of it.  The native second-order pass exists for the
# grid, PPNG3, Identity, Frequency, TriangleWave, SphericalHarmonics and Empty encodings, for a Composite of those (Concatenation,
# Sum or Product) and for CutlassMLP networks, alone or behind one of those encodings; FullyFusedMLP, OneBlob, PPNG1 / PPNG2 and a
# Composite that holds one of them (OneBlobFrequency / NRC) raise the reference's "not implemented error" (for a network: ask for
# "otype": "CutlassMLP").
# ----------------------------------------------------------------------------------------------------------------------
class _Call:
    """What one forward call leaves behind for its backward passes."""

    __slots__ = ("native", "native_ctx", "loss_scale", "wants_input", "wants_params", "max_level")

    def __init__(self, native, loss_scale, wants_input, wants_params, max_level=None):
        self.native = native
        self.native_ctx = None
        self.loss_scale = loss_scale
        self.wants_input = wants_input
        self.wants_params = wants_params
        self.max_level = max_level  # None, or the max_level setting of the forward pass: (value, per-sample array padded to the batch or None)

    @contextlib.contextmanager
    def setting(self):
        """The call's max_level in force on the native module (its backward passes belong to the forward pass's setting); the one
        in force before comes back afterwards."""
        if self.max_level is None:
            yield
            return
        native = self.native
        previous = (native.max_level(), native.max_level_gpu())
        native.set_max_level(self.max_level[0])
        native.set_max_level_gpu(self.max_level[1])
        try:
            yield
        finally:
            native.set_max_level(previous[0])
            native.set_max_level_gpu(previous[1])

    def flagged(self, input, params, wants_input=None, wants_params=None):
        """The native entry points key on requires_grad (bindings.cpp:85, 126-131): aliases that carry exactly the flags of this call."""
        wi = self.wants_input if wants_input is None else wants_input
        wp = self.wants_params if wants_params is None else wants_params
        return input.detach().requires_grad_(wi), params.detach().requires_grad_(wp)

    def first_order(self, input, params, output, doutput):
        """(dL/dinput, dL/dparams) for an upstream gradient doutput; None where the call did not ask for one."""
        inp, par = self.flagged(input, params)
        with self.setting():
            gi, gp = self.native.bwd(self.native_ctx, inp, par, output, (doutput * self.loss_scale).contiguous())
        inv = 1.0 / self.loss_scale
        return (None if gi is None else gi * inv), (None if gp is None else gp * inv)

    def second_order(self, input, params, doutput, d_input_grad, wants_doutput, wants_input, wants_params):
        """Gradients of <d_input_grad, dL/dinput> with respect to (doutput, input, params).  dL/dinput is linear in doutput: the
        term for doutput carries no loss scale, the other two were computed at loss_scale."""
        inp, par = self.flagged(input, params, wants_input, wants_params)
        scaled = (doutput.detach() * self.loss_scale).contiguous().requires_grad_(wants_doutput)
        with self.setting():
            g_doutput, g_params, g_input = self.native.bwd_bwd_input(self.native_ctx, inp, par, d_input_grad.contiguous().float(), scaled)
        inv = 1.0 / self.loss_scale
        return g_doutput, (None if g_input is None else g_input * inv), (None if g_params is None else g_params * inv)


class _Evaluate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, params, native, loss_scale, *max_level):
        # (max_level: optional, the setting recorded by Module._max_level_of_call)
        call = _Call(native, loss_scale, ctx.needs_input_grad[0], ctx.needs_input_grad[1], max_level[0] if max_level else None)
        ctx.n_inputs = 4 + len(max_level)
        inp, par = call.flagged(input, params)
        with call.setting():
            call.native_ctx, output = native.fwd(inp, par)  # no flag set: inference mode, no context
        ctx.call = call
        ctx.save_for_backward(input, params, output)
        ctx.set_materialize_grads(False)
        return output

    @staticmethod
    def backward(ctx, doutput):
        if doutput is None:
            return (None,) * ctx.n_inputs
        if not doutput.is_cuda:
            warnings.warn("doutput must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
            doutput = doutput.cuda()
        input, params, output = ctx.saved_tensors
        g_input, g_params = _Differentiate.apply(doutput, input, params, output, ctx.call)
        return (g_input, g_params) + (None,) * (ctx.n_inputs - 2)


class _Differentiate(torch.autograd.Function):
    """The first-order backward pass as a differentiable function of (doutput, input, params)."""

    @staticmethod
    def forward(ctx, doutput, input, params, output, call):
        ctx.call = call
        ctx.save_for_backward(doutput, input, params)
        ctx.set_materialize_grads(False)
        with torch.no_grad():
            g_input, g_params = call.first_order(input, params, output, doutput)
        if g_params is not None:
            ctx.mark_non_differentiable(g_params)  # like the reference: nothing flows back from dL_dparams
        return g_input, g_params

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_input_grad, _d_params_grad):
        if d_input_grad is None:
            return None, None, None, None, None
        doutput, input, params = ctx.saved_tensors
        wants_doutput, wants_input, wants_params = ctx.needs_input_grad[:3]
        g_doutput, g_input, g_params = ctx.call.second_order(input, params, doutput, d_input_grad, wants_doutput, wants_input, wants_params)
        return g_doutput, g_input, g_params, None, None


class _InputJvp(torch.autograd.Function):
    """input_jvp attached to autograd with respect to (input, params, tangents): first order only."""

    @staticmethod
    def forward(ctx, input, params, tangents, native, loss_scale, want_output, max_level):
        call = _Call(native, loss_scale, ctx.needs_input_grad[0], ctx.needs_input_grad[1], max_level)
        ctx.wants_tangents = ctx.needs_input_grad[2]
        with call.setting():
            call.native_ctx, jvp, output = native.input_jvp_fwd(input.detach(), params.detach(), tangents.detach(), want_output)
        ctx.call = call
        ctx.save_for_backward(input, params, tangents)
        ctx.set_materialize_grads(False)
        if not want_output:
            output = jvp.new_empty(0)
            ctx.mark_non_differentiable(output)
        return jvp, output

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_jvp, d_output):
        if d_jvp is None and d_output is None:
            return (None,) * 7
        input, params, tangents = ctx.saved_tensors
        call = ctx.call
        native = call.native
        dtype = _torch_precision(native.output_precision())
        n, n_tangents = tangents.shape[0], tangents.shape[1]
        if d_jvp is None:
            # only the output entered the loss: the plain forward and first-order backward pass, no pass per tangent
            g_input = g_params = None
            if call.wants_input or call.wants_params:
                inp, par = call.flagged(input, params)
                with call.setting():
                    plain_ctx, output = native.fwd(inp, par)
                    g_input, g_params = native.bwd(plain_ctx, inp, par, output, (d_output * call.loss_scale).to(dtype).contiguous())
            inv = 1.0 / call.loss_scale
            return (None if g_input is None else g_input * inv, None if g_params is None else g_params * inv,
                    torch.zeros_like(tangents) if ctx.wants_tangents else None, None, None, None, None)
        # (cotangents at loss_scale in the output precision, the gradients divided by it again: as _Call.first_order)
        d_jvp = (d_jvp * call.loss_scale).to(dtype).contiguous()
        if d_output is not None:
            d_output = (d_output * call.loss_scale).to(dtype).contiguous()
        with call.setting():
            g_params, g_input, g_tangents = native.input_jvp_bwd(call.native_ctx, input.detach(), params.detach(), tangents.detach(), d_jvp, d_output,
                                                                call.wants_params, call.wants_input, ctx.wants_tangents)
        inv = 1.0 / call.loss_scale
        return (None if g_input is None else g_input * inv, None if g_params is None else g_params * inv, None if g_tangents is None else g_tangents * inv, None, None, None, None)


def _pad_rows(x, multiple):
    """x with its row count rounded up to a multiple (zero rows appended); the batch granularity of the kernels (common.h:235)"""
    n = x.shape[0]
    padded = -(-n // multiple) * multiple
    if padded == n:
        return x
    buf = x.new_zeros((padded,) + tuple(x.shape[1:]))
    buf[:n] = x
    return buf


class _WorkingCopy(torch.autograd.Function):
    """The parameters in the module's working precision.  By default this is a cast on every call, like the reference binding
    (modules.py:205 there: `self.params.to(_torch_precision(...))`).  The cast is the only per-call cost that grows with the model
    (67 MB read + 22 MB written for the C3a grid), so a module can be told to keep the copy between calls
    (`module.reuse_working_copy = True`): it is then rebuilt when the fp32 master's version counter or address changes -- optimizer
    steps, `load_state_dict`, `copy_` on the parameter, a replaced `.data`.  Writes THROUGH `.data` (`p.data.copy_(ema)`, as
    torch_ema's copy_to / restore do, `p.data.clamp_()`) change neither: after such a write call `invalidate_working_copy()`, or
    leave the reuse off.  `tcnn.optimizers.Optimizer` turns the reuse on for its modules and installs the half weights its step wrote as the
    copy (same key), so that no cast runs at all.  The gradient goes back as a plain cast to fp32."""

    @staticmethod
    def forward(ctx, params, owner):
        if not owner.reuse_working_copy:
            return params.detach().to(owner.dtype).contiguous()
        key = (params._version, params.data_ptr(), params.device)
        if owner._working_key != key:
            owner._working_copy = params.detach().to(owner.dtype).contiguous()
            owner._working_key = key
        return owner._working_copy.detach()  # a fresh alias per call: each call's graph node owns its own tensor object

    @staticmethod
    def backward(ctx, grad):
        return grad.to(torch.float32), None


class Module(torch.nn.Module):
    """Base of `Network`, `Encoding`, `NetworkWithInputEncoding` (reference: modules.py:162-217): an fp32 `params` Parameter
    initialised by the native module from `seed`, `forward(x)` for [n, n_input_dims] -> [n, n_output_dims] with any n."""

    def __init__(self, seed=1337):
        super().__init__()
        _require_gpu()
        self.seed = seed
        self._attach_native()
        self.params = torch.nn.Parameter(self.native_tcnn_module.initial_params(seed), requires_grad=True)

    def _attach_native(self):
        """(re)creates everything that is derived from the configuration alone: the native handle and what it reports"""
        self.native_tcnn_module = self._native_tcnn_module()
        precision = self.native_tcnn_module.param_precision()
        self.dtype = _torch_precision(precision)
        self.loss_scale = _C.default_loss_scale(precision)
        self._working_copy, self._working_key = None, None
        if not hasattr(self, "reuse_working_copy"):
            self.reuse_working_copy = False  # opt-in (see _WorkingCopy): the default casts on every call like the reference

    def invalidate_working_copy(self):
        """Forget the kept half-precision copy of the parameters (needed after writes through `params.data` when
        `reuse_working_copy` is on: those do not show in the parameter's version counter)."""
        self._working_copy, self._working_key = None, None

    def forward(self, x):
        if not x.is_cuda:
            warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
            x = x.cuda()
        n = x.shape[0]
        rows = _pad_rows(x.to(torch.float), _C.batch_size_granularity()).contiguous()
        if self.params.dtype == self.dtype:
            working = self.params.contiguous()
        else:
            working = _WorkingCopy.apply(self.params, self)
        output = _Evaluate.apply(rows, working, self.native_tcnn_module, self.loss_scale, self._max_level_of_call(n, rows))
        return output[:n, : self.n_output_dims]

    def input_gradient(self, x, dim=0, backprop_scale=None, return_output=False):
        """d output[dim] / d x at inference (the reference's DifferentiableObject::input_gradient, object.h:342-366): float32
        [n, n_input_dims] for any n, computed outside autograd on the module's current parameters -- nothing requires or receives a
        gradient.  dim counts the native (padded) output columns; backprop_scale (default: the module's loss scale) is the magnitude
        the one-hot is seeded with and divided out again.  return_output=True: (gradient, output[:n, :n_output_dims]) of the same pass."""
        with torch.no_grad():
            x = x.detach()
            if not x.is_cuda:
                warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
                x = x.cuda()
            n = x.shape[0]
            rows = _pad_rows(x.to(torch.float), _C.batch_size_granularity()).contiguous()
            working = self.params.detach().to(self.dtype).contiguous()
            scale = self.loss_scale if backprop_scale is None else backprop_scale
            native = self.native_tcnn_module
            call = _Call(native, scale, False, False, self._max_level_of_call(n, rows))
            with call.setting():
                gradient, output = native.input_gradient(rows, working, dim, scale, return_output)
            gradient = gradient[:n]
            return (gradient, output[:n, : self.n_output_dims]) if return_output else gradient

    def input_jacobian(self, x, dims=None, backprop_scale=None, return_output=False):
        """input_gradient for several output columns from ONE forward pass: float32 [n, len(dims), n_input_dims] for any n, where
        [:, k, :] is bit for bit input_gradient(x, dims[k], backprop_scale).  dims (default: range(n_output_dims)) count the native
        (padded) output columns, in any order, repeats allowed.  Outside autograd and under the max_level setting in force, as
        input_gradient.  return_output=True: (jacobian, output[:n, :n_output_dims]) of the same pass."""
        with torch.no_grad():
            x = x.detach()
            if not x.is_cuda:
                warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
                x = x.cuda()
            n = x.shape[0]
            rows = _pad_rows(x.to(torch.float), _C.batch_size_granularity()).contiguous()
            working = self.params.detach().to(self.dtype).contiguous()
            scale = self.loss_scale if backprop_scale is None else backprop_scale
            native = self.native_tcnn_module
            call = _Call(native, scale, False, False, self._max_level_of_call(n, rows))
            with call.setting():
                jacobian, output = native.input_jacobian(rows, working, range(self.n_output_dims) if dims is None else dims, scale, return_output)
            jacobian = jacobian[:n]
            return (jacobian, output[:n, : self.n_output_dims]) if return_output else jacobian

    def input_jvp(self, x, tangents, return_output=False, differentiable=False):
        """Forward mode: every output's derivative along given input directions, for any n.  tangents [n, T, n_input_dims] gives
        [n, T, n_output_dims] in the module's output precision with [:, t, :] = J(x) tangents[:, t, :]; a 2-D tangents [n, n_input_dims]
        means T = 1 and gives [n, n_output_dims].  Outside autograd (not differentiable) and under the max_level setting in force, as
        input_gradient.  There is no backprop_scale: the map is linear in the tangent, so scale the tangent if half precision might
        overflow.  return_output=True: (jvp, output[:n, :n_output_dims]) of the same pass.
        differentiable=True: the same values, attached to autograd with respect to `params`, x and tangents, whichever require grad --
        J v in a loss (first order only: a second backward through the graph raises).  Cotangents are multiplied by the module's
        loss_scale and the gradients divided by it again, as forward() does."""
        if differentiable:
            return self._input_jvp_differentiable(x, tangents, return_output)
        with torch.no_grad():
            x = x.detach()
            if not x.is_cuda:
                warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
                x = x.cuda()
            n = x.shape[0]
            v = tangents.detach().to(device=x.device, dtype=torch.float)
            flat = v.dim() == 2
            if flat:
                v = v[:, None, :]
            if v.dim() != 3 or v.shape[0] != n or v.shape[1] < 1 or v.shape[2] != self.n_input_dims:
                raise ValueError("input_jvp: tangents must be [n, T, n_input_dims] or [n, n_input_dims] with T >= 1, got %s" % (tuple(tangents.shape),))
            granularity = _C.batch_size_granularity()
            rows = _pad_rows(x.to(torch.float), granularity).contiguous()
            v = _pad_rows(v.reshape(n, -1), granularity).reshape(rows.shape[0], -1, self.n_input_dims).contiguous()
            working = self.params.detach().to(self.dtype).contiguous()
            native = self.native_tcnn_module
            call = _Call(native, self.loss_scale, False, False, self._max_level_of_call(n, rows))
            with call.setting():
                jvp, output = native.input_jvp(rows, working, v, return_output)
            jvp = jvp[:n, :, : self.n_output_dims]
            if flat:
                jvp = jvp[:, 0]
            return (jvp, output[:n, : self.n_output_dims]) if return_output else jvp

    def _input_jvp_differentiable(self, x, tangents, return_output):
        if not x.is_cuda:
            warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
            x = x.cuda()
        n = x.shape[0]
        v = tangents.to(device=x.device, dtype=torch.float)
        flat = v.dim() == 2
        if flat:
            v = v[:, None, :]
        if v.dim() != 3 or v.shape[0] != n or v.shape[1] < 1 or v.shape[2] != self.n_input_dims:
            raise ValueError("input_jvp: tangents must be [n, T, n_input_dims] or [n, n_input_dims] with T >= 1, got %s" % (tuple(tangents.shape),))
        granularity = _C.batch_size_granularity()
        rows = _pad_rows(x.to(torch.float), granularity).contiguous()
        v = _pad_rows(v.reshape(n, -1), granularity).reshape(rows.shape[0], -1, self.n_input_dims).contiguous()
        if self.params.dtype == self.dtype:
            working = self.params.contiguous()
        else:
            working = _WorkingCopy.apply(self.params, self)
        jvp, output = _InputJvp.apply(rows, working, v, self.native_tcnn_module, self.loss_scale, return_output, self._max_level_of_call(n, rows))
        jvp = jvp[:n, :, : self.n_output_dims]  # (padded rows and output columns receive zero cotangent through the slices)
        if flat:
            jvp = jvp[:, 0]
        return (jvp, output[:n, : self.n_output_dims]) if return_output else jvp

    # --- max_level of the grid encoding(s) (the reference's GridEncoding::set_max_level / set_max_level_gpu, grid_interface.h:101-123).
    # Every forward call records the setting in force; its backward and double-backward passes run under that setting.
    def set_max_level(self, value):
        """A fraction of the grid levels: `value * n_levels` levels produce output (1000, the default: every level)."""
        self.native_tcnn_module.set_max_level(value)
        self._max_level_value = float(value)

    @property
    def max_level(self):
        return self.native_tcnn_module.max_level()

    def set_max_level_gpu(self, per_sample):
        """One max_level per row (instant-ngp's random max level): a contiguous float32 tensor on the module's device with at
        least as many values as the rows of every later call (the module keeps a reference), or None to go back to the scalar."""
        if per_sample is not None:
            if not isinstance(per_sample, torch.Tensor) or per_sample.dtype != torch.float32 or not per_sample.is_contiguous() or per_sample.dim() != 1:
                raise RuntimeError("tcnn: the per-sample max_level must be a contiguous one-dimensional float32 tensor")
            if per_sample.device != self.params.device:
                raise RuntimeError(f"tcnn: the per-sample max_level lives on {per_sample.device}, the module on {self.params.device}")
        self.native_tcnn_module.set_max_level_gpu(per_sample)
        self._max_level_tensor = per_sample

    @property
    def max_level_gpu(self):
        return getattr(self, "_max_level_tensor", None)

    def _max_level_of_call(self, n, rows):
        """None while max_level was never set on this module, else (value, per-sample array padded to the rows of this call)"""
        value, per_sample = getattr(self, "_max_level_value", None), getattr(self, "_max_level_tensor", None)
        if value is None and per_sample is None:
            return None
        if value is None:
            value = 1000.0
        if per_sample is not None:
            if per_sample.numel() < n:
                raise RuntimeError(f"tcnn: the per-sample max_level holds {per_sample.numel()} values for a batch of {n} rows")
            if per_sample.device != rows.device:
                raise RuntimeError(f"tcnn: the per-sample max_level lives on {per_sample.device}, the input on {rows.device}")
            per_sample = per_sample[:n] if rows.shape[0] == n else _pad_rows(per_sample[:n], rows.shape[0])  # the kernels read one value per padded row
        return (value, per_sample)

    # native handles do not pickle: drop them, and rebuild them from the configuration on the other side
    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in ("native_tcnn_module", "_working_copy", "_working_key", "_max_level_value", "_max_level_tensor")}

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._attach_native()

    def extra_repr(self):
        return (f"n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, seed={self.seed}, dtype={self.dtype}, "
                f"hyperparams={self.native_tcnn_module.hyperparams()}")


_PRECISIONS = {None: None, torch.float32: _C.Precision.Fp32, torch.float16: _C.Precision.Fp16}


def _network_precision(what, dtype):
    """The precision of a module with a network: half unless dtype says torch.float32 (None: half, whatever the preferred precision)."""
    if dtype not in _PRECISIONS:
        raise ValueError(f"{what} only supports fp32 or fp16 precision, but got {dtype}")
    return _C.Precision.Fp16 if dtype is None else _PRECISIONS[dtype]


def _needs_networks(what):
    if not _C.has_networks():
        raise RuntimeError(f"Cannot create `{what}` because tiny-cuda-nn was not compiled with neural network support.")


class NetworkWithInputEncoding(Module):
    """Input encoding followed by a neural network: [:, n_input_dims] float -> [:, n_output_dims] in `dtype` (None: half).
    Arguments as in the reference (modules.py:219-260): dimensions, the `encoding` and `network` configuration dicts, seed.
    dtype=torch.float32 is the reference's full-precision build as a choice per module: the encoding's fp32 form in front of a
    CutlassMLP that computes in fp32 throughout -- no working copy of the parameters, no cast, loss scale 1, float32 output
    (`"otype": "FullyFusedMLP"` is refused as in that build).  Train such a module with torch.optim."""

    def __init__(self, n_input_dims, n_output_dims, encoding_config, network_config, seed=1337, dtype=None):
        _needs_networks("NetworkWithInputEncoding")
        self.precision = _network_precision("NetworkWithInputEncoding", dtype)
        self.n_input_dims, self.n_output_dims = n_input_dims, n_output_dims
        self.encoding_config, self.network_config = encoding_config, network_config
        super().__init__(seed=seed)

    def _native_tcnn_module(self):
        # (a module pickled before `dtype` existed carries no precision: half)
        return _create(_C.lib.tcnn_create_network_with_input_encoding_precision, self.n_input_dims, self.n_output_dims,
                       _C.to_json_bytes(self.encoding_config), _C.to_json_bytes(self.network_config), getattr(self, "precision", _C.Precision.Fp16))


class Network(Module):
    """Neural network on raw inputs (an Identity encoding inside, cpp_api.cu:151-153); arguments as modules.py:262-292, and
    `dtype` as for NetworkWithInputEncoding (None: half; torch.float32: a CutlassMLP in full precision)."""

    def __init__(self, n_input_dims, n_output_dims, network_config, seed=1337, dtype=None):
        _needs_networks("Network")
        self.precision = _network_precision("Network", dtype)
        self.n_input_dims, self.n_output_dims = n_input_dims, n_output_dims
        self.network_config = network_config
        super().__init__(seed=seed)

    def _native_tcnn_module(self):
        return _create(_C.lib.tcnn_create_network_precision, self.n_input_dims, self.n_output_dims, _C.to_json_bytes(self.network_config),
                       getattr(self, "precision", _C.Precision.Fp16))


class Encoding(Module):
    """Input encoding: [:, n_input_dims] float -> [:, n_output_dims] in `dtype` (default: the preferred precision, half);
    arguments as modules.py:294-329.  n_output_dims is what the native encoding reports."""

    _PRECISIONS = _PRECISIONS

    def __init__(self, n_input_dims, encoding_config, seed=1337, dtype=None):
        if dtype not in self._PRECISIONS:
            raise ValueError(f"Encoding only supports fp32 or fp16 precision, but got {dtype}")
        self.n_input_dims = n_input_dims
        self.encoding_config = encoding_config
        self.precision = _C.preferred_precision() if dtype is None else self._PRECISIONS[dtype]
        super().__init__(seed=seed)

    def _attach_native(self):
        super()._attach_native()
        self.n_output_dims = self.native_tcnn_module.n_output_dims()

    def _native_tcnn_module(self):
        return _create(_C.lib.tcnn_create_encoding, self.n_input_dims, _C.to_json_bytes(self.encoding_config), self.precision)
