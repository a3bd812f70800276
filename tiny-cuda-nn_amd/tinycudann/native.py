"""Python view of the C++ user API (boundary A): create_from_config / Trainer / training_step / inference.

The reference exposes this API to C++ callers only (include/tiny-cuda-nn/config.h:46-63, trainer.h:48-363; used by
samples/mlp_learning_an_image.cu:252-300 and benchmarks/image/bench_ours.cu:188-331).  bench.py and the parity tests
drive the very same entry points through the C ABI with torch tensors as device buffers.
"""
import ctypes as C
import json

import torch

from . import _C

LAYOUT_SOA, LAYOUT_AOS = 0, 1
GRADIENT_IGNORE, GRADIENT_OVERWRITE, GRADIENT_ACCUMULATE = 0, 1, 2


_PRECISIONS = {None: _C.Precision.Fp16, torch.float16: _C.Precision.Fp16, torch.float32: _C.Precision.Fp32}


def _trainer_precision(dtype):
    """The precision of a trainer: half unless dtype says torch.float32 (checked before the GPU is asked for)."""
    if dtype not in _PRECISIONS:
        raise ValueError(f"Trainer only supports fp32 or fp16 precision, but got {dtype}")
    return _PRECISIONS[dtype]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(stream=None):
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream


class ForwardContext:
    """Trainer::ForwardContext (trainer.h:89-95)."""

    def __init__(self, handle, n, padded_out, dtype=torch.half):
        self._h = handle
        self.n = n
        self.padded_out = padded_out
        self.dtype = dtype  # of output and dL_doutput: the trainer's

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _C is not None and getattr(_C, 'lib', None) is not None:  # modules may already be torn down at exit
            _C.lib.tcnn_train_ctx_destroy(h)

    def _view(self, accessor, dtype, itemsize):
        # copy the device buffer into a fresh torch tensor (the context owns the original).  The fused step's context pads dL_doutput / L
        # inside the accessor, on the step's stream: synchronise after the call, not before.
        ptr = accessor(self._h)
        if not ptr:
            raise RuntimeError(_C.lib.tcnn_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        out = torch.empty((self.n, self.padded_out), dtype=dtype, device="cuda")
        _C.memcpy_dtod(out.data_ptr(), ptr, self.n * self.padded_out * itemsize)
        return out

    def output(self):
        return self._view(_C.lib.tcnn_train_ctx_output, self.dtype, self.dtype.itemsize)

    def dL_doutput(self):
        return self._view(_C.lib.tcnn_train_ctx_dL_doutput, self.dtype, self.dtype.itemsize)

    def L(self):
        return self._view(_C.lib.tcnn_train_ctx_L, torch.float32, 4)


class Trainer:
    """tcnn::Trainer<float, half, half> + the NetworkWithInputEncoding it drives.  dtype=torch.float32: Trainer<float, float, float> --
    the fp32 module, one float parameter vector, float output / dL_doutput / gradients, loss scale 1, every step unfused."""

    def __init__(self, n_input_dims, n_output_dims, config, seed=1337, dtype=None):
        precision = _trainer_precision(dtype)
        if not torch.cuda.is_available():
            raise EnvironmentError("tcnn_amd needs a ROCm GPU (gfx950): torch.cuda.is_available() is False.")
        torch.cuda.init()
        h = C.c_void_p()
        _C.check(_C.lib.tcnn_create_from_config_precision(n_input_dims, n_output_dims, _C.to_json_bytes(config), seed, precision, C.byref(h)))
        self._h = h
        self.dtype = torch.float32 if precision == _C.Precision.Fp32 else torch.half
        self.default_loss_scale = _C.default_loss_scale(precision)
        self.n_input_dims = n_input_dims
        self.n_output_dims = n_output_dims
        self.padded_output_width = int(_C.lib.tcnn_trainer_padded_output_width(h))
        self._max_level_gpu = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _C is not None and getattr(_C, 'lib', None) is not None:  # modules may already be torn down at exit
            _C.lib.tcnn_trainer_destroy(h)

    # -- trainer.h:163-190
    def training_step(self, input, target, data_pdf=None, run_optimizer=True, dL_dinput=None, use_inference_params=False,
                      gradient_mode=GRADIENT_OVERWRITE, external_dL_dy=None, input_layout=LAYOUT_AOS, stream=None):
        n = input.shape[0] if input_layout == LAYOUT_AOS else input.shape[1]
        self._check_max_level_rows(n)
        ctx = C.c_void_p()
        _C.check(_C.lib.tcnn_trainer_training_step(self._h, _stream(stream), n, _ptr(input), input_layout, _ptr(target), _ptr(data_pdf),
                                                   int(run_optimizer), _ptr(dL_dinput), int(use_inference_params), gradient_mode,
                                                   _ptr(self._checked_dy(external_dL_dy)), C.byref(ctx)))
        return ForwardContext(ctx, n, self.padded_output_width, self.dtype)

    def _checked_dy(self, external_dL_dy):
        # (an fp32 trainer reads floats; what a half trainer is given passes through as it always did)
        if external_dL_dy is not None and self.dtype == torch.float32 and external_dL_dy.dtype != torch.float32:
            raise TypeError(f"tcnn: external_dL_dy must be {self.dtype}, the trainer's precision, not {external_dL_dy.dtype}")
        return external_dL_dy

    # -- measurement hook (include/tcnn_amd.h): HIP events around the pieces of the next fused training step
    PROFILE_PIECES = ("encode", "mlp_kernel", "encoding_backward", "optimizer")

    def profile_next_step(self):
        _C.check(_C.lib.tcnn_trainer_profile_next_step(self._h))

    def params_updated_in_flush(self):
        """parameters whose optimizer update the last training_step applied inside the reduction of the weight gradients: all of them, or 0 (tcnn_amd.h)"""
        return int(_C.lib.tcnn_trainer_params_updated_in_flush(self._h))

    def image_preps(self):
        """launches of the weight-rearranging kernel by this trainer's training steps so far (tcnn_amd.h: tcnn_trainer_image_preps)"""
        return int(_C.lib.tcnn_trainer_image_preps(self._h))

    def optimizer_prologue_steps(self):
        """training steps whose optimizer launch also finished the backward pass's gradients (tcnn_amd.h: tcnn_trainer_optimizer_prologue_steps)"""
        return int(_C.lib.tcnn_trainer_optimizer_prologue_steps(self._h))

    def list_scatters(self):
        """backward passes of the grid encoding that ran the list-fed gradient kernel (tcnn_amd.h: tcnn_trainer_list_scatters)"""
        return int(_C.lib.tcnn_trainer_list_scatters(self._h))

    def list_gradient_tails(self):
        """training steps whose MLP kernel stored dL/dy in the order of the grid's hit lists itself, so that no k_grid_list_gradients
        launch ran (tcnn_amd.h: tcnn_trainer_list_gradient_tails)"""
        return int(_C.lib.tcnn_trainer_list_gradient_tails(self._h))

    def last_step_kernel(self):
        """short name of the MLP training kernel the last training_step launched, e.g. "r32", "regs", "train<64,1,8,8>/act" or "unfused"
        (tcnn_amd.h: tcnn_trainer_last_step_kernel)"""
        return _C.lib.tcnn_trainer_last_step_kernel(self._h).decode()

    def context_keeps_slabs(self, ctx):
        """whether `ctx` owns the weight-gradient slabs the optimizer's launch reduces (tcnn_amd.h: tcnn_train_ctx_keeps_weight_gradient_slabs)"""
        return bool(_C.lib.tcnn_train_ctx_keeps_weight_gradient_slabs(self._h, ctx._h))

    def scatter_wide_fallbacks(self):
        """tasks of the grid gradient kernel that could not prove their packed 32-bit sums and ran the 64-bit passes (tcnn_amd.h)"""
        return int(_C.lib.tcnn_trainer_scatter_wide_fallbacks(self._h))

    def profile_collect(self, stream=None):
        """-> ({piece: mean milliseconds per profiled step}, number of profiled steps)"""
        ms = (C.c_float * 4)()
        n = C.c_uint32()
        _C.check(_C.lib.tcnn_trainer_profile_collect(self._h, _stream(stream), ms, C.byref(n)))
        k = max(n.value, 1)
        return {name: ms[i] / k for i, name in enumerate(self.PROFILE_PIECES)}, n.value

    # -- trainer.h:205-207
    def loss(self, ctx, stream=None):
        out = C.c_float()
        _C.check(_C.lib.tcnn_trainer_loss(self._h, _stream(stream), ctx._h, C.byref(out)))
        return out.value

    def forward(self, input, target, loss_scale=None, data_pdf=None, prepare_input_gradients=False, external_dL_dy=None, input_layout=LAYOUT_AOS, stream=None):
        n = input.shape[0] if input_layout == LAYOUT_AOS else input.shape[1]
        self._check_max_level_rows(n)
        ctx = C.c_void_p()
        loss_scale = self.default_loss_scale if loss_scale is None else loss_scale  # (128 for half, 1 for an fp32 trainer)
        _C.check(_C.lib.tcnn_trainer_forward(self._h, _stream(stream), loss_scale, n, _ptr(input), input_layout, _ptr(target), _ptr(data_pdf), 0,
                                             int(prepare_input_gradients), _ptr(self._checked_dy(external_dL_dy)), C.byref(ctx)))
        return ForwardContext(ctx, n, self.padded_output_width, self.dtype)

    def backward(self, ctx, input, dL_dinput=None, gradient_mode=GRADIENT_OVERWRITE, input_layout=LAYOUT_AOS, stream=None):
        self._check_max_level_rows(ctx.n)
        _C.check(_C.lib.tcnn_trainer_backward(self._h, _stream(stream), ctx._h, ctx.n, _ptr(input), input_layout, _ptr(dL_dinput), 0, gradient_mode))

    def optimizer_step(self, loss_scale=None, stream=None):
        loss_scale = self.default_loss_scale if loss_scale is None else loss_scale
        _C.check(_C.lib.tcnn_trainer_optimizer_step(self._h, _stream(stream), loss_scale))

    # -- object.h:147-176: network->inference(stream, input, output)
    def inference(self, input, output=None, input_layout=LAYOUT_AOS, output_layout=LAYOUT_AOS, stream=None):
        n = input.shape[0] if input_layout == LAYOUT_AOS else input.shape[1]
        if output is None:
            shape = (n, self.n_output_dims) if output_layout == LAYOUT_AOS else (self.n_output_dims, n)
            output = torch.empty(shape, dtype=torch.float32, device=input.device)
        self._check_max_level_rows(n)
        _C.check(_C.lib.tcnn_trainer_inference(self._h, _stream(stream), n, _ptr(input), input_layout, _ptr(output), output_layout, 1))
        return output

    # -- object.h:342-366: network->input_gradient(stream, dim, input, d_dinput, backprop_scale) on the inference parameters
    def input_gradient(self, input, dim=0, backprop_scale=None, d_dinput=None, stream=None):
        """d output[dim] / d input, float32 [n, n_input_dims] (AoS, n a multiple of the batch granularity); dim counts padded columns"""
        n = input.shape[0]
        if d_dinput is None:
            d_dinput = torch.empty((n, input.shape[1]), dtype=torch.float32, device=input.device)
        assert input.dtype == torch.float32 and input.is_contiguous() and d_dinput.dtype == torch.float32 and d_dinput.is_contiguous() and d_dinput.shape == input.shape
        self._check_max_level_rows(n)
        scale = self.default_loss_scale if backprop_scale is None else backprop_scale
        _C.check(_C.lib.tcnn_trainer_input_gradient(self._h, _stream(stream), n, int(dim), _ptr(input), _ptr(d_dinput), float(scale)))
        return d_dinput

    def input_jacobian(self, input, dims, backprop_scale=None, jacobian=None, stream=None):
        """d output[dims[k]] / d input for every k from one forward pass, float32 [n, len(dims), n_input_dims]; [:, k, :] is bit for bit
        input_gradient(input, dims[k], backprop_scale).  dims count padded columns."""
        n = input.shape[0]
        dims = [int(d) for d in dims]
        shape = (n, len(dims), input.shape[1])
        if jacobian is None:
            jacobian = torch.empty(shape, dtype=torch.float32, device=input.device)
        assert input.dtype == torch.float32 and input.is_contiguous() and jacobian.dtype == torch.float32 and jacobian.is_contiguous() and tuple(jacobian.shape) == shape
        self._check_max_level_rows(n)
        scale = self.default_loss_scale if backprop_scale is None else backprop_scale
        _C.check(_C.lib.tcnn_trainer_input_jacobian(self._h, _stream(stream), n, (C.c_uint32 * len(dims))(*dims), len(dims), _ptr(input), _ptr(jacobian), float(scale)))
        return jacobian

    def input_jvp(self, input, tangents, jvp=None, stream=None):
        """J(x) tangents[:, t, :] for every t on the trainer's inference parameters: [n, T, padded output width] in the trainer's precision,
        from float32 tangents [n, T, n_input_dims].  No backprop_scale: the map is linear in the tangent."""
        n, n_tangents = input.shape[0], tangents.shape[1]
        shape = (n, n_tangents, self.padded_output_width)
        if jvp is None:
            jvp = torch.empty(shape, dtype=self.dtype, device=input.device)
        assert input.dtype == torch.float32 and input.is_contiguous() and tangents.dtype == torch.float32 and tangents.is_contiguous()
        assert tuple(tangents.shape) == (n, n_tangents, input.shape[1]) and jvp.dtype == self.dtype and jvp.is_contiguous() and tuple(jvp.shape) == shape
        self._check_max_level_rows(n)
        _C.check(_C.lib.tcnn_trainer_input_jvp(self._h, _stream(stream), n, n_tangents, _ptr(input), _ptr(tangents), _ptr(jvp)))
        return jvp

    def input_jvp_forward(self, input, tangents, want_output=False, stream=None):
        """input_jvp on the trainer's TRAINING parameters with a context for input_jvp_backward: (context, jvp, padded output or None)
        (tcnn_amd.h: tcnn_trainer_input_jvp_forward)"""
        from .modules import NativeContext

        n, n_tangents = input.shape[0], tangents.shape[1]
        assert input.dtype == torch.float32 and input.is_contiguous() and tangents.dtype == torch.float32 and tangents.is_contiguous()
        assert tuple(tangents.shape) == (n, n_tangents, input.shape[1])
        self._check_max_level_rows(n)
        jvp = torch.empty((n, n_tangents, self.padded_output_width), dtype=self.dtype, device=input.device)
        output = torch.empty((n, self.padded_output_width), dtype=self.dtype, device=input.device) if want_output else None
        h = C.c_void_p()
        _C.check(_C.lib.tcnn_trainer_input_jvp_forward(self._h, _stream(stream), n, n_tangents, _ptr(input), _ptr(tangents), _ptr(jvp), _ptr(output), C.byref(h)))
        return NativeContext(h), jvp, output

    def input_jvp_backward(self, ctx, input, tangents, dL_djvp, dL_doutput=None, want_input=True, want_tangents=True, gradient_mode=GRADIENT_OVERWRITE, stream=None):
        """The gradients of sum_t <dL_djvp[:, t], J v_t> + <dL_doutput, f(x)>: the parameters' into the trainer's gradient buffer under
        gradient_mode (optimizer_step reads it; no loss scale inside), and (dL_dinput, dL_dtangents), None where not wanted
        (tcnn_amd.h: tcnn_trainer_input_jvp_backward)"""
        n, n_tangents = input.shape[0], tangents.shape[1]
        assert dL_djvp.dtype == self.dtype and dL_djvp.is_contiguous() and tuple(dL_djvp.shape) == (n, n_tangents, self.padded_output_width)
        assert dL_doutput is None or (dL_doutput.dtype == self.dtype and dL_doutput.is_contiguous() and tuple(dL_doutput.shape) == (n, self.padded_output_width))
        self._check_max_level_rows(n)
        dL_dinput = torch.empty((n, input.shape[1]), dtype=torch.float32, device=input.device) if want_input else None
        dL_dtangents = torch.empty((n, n_tangents, input.shape[1]), dtype=torch.float32, device=input.device) if want_tangents else None
        _C.check(_C.lib.tcnn_trainer_input_jvp_backward(self._h, _stream(stream), ctx._h, n, n_tangents, _ptr(input), _ptr(tangents), _ptr(dL_djvp), _ptr(dL_doutput),
                                                        _ptr(dL_dinput), _ptr(dL_dtangents), gradient_mode))
        return dL_dinput, dL_dtangents

    # -- object.h:133-145: network->inference_mixed_precision(stream, input, output): half [n][padded_output_width]
    def inference_half(self, input, output=None, input_layout=LAYOUT_AOS, stream=None):
        if self.dtype != torch.half:
            raise TypeError("tcnn: inference_half is the half trainer's; an fp32 trainer's own output is what inference() returns")
        n = input.shape[0] if input_layout == LAYOUT_AOS else input.shape[1]
        if output is None:
            output = torch.empty((n, self.padded_output_width), dtype=torch.half, device=input.device)
        assert output.dtype == torch.half and output.is_contiguous() and output.shape == (n, self.padded_output_width)
        self._check_max_level_rows(n)
        _C.check(_C.lib.tcnn_trainer_inference_mixed_precision(self._h, _stream(stream), n, _ptr(input), input_layout, _ptr(output), 1))
        return output

    # -- max_level of the model's grid encoding(s) (GridEncoding::set_max_level / max_level / set_max_level_gpu, grid_interface.h:101-123):
    # read by every later training_step / forward / backward / inference call
    def set_max_level(self, value):
        """A fraction of the grid levels: `value * n_levels` levels produce output (1000, the default: every level)."""
        _C.check(_C.lib.tcnn_trainer_set_max_level(self._h, float(value)))

    @property
    def max_level(self):
        value = float(_C.lib.tcnn_trainer_max_level(self._h))
        if value != value and _C.lib.tcnn_last_error():  # NaN: an error, or a NaN that was set (tcnn_last_error() is empty then)
            raise RuntimeError(_C.lib.tcnn_last_error().decode("utf-8", "replace"))
        return value

    def set_max_level_gpu(self, per_sample):
        """One max_level per row: a contiguous float32 device tensor with at least as many values as the rows of every later call
        (the trainer keeps a reference), or None to go back to the scalar."""
        if per_sample is not None:
            if not isinstance(per_sample, torch.Tensor) or per_sample.dtype != torch.float32 or not per_sample.is_contiguous() or not per_sample.is_cuda:
                raise RuntimeError("tcnn: the per-sample max_level must be a contiguous float32 device tensor")
        _C.check(_C.lib.tcnn_trainer_set_max_level_gpu(self._h, _ptr(per_sample)))
        self._max_level_gpu = per_sample

    @property
    def max_level_gpu(self):
        return self._max_level_gpu

    def _check_max_level_rows(self, n):
        if self._max_level_gpu is not None and self._max_level_gpu.numel() < n:
            raise RuntimeError(f"tcnn: the per-sample max_level holds {self._max_level_gpu.numel()} values for a batch of {n} rows")

    @property
    def n_params(self):
        return int(_C.lib.tcnn_trainer_n_params(self._h))

    def _copy_out(self, ptr, dtype, itemsize):
        torch.cuda.synchronize()
        out = torch.empty(self.n_params, dtype=dtype, device="cuda")
        _C.memcpy_dtod(out.data_ptr(), ptr, self.n_params * itemsize)
        return out

    def params_full_precision(self):
        return self._copy_out(_C.lib.tcnn_trainer_params_full_precision(self._h), torch.float32, 4)

    def params(self):
        return self._copy_out(_C.lib.tcnn_trainer_params(self._h), self.dtype, self.dtype.itemsize)

    def params_inference(self):
        """trainer.h:234: the parameters inference runs with (the optimizer's EMA weights if it keeps any)."""
        return self._copy_out(_C.lib.tcnn_trainer_params_inference(self._h), self.dtype, self.dtype.itemsize)

    def param_gradients(self):
        return self._copy_out(_C.lib.tcnn_trainer_param_gradients(self._h), self.dtype, self.dtype.itemsize)

    def set_params_full_precision(self, params):
        params = params.contiguous().float()
        _C.check(_C.lib.tcnn_trainer_set_params_full_precision(self._h, _ptr(params), params.numel(), int(params.is_cuda)))

    def set_params(self, params_half):
        """params_half: in the trainer's dtype (half; float32 for an fp32 trainer)"""
        params_half = params_half.contiguous().to(self.dtype)
        _C.check(_C.lib.tcnn_trainer_set_params(self._h, _ptr(params_half), params_half.numel(), int(params_half.is_cuda)))

    def update_hyperparams(self, cfg):
        _C.check(_C.lib.tcnn_trainer_update_hyperparams(self._h, _C.to_json_bytes(cfg)))

    def hyperparams(self):
        return json.loads(_C.lib.tcnn_trainer_hyperparams(self._h).decode())

    def network_hyperparams(self):
        return json.loads(_C.lib.tcnn_trainer_network_hyperparams(self._h).decode())

    def optimizer_step_count(self):
        return int(_C.lib.tcnn_trainer_optimizer_step_count(self._h))

    def serialize(self, serialize_optimizer=False):
        """trainer.h:275-291 as MessagePack bytes (what json::to_msgpack(trainer->serialize()) yields in the reference's callers)."""
        ptr, size = _C.C.c_void_p(), _C.C.c_size_t()
        _C.check(_C.lib.tcnn_trainer_serialize(self._h, int(bool(serialize_optimizer)), _C.C.byref(ptr), _C.C.byref(size)))
        return _C.C.string_at(ptr, size.value)

    def deserialize(self, data):
        """trainer.h:293-315: MessagePack bytes of a snapshot object ("params_type" "__half" or "float")."""
        data = bytes(data)
        _C.check(_C.lib.tcnn_trainer_deserialize(self._h, data, len(data)))


class TrainableModel:
    """config.h:46-51: {loss, optimizer, network, trainer}; here network and trainer are the same native object."""

    def __init__(self, trainer):
        self.trainer = trainer
        self.network = trainer


def create_from_config(n_input_dims, n_output_dims, config, seed=1337, dtype=None):
    """tcnn::create_from_config (config.h:53-63); dtype=torch.float32: the fp32 trainer."""
    return TrainableModel(Trainer(n_input_dims, n_output_dims, config, seed, dtype))
