"""The library's losses for tensors that are the caller's: `tcnn.losses.Loss(config)`.

The losses a `tcnn.Trainer` evaluates -- L2, RelativeL2, RelativeL2Luminance, L1, RelativeL1, Mape, Smape, CrossEntropy, Variance
(losses/*.h of the reference, `data_pdf` included) -- for callers whose predictions are not a trainer's: a renderer between the network
and the loss, a PyTorch loop over the modules, or `Trainer.training_step(external_dL_dy=...)`:

    loss_fn = tcnn.losses.Loss("RelativeL2")
    loss = loss_fn(my_renderer(model(x)), target)      # 0-d fp32, the number trainer->loss() reports
    loss.backward()                                    # one launch: dL/dprediction, rounded once to the prediction's dtype

    loss, dL_dy = loss_fn.evaluate(ctx.output()[:, :3], target, loss_scale=128.0, out_gradient=dy_padded)   # no autograd, one pass
    trainer.training_step(x, target, external_dL_dy=dL_dy)

Every element goes through the device code the trainer's own loss kernels run (`tcnn_loss_evaluate`, include/tcnn_amd.h), so values and
gradients carry the trainer's bits; a restatement in torch ops differs in division order and in where the result is rounded to half, and
costs about ten element-wise launches plus autograd's backward.  The forward pass launches the sum only (no values matrix is stored), the
backward pass the gradient only, with autograd's incoming gradient read on the device and folded in before the one rounding.
Everything runs on the current stream and nothing synchronises.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _C

PRECISION = {torch.float32: _C.Precision.Fp32, torch.float16: _C.Precision.Fp16}


def loss_type(config):
    """The library's type number of a loss configuration: a dict with "otype", or the name (tcnn_loss_type; needs no device)."""
    if isinstance(config, str):
        config = {"otype": config}
    out = C.c_int()
    _C.check(_C.lib.tcnn_loss_type(_C.to_json_bytes(config), C.byref(out)))
    return out.value


def loss_name(type_number):
    name = _C.lib.tcnn_loss_name(int(type_number))
    if name is None:
        _C.check(1)
    return name.decode()


def _rows(t, what, prediction):
    """target / data_pdf: compact fp32 [n, dims] on the prediction's device"""
    if t is None:
        return None
    if t.shape != prediction.shape:
        raise RuntimeError(f"tcnn: {what} must have the prediction's shape {list(prediction.shape)}, not {list(t.shape)}")
    if t.device != prediction.device:
        raise RuntimeError(f"tcnn: {what} lives on {t.device}, the prediction on {prediction.device}")
    if t.requires_grad:
        t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _prediction(p):
    """[n, dims] half or float on the GPU, unit column stride, row stride >= dims: taken as it is (a slice of a padded output is not copied)"""
    if not p.is_cuda:
        raise RuntimeError("tcnn: the prediction must live on the GPU")
    if p.dtype not in PRECISION:
        raise RuntimeError(f"tcnn: the prediction must be float16 or float32, not {p.dtype}")
    n, dims = p.shape
    if n > 0 and dims > 0 and (p.stride(1) != 1 or p.stride(0) < dims):
        p = p.contiguous()
    return p


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # the current stream's handle without a Stream object around it
_evaluate = _C.lib.tcnn_loss_evaluate


def _launch(type_number, prediction, target, data_pdf, loss_scale, scale_dev, values, gradients, loss_sum):
    """tcnn_loss_evaluate on the current stream of the prediction's device; the tensors have been checked"""
    index = prediction.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _launch(type_number, prediction, target, data_pdf, loss_scale, scale_dev, values, gradients, loss_sum)
    n, dims = prediction.shape
    stride = prediction.stride(0) if n > 1 else max(prediction.stride(0), dims)  # (one row: torch reports any stride)
    stream = _raw_stream(index) if _raw_stream is not None else torch.cuda.current_stream().cuda_stream
    if _evaluate(type_number, stream, loss_scale, None if scale_dev is None else scale_dev.data_ptr(), n, dims, prediction.data_ptr(), stride,
                                 PRECISION[prediction.dtype], target.data_ptr(), None if data_pdf is None else data_pdf.data_ptr(),
                                 None if values is None else values.data_ptr(), 0 if values is None else values.shape[1],
                                 None if gradients is None else gradients.data_ptr(), 0 if gradients is None else gradients.shape[1],
                                 None if loss_sum is None else loss_sum.data_ptr()):
        _C.check(1)


class _LossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction, target, data_pdf, type_number):
        p = _prediction(prediction)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        _launch(type_number, p, target, data_pdf, 1.0, None, None, None, loss)
        ctx.type_number = type_number
        ctx.save_for_backward(p, target, data_pdf)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        p, target, data_pdf = ctx.saved_tensors
        if grad_output.dtype != torch.float32 or grad_output.device != p.device:
            grad_output = grad_output.to(device=p.device, dtype=torch.float32)
        gradient = torch.empty(p.shape, dtype=p.dtype, device=p.device)
        _launch(ctx.type_number, p, target, data_pdf, 1.0, grad_output, None, gradient, None)  # (0-d: one float wherever it lies)
        return gradient, None, None, None


class Loss(torch.nn.Module):
    """config: a loss configuration ({"otype": "RelativeL2"}), or the name.  No parameters, no state."""

    def __init__(self, config):
        super().__init__()
        self.config = {"otype": config} if isinstance(config, str) else dict(config)
        self.type = loss_type(self.config)  # "Invalid loss type: X" is raised here
        self.name = loss_name(self.type)

    def hyperparams(self):
        return dict(self.config)

    def extra_repr(self):
        return f"otype={self.name}"

    def _inputs(self, prediction, target, data_pdf):
        if not isinstance(prediction, torch.Tensor) or prediction.dim() != 2:
            raise RuntimeError("tcnn: the prediction must be a tensor of shape [n, dims]")
        return _rows(target, "the target", prediction), _rows(data_pdf, "data_pdf", prediction)

    def forward(self, prediction, target, data_pdf=None):
        """The loss as a 0-d fp32 tensor (the sum of the per-element values, each divided by n * dims), differentiable with respect to
        `prediction` only.  prediction: [n, dims] half or float on the GPU; target, data_pdf: fp32 [n, dims]."""
        target, data_pdf = self._inputs(prediction, target, data_pdf)
        if prediction.requires_grad and torch.is_grad_enabled():
            return _LossFunction.apply(prediction, target, data_pdf, self.type)
        p = _prediction(prediction)  # nothing is saved
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        _launch(self.type, p, target, data_pdf, 1.0, None, None, None, loss)
        return loss

    @torch.no_grad()
    def evaluate(self, prediction, target, data_pdf=None, loss_scale=1.0, out_gradient=None, want_values=False):
        """-> (loss, gradient[, values]) from one pass, without autograd: what Trainer.training_step(external_dL_dy=...) takes.
        gradient: loss_scale * dL/dprediction in the prediction's dtype, [n, dims] -- or `out_gradient`, a contiguous [n, S] tensor with
        S >= dims whose padding columns come back zero.  values: fp32 [n, dims], the per-element loss."""
        target, data_pdf = self._inputs(prediction, target, data_pdf)
        p = _prediction(prediction.detach())
        n, dims = p.shape
        if out_gradient is None:
            out_gradient = torch.empty((n, dims), dtype=p.dtype, device=p.device)
        elif not (isinstance(out_gradient, torch.Tensor) and out_gradient.dim() == 2 and out_gradient.shape[0] == n and out_gradient.shape[1] >= dims
                  and out_gradient.dtype == p.dtype and out_gradient.device == p.device and out_gradient.is_contiguous()):
            raise RuntimeError(f"tcnn: out_gradient must be a contiguous {p.dtype} tensor of shape [{n}, S] with S >= {dims} on {p.device}")
        values = torch.empty((n, dims), dtype=torch.float32, device=p.device) if want_values else None
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        _launch(self.type, p, target, data_pdf, float(loss_scale), None, values, out_gradient, loss)
        return (loss, out_gradient, values) if want_values else (loss, out_gradient)
