"""The library's losses on predictions that are the caller's: tcnn_loss_type / tcnn_loss_name / tcnn_loss_evaluate (include/tcnn_amd.h,
k_loss_eval.hip) and tcnn.losses.Loss.  CPU: names, the argument checks (made before anything touches a device), and the float32 numpy
restatement of loss_element pinned to the oracle.  GPU: the same bits as the trainer's own route, the oracle / numpy per element over
every shape at which the kernel takes another path, an exact sum, autograd, and a training run fed through external_dL_dy."""
import ctypes as C

import numpy as np
import pytest

LOSSES = ["L2", "RelativeL2", "RelativeL2Luminance", "L1", "RelativeL1", "Mape", "Smape", "CrossEntropy", "Variance"]
TYPE_NUMBERS = {"L2": 0, "RelativeL2": 1, "L1": 2, "RelativeL1": 3, "Mape": 4, "Smape": 5, "CrossEntropy": 6, "Variance": 7, "RelativeL2Luminance": 8}
F = np.float32
FP32, FP16 = 0, 1
U = 2.0 ** -24  # unit roundoff of float32


# ------------------------------------------------------------------------------------------------------------------ yardsticks
def np_loss(name, p, t, pdf, loss_scale):
    """loss_element (loss_device.h) in float32 numpy, operation by operation: p, t, pdf float32 [n, dims] -> (values, gradients before
    their cast to the prediction's type), both float32."""
    p, t = np.ascontiguousarray(p, dtype=F), np.ascontiguousarray(t, dtype=F)
    pdf = np.ones_like(p) if pdf is None else np.ascontiguousarray(pdf, dtype=F)
    n_total, ls = F(p.size), F(loss_scale)
    d = p - t
    if name == "CrossEntropy":
        factor = -t / pdf / n_total
        return factor * np.log(p), ls * (factor / p)
    if name == "Variance":
        factor = t * t / pdf / n_total
        return factor / p - factor / pdf, ls * (-factor / (p * p))
    if name == "L2":
        v, g = d * d / pdf / n_total, F(2) * d / pdf
    elif name == "RelativeL2":
        q = p * p + F(0.01)
        v, g = d * d / q / pdf / n_total, F(2) * d / q / pdf
    elif name == "RelativeL2Luminance":
        r, gr, b = p[:, 0], p[:, 1], p[:, 2]
        if p.shape[1] >= 6:
            r, gr, b = r + p[:, 3], gr + p[:, 4], b + p[:, 5]
        lum = (F(0.299) * r + F(0.587) * gr + F(0.114) * b)[:, None]
        q = lum * lum + F(0.01)
        v, g = d * d / q / pdf / n_total, F(2) * d / q / pdf
    elif name == "L1":
        v, g = np.abs(d) / pdf / n_total, np.copysign(F(1) / pdf, d)
    else:
        base = {"RelativeL1": np.abs(p), "Mape": np.abs(t), "Smape": F(0.5) * (np.abs(t) + np.abs(p))}[name]
        s = F(1) / (base + F(1e-2)) / pdf
        v, g = np.abs(d) * s / n_total, np.copysign(s, d)
    assert v.dtype == F and g.dtype == F
    return v, ls * g / n_total


def benign(n, dims, seed):
    """the existing tests' range: predictions and targets in [0.05, 2.0], pdf in [0.5, 2.0]; the predictions are halves, as float32"""
    rs = np.random.RandomState(seed)
    p = rs.uniform(0.05, 2.0, (n, dims)).astype(np.float16).astype(F)
    return p, rs.uniform(0.05, 2.0, (n, dims)).astype(F), rs.uniform(0.5, 2.0, (n, dims)).astype(F)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_values(name, got, want):
    if name == "CrossEntropy":  # logf: device / libm / numpy
        assert np.allclose(got, want, rtol=1e-5, atol=1e-10)
    else:
        assert np.array_equal(bits(got), bits(want))


@pytest.fixture(scope="module")
def lib(tcnn):
    from tinycudann import _C

    return _C.lib


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_loss_type_accepts_the_nine_names_case_insensitively(lib):
    for name, number in TYPE_NUMBERS.items():
        for spelling in (name, name.lower(), name.upper()):
            out = C.c_int(-1)
            assert lib.tcnn_loss_type(('{"otype": "%s"}' % spelling).encode(), C.byref(out)) == 0, lib.tcnn_last_error()
            assert out.value == number
        assert lib.tcnn_loss_name(number) == name.encode()
    assert sorted(TYPE_NUMBERS) == sorted(LOSSES)


def test_loss_type_rejects_an_unknown_name(lib, tcnn):
    out = C.c_int(-1)
    assert lib.tcnn_loss_type(b'{"otype": "Huber"}', C.byref(out)) != 0
    assert lib.tcnn_last_error() == b"Invalid loss type: Huber"
    assert lib.tcnn_loss_name(9) is None and b"Invalid loss type: 9" in lib.tcnn_last_error()
    assert lib.tcnn_loss_name(-1) is None
    with pytest.raises(RuntimeError, match="Invalid loss type: Huber"):
        tcnn.losses.Loss("Huber")
    with pytest.raises(RuntimeError, match="Invalid loss type: Huber"):
        tcnn.losses.Loss({"otype": "Huber"})


def test_loss_module_needs_no_device_to_exist(tcnn):
    loss = tcnn.losses.Loss({"otype": "relativel2luminance"})
    assert loss.name == "RelativeL2Luminance" and loss.type == 8
    assert loss.hyperparams() == {"otype": "relativel2luminance"}
    assert "RelativeL2Luminance" in repr(loss)
    assert tcnn.losses.Loss("Smape").hyperparams() == {"otype": "Smape"}
    assert list(loss.parameters()) == []


def _call(lib, type_number=1, n=256, dims=3, prediction=0x1000, p_stride=16, precision=FP16, target=0x2000, values=0x3000, v_stride=16, gradients=0x4000, g_stride=16,
          loss_sum=0x5000):
    """tcnn_loss_evaluate with addresses that are never dereferenced: each of these calls must fail in the host-side checks"""
    return lib.tcnn_loss_evaluate(type_number, None, 1.0, None, n, dims, prediction, p_stride, precision, target, None, values, v_stride, gradients, g_stride, loss_sum)


@pytest.mark.parametrize("kwargs, message", [
    (dict(p_stride=2), "the prediction stride 2 is smaller than dims 3"),
    (dict(g_stride=2), "the gradients stride 2 is smaller than dims 3"),
    (dict(v_stride=1), "the values stride 1 is smaller than dims 3"),
    (dict(type_number=8, dims=2), "RelativeL2Luminance reads three channels per row and needs dims >= 3, got 2"),
    (dict(values=None, gradients=None, loss_sum=None), "no output requested"),
    (dict(prediction=None), "prediction and target must not be NULL"),
    (dict(target=None), "prediction and target must not be NULL"),
    (dict(dims=0), "dims must be at least 1"),
    (dict(precision=2), "Unknown precision 2"),
    (dict(type_number=9), "Invalid loss type: 9"),
    (dict(n=1 << 28, p_stride=16), "n * stride must be below 2^32"),
    (dict(n=1 << 28, p_stride=3, v_stride=3, g_stride=16), "n * stride must be below 2^32"),
])
def test_arguments_are_checked_before_anything_touches_a_device(lib, kwargs, message):
    assert _call(lib, **kwargs) != 0
    assert message in lib.tcnn_last_error().decode()


def test_strides_of_outputs_that_are_not_requested_are_not_checked(lib):
    # (the call still fails -- at the NULL target, the last check -- so nothing is launched)
    assert _call(lib, values=None, v_stride=0, target=None) != 0
    assert "prediction and target must not be NULL" in lib.tcnn_last_error().decode()


@pytest.mark.parametrize("dims", [3, 6])
@pytest.mark.parametrize("name", LOSSES)
def test_numpy_restatement_matches_the_oracle_on_half_inputs(tcnn, oracle, name, dims):
    """the yardstick the GPU tests use for float predictions, pinned to the oracle (which takes half predictions)"""
    assert tcnn.losses.loss_name(TYPE_NUMBERS[name]) == name  # the name the yardstick goes by is the library's name for that type
    n = 256
    p, t, pdf = benign(n, dims, seed=dims)
    pred_h = oracle.half_bits(p)
    assert np.array_equal(oracle.half_to_f32(pred_h), p)
    for with_pdf in (pdf, None):
        want_v, want_g = oracle.loss_evaluate(name, pred_h, t, loss_scale=128.0, data_pdf=with_pdf)
        got_v, got_g = np_loss(name, p, t, with_pdf, 128.0)
        assert_values(name, got_v, want_v)
        assert np.array_equal(bits(got_g.astype(np.float16)), want_g)


# ------------------------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def raw_evaluate(tcnn, name, pred, t, pdf, loss_scale, v_stride, g_stride):
    """tcnn_loss_evaluate with every output and free strides: pred is a torch view [n, dims] -> (values [n, v_stride], gradients [n, g_stride], sum)"""
    import torch

    from tinycudann import _C

    n, dims = pred.shape
    values = torch.full((n, v_stride), 7.0, dtype=torch.float32, device="cuda")
    gradients = torch.full((n, g_stride), 7.0, dtype=pred.dtype, device="cuda")
    loss = torch.full((), 7.0, dtype=torch.float32, device="cuda")
    stride = pred.stride(0) if n > 1 else max(pred.stride(0), dims)
    assert pred.stride(1) == 1 or dims == 1
    _C.check(_C.lib.tcnn_loss_evaluate(TYPE_NUMBERS[name], torch.cuda.current_stream().cuda_stream, loss_scale, None, n, dims, pred.data_ptr(), stride,
                                       FP16 if pred.dtype == torch.half else FP32, t.data_ptr(), None if pdf is None else pdf.data_ptr(), values.data_ptr(), v_stride,
                                       gradients.data_ptr(), g_stride, loss.data_ptr()))
    return values.cpu().numpy(), gradients.cpu().numpy(), float(loss.item())


def assert_sum_within_bound(loss, values):
    """any order of float32 additions of N values is within (N - 1) u sum|v| of their exact sum"""
    v = np.asarray(values, dtype=np.float64).ravel()
    assert abs(float(loss) - v.sum()) <= (v.size - 1) * U * np.abs(v).sum(), (float(loss), v.sum())


@gpu
@pytest.mark.parametrize("dtype_name", ["half", "float"])
@pytest.mark.parametrize("name", LOSSES)
def test_same_bits_as_the_trainers_own_route(tcnn, oracle, name, dtype_name):
    import torch

    from conftest import CONFIG_C3B

    dtype = torch.half if dtype_name == "half" else torch.float32
    loss_scale = 128.0 if dtype == torch.half else 1.0
    cfg = {**CONFIG_C3B, "loss": {"otype": name}}
    if name in ("CrossEntropy", "Variance"):
        cfg["network"] = {**CONFIG_C3B["network"], "output_activation": "Exponential"}  # predictions must be positive
    if dtype == torch.float32:  # (FullyFusedMLP is the half network, as in the reference: the float trainer runs the same shape as CutlassMLP)
        cfg["network"] = {**cfg["network"], "otype": "CutlassMLP"}
    tr = tcnn.Trainer(2, 3, cfg, seed=1337, dtype=None if dtype == torch.half else dtype)
    n = 1024
    x, t = oracle.synthetic_batch(n, 2, 3, seed=42)
    t = torch.from_numpy(np.ascontiguousarray(t * 0.9 + 0.05)).cuda()
    pdf = torch.from_numpy(np.random.RandomState(3).uniform(0.5, 2.0, (n, 3)).astype(F)).cuda()
    ctx = tr.forward(torch.from_numpy(x).cuda(), t, loss_scale=loss_scale, data_pdf=pdf)
    out = ctx.output()
    assert out.dtype == dtype and out.shape[1] == tr.padded_output_width
    dy = torch.zeros((n, tr.padded_output_width), dtype=dtype, device="cuda")
    loss, gradient, values = tcnn.losses.Loss(name).evaluate(out[:, :3], t, pdf, loss_scale=loss_scale, out_gradient=dy, want_values=True)
    assert gradient is dy
    assert np.array_equal(bits(gradient.cpu().numpy()), bits(ctx.dL_doutput().cpu().numpy()))  # every column, the padding included
    want_values = ctx.L().cpu().numpy()[:, :3]
    assert np.array_equal(bits(values.cpu().numpy()), bits(want_values))
    assert_sum_within_bound(loss.item(), want_values)


SHAPE_NS = (1, 255, 257, 1000)


# (RelativeL2Luminance reads three channels: dims >= 3 -- test_arguments_are_checked_before_anything_touches_a_device has the refusal)
SHAPE_CASES = [(name, dims) for name in LOSSES for dims in (1, 3, 4, 5, 6, 16) if not (name == "RelativeL2Luminance" and dims < 3)]


@gpu
@pytest.mark.parametrize("name, dims", SHAPE_CASES)
def test_against_the_oracle_and_numpy_over_shapes_and_strides(tcnn, oracle, name, dims):
    """half predictions against the oracle, float predictions against the numpy restatement: n below, at and above one block and one
    vector; compact and padded prediction rows; compact and padded output rows; and a prediction base off by one element (no 16-byte
    alignment: the one-element-per-thread kernel)"""
    import torch

    loss_scale = 128.0
    for n in SHAPE_NS:
        p, t, pdf = benign(n, dims, seed=1000 * dims + n)
        want = {}
        v, g = oracle.loss_evaluate(name, oracle.half_bits(p), t, loss_scale=loss_scale, data_pdf=pdf)
        want[torch.half] = (v, g)
        v, g = np_loss(name, p, t, pdf, loss_scale)
        want[torch.float32] = (v, bits(g))
        t_dev, pdf_dev = torch.from_numpy(t).cuda(), torch.from_numpy(pdf).cuda()
        for dtype in (torch.half, torch.float32):
            want_v, want_g = want[dtype]
            for p_stride, offset in ((dims, 0), (16, 0), (dims, 1), (16, 1)):
                flat = torch.full((n * p_stride + offset,), 3.0, dtype=dtype, device="cuda")  # (padding columns: a value no loss result contains)
                rows = flat[offset:].view(n, p_stride)
                rows[:, :dims] = torch.from_numpy(p).cuda().to(dtype)
                pred = rows[:, :dims]
                assert pred.data_ptr() % 16 == (0 if offset == 0 else pred.element_size())
                # (differing strides: one output stored 16 bytes at a time, the other element by element, in the same launch)
                for v_stride, g_stride in ((dims, dims), (16, 16), (dims, 16), (16, dims)):
                    got_v, got_g, got_sum = raw_evaluate(tcnn, name, pred, t_dev, pdf_dev, loss_scale, v_stride, g_stride)
                    where = (name, dims, n, dtype, p_stride, offset, v_stride, g_stride)
                    assert np.array_equal(bits(got_g[:, :dims]), want_g), where
                    assert_values(name, got_v[:, :dims], want_v)
                    assert not got_v[:, dims:].any() and not bits(got_g[:, dims:]).any(), where  # +0.0 in every padding column
                    assert_sum_within_bound(got_sum, got_v[:, :dims])


@gpu
@pytest.mark.parametrize("dtype_name", ["half", "float"])
@pytest.mark.parametrize("n, dims", [(1024, 4), (4096, 1), (512, 16)])
def test_the_reduction_drops_and_duplicates_nothing(tcnn, n, dims, dtype_name):
    """L1 without pdf on differences that are multiples of 1/8 and n * dims a power of two: every value and every partial sum is exact in
    float32, so the sum has to be THE sum, bit for bit -- and has to move when one element does"""
    import torch

    dtype = torch.half if dtype_name == "half" else torch.float32
    rs = np.random.RandomState(n + dims)
    p = (rs.randint(0, 17, (n, dims)) / 8.0).astype(F)  # exactly representable in half
    t = (rs.randint(0, 17, (n, dims)) / 8.0).astype(F)
    loss_fn = tcnn.losses.Loss("L1")
    t_dev = torch.from_numpy(t).cuda()

    def run(p_host):
        pred = torch.from_numpy(p_host).cuda().to(dtype)
        with_sum_only = loss_fn(pred, t_dev)
        with_everything, _, values = loss_fn.evaluate(pred, t_dev, want_values=True)
        assert np.array_equal(bits(values.cpu().numpy()), bits((np.abs(p_host - t) / F(n * dims)).astype(F)))
        assert bits(np.array(with_sum_only.item(), dtype=F)) == bits(np.array(with_everything.item(), dtype=F))
        return with_sum_only.item()

    exact = np.abs(p.astype(np.float64) - t).sum() / (n * dims)
    assert float(F(exact)) == exact  # representable: sum|d| is an integer number of eighths below 2^24
    assert run(p) == exact
    p2 = p.copy()
    p2[n // 2, dims - 1] = t[n // 2, dims - 1] + 4.0  # a difference no element had: the sum must change by it
    exact2 = np.abs(p2.astype(np.float64) - t).sum() / (n * dims)
    assert exact2 != exact and run(p2) == exact2


def _slices(torch, n, dims, dtype, p):
    """(label, view [n, dims] holding p) for predictions that are slices of something larger: only the n rows of dims values are the
    caller's to read -- the columns behind a row's last value may lie behind the end of the allocation"""
    vec = 8 if dtype == torch.half else 4
    values = torch.from_numpy(p).cuda().to(dtype)
    # rows of stride 16 in a buffer of exactly (n - 1) * 16 + dims elements: the last row ends where the buffer ends
    exact = torch.full(((n - 1) * 16 + dims,), 3.0, dtype=dtype, device="cuda")
    view = torch.as_strided(exact, (n, dims), (16, 1))
    view.copy_(values)
    yield "exact-size buffer", view
    # the same behind a column offset of one vector (an aligned base again): out[:, vec : vec + dims] of an [n, 16] matrix cut off after its last value
    shifted = torch.full((vec + (n - 1) * 16 + dims,), 3.0, dtype=dtype, device="cuda")
    view = torch.as_strided(shifted, (n, dims), (16, 1), vec)
    view.copy_(values)
    yield "column offset, exact-size buffer", view
    # every other row of an [2 n - 1, 16] matrix: stride 32, nothing behind the last row's 16 columns
    rows = torch.full((2 * n - 1, 16), 3.0, dtype=dtype, device="cuda")
    view = rows[::2, :dims]
    view.copy_(values)
    yield "every other row", view


@gpu
@pytest.mark.parametrize("dims", [3, 6])
@pytest.mark.parametrize("name", ["L2", "RelativeL2Luminance"])
def test_slices_of_larger_matrices_are_read_inside_their_rows(tcnn, oracle, name, dims):
    """aligned bases and strides of whole vectors, so the 16-byte path runs: results against the oracle (half) and numpy (float)"""
    import torch

    n, loss_scale = 257, 128.0
    p, t, pdf = benign(n, dims, seed=77 + dims)
    t_dev, pdf_dev = torch.from_numpy(t).cuda(), torch.from_numpy(pdf).cuda()
    want_v, want_g = oracle.loss_evaluate(name, oracle.half_bits(p), t, loss_scale=loss_scale, data_pdf=pdf)
    want_v32, want_g32 = np_loss(name, p, t, pdf, loss_scale)
    for dtype, (wv, wg) in ((torch.half, (want_v, want_g)), (torch.float32, (want_v32, bits(want_g32)))):
        for label, pred in _slices(torch, n, dims, dtype, p):
            assert pred.data_ptr() % 16 == 0 and pred.stride(0) % 8 == 0, label
            for v_stride, g_stride in ((dims, dims), (16, 16), (dims, 16)):
                got_v, got_g, got_sum = raw_evaluate(tcnn, name, pred, t_dev, pdf_dev, loss_scale, v_stride, g_stride)
                assert np.array_equal(bits(got_g[:, :dims]), wg), (label, dtype, v_stride, g_stride)
                assert_values(name, got_v[:, :dims], wv)
                assert not got_v[:, dims:].any() and not bits(got_g[:, dims:]).any()
                assert_sum_within_bound(got_sum, got_v[:, :dims])


@gpu
def test_a_column_slice_of_a_matrix_that_fills_its_allocation(tcnn, oracle):
    """2^21 x 16 halves are 64 MiB, a size at which an allocation is a segment of its own, with nothing promised behind it: out[:, 8:11] has an aligned base and
    stride 16, and its last row's values are the last thing the kernel may read"""
    import torch

    n, dims = 1 << 21, 3
    p, t, _ = benign(n, dims, seed=21)
    out = torch.full((n, 16), 3.0, dtype=torch.half, device="cuda")
    out[:, 8:11] = torch.from_numpy(p).cuda().half()
    loss, gradient = tcnn.losses.Loss("L2").evaluate(out[:, 8:11], torch.from_numpy(t).cuda(), loss_scale=128.0)
    want_v, want_g = oracle.loss_evaluate("L2", oracle.half_bits(p), t, loss_scale=128.0)
    assert np.array_equal(bits(gradient.cpu().numpy()), want_g)
    assert_sum_within_bound(loss.item(), want_v)


@gpu
def test_two_runs_give_the_same_bits(tcnn):
    import torch

    p, t, pdf = benign(1000, 3, seed=5)
    loss_fn = tcnn.losses.Loss("RelativeL2")
    pred, t_dev, pdf_dev = torch.from_numpy(p).cuda().half(), torch.from_numpy(t).cuda(), torch.from_numpy(pdf).cuda()
    first = [bits(np.array(loss_fn(pred, t_dev, pdf_dev).item(), dtype=F)) for _ in range(2)]
    assert first[0] == first[1]
    a, b = loss_fn.evaluate(pred, t_dev, pdf_dev, loss_scale=128.0), loss_fn.evaluate(pred, t_dev, pdf_dev, loss_scale=128.0)
    assert bits(np.array(a[0].item(), dtype=F)) == bits(np.array(b[0].item(), dtype=F)) == first[0]
    assert np.array_equal(bits(a[1].cpu().numpy()), bits(b[1].cpu().numpy()))


@gpu
def test_no_rows_is_no_launch_and_a_zero_sum(tcnn):
    import torch

    loss_fn = tcnn.losses.Loss("L2")
    loss, gradient = loss_fn.evaluate(torch.empty((0, 3), dtype=torch.half, device="cuda"), torch.empty((0, 3), device="cuda"))
    assert loss.item() == 0.0 and gradient.shape == (0, 3)


@gpu
@pytest.mark.parametrize("name", LOSSES)
def test_autograd(tcnn, name):
    import torch

    n, dims = 1000, 3
    p, t, pdf = benign(n, dims, seed=11)
    t_dev, pdf_dev = torch.from_numpy(t).cuda(), torch.from_numpy(pdf).cuda()
    loss_fn = tcnn.losses.Loss(name)

    def leaf():
        return torch.from_numpy(p).cuda().half().requires_grad_()

    # the gradient of the loss itself: evaluate()'s at loss scale 1
    pred = leaf()
    loss = loss_fn(pred, t_dev, pdf_dev)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad
    loss.backward()
    want_loss, want_g = loss_fn.evaluate(pred, t_dev, pdf_dev, loss_scale=1.0)
    assert pred.grad.dtype == torch.half and pred.grad.shape == (n, dims) and pred.grad.is_contiguous()
    assert np.array_equal(bits(pred.grad.cpu().numpy()), bits(want_g.cpu().numpy()))
    assert bits(np.array(loss.item(), dtype=F)) == bits(np.array(want_loss.item(), dtype=F))
    # a second backward pass through the same graph is torch's error
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        loss.backward()

    # the incoming gradient is folded in before the ONE rounding to half: 1024 x loss == loss scale 1024
    pred = leaf()
    (1024 * loss_fn(pred, t_dev)).backward()
    _, want_g = loss_fn.evaluate(pred, t_dev, loss_scale=1024.0)
    assert np.array_equal(bits(pred.grad.cpu().numpy()), bits(want_g.cpu().numpy()))

    # a slice of a padded output: taken without a copy, the gradient arrives through the slice
    out16 = torch.full((n, 16), 3.0, dtype=torch.half, device="cuda")
    out16[:, :dims] = torch.from_numpy(p).cuda().half()
    out16.requires_grad_()
    view = out16[:, :dims]
    assert not view.is_contiguous()
    loss_fn(view, t_dev, pdf_dev).backward()
    _, want_g = loss_fn.evaluate(out16.detach()[:, :dims], t_dev, pdf_dev, loss_scale=1.0)
    assert np.array_equal(bits(out16.grad[:, :dims].cpu().numpy()), bits(want_g.cpu().numpy()))
    assert not bits(out16.grad[:, dims:].cpu().numpy()).any()

    # no_grad: the same scalar, nothing to differentiate
    with torch.no_grad():
        quiet = loss_fn(leaf(), t_dev, pdf_dev)
    assert not quiet.requires_grad and quiet.grad_fn is None
    assert bits(np.array(quiet.item(), dtype=F)) == bits(np.array(loss.item(), dtype=F))


@gpu
def test_wrong_inputs_are_runtime_errors(tcnn):
    import torch

    loss_fn = tcnn.losses.Loss("RelativeL2Luminance")
    t = torch.zeros((256, 2), device="cuda")
    with pytest.raises(RuntimeError, match="needs dims >= 3, got 2"):
        loss_fn(torch.ones((256, 2), dtype=torch.half, device="cuda"), t)
    with pytest.raises(RuntimeError, match="the target must have the prediction's shape"):
        loss_fn(torch.ones((256, 3), dtype=torch.half, device="cuda"), t)
    with pytest.raises(RuntimeError, match="float16 or float32"):
        loss_fn(torch.ones((256, 2), dtype=torch.float64, device="cuda"), t)
    with pytest.raises(RuntimeError, match="out_gradient must be a contiguous"):
        tcnn.losses.Loss("L2").evaluate(torch.ones((256, 2), dtype=torch.half, device="cuda"), t, out_gradient=torch.zeros((256, 16), device="cuda"))


@gpu
def test_training_through_external_dL_dy(tcnn, oracle):
    """30 steps of a trainer whose dL/dy comes from Loss("L1").evaluate on the trainer's own forward output"""
    import torch

    from conftest import CONFIG_C3B

    tr = tcnn.Trainer(2, 3, {**CONFIG_C3B, "loss": {"otype": "L1"}}, seed=1337)
    loss_fn = tcnn.losses.Loss("L1")
    n = 1024
    dy = torch.zeros((n, tr.padded_output_width), dtype=torch.half, device="cuda")

    def batch(seed):
        x, t = oracle.synthetic_batch(n, 2, 3, seed=seed)
        return torch.from_numpy(x).cuda(), torch.from_numpy(np.ascontiguousarray(t * 0.9 + 0.05)).cuda()

    def loss_on(x, t):
        ctx = tr.forward(x, t)
        return loss_fn.evaluate(ctx.output()[:, :3], t, loss_scale=128.0, out_gradient=dy)[0].item()

    x0, t0 = batch(42)
    first = loss_on(x0, t0)
    for s in range(30):
        x, t = batch(100 + s)
        loss_on(x, t)  # fills dy
        tr.training_step(x, t, external_dL_dy=dy)
    last = loss_on(x0, t0)
    assert tr.optimizer_step_count() == 30
    assert np.isfinite(last) and last < first, (first, last)
