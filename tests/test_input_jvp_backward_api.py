"""Training through input_jvp (tcnn_module_input_jvp_forward / _backward: the gradients of sum_t <dL_djvp_t, J v_t> + <dL_doutput, f(x)> by
parameters, input and tangents) through the C ABI and the C++ headers, without a GPU: the symbols exist with their signatures, the header
methods compile with a plain C++14 compiler and link, and every bad call -- NULL tangents or dL_djvp, n_tangents of 0, a batch size off the
granularity, a module without a tangent (PPNG1, PPNG2, a Composite holding one), dL_dinput behind a OneBlob encoding, a context of another
call kind -- is refused with its message before anything is allocated or launched (modules are made without a device, the pointers are fake
and never read, contexts come from calls on an empty batch) and leaves the route strings alone.  What the routes compute is
tests/test_input_jvp_backward_gpu.py's."""
import ctypes as C
import json
import os
import subprocess

import pytest

from conftest import ROOT
from test_grid_max_level_api import _hip_libdir
from test_input_gradient_api import GRID, LIBDIR, NET, TCNN_ERROR, _modules
from test_input_jvp_api import NO_TANGENT

SRC = os.path.join(ROOT, "tests", "cpp", "input_jvp_backward_api.cpp")
INVALID_CONTEXT = b"Module::bwd: called with invalid context. fwd likely (mistakenly) ran in inference mode."
IGNORE, OVERWRITE, ACCUMULATE = 0, 1, 2


@pytest.fixture(scope="module")
def lib(tcnn):
    from tinycudann import _C

    return _C


@pytest.fixture(scope="module")
def binary(tcnn, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "input_jvp_backward_api")
    hip = _hip_libdir()
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", f"-I{os.path.join(ROOT, 'include')}", SRC, f"-L{LIBDIR}", "-ltcnn_amd",
           f"-Wl,-rpath,{LIBDIR}", f"-Wl,-rpath,{hip}", f"-Wl,-rpath-link,{hip}", "-o", out]
    subprocess.check_call(cmd)
    return out


def test_header_methods_compile_link_and_refuse_bad_calls(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host checks ok" in r.stdout


def test_symbols_and_signatures(lib):
    u32, vp, i = C.c_uint32, C.c_void_p, C.c_int
    f = lib.lib.tcnn_module_input_jvp_forward  # (m, stream, n, T, input, tangents, jvp, output, params, ctx_out)
    assert f.restype is i and list(f.argtypes) == [vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    f = lib.lib.tcnn_module_input_jvp_backward  # (m, stream, ctx, n, T, input, tangents, dL_djvp, dL_doutput, params, dL_dparams, dL_dinput, dL_dtangents, mode)
    assert f.restype is i and list(f.argtypes) == [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, i]
    f = lib.lib.tcnn_module_last_input_jvp_backward_route
    assert f.restype is C.c_char_p and list(f.argtypes) == [vp]
    f = lib.lib.tcnn_trainer_input_jvp_forward
    assert f.restype is i and list(f.argtypes) == [vp, vp, u32, u32, vp, vp, vp, vp, vp]
    f = lib.lib.tcnn_trainer_input_jvp_backward
    assert f.restype is i and list(f.argtypes) == [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, i]
    header = open(os.path.join(ROOT, "include", "tcnn_amd.h")).read()
    for name in ("tcnn_module_input_jvp_forward", "tcnn_module_input_jvp_backward", "tcnn_module_last_input_jvp_backward_route", "tcnn_trainer_input_jvp_forward",
                 "tcnn_trainer_input_jvp_backward"):
        assert name + "(" in header


def _routes(L, h):
    return (L.tcnn_module_last_input_jvp_backward_route(h), L.tcnn_module_last_input_jvp_route(h), L.tcnn_module_last_input_gradient_route(h),
            L.tcnn_module_last_input_jacobian_route(h))


NONE = (b"none",) * 4


def _jvp_context(lib, h, n_tangents):
    """a context of input_jvp_forward on an empty batch: nothing runs"""
    ctx = C.c_void_p()
    fake = C.c_void_p(0x1000)
    lib.check(lib.lib.tcnn_module_input_jvp_forward(h, None, 0, n_tangents, None, fake, fake, None, None, C.byref(ctx)))
    assert ctx.value
    return ctx


def test_forward_refuses_what_input_jvp_refuses(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)  # never read: every error comes first
    for h in _modules(lib):
        try:
            ctx = C.c_void_p()
            assert L.tcnn_module_input_jvp_forward(h, None, 256, 1, fake, None, fake, None, fake, C.byref(ctx)) == TCNN_ERROR
            assert b"tangents" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp_forward(h, None, 256, 1, fake, fake, None, None, fake, C.byref(ctx)) == TCNN_ERROR
            assert b"jvp" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp_forward(h, None, 256, 0, fake, fake, fake, None, fake, C.byref(ctx)) == TCNN_ERROR
            assert b"n_tangents" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp_forward(h, None, 300, 2, fake, fake, fake, None, fake, C.byref(ctx)) == TCNN_ERROR
            assert b"BATCH_SIZE_GRANULARITY" in L.tcnn_last_error()
            assert not ctx.value  # a refused call leaves no context
            assert _routes(L, h) == NONE
        finally:
            L.tcnn_module_destroy(h)


def test_backward_arguments_are_checked_before_anything_runs(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)
    for h in _modules(lib):
        ctx = _jvp_context(lib, h, 2)
        try:
            assert L.tcnn_module_last_input_jvp_backward_route(h) == b"none"
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 256, 2, fake, None, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
            assert b"tangents" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 256, 2, fake, fake, None, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
            assert b"dL_djvp" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 256, 0, fake, fake, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
            assert b"n_tangents" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 300, 2, fake, fake, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
            assert b"BATCH_SIZE_GRANULARITY" in L.tcnn_last_error()
            # the context is of a call on 0 rows with 2 tangents
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 256, 2, fake, fake, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
            assert b"context" in L.tcnn_last_error()
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 3, fake, fake, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
            assert b"context" in L.tcnn_last_error()
            # a gradient mode that asks for gradients needs somewhere to put them
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 2, fake, fake, fake, None, fake, None, fake, fake, ACCUMULATE) == TCNN_ERROR
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 2, fake, fake, fake, None, fake, fake, fake, fake, 7) == TCNN_ERROR
            assert L.tcnn_module_input_jvp_backward(h, None, None, 0, 2, fake, fake, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
            assert L.tcnn_last_error() == INVALID_CONTEXT
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 2, None, fake, fake, None, None, fake, fake, fake, OVERWRITE) == 0  # an empty batch is no work
            assert _routes(L, h) == NONE
        finally:
            L.tcnn_context_destroy(ctx)
            L.tcnn_module_destroy(h)


def test_a_context_of_another_call_kind_is_refused(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)
    h = C.c_void_p()
    lib.check(L.tcnn_create_network_with_input_encoding(3, 3, json.dumps(GRID).encode(), json.dumps(NET).encode(), C.byref(h)))
    forward_ctx, jvp_ctx = C.c_void_p(), _jvp_context(lib, h, 1)
    lib.check(L.tcnn_module_forward(h, None, 0, None, None, None, 1, C.byref(forward_ctx)))  # (an empty batch: nothing runs)
    try:
        assert L.tcnn_module_input_jvp_backward(h, None, forward_ctx, 0, 1, fake, fake, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
        assert L.tcnn_last_error() == INVALID_CONTEXT
        assert L.tcnn_module_backward(h, None, jvp_ctx, 0, fake, fake, fake, fake, fake, fake) == TCNN_ERROR
        assert L.tcnn_last_error() == INVALID_CONTEXT
        assert L.tcnn_module_backward_backward_input(h, None, jvp_ctx, 0, fake, fake, fake, fake, fake, fake, fake) == TCNN_ERROR
        assert b"called with invalid context" in L.tcnn_last_error()
        assert _routes(L, h) == NONE
    finally:
        L.tcnn_context_destroy(forward_ctx)
        L.tcnn_context_destroy(jvp_ctx)
        L.tcnn_module_destroy(h)


def test_modules_without_a_tangent_are_refused(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)
    for n_in, encoding, name in NO_TANGENT:
        made = []
        h = C.c_void_p()
        lib.check(L.tcnn_create_encoding(n_in, json.dumps(encoding).encode(), 1, C.byref(h)))
        made.append(h)
        h = C.c_void_p()
        net = {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
        lib.check(L.tcnn_create_network_with_input_encoding(n_in, 3, json.dumps(encoding).encode(), json.dumps(net).encode(), C.byref(h)))
        made.append(h)
        for h, who in zip(made, (name, b"NetworkWithInputEncoding")):
            other = C.c_void_p()
            lib.check(L.tcnn_create_network(16, 3, json.dumps(net).encode(), C.byref(other)))
            ctx = _jvp_context(lib, other, 2)  # (this module makes none: its forward call is refused)
            try:
                refused = C.c_void_p()
                assert L.tcnn_module_input_jvp_forward(h, None, 256, 2, fake, fake, fake, None, fake, C.byref(refused)) == TCNN_ERROR
                assert L.tcnn_last_error() == b"input_jvp: not implemented for " + who
                assert not refused.value
                assert L.tcnn_module_input_jvp_backward(h, None, ctx, 256, 2, fake, fake, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
                assert L.tcnn_last_error() == b"input_jvp: not implemented for " + who
                assert _routes(L, h) == NONE
            finally:
                L.tcnn_context_destroy(ctx)
                L.tcnn_module_destroy(other)
                L.tcnn_module_destroy(h)


def test_dL_dinput_behind_oneblob_is_refused_and_the_rest_is_not(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)
    oneblob = {"otype": "OneBlob", "n_bins": 16}
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    made = []
    h = C.c_void_p()
    lib.check(L.tcnn_create_network_with_input_encoding(3, 3, json.dumps(oneblob).encode(), json.dumps(net).encode(), C.byref(h)))
    made.append((h, b"NetworkWithInputEncoding"))
    h = C.c_void_p()
    lib.check(L.tcnn_create_encoding(3, json.dumps(oneblob).encode(), 1, C.byref(h)))
    made.append((h, b"OneBlob"))
    for h, who in made:
        ctx = _jvp_context(lib, h, 2)
        try:
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 2, fake, fake, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR
            assert L.tcnn_last_error() == b"input_jvp_backward: dL_dinput not implemented for " + who
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 2, fake, fake, fake, None, fake, None, fake, None, IGNORE) == TCNN_ERROR
            assert L.tcnn_last_error() == b"input_jvp_backward: dL_dinput not implemented for " + who
            # dL_dparams and dL_dtangents are served (an empty batch: accepted, nothing runs)
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 2, None, fake, fake, None, None, fake, None, fake, OVERWRITE) == 0
            assert _routes(L, h) == NONE
        finally:
            L.tcnn_context_destroy(ctx)
            L.tcnn_module_destroy(h)


def test_dL_dparams_is_refused_where_a_composite_holds_oneblob_beside_parameters(lib):
    """the tangent of such a Composite exists (input_jvp serves it), but the grid's share of dL_dparams is its second-order pass, which the
    Composite as a whole does not have: refused as dL_dinput is, dL_dtangents served (DESIGN.md "Training through input_jvp / What is left")"""
    L = lib.lib
    fake = C.c_void_p(0x1000)
    enc = {"otype": "Composite", "nested": [{"otype": "OneBlob", "n_bins": 16, "n_dims_to_encode": 2}, dict(GRID, n_dims_to_encode=3)]}
    made = []
    h = C.c_void_p()
    lib.check(L.tcnn_create_encoding(5, json.dumps(enc).encode(), 1, C.byref(h)))
    made.append((h, b"Composite"))
    h = C.c_void_p()
    lib.check(L.tcnn_create_network_with_input_encoding(5, 3, json.dumps(enc).encode(), json.dumps(NET).encode(), C.byref(h)))
    made.append((h, b"NetworkWithInputEncoding"))
    for h, who in made:
        ctx = _jvp_context(lib, h, 2)
        try:
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 2, fake, fake, fake, None, fake, fake, None, fake, OVERWRITE) == TCNN_ERROR
            assert L.tcnn_last_error() == b"input_jvp_backward: dL_dparams not implemented for " + who
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 2, fake, fake, fake, None, fake, None, fake, None, IGNORE) == TCNN_ERROR
            assert L.tcnn_last_error() == b"input_jvp_backward: dL_dinput not implemented for " + who
            assert L.tcnn_module_input_jvp_backward(h, None, ctx, 0, 2, None, fake, fake, None, None, None, None, fake, IGNORE) == 0  # dL_dtangents alone
            assert _routes(L, h) == NONE
        finally:
            L.tcnn_context_destroy(ctx)
            L.tcnn_module_destroy(h)


def test_null_handles_report_an_error(lib):
    L = lib.lib
    fake = C.c_void_p(0x1000)
    ctx = C.c_void_p()
    assert L.tcnn_module_input_jvp_forward(None, None, 256, 1, fake, fake, fake, None, fake, C.byref(ctx)) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_module_input_jvp_backward(None, None, fake, 256, 1, fake, fake, fake, None, fake, fake, fake, fake, OVERWRITE) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_trainer_input_jvp_forward(None, None, 256, 1, fake, fake, fake, None, C.byref(ctx)) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_trainer_input_jvp_backward(None, None, fake, 256, 1, fake, fake, fake, None, None, None, OVERWRITE) == TCNN_ERROR and L.tcnn_last_error()
    assert L.tcnn_module_last_input_jvp_backward_route(None) is None and b"null module" in L.tcnn_last_error()


def test_python_surfaces_exist(tcnn):
    import inspect

    from tinycudann.modules import Module, NativeModule

    assert callable(NativeModule.input_jvp_fwd) and callable(NativeModule.input_jvp_bwd) and callable(NativeModule.last_input_jvp_backward_route)
    assert callable(tcnn.Trainer.input_jvp_forward) and callable(tcnn.Trainer.input_jvp_backward)
    parameters = inspect.signature(Module.input_jvp).parameters
    assert list(parameters) == ["self", "x", "tangents", "return_output", "differentiable"]
    assert parameters["differentiable"].default is False and parameters["return_output"].default is False
    for cls in (tcnn.Encoding, tcnn.Network, tcnn.NetworkWithInputEncoding):
        assert cls.input_jvp is Module.input_jvp
