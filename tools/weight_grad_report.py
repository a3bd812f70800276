"""Per case and layer: the GPU's weight-gradient ratio against the oracle beside the CPU yardstick (tests/grad_checks.py).

    python tools/weight_grad_report.py > profiles/weight_gradient_parity.txt

Ratio = worst |a - b| / (3e-2 |b| + 1e-3 max_layer|b| + q) of the layer, b the oracle's fp32 gradient; <= 1 passes
(tests/test_training_step_matrix.py).  "gpu": the kernel's half gradients (q = 2^-24); "unfused": the same step with TCNN_AMD_FUSED_STEP=0;
"f64": float64 sums with the reference's roundings to half (q = 0; piecewise-linear activations only) -- what the order of summation alone
does; "half": the oracle's own half gradients against its fp32 ones (q = 2^-24) -- what the fp16 store alone does.  Every kernel form of
test_training_step_matrix.FORM_CASES and PDF_CASES, with the grid as initialised ("init") and drawn from U(-1, 1) ("o1"); then the
bit-exact cases of tests/test_weight_gradients_exact.py: the number of half gradients that differ from the oracle's.
"""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tiny-cuda-nn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import oracle  # noqa: E402
import tinycudann as tcnn  # noqa: E402

import grad_checks as gc  # noqa: E402
import test_training_step_matrix as M  # noqa: E402
import test_weight_gradients_exact as X  # noqa: E402
from test_gpu_parity import _f32, _t  # noqa: E402


class _Env:
    """the part of pytest's monkeypatch that test_training_step_matrix._run uses"""

    @contextlib.contextmanager
    def context(self):
        saved = dict(os.environ)
        try:
            yield self
        finally:
            os.environ.clear()
            os.environ.update(saved)

    def setenv(self, k, v):
        os.environ[k] = v


def fmt(ratios):
    return " ".join(f"{r:7.3f}" for r in ratios)


def main():
    oracle.build()
    env = _Env()
    first = [(c[0], M._cfg(c[1], c[3], c[4], c[5], c[6]), c[2], c[7], c[8], c[9], c[10], c[6], None) for c in M.FORM_CASES] + \
            [(f"pdf_{c[0]}_{loss}", {**c[1], "loss": {"otype": loss}}, c[2], c[3], c[4], c[5], c[6], None, 3) for c in M.PDF_CASES for loss in ("L2", "RelativeL2")]
    print("weight gradients against the oracle, per layer (first layer first): worst element's share of the per-layer bar, <= 1 passes")
    worst = 0.0
    for regime, cases in (("init", first), ("o1", M.NORMAL_RANGE_CASES)):
        for case in cases:
            name, cfg, n_in, n_out, n, e, kernel, _, _ = case
            x, t, pdf = M.normal_range_inputs(oracle, case)
            ref = oracle.Trainer(n_in, n_out, cfg, seed=1337)
            if regime == "o1":
                ref.params = M.o1_grid_params(oracle, ref)
            net = ref.model.network
            n_net, slices = net.n_params, gc.layer_slices(net)
            grads32 = np.zeros(ref.model.n_params, dtype=np.float32)
            ref.training_step(x, t, run_optimizer=False, grads_f32=grads32, data_pdf=pdf)
            want = grads32[:n_net]
            kw = {} if pdf is None else {"data_pdf": _t(pdf)}
            got = M._run(tcnn, env, n_in, n_out, cfg, e, x, t, params_half=ref.params, **kw)
            print(f"{regime:4s} {name:28s} {got['kernel']:24s} n = {n}")
            r = gc.weight_grad_ratios(_f32(got["g"])[:n_net], want, slices, 3e-2, True)
            worst = max(worst, max(r))
            print(f"       gpu     {fmt(r)}")
            if got["kernel"] != "unfused":
                unf = M._run(tcnn, env, n_in, n_out, cfg, {**e, "TCNN_AMD_FUSED_STEP": "0"}, x, t, params_half=ref.params, **kw)
                r = gc.weight_grad_ratios(_f32(unf["g"])[:n_net], want, slices, 3e-2, True)
                worst = max(worst, max(r))
                print(f"       unfused {fmt(r)}")
            if cfg["network"]["activation"] in ("ReLU", "LeakyReLU", "None") and cfg["network"]["output_activation"] in ("None", "ReLU", "Sigmoid"):
                enc_out, _ = ref.model.encoding.forward(x, np.ascontiguousarray(ref.params[n_net:]))
                st = gc.float64_step(oracle.half_to_f32(enc_out), oracle.half_to_f32(ref.params[:n_net]), slices, cfg["network"]["activation"],
                                     cfg["network"]["output_activation"], loss=cfg["loss"]["otype"], target=t, n_out=n_out, data_pdf=pdf)
                print(f"       f64     {fmt(gc.weight_grad_ratios(st['grads'], want, slices, 3e-2, False))}")
            print(f"       half    {fmt(gc.weight_grad_ratios(oracle.half_to_f32(ref.grads[:n_net]), want, slices, 3e-2, True))}"
                  f"   subnormal share {max(gc.subnormal_share(ref.grads[:n_net], slices)):.3f}")
    print(f"worst gpu / unfused ratio of all cases: {worst:.3f}")
    print()
    print("exact setting (tests/test_weight_gradients_exact.py): half gradients that differ from the oracle's bits")
    total = 0
    for case, e, kernel in X.RUNS:
        cfg, slices, w, x, dy, want, _ = X._oracle_step(oracle, case)
        name, got = X._gpu_step(tcnn, env, case, cfg, e, w, x, dy)
        diff = int(np.count_nonzero(got != want))
        total += diff
        print(f"{X._run_id((case, e, kernel)):72s} {name:24s} {diff} of {want.size}")
    print(f"differing half gradients in all exact cases: {total}")


if __name__ == "__main__":
    main()
