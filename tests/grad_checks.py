"""Per-layer, per-element checks of the MLP's weight gradients, and the inputs of the setting in which they are exact.

A plain module the tests import (no fixtures, no GPU).  The norm-wise bar the suite used so far,

    rel_err(g[:n_net], grads32[:n_net]) < 3e-2          # max|a - b| / max|b| over ALL layers at once

lets a whole layer be wrong when its gradients are small beside the network's largest (the first layer's maximum is 6-23 % of it, in
Softplus / Exponential networks 5e-6 of it).  weight_grad_ratios is elem_close (test_gpu_parity) with the maximum taken per layer.
"""
import numpy as np

Q_HALF = 2.0 ** -24  # one fp16 subnormal step


def layer_slices(mlp):
    """(offset, rows, cols) of every weight matrix of an oracle.Mlp: row-major [rows][cols], in the order of orc_mlp_backward"""
    out, off = [], 0
    for rows, cols in mlp.layer_sizes():
        out.append((off, int(rows), int(cols)))
        off += int(rows) * int(cols)
    return out


def _layers(v, slices):
    v = np.asarray(v)
    return [v[o:o + r * c].reshape(r, c) for o, r, c in slices]


def weight_grad_worst(got, want_f32, slices, rtol, half_stored):
    """per layer (ratio, row, col, got, want) of the element with the worst |a - b| / (rtol |b| + 1e-3 max_layer|b| + q); q = 2^-24 when `got`
    went through an fp16 store (half a subnormal step of rounding, half a step for landing on the neighbour), else 0"""
    q = Q_HALF if half_stored else 0.0
    res = []
    for a, b in zip(_layers(got, slices), _layers(want_f32, slices)):
        a, b = a.astype(np.float64), b.astype(np.float64)
        bound = rtol * np.abs(b) + 1e-3 * float(np.max(np.abs(b))) + q
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, np.abs(a - b) / np.where(bound > 0, bound, 1.0), np.where(a == b, 0.0, np.inf))
        ratio = np.where(np.isfinite(a), ratio, np.inf)
        r, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        res.append((float(ratio[r, c]), int(r), int(c), float(a[r, c]), float(b[r, c])))
    return res


def weight_grad_ratios(got, want_f32, slices, rtol, half_stored):
    """the worst ratio of every layer; <= 1 passes"""
    return [w[0] for w in weight_grad_worst(got, want_f32, slices, rtol, half_stored)]


def assert_weight_grads_close(got, want_f32, slices, rtol, half_stored, what=""):
    for l, (ratio, r, c, a, b) in enumerate(weight_grad_worst(got, want_f32, slices, rtol, half_stored)):
        assert ratio <= 1.0, f"{what}: layer {l} of {len(slices)}, row {r}, column {c}: got {a!r}, want {b!r}, {ratio:.3g} x the per-layer bar (rtol {rtol})"


def structural_zero_mask(want_f32, slices):
    """boolean mask over the network's parameters: True in whole rows and whole columns that are exactly zero in the oracle's fp32 gradient"""
    mask = np.zeros(sum(r * c for _, r, c in slices), dtype=bool)
    for (o, r, c), b in zip(slices, _layers(want_f32, slices)):
        m = np.zeros((r, c), dtype=bool)
        m[~np.any(b != 0, axis=1), :] = True
        m[:, ~np.any(b != 0, axis=0)] = True
        mask[o:o + r * c] = m.ravel()
    return mask


def assert_structural_zeros(got, want_f32, slices, what=""):
    """rows and columns the oracle leaves exactly zero (padded output rows, zero-padded input columns) are +-0 in `got`, bit for bit"""
    got = np.asarray(got)
    n = sum(r * c for _, r, c in slices)
    mask = structural_zero_mask(want_f32, slices)
    if got.dtype == np.uint16:
        bad = mask & ((got[:n] & 0x7FFF) != 0)
    else:
        bad = mask & ~(got[:n] == 0)  # NaN is not zero
    if np.any(bad):
        i = int(np.flatnonzero(bad)[0])
        l = max(k for k, (o, _, _) in enumerate(slices) if o <= i)
        o, _, c = slices[l]
        raise AssertionError(f"{what}: layer {l}, row {(i - o) // c}, column {(i - o) % c}: {got[i]!r} where the gradient is structurally zero "
                             f"({int(np.count_nonzero(bad))} such elements)")


def subnormal_share(grads_half_bits, slices):
    """per layer the share of the non-zero half gradients that are fp16 subnormals"""
    out = []
    for b in _layers(np.asarray(grads_half_bits, dtype=np.uint16), slices):
        mag = b & 0x7FFF
        nz = np.count_nonzero(mag)
        out.append(float(np.count_nonzero((mag != 0) & (mag < 0x0400))) / max(nz, 1))
    return out


# ---------------------------------------------------------------------------------------------------- the float64 yardstick
def _h(a, rounding):
    """what the reference keeps as a half: rounded to fp16 (as float64 again), or left alone when `rounding` is off"""
    return a.astype(np.float16).astype(np.float64) if rounding else a


def loss_gradient(loss, pred, target, n_out, loss_scale=128.0, data_pdf=None, rounding=True):
    """dL/d(prediction) of L2 / RelativeL2 in float32 as the reference's loss kernels form it, [n][padded], zero beyond n_out"""
    n, padded = pred.shape
    p = pred[:, :n_out].astype(np.float32)
    d = p - np.asarray(target, dtype=np.float32)
    pdf = np.float32(1) if data_pdf is None else np.asarray(data_pdf, dtype=np.float32)
    if loss.lower() == "relativel2":
        g = np.float32(2) * d / (p * p + np.float32(0.01)) / pdf
    elif loss.lower() == "l2":
        g = np.float32(2) * d / pdf
    else:
        raise ValueError(loss)
    out = np.zeros((n, padded), dtype=np.float64)
    out[:, :n_out] = _h((np.float32(loss_scale) * g / np.float32(n * n_out)).astype(np.float64), rounding)
    return out


def float64_step(x_half, params_half, slices, activation, output_activation="None", *, external_dL_dy=None, loss=None, target=None, n_out=None,
                 data_pdf=None, loss_scale=128.0, rounding=True):
    """Forward, loss gradient and backward of the MLP with float64 sums, and an fp16 rounding wherever the reference stores a half
    (pre-activations, activations, dL/dhidden): the reference's arithmetic with another summation order -- which is how a matrix-core kernel
    differs from the oracle.  x_half: [n][in] values of the network's (encoded) input; params_half: the half weights' values; hidden
    activation ReLU, LeakyReLU or None; output activation None, ReLU or Sigmoid.  rounding=False leaves every value unrounded (the exact
    setting's test asks whether rounding would have changed anything).
    Returns {"grads": float64 [n_params], "ins": per layer its input, "douts": per layer dL/d(its pre-activation), "out"}."""
    act, oact = activation.lower(), output_activation.lower()
    if act not in ("relu", "leakyrelu", "none") or oact not in ("none", "relu", "sigmoid"):
        raise ValueError("float64_step restates piecewise-linear hidden activations (and a None / ReLU / Sigmoid output) only")
    Ws = [w.astype(np.float64) for w in _layers(np.asarray(params_half, dtype=np.float64), slices)]
    slope = _h(np.array(0.01), rounding)

    def fwd(name, pre):
        if name == "relu":
            return np.where(pre > 0, pre, 0.0)
        if name == "leakyrelu":
            return _h(pre * np.where(pre > 0, 1.0, slope), rounding)
        if name == "sigmoid":
            return _h((1.0 / (1.0 + np.exp(-pre.astype(np.float32)))).astype(np.float64), rounding)
        return pre

    def bwd(name, g, y):
        if name == "relu":
            return np.where(y > 0, g, 0.0)
        if name == "leakyrelu":
            return _h(g * np.where(y > 0, 1.0, slope), rounding)
        if name == "sigmoid":
            return _h(g * _h(y * _h((1.0 - y.astype(np.float32)).astype(np.float64), rounding), rounding), rounding)
        return g

    h = np.asarray(x_half, dtype=np.float64)
    ins = []
    for l, W in enumerate(Ws):
        ins.append(h)
        pre = _h(h @ W.T, rounding)
        h = fwd(oact if l == len(Ws) - 1 else act, pre)
    out = h
    if external_dL_dy is not None:
        g = np.asarray(external_dL_dy, dtype=np.float64)
    else:
        g = loss_gradient(loss, out, target, n_out, loss_scale, data_pdf, rounding)
    g = bwd(oact, g, out)
    douts, grads = [None] * len(Ws), [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        douts[l] = g
        grads[l] = g.T @ ins[l]
        if l > 0:
            g = bwd(act, _h(g @ Ws[l], rounding), ins[l])
    return {"grads": np.concatenate([g_.ravel() for g_ in grads]), "ins": ins, "douts": douts, "out": out}


# ---------------------------------------------------------------------------------------------------- the exact setting
def exact_case(n_in, width, hidden, act, n_out, n, x_levels=4, dy_den=8, nonzero=1 / 8, out_nonzero=1 / 2, seed=5):
    """Inputs that make a training step's weight gradients exact: Identity-encoded x in {0, 1/4, 1/2, 3/4} (x_levels = 2: {0, 1/2}), weights
    in {-1, 0, 1} with a share `nonzero` of non-zeros (`out_nonzero` in the last matrix, so that most hidden units reach an output), external dL/dy in multiples of 1/dy_den within +-2, zero in every 7th row and beyond
    n_out.  Every fp32 sum is then exact in any order, ReLU cannot flip, and the one rounding to half is determined --
    tests/test_grad_checks.py proves these conditions on the CPU for every case a GPU test uses."""
    return {"n_in": n_in, "width": width, "hidden": hidden, "act": act, "n_out": n_out, "n": n, "x_levels": x_levels, "dy_den": dy_den, "nonzero": nonzero, "out_nonzero": out_nonzero, "seed": seed}


def exact_case_id(c):
    return f"{c['n_in']}x{c['width']}x{c['hidden']}_{c['act'].lower()}_o{c['n_out']}_n{c['n']}"


def exact_case_config(c):
    otype = "FullyFusedMLP" if c["width"] in (16, 32, 64, 128) and c["hidden"] > 0 else "CutlassMLP"
    return {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6},
            "encoding": {"otype": "Identity"},
            "network": {"otype": otype, "activation": c["act"], "output_activation": "None", "n_neurons": c["width"], "n_hidden_layers": c["hidden"]}}


def exact_case_inputs(c, n_params, padded_out):
    """(weights float32 [n_params], x float32 [n][n_in], dL/dy float32 [n][padded_out]) of an exact case"""
    rs = np.random.RandomState(c["seed"])
    nz, nzo = c["nonzero"], c["out_nonzero"]
    w = rs.choice([-1.0, 0.0, 1.0], size=n_params, p=[nz / 2, 1 - nz, nz / 2]).astype(np.float32)
    n_last = padded_out * (c["width"] if c["hidden"] > 0 else c["n_in"])
    w[n_params - n_last:] = rs.choice([-1.0, 0.0, 1.0], size=n_last, p=[nzo / 2, 1 - nzo, nzo / 2])
    step = 1.0 / 4 if c["x_levels"] == 4 else 1.0 / 2
    x = (rs.randint(0, c["x_levels"], size=(c["n"], c["n_in"])) * step).astype(np.float32)
    dy = (rs.randint(-2 * c["dy_den"], 2 * c["dy_den"] + 1, size=(c["n"], padded_out)) / float(c["dy_den"])).astype(np.float32)
    dy[::7] = 0
    dy[:, c["n_out"]:] = 0
    return w, np.ascontiguousarray(x), np.ascontiguousarray(dy)


def _quantum(a):
    """the largest power of two that divides every non-zero element of a float64 array"""
    nz = a[a != 0]
    if nz.size == 0:
        return 1.0
    m, e = np.frexp(nz)  # nz = m 2^e, 0.5 <= |m| < 1; the mantissa's lowest set bit
    mi = np.abs(m * 2.0 ** 53).astype(np.uint64)
    low = (mi & (~mi + np.uint64(1))).astype(np.float64)
    return float(np.min(low * 2.0 ** (e.astype(np.float64) - 53)))


def exactness_report(c, params_half, x, dy, slices):
    """The conditions of the exact setting, from unrounded float64 values.  Returns {"representable", "max_log2_terms", "max_abs_grad", "grads"}:
    every activation and every dL/dhidden is an fp16 value; the worst, over all weights and all matrix-vector sums, of
    log2(sum |a_i| |b_i| / quantum) (below 24: every fp32 partial sum is exact in any order); max |dW|; and dW itself, unrounded."""
    st = float64_step(x, params_half, slices, c["act"], external_dL_dy=dy, rounding=False)
    vals = st["ins"] + st["douts"] + [st["out"]]
    representable = all(np.array_equal(v.astype(np.float16).astype(np.float64), v) for v in vals)
    Ws = _layers(np.asarray(params_half, dtype=np.float64), slices)
    worst = 0.0
    for W, a, g in zip(Ws, st["ins"], st["douts"]):
        aw, ag, absW = np.abs(a), np.abs(g), np.abs(W)
        qa, qg = _quantum(a), _quantum(g)
        worst = max(worst, float(np.max(ag.T @ aw)) / (qa * qg))     # weight gradient: sum over the batch
        worst = max(worst, float(np.max(aw @ absW.T)) / qa)          # forward: sum over the layer's inputs (weights are -1, 0, 1)
        worst = max(worst, float(np.max(ag @ absW)) / qg)            # backward: sum over the layer's outputs
    return {"representable": representable, "max_log2_terms": float(np.log2(max(worst, 1.0))), "max_abs_grad": float(np.max(np.abs(st["grads"]))), "grads": st["grads"]}
