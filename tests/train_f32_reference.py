"""The yardstick of full-precision training: the nine losses (losses/*.h) and every optimizer (optimizers/*.h) restated in numpy, every
array and every operation in np.float32, op by op in the reference's order -- what Loss<float> and Optimizer<float> compute when IEEE
operations are not contracted.  Never the code under test; no GPU in here.

Pinned on the CPU by tests/test_fp32_training.py: with weight dtype half it reproduces oracle.py's optimizers bit for bit, and the float
loss on half-representable predictions gives the oracle's values, and gradients whose rounding to half gives the oracle's bits.

dtype parameters: `wdtype` is the optimizer's weight type W (np.float16: a half working copy beside the fp32 master weights; np.float32:
ONE float vector), `gdtype` the gradients' (np.float16 values arrive as float32 arrays holding halves; it only matters to Batched, which
rounds its mean to half on the way to the nested optimizer when the gradients are half)."""
import numpy as np

F = np.float32
ONE = F(1)


def _f(a):
    return np.asarray(a, dtype=F)


# ------------------------------------------------------------------------------------------------------------------------ losses
LOSSES = ("L2", "RelativeL2", "RelativeL2Luminance", "L1", "RelativeL1", "Mape", "Smape", "CrossEntropy", "Variance")


def loss(loss_type, prediction, target, loss_scale, data_pdf=None):
    """prediction [n][stride] float32 (the padded output), target / data_pdf [n][dims].  Returns (values, gradients), both [n][stride] float32:
    the reference's expressions in fp32; padded columns 0.  The gradient is loss_scale * gradient / n_total as a float (P = float: the cast
    is no rounding; round it to half for P = half)."""
    name = loss_type.lower()
    assert name in [l.lower() for l in LOSSES], loss_type
    pred_all = _f(prediction)
    n, stride = pred_all.shape
    target = _f(target)
    dims = target.shape[1]
    pred = pred_all[:, :dims]
    pdf = np.ones_like(target) if data_pdf is None else _f(data_pdf)
    n_total = F(n * dims)  # (float)n_total of the kernel's uint32: exact
    ls = F(loss_scale)
    difference = pred - target
    own_n_total = False
    with np.errstate(all="ignore"):
        if name in ("relativel2", "relativel2luminance"):
            if name == "relativel2":
                base = pred
            else:
                r, g, b = pred_all[:, 0], pred_all[:, 1], pred_all[:, 2]
                if dims >= 6:
                    r, g, b = r + pred_all[:, 3], g + pred_all[:, 4], b + pred_all[:, 5]
                base = ((F(0.299) * r + F(0.587) * g) + F(0.114) * b)[:, None]
            sq = base * base + F(0.01)
            value = difference * difference / sq / pdf / n_total
            gradient = F(2) * difference / sq / pdf
        elif name == "l1":
            value = np.abs(difference) / pdf / n_total
            gradient = np.copysign(ONE / pdf, difference)
        elif name in ("relativel1", "mape", "smape"):
            if name == "relativel1":
                denominator = np.abs(pred) + F(1e-2)
            elif name == "mape":
                denominator = np.abs(target) + F(1e-2)
            else:
                denominator = F(0.5) * (np.abs(target) + np.abs(pred)) + F(1e-2)
            scale = ONE / denominator / pdf
            value = np.abs(difference) * scale / n_total
            gradient = np.copysign(scale, difference)
        elif name == "crossentropy":
            factor = -target / pdf / n_total
            value = factor * np.log(pred)
            gradient = factor / pred
            own_n_total = True
        elif name == "variance":
            factor = target * target / pdf / n_total
            value = factor / pred - factor / pdf
            gradient = -factor / (pred * pred)
            own_n_total = True
        else:
            value = difference * difference / pdf / n_total
            gradient = F(2) * difference / pdf
        gradient = ls * gradient if own_n_total else ls * gradient / n_total
    values, grads = np.zeros((n, stride), dtype=F), np.zeros((n, stride), dtype=F)
    values[:, :dims] = value
    grads[:, :dims] = gradient
    assert value.dtype == F and gradient.dtype == F
    return values, grads


def loss_float64(loss_type, prediction, target, data_pdf=None):
    """the VALUES in float64 (for CrossEntropy, whose logf is not correctly rounded on any device), [n][dims]"""
    assert loss_type.lower() == "crossentropy"
    target = np.asarray(target, dtype=np.float64)
    pred = np.asarray(prediction, dtype=np.float64)[:, : target.shape[1]]
    pdf = np.ones_like(target) if data_pdf is None else np.asarray(data_pdf, dtype=np.float64)
    return -target / pdf / target.size * np.log(pred)


# -------------------------------------------------------------------------------------------------------------------- optimizers
def _ci(d, key, default):
    for k, v in d.items():
        if k.lower() == key.lower():
            return v
    return default


def _store(w, new, mask=None):
    """the working copy of the new weights: (W)new_weight.  w is None for W = float (the master vector is the working vector)."""
    if w is None:
        return
    if mask is None:
        w[:] = new.astype(w.dtype)
    else:
        w[mask] = new[mask].astype(w.dtype)


class Adam:
    """optimizers/adam.h:48-188 (this fork: a non-matrix parameter with a zero gradient is skipped and has a step count of its own)"""

    def __init__(self, cfg, wdtype, gdtype):
        g = lambda k, d: F(_ci(cfg, k, d))
        self.lr, self.beta1, self.beta2, self.epsilon, self.l2_reg = g("learning_rate", 1e-3), g("beta1", 0.9), g("beta2", 0.999), g("epsilon", 1e-8), g("l2_reg", 1e-8)
        self.relative_decay, self.absolute_decay, self.clipping = g("relative_decay", 0.0), g("absolute_decay", 0.0), g("clipping_magnitude", 0.0)
        self.non_matrix_factor = g("non_matrix_learning_rate_factor", 1.0)
        self.adabound = bool(_ci(cfg, "adabound", False))
        self.opt_matrix, self.opt_non_matrix = bool(_ci(cfg, "optimize_matrix_params", True)), bool(_ci(cfg, "optimize_non_matrix_params", True))
        self.current_step = 0

    def allocate(self, n, layer_sizes):
        self.n = n
        self.m1, self.m2 = np.zeros(n, dtype=F), np.zeros(n, dtype=F)
        self.steps = np.zeros(n, dtype=np.uint32)
        self.n_matrix = int(sum(int(r) * int(c) for r, c in layer_sizes))

    def _debias(self, t):  # adam.h:97-98, scalar float32 operations
        t = F(t)
        return np.sqrt(ONE - np.power(self.beta2, t)) / (ONE - np.power(self.beta1, t))

    def step(self, loss_scale, w_fp, w, g):
        self.current_step += 1
        lower, upper = F(0), np.finfo(F).max
        if self.adabound:  # adam.h:157-160
            lower = F(0.1) - F(0.1) / ((ONE - self.beta2) * F(self.current_step) + ONE)
            upper = F(0.1) + F(0.1) / ((ONE - self.beta2) * F(self.current_step))
        is_matrix = np.arange(self.n) < self.n_matrix
        with np.errstate(all="ignore"):
            gradient = _f(g) / F(loss_scale)
            updated = np.where(is_matrix, self.opt_matrix, self.opt_non_matrix & (gradient != 0))
            weight = w_fp.copy()
            gradient = np.where(is_matrix, gradient + self.l2_reg * weight, gradient)
            gradient_sq = gradient * gradient
            first = self.beta1 * self.m1 + (ONE - self.beta1) * gradient
            second = self.beta2 * self.m2 + (ONE - self.beta2) * gradient_sq
            lr = np.where(is_matrix, self.lr, self.lr * self.non_matrix_factor).astype(F)
            step = self.steps + np.uint32(1)
            debias = np.zeros(self.n, dtype=F)  # (of the updated parameters; the others' results are dropped)
            for t in np.unique(step[updated]):
                debias[step == t] = self._debias(int(t))
            lr = lr * debias
            effective = np.minimum(np.maximum(lr / (np.sqrt(second) + self.epsilon), lower), upper)
            decayed = (ONE - self.relative_decay * lr) * weight - np.copysign(self.absolute_decay * lr, weight)
            new = decayed - effective * first
            if self.clipping != 0:
                new = np.minimum(np.maximum(new, -self.clipping), self.clipping)
        for a in (first, second, new):
            assert a.dtype == F
        w_fp[updated] = new[updated]
        self.m1[updated] = first[updated]
        self.m2[updated] = second[updated]
        self.steps[updated] = step[updated]
        _store(w, new, updated)

    def learning_rate(self):
        return float(self.lr)

    def set_learning_rate(self, v):
        self.lr = F(v)

    def step_count(self):
        return self.current_step

    def custom_weights(self):
        return None


class Sgd:
    """optimizers/sgd.h:44-72"""

    def __init__(self, cfg, wdtype, gdtype):
        self.lr, self.l2_reg = F(_ci(cfg, "learning_rate", 1e-3)), F(_ci(cfg, "l2_reg", 1e-8))
        self.current_step = 0

    def allocate(self, n, layer_sizes):
        self.n = n

    def step(self, loss_scale, w_fp, w, g):
        self.current_step += 1
        gradient = _f(g) / F(loss_scale)
        gradient = gradient + self.l2_reg * w_fp
        new = w_fp - self.lr * gradient
        assert new.dtype == F
        w_fp[:] = new
        _store(w, new)

    def learning_rate(self):
        return float(self.lr)

    def set_learning_rate(self, v):
        self.lr = F(v)

    def step_count(self):
        return self.current_step

    def custom_weights(self):
        return None


class Novograd:
    """optimizers/novograd.h:44-167: one second moment per layer; only the weight matrices are walked"""

    def __init__(self, cfg, wdtype, gdtype):
        g = lambda k, d: F(_ci(cfg, k, d))
        self.lr, self.beta1, self.beta2, self.epsilon = g("learning_rate", 1e-3), g("beta1", 0.9), g("beta2", 0.999), g("epsilon", 1e-8)
        self.relative_decay, self.absolute_decay = g("relative_decay", 0.0), g("absolute_decay", 0.0)
        self.current_step = 0

    def allocate(self, n, layer_sizes):
        self.layers = [int(r) * int(c) for r, c in layer_sizes]
        self.first = np.zeros(n, dtype=F)
        self.second = np.zeros(len(self.layers), dtype=F)

    def step(self, loss_scale, w_fp, w, g):
        self.current_step += 1
        ls = F(loss_scale)
        beta1 = F(0) if self.current_step == 1 else self.beta1  # exact values on the first step
        beta2 = F(0) if self.current_step == 1 else self.beta2
        off = 0
        for i, size in enumerate(self.layers):
            sl = slice(off, off + size)
            gl = _f(g[sl])
            norm = F(np.sum(gl * gl, dtype=F))  # an fp32 sum whose order is not specified
            self.second[i] = beta2 * self.second[i] + (ONE - beta2) * norm / ls / ls
            gradient = gl / ls
            first = beta1 * self.first[sl] + (ONE - beta1) * gradient / (np.sqrt(self.second[i]) + self.epsilon)
            self.first[sl] = first
            weight = w_fp[sl]
            decayed = (ONE - self.relative_decay * self.lr) * weight - np.copysign(self.absolute_decay * self.lr, weight)
            new = decayed - self.lr * first
            assert new.dtype == F
            w_fp[sl] = new
            if w is not None:
                w[sl] = new.astype(w.dtype)
            off += size

    def learning_rate(self):
        return float(self.lr)

    def set_learning_rate(self, v):
        self.lr = F(v)

    def step_count(self):
        return self.current_step

    def custom_weights(self):
        return None


class _Wrapper:
    def learning_rate(self):
        return self.nested.learning_rate()

    def set_learning_rate(self, v):
        self.nested.set_learning_rate(v)

    def step_count(self):
        return self.nested.step_count()

    def custom_weights(self):
        return self.nested.custom_weights()


class ExponentialDecay(_Wrapper):
    """optimizers/exponential_decay.h:45-160"""

    def __init__(self, cfg, wdtype, gdtype):
        self.nested = create_optimizer(_ci(cfg, "nested", {}), wdtype, gdtype)
        self.decay_base = F(_ci(cfg, "decay_base", 0.1))
        self.decay_interval, self.decay_start, self.decay_end = int(_ci(cfg, "decay_interval", 10000)), int(_ci(cfg, "decay_start", 10000)), int(_ci(cfg, "decay_end", 10000000))
        self.factor = F(1.0)
        self.base_lr = F(self.nested.learning_rate())

    def allocate(self, n, layer_sizes):
        self.nested.allocate(n, layer_sizes)

    def step(self, loss_scale, w_fp, w, g):
        s = self.step_count()
        if s == 0:
            self.factor = F(1.0)
        if s >= self.decay_start and (s - self.decay_start) % self.decay_interval == 0 and s <= self.decay_end:
            self.factor = F(self.factor * self.decay_base)
        self.nested.set_learning_rate(F(self.base_lr * self.factor))
        self.nested.step(loss_scale, w_fp, w, g)

    def learning_rate(self):
        return float(F(self.base_lr * self.factor))

    def set_learning_rate(self, v):
        self.base_lr = F(F(v) / self.factor)
        self.nested.set_learning_rate(F(self.base_lr * self.factor))


class Ema(_Wrapper):
    """optimizers/ema.h:44-132: the debiased moving average of the weights, kept as W (with full_precision and W = half: also in fp32)"""

    def __init__(self, cfg, wdtype, gdtype):
        self.nested = create_optimizer(_ci(cfg, "nested", {}), wdtype, gdtype)
        self.decay = F(_ci(cfg, "decay", 0.99))
        self.full_precision = bool(_ci(cfg, "full_precision", False))
        self.wdtype = wdtype

    def allocate(self, n, layer_sizes):
        self.nested.allocate(n, layer_sizes)
        self.weights_ema = np.zeros(n, dtype=self.wdtype)
        self.tmp = np.zeros(n, dtype=F) if self.full_precision else None

    def step(self, loss_scale, w_fp, w, g):
        self.nested.step(loss_scale, w_fp, w, g)
        s = self.nested.step_count()
        debias_old = ONE - F(float(self.decay) ** (s - 1))  # ema.h:103-104: std::pow(float, uint32_t) in double, rounded to float
        debias_new = ONE / (ONE - F(float(self.decay) ** s))
        weights = self.nested.custom_weights()
        if weights is None:
            weights = w_fp if w is None else w  # reads weights[i] as W
        previous = self.tmp if self.full_precision else self.weights_ema.astype(F)
        filtered = (previous * self.decay * debias_old + weights.astype(F) * (ONE - self.decay)) * debias_new
        assert filtered.dtype == F
        if self.full_precision:
            self.tmp[:] = filtered
        self.weights_ema[:] = filtered.astype(self.wdtype)

    def custom_weights(self):
        return self.weights_ema


class Average(_Wrapper):
    """optimizers/average.h:44-124: the mean of the weights after each of the last n_samples steps, kept as W"""

    def __init__(self, cfg, wdtype, gdtype):
        self.nested = create_optimizer(_ci(cfg, "nested", {}), wdtype, gdtype)
        self.n_samples = int(_ci(cfg, "n_samples", 128))
        self.wdtype = wdtype

    def allocate(self, n, layer_sizes):
        self.nested.allocate(n, layer_sizes)
        self.samples = np.zeros((self.n_samples, n), dtype=self.wdtype)
        self.average = np.zeros(n, dtype=self.wdtype)

    def step(self, loss_scale, w_fp, w, g):
        self.nested.step(loss_scale, w_fp, w, g)
        weights = w_fp if w is None else w
        cur = self.samples[self.step_count() % self.n_samples]
        delta = (weights.astype(F) - cur.astype(F)) / F(self.n_samples)
        self.average[:] = (self.average.astype(F) + delta).astype(self.wdtype)
        cur[:] = weights

    def custom_weights(self):
        return self.average


class Batched(_Wrapper):
    """optimizers/batched.h:44-89: the nested optimizer steps once per batch_size_multiplier calls, on the mean gradient (fp32 gradients
    reach it as the fp32 mean; half gradients as that mean rounded to half)"""

    def __init__(self, cfg, wdtype, gdtype):
        self.nested = create_optimizer(_ci(cfg, "nested", {}), wdtype, gdtype)
        self.multiplier = int(_ci(cfg, "batch_size_multiplier", 16))
        self.gdtype = gdtype
        self.current_step = 0

    def allocate(self, n, layer_sizes):
        self.nested.allocate(n, layer_sizes)
        self.pool = np.zeros(n, dtype=F)

    def step(self, loss_scale, w_fp, w, g):
        if self.current_step % self.multiplier == 0:
            self.pool[:] = 0
        self.pool += _f(g) / F(self.multiplier)
        self.current_step += 1
        if self.current_step % self.multiplier == 0:
            mean = self.pool.astype(np.float16).astype(F) if self.gdtype == np.float16 else self.pool
            self.nested.step(loss_scale, w_fp, w, mean)

    def step_count(self):
        return self.current_step


class Lookahead(_Wrapper):
    """optimizers/lookahead.h:44-98: slow weights (kept as W) <- slow (1 - alpha) + fast alpha every n_steps steps; the fast ones restart there"""

    def __init__(self, cfg, wdtype, gdtype):
        self.nested = create_optimizer(_ci(cfg, "nested", {}), wdtype, gdtype)
        self.alpha = F(_ci(cfg, "alpha", 0.5))
        self.n_steps = int(_ci(cfg, "n_steps", 16))
        self.wdtype = wdtype

    def allocate(self, n, layer_sizes):
        self.nested.allocate(n, layer_sizes)
        self.lookahead = np.zeros(n, dtype=self.wdtype)

    def step(self, loss_scale, w_fp, w, g):
        s = self.nested.step_count()
        if s == 0:
            self.lookahead[:] = w_fp if w is None else w
        if s % self.n_steps == 0:
            new = self.lookahead.astype(F) * (ONE - self.alpha) + w_fp * self.alpha
            assert new.dtype == F
            w_fp[:] = new
            self.lookahead[:] = new.astype(self.wdtype)
            if w is not None:
                w[:] = self.lookahead
        self.nested.step(loss_scale, w_fp, w, g)

    def custom_weights(self):
        return self.lookahead


def slice_layer_sizes(layer_sizes, offset):
    out, pos = [], 0
    for r, c in layer_sizes:
        if pos < offset < pos + r * c:
            raise RuntimeError("Invalid slice. Can't slice within a layer.")
        if pos >= offset:
            out.append((r, c))
        pos += r * c
    return out


class Composite:
    """optimizers/composite.h:76-135: nested[i] owns the next n_params_to_optimize weights; the custom weights are gathered"""

    def __init__(self, cfg, wdtype, gdtype):
        self.offsets, self.nested = [0], []
        for c in _ci(cfg, "nested", None):
            self.nested.append(create_optimizer(c, wdtype, gdtype))
            self.offsets.append(self.offsets[-1] + int(_ci(c, "n_params_to_optimize", 0)))
        self.wdtype = wdtype
        self.custom = None

    def allocate(self, n, layer_sizes):
        for i, o in enumerate(self.nested):
            o.allocate(self.offsets[i + 1] - self.offsets[i], slice_layer_sizes(layer_sizes, self.offsets[i]))
        if any(o.custom_weights() is not None for o in self.nested):
            self.custom = np.zeros(n, dtype=self.wdtype)

    def step(self, loss_scale, w_fp, w, g):
        weights = w_fp if w is None else w
        for i, o in enumerate(self.nested):
            a, b = self.offsets[i], self.offsets[i + 1]
            o.step(loss_scale, w_fp[a:b], None if w is None else w[a:b], g[a:b])
            if self.custom is not None:
                self.custom[a:b] = weights[a:b] if o.custom_weights() is None else o.custom_weights()
        if self.custom is not None:
            self.custom[self.offsets[-1]:] = weights[self.offsets[-1]:]

    def learning_rate(self):
        return 1.0

    def step_count(self):
        return self.nested[0].step_count()

    def custom_weights(self):
        return self.custom


_OPTIMIZERS = {"adam": Adam, "sgd": Sgd, "novograd": Novograd, "exponentialdecay": ExponentialDecay, "ema": Ema, "average": Average, "batched": Batched,
               "lookahead": Lookahead, "composite": Composite}


def create_optimizer(cfg, wdtype=np.float32, gdtype=np.float32):
    """wdtype: np.float16 or np.float32 (step(loss_scale, w_fp, w, g): w is the float16 working copy, or None for float32 weights);
    g: float32 values (for gdtype np.float16: halves held in a float32 array)"""
    assert wdtype in (np.float16, np.float32) and gdtype in (np.float16, np.float32)
    assert not (wdtype == np.float32 and gdtype == np.float16), "float weights imply fp32 gradients"
    return _OPTIMIZERS[str(_ci(cfg, "otype", "Adam")).lower()](cfg, wdtype, gdtype)
