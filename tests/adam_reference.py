"""One Adam step (optimizers/adam.h:48-188) held per element: inputs that reach every branch of adam_one, the option sets one by one, and
assert_adam_step, which compares the state after one step on two sides -- an implementation and a reference -- from the state before it.

The only arithmetic of the step that is not an IEEE operation is powf in the debiasing factor sqrtf(1 - powf(beta2, t)) / (1 - powf(beta1, t)),
common to all parameters with the same count t.  Both sides are built without contraction, so the moments and the counts are compared bit for
bit, and the weights within what K_POWF + K_HOST float steps in each powf can move the factor (eps_t below).

K_POWF is measured on the device against float64 rounded once (tools/libm_f32_ulp.py, profiles/libm_f32_ulp.txt); K_HOST is computed by the
test from the host's own powf against the same yardstick (k_host).  No kernel of the project in here, and no GPU.
"""
import numpy as np

F = np.float32
D = np.float64
U = 2.0 ** -24  # half a float step, relative

K_POWF = 1  # measured, profiles/libm_f32_ulp.txt: the device's powf(beta, t) over BETAS x POW_STEPS, worst distance in float steps, as it is

BETAS = (0.9, 0.99, 0.8, 0.95, 0.999)  # every beta1 / beta2 a test of the suite sets
POW_STEPS = range(1, 65)

BASE = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8, "l2_reg": 0.0}
NUMERIC = {"l2_reg": 1e-2, "relative_decay": 0.05, "absolute_decay": 1e-3, "clipping_magnitude": 0.3, "adabound": True,
           "non_matrix_learning_rate_factor": 0.25, "epsilon": 1e-3}
OPTION_SETS = {"base": dict(BASE), **{k: {**BASE, k: v} for k, v in NUMERIC.items()},
               "frozen_matrix": {**BASE, "optimize_matrix_params": False}, "frozen_grid": {**BASE, "optimize_non_matrix_params": False},
               "full": {**BASE, **NUMERIC}}
FULL = OPTION_SETS["full"]
DEFAULTS = {"relative_decay": 0.0, "absolute_decay": 0.0, "clipping_magnitude": 0.0, "non_matrix_learning_rate_factor": 1.0, "adabound": False,
            "optimize_matrix_params": True, "optimize_non_matrix_params": True}
MID_RUN_CHANGE = {"beta1": 0.8, "beta2": 0.95, "learning_rate": 3e-3}

N_STEPS = 5
SENTINEL = np.uint16(0x3E00)  # 1.5 as a half: no weight of these tests is near it
STANDARD = (8195, [(16, 31), (31, 9)])  # n_matrix = 775 is no multiple of 4, and 3 parameters form a ragged tail


def n_matrix_of(layers):
    return int(sum(int(r) * int(c) for r, c in layers))


def option(cfg, key):
    return cfg.get(key, DEFAULTS[key]) if key in DEFAULTS else cfg[key]


# ------------------------------------------------------------------------------------------------------------------------ inputs
def initial_weights(n, seed=7):
    """uniform in +-0.5; every 11th entry an exact zero, of alternating sign (copysignf(absolute_decay * lr, w) sees both)"""
    w = np.random.RandomState(seed).uniform(-0.5, 0.5, n).astype(F)
    w[3::22] = F(0.0)
    w[14::22] = F(-0.0)
    return w


def gradient_bits(n, n_matrix, step, seed=100):
    """half bits of one step's gradients: magnitudes log-uniform over 2^-24 .. 2^15 (half subnormals to near the half maximum), random signs,
    all finite and none zero -- and then, from the quad that holds the first non-matrix parameter on, a third of the quads all zero, a third
    with exactly one zero lane, the rest untouched.  The thirds and the lane rotate with the step; the zeros alternate between +0.0 and -0.0."""
    rs = np.random.RandomState(seed + step)
    g = np.exp2(rs.uniform(-24.0, 15.0, n)) * np.where(rs.randint(0, 2, n) == 1, -1.0, 1.0)
    bits = g.astype(np.float16).view(np.uint16)
    assert np.all((bits & 0x7FFF) != 0) and np.all((bits & 0x7C00) != 0x7C00)
    i = np.arange(n)
    q = i // 4
    kind = (q + step) % 3
    behind = q >= n_matrix // 4
    zero = behind & ((kind == 0) | ((kind == 1) & (i % 4 == (q // 3 + step) % 4)))
    sign = np.where((q + i + step) % 2 == 1, 0x8000, 0).astype(np.uint16)
    return np.where(zero, sign, bits).astype(np.uint16)


def half_to_float(bits):
    return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(F)


def float_to_half_bits(a):
    return np.ascontiguousarray(a, dtype=F).astype(np.float16).view(np.uint16)


def unscaled(g, loss_scale):
    """the float gradient of adam.h:70 from half bits (uint16) or fp32 gradients"""
    g = half_to_float(g) if g.dtype == np.uint16 else np.asarray(g, dtype=F)
    return g / F(loss_scale)


def skipped_mask(cfg, n, n_matrix, g, loss_scale):
    """adam.h:76-84: the parameters this step leaves alone"""
    is_matrix = np.arange(n) < n_matrix
    return np.where(is_matrix, not option(cfg, "optimize_matrix_params"), (not option(cfg, "optimize_non_matrix_params")) | (unscaled(g, loss_scale) == 0))


def half_with_sentinel(w_fp, skipped):
    """the half working copy in front of a step: the cast of the master weights, and where the step must not store, a value that is NOT that cast"""
    h = float_to_half_bits(w_fp)
    h[skipped] = SENTINEL
    return h


# ---------------------------------------------------------------------------------------------- the host's powf and the tolerance
def float_steps(a, b):
    """distance of positive floats in float steps"""
    return np.abs(np.asarray(a, dtype=F).view(np.int32).astype(np.int64) - np.asarray(b, dtype=F).view(np.int32).astype(np.int64))


def pow_arguments():
    """[(beta, t)] as float32 [m][2]: what adam_debias hands powf in this suite"""
    return np.array([(b, t) for b in BETAS for t in POW_STEPS], dtype=F)


def pow_rounded(args):
    """powf of float32 [m][2] as the float64 value rounded once"""
    a = np.asarray(args, dtype=F).astype(D)
    return np.power(a[:, 0], a[:, 1]).astype(F)


def k_host(powf=None):
    """The host's float32 powf against float64 rounded once over pow_arguments(), in float steps: numpy's (the restatements'), and `powf`
    (a ctypes function float(float, float): the C library's, which the oracle calls) when given."""
    args = pow_arguments()
    want = pow_rounded(args)
    k = int(float_steps(np.power(args[:, 0], args[:, 1]), want).max())
    if powf is not None:
        got = np.array([powf(float(b), float(t)) for b, t in args], dtype=F)
        k = max(k, int(float_steps(got, want).max()))
    return k


def eps_t(beta1, beta2, t, k_powf, k_host_):
    """relative distance allowed between two sides' debiasing factors at count t: K float steps in each powf, propagated to first order
    through sqrtf(1 - p2) / (1 - p1), and 4 for the correctly rounded subtractions, square root and division of the two sides"""
    p1, p2 = np.power(D(F(beta1)), t.astype(D)), np.power(D(F(beta2)), t.astype(D))
    return U * ((k_powf + k_host_) * (0.5 * p2 / (1 - p2) + p1 / (1 - p1)) + 4)


# ------------------------------------------------------------------------------------------------- the restatement, and its mutants
MUTANTS = ("absolute_decay_sign", "l2_reg_on_non_matrix", "factor_ignored", "clip_before_step", "common_step_debias", "negative_zero_is_a_gradient",
           "skipped_half_rewritten", "adabound_previous_step", "frozen_class_moves_moments")


class AdamVariant:
    """adam.h:48-188 in np.float32, op by op -- and, with `mutant`, with exactly one thing wrong.  step() works on copies and returns the state
    after the step: {"w_fp", "w_half" (uint16), "m1", "m2", "steps"}."""

    def __init__(self, cfg, n, n_matrix, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.cfg, self.n, self.n_matrix, self.mutant = dict(cfg), n, n_matrix, mutant
        self.m1, self.m2, self.steps = np.zeros(n, dtype=F), np.zeros(n, dtype=F), np.zeros(n, dtype=np.uint32)
        self.current_step = 0

    def update(self, delta):
        self.cfg.update(delta)

    def step(self, loss_scale, w_fp, w_half, g):
        c, mutant, one = self.cfg, self.mutant, F(1)
        h = lambda k: F(option(c, k))
        self.current_step += 1
        lower, upper = F(0), np.finfo(F).max
        if option(c, "adabound"):
            t = F(self.current_step - 1 if mutant == "adabound_previous_step" else self.current_step)
            with np.errstate(all="ignore"):
                lower, upper = F(0.1) - F(0.1) / ((one - h("beta2")) * t + one), F(0.1) + F(0.1) / ((one - h("beta2")) * t)
        is_matrix = np.arange(self.n) < self.n_matrix
        with np.errstate(all="ignore"):
            gradient = unscaled(g, loss_scale)
            nonzero = gradient != 0
            if mutant == "negative_zero_is_a_gradient":
                nonzero |= np.signbit(gradient)
            updated = np.where(is_matrix, bool(option(c, "optimize_matrix_params")), bool(option(c, "optimize_non_matrix_params")) & nonzero)
            weight = w_fp.copy()
            gradient = gradient + h("l2_reg") * weight if mutant == "l2_reg_on_non_matrix" else np.where(is_matrix, gradient + h("l2_reg") * weight, gradient)
            first = h("beta1") * self.m1 + (one - h("beta1")) * gradient
            second = h("beta2") * self.m2 + (one - h("beta2")) * (gradient * gradient)
            factor = one if mutant == "factor_ignored" else h("non_matrix_learning_rate_factor")
            lr = np.where(is_matrix, h("learning_rate"), h("learning_rate") * factor).astype(F)
            count = self.steps + np.uint32(1)
            own = np.full(self.n, self.current_step, dtype=np.uint32) if mutant == "common_step_debias" else count
            debias = np.zeros(self.n, dtype=F)
            for t in np.unique(own[updated]):
                debias[own == t] = np.sqrt(one - np.power(h("beta2"), F(t))) / (one - np.power(h("beta1"), F(t)))
            lr = lr * debias
            effective = np.minimum(np.maximum(lr / (np.sqrt(second) + h("epsilon")), lower), upper)
            clip = h("clipping_magnitude")
            if mutant == "clip_before_step" and clip != 0:
                weight = np.minimum(np.maximum(weight, -clip), clip)
            absolute = np.copysign(h("absolute_decay") * lr, weight)
            decayed = (one - h("relative_decay") * lr) * weight - (-absolute if mutant == "absolute_decay_sign" else absolute)
            new = decayed - effective * first
            if mutant != "clip_before_step" and clip != 0:
                new = np.minimum(np.maximum(new, -clip), clip)
        moments = updated | ~np.where(is_matrix, bool(option(c, "optimize_matrix_params")), bool(option(c, "optimize_non_matrix_params"))) if mutant == "frozen_class_moves_moments" else updated
        out_fp, out_h = w_fp.copy(), w_half.copy()
        out_fp[updated] = new[updated]
        stored = np.ones(self.n, dtype=bool) if mutant == "skipped_half_rewritten" else updated
        out_h[stored] = float_to_half_bits(out_fp)[stored]
        self.m1[moments], self.m2[moments] = first[moments], second[moments]
        self.steps[updated] = count[updated]
        return {"w_fp": out_fp, "w_half": out_h, "m1": self.m1.copy(), "m2": self.m2.copy(), "steps": self.steps.copy()}


class RestatementSide:
    """tests/train_f32_reference.py's Adam (half weights, half gradients) behind the interface of AdamVariant"""

    def __init__(self, cfg, n, layers):
        import train_f32_reference as tr

        self.opt = tr.create_optimizer(cfg, np.float16, np.float16)
        self.opt.allocate(n, layers)

    def step(self, loss_scale, w_fp, w_half, g):
        assert g.dtype == np.uint16
        w_fp, w = w_fp.copy(), w_half.copy().view(np.float16)
        self.opt.step(loss_scale, w_fp, w, half_to_float(g))
        return {"w_fp": w_fp, "w_half": w.view(np.uint16), "m1": self.opt.m1.copy(), "m2": self.opt.m2.copy(), "steps": self.opt.steps.copy()}


class OracleSide:
    """oracle.py's Adam (orc_adam_step) behind the same interface"""

    def __init__(self, oracle, cfg, n, layers):
        self.opt = oracle.create_optimizer(cfg)
        self.opt.allocate(n, layers)

    def update(self, delta):
        self.opt.update_hyperparams(delta)

    def step(self, loss_scale, w_fp, w_half, g):
        assert g.dtype == np.uint16
        w_fp, w_half = w_fp.copy(), w_half.copy()
        self.opt.step(loss_scale, w_fp, w_half, np.ascontiguousarray(g))
        adams = getattr(self.opt, "nested", [self.opt])  # (a Composite of Adams: the slices' states side by side, zeros behind the last)
        tail = w_fp.size - sum(o.n for o in adams)
        gather = lambda key, dtype: np.concatenate([getattr(o, key) for o in adams] + [np.zeros(tail, dtype=dtype)])
        return {"w_fp": w_fp, "w_half": w_half, "m1": gather("m1", F), "m2": gather("m2", F), "steps": gather("steps", np.uint32)}


# ------------------------------------------------------------------------------------------------------------------ the comparator
def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _changed(before, after):
    return (_bits(before["w_fp"]) != _bits(after["w_fp"])) | (_bits(before["m1"]) != _bits(after["m1"])) | (_bits(before["m2"]) != _bits(after["m2"])) | (before["steps"] != after["steps"])


def step_quantities(cfg, n_matrix, loss_scale, common_step, before, g):
    """what the bound and the exercise assertions need, in float64 from the state before the step: the new first moment, the unclamped and the
    clamped effective rate, the debiased learning rate, each parameter's new count, and the bounds of adabound"""
    h = lambda k: D(F(option(cfg, k)))
    n = before["w_fp"].size
    is_matrix = np.arange(n) < n_matrix
    w = before["w_fp"].astype(D)
    with np.errstate(all="ignore"):
        gradient = unscaled(g, loss_scale).astype(D)
        gradient = np.where(is_matrix, gradient + h("l2_reg") * w, gradient)
        m1 = h("beta1") * before["m1"].astype(D) + (1 - h("beta1")) * gradient
        m2 = h("beta2") * before["m2"].astype(D) + (1 - h("beta2")) * gradient * gradient
        t = before["steps"].astype(np.int64) + 1
        p1, p2 = np.power(h("beta1"), t.astype(D)), np.power(h("beta2"), t.astype(D))
        lr = h("learning_rate") * np.where(is_matrix, 1.0, h("non_matrix_learning_rate_factor")) * np.sqrt(1 - p2) / (1 - p1)
        lower, upper = 0.0, D(np.finfo(F).max)
        if option(cfg, "adabound"):
            lower, upper = 0.1 - 0.1 / ((1 - h("beta2")) * common_step + 1), 0.1 + 0.1 / ((1 - h("beta2")) * common_step)
        raw = lr / (np.sqrt(m2) + h("epsilon"))
        eff = np.minimum(np.maximum(raw, lower), upper)
    return {"w": w, "m1": m1, "raw": raw, "eff": eff, "lr": lr, "t": t, "lower": lower, "upper": upper}


def assert_adam_step(cfg, n_matrix, loss_scale, common_step, before, g, got, want, k_powf, k_host_, what=""):
    """One step from `before` with gradients g (half bits, or fp32 values), as `got` (the implementation) and `want` (the reference) left it:
    states {"w_fp", "w_half" (uint16), "m1", "m2", "steps"}.  common_step: the optimizer's own count of this step.  Returns the largest
    ratio of a weight's error to its bound (measured before the weights are asserted)."""
    n = before["w_fp"].size
    for key in ("m1", "m2"):
        bad = np.flatnonzero(_bits(got[key]) != _bits(want[key]))
        assert bad.size == 0, f"{what}: {key} differs in {bad.size} places, first at {bad[0]}: {got[key][bad[0]]!r} != {want[key][bad[0]]!r}"
    bad = np.flatnonzero(np.asarray(got["steps"], dtype=np.uint32) != want["steps"])
    assert bad.size == 0, f"{what}: step counts differ in {bad.size} places, first at {bad[0]}: {got['steps'][bad[0]]} != {want['steps'][bad[0]]}"
    changed_got, changed = _changed(before, got), _changed(before, want)
    bad = np.flatnonzero(changed_got != changed)
    assert bad.size == 0, f"{what}: the set of parameters the step changed differs in {bad.size} places, first at {bad[0]}"
    updated = want["steps"] != before["steps"]
    assert np.array_equal(updated, changed)  # (an updated parameter's count always moves)
    assert np.all(np.isfinite(want["w_fp"])) and np.all(np.isfinite(got["w_fp"])), what
    # fp32 weights, per element
    q = step_quantities(cfg, n_matrix, loss_scale, common_step, before, g)
    e = eps_t(option(cfg, "beta1"), option(cfg, "beta2"), q["t"], k_powf, k_host_)
    h = lambda k: D(F(option(cfg, k)))
    move = np.abs(q["eff"] * q["m1"])
    bound = e * (move + q["lr"] * (h("relative_decay") * np.abs(q["w"]) + h("absolute_decay"))) + 4 * U * np.maximum(np.abs(q["w"]), move)
    err = np.abs(got["w_fp"].astype(D) - want["w_fp"].astype(D))
    ratio = float(np.max(np.where(updated, err / np.maximum(bound, 1e-300), 0.0))) if updated.any() else 0.0
    bad = np.flatnonzero(updated & ~(err <= bound))
    assert bad.size == 0, (f"{what}: {bad.size} weights beyond their bound, worst {ratio:.3g} x; first at {bad[0]} (count {q['t'][bad[0]]}): "
                           f"{got['w_fp'][bad[0]]!r} against {want['w_fp'][bad[0]]!r}, bound {bound[bad[0]]:.3e}")
    assert np.array_equal(_bits(got["w_fp"])[~updated], _bits(before["w_fp"])[~updated]), what
    clip = F(option(cfg, "clipping_magnitude"))
    if clip != 0:
        on_clip = updated & (np.abs(want["w_fp"]) == clip)
        bad = np.flatnonzero(on_clip & (_bits(got["w_fp"]) != _bits(want["w_fp"])))
        assert bad.size == 0, f"{what}: {bad.size} weights the reference clips are not exactly +-{clip}, first at {bad[0]}: {got['w_fp'][bad[0]]!r}"
    # half weights: the rounding of the implementation's OWN new weight where it updated, untouched bits elsewhere
    own = float_to_half_bits(got["w_fp"])
    bad = np.flatnonzero(updated & (got["w_half"] != own))
    assert bad.size == 0, f"{what}: {bad.size} half weights are not the rounding of the new fp32 weight, first at {bad[0]}"
    bad = np.flatnonzero(~updated & (got["w_half"] != before["w_half"]))
    assert bad.size == 0, f"{what}: {bad.size} half weights of skipped parameters were written, first at {bad[0]}"
    return ratio


class Exercise:
    """What a run's inputs reached, gathered from the reference side alone step by step, and asserted at the end (check)."""

    def __init__(self, cfg):
        self.cfg = dict(cfg)
        self.updated = self.clipped = self.at_lower = self.at_upper = 0
        self.signs = set()
        self.counts = set()

    def step(self, cfg, n_matrix, loss_scale, common_step, before, g, want):
        n = before["w_fp"].size
        is_matrix = np.arange(n) < n_matrix
        updated = want["steps"] != before["steps"]
        changed = _changed(before, want) | (before["w_half"] != want["w_half"])
        if not option(cfg, "optimize_matrix_params"):
            assert not changed[is_matrix].any(), "a frozen matrix weight changed"
        if not option(cfg, "optimize_non_matrix_params"):
            assert not changed[~is_matrix].any(), "a frozen non-matrix parameter changed"
        q = step_quantities(cfg, n_matrix, loss_scale, common_step, before, g)
        self.updated += int(updated.sum())
        clip = F(option(cfg, "clipping_magnitude"))
        if clip != 0:
            self.clipped += int((updated & (np.abs(want["w_fp"]) == clip)).sum())
        self.at_lower += int((updated & (q["raw"] < q["lower"])).sum())
        self.at_upper += int((updated & (q["raw"] > q["upper"])).sum())
        w = before["w_fp"][updated]
        for name, hit in (("+", w > 0), ("-", w < 0), ("+0", (w == 0) & ~np.signbit(w)), ("-0", (w == 0) & np.signbit(w))):
            if hit.any():
                self.signs.add(name)
        self.counts |= set(int(c) for c in np.unique(want["steps"]))

    def check(self, n_steps=N_STEPS):
        cfg = self.cfg
        assert self.updated > 0
        if option(cfg, "clipping_magnitude") != 0:
            share = self.clipped / self.updated
            assert 0.01 < share < 0.99, f"clipping binds for {share:.1%} of the updated parameters"
        if option(cfg, "adabound"):
            lo, hi = self.at_lower / self.updated, self.at_upper / self.updated
            assert lo > 0.01 and hi > 0.01, f"adabound: the lower bound binds for {lo:.1%}, the upper for {hi:.1%}"
        if option(cfg, "absolute_decay") != 0:
            assert self.signs == {"+", "-", "+0", "-0"}, self.signs
        if n_steps >= N_STEPS and option(cfg, "optimize_non_matrix_params"):
            want = {2, 3, 4, 5} if option(cfg, "optimize_matrix_params") else {2, 3, 4}
            assert want <= self.counts, f"step counts {sorted(self.counts)}"


def one_slice(cfg, n, layers):
    """[(offset, count, configuration, matrix weights at the slice's front)]: one Adam on the whole vector"""
    return [(0, n, dict(cfg), n_matrix_of(layers))]


def run(slices, n, reference, implementation, k_powf, k_host_, loss_scale=128.0, n_steps=N_STEPS, changes=None, gradients=None, check_exercise=True, what=""):
    """Both sides through n_steps from the same weights; `slices`: what each Adam of the optimizer owns (one_slice, or a Composite's).  Before
    every step both get the reference's weights (and a half vector with the sentinel where the step must not store); their moments and
    counts are their own, and are compared bit for bit after every step.  changes: {steps done: hyperparameters} applied to both sides
    (update()) and to every slice at that point.  gradients: bits -> what the implementation is handed (default: the half bits themselves).
    check_exercise=False: for a loss scale the inputs were not made for, which moves the unscaled gradients so far that a branch cannot bind
    (under 2^17 every effective rate lies above adabound's lower bound); a frozen class is held still either way.
    Returns (largest error-to-bound ratio, the Exercise)."""
    slices = [(a, c, dict(cfg), nm) for a, c, cfg, nm in slices]
    zeros_from = min([a + nm for a, c, _, nm in slices if nm < c] or [n])
    end = max(a + c for a, c, _, _ in slices)
    w_fp = initial_weights(n)
    state = {"m1": np.zeros(n, dtype=F), "m2": np.zeros(n, dtype=F), "steps": np.zeros(n, dtype=np.uint32)}
    exercise, worst = Exercise(slices[-1][2]), 0.0
    for s in range(n_steps):
        if changes and s in changes:
            for _, _, cfg, _ in slices:
                cfg.update(changes[s])
            reference.update(changes[s])
            implementation.update(changes[s])
        g = gradient_bits(n, zeros_from, s)
        skipped = np.ones(n, dtype=bool)
        for a, c, cfg, nm in slices:
            skipped[a:a + c] = skipped_mask(cfg, c, nm, g[a:a + c], loss_scale)
        w_half = half_with_sentinel(w_fp, skipped)
        before = {"w_fp": w_fp, "w_half": w_half, **state}
        want = reference.step(loss_scale, w_fp, w_half, g)
        got = implementation.step(loss_scale, w_fp, w_half, g if gradients is None else gradients(g))
        for a, c, cfg, nm in slices:
            cut = lambda d: {k: v[a:a + c] for k, v in d.items()}
            exercise.step(cfg, nm, loss_scale, s + 1, cut(before), g[a:a + c], cut(want))
            worst = max(worst, assert_adam_step(cfg, nm, loss_scale, s + 1, cut(before), g[a:a + c], cut(got), cut(want), k_powf, k_host_, what=f"{what} [{a}, {a + c}) step {s + 1}"))
        for side in (want, got):  # what belongs to no Adam stays as it is
            assert np.array_equal(_bits(side["w_fp"][end:]), _bits(w_fp[end:])) and np.array_equal(side["w_half"][end:], w_half[end:]), what
        w_fp, state = want["w_fp"], {k: want[k] for k in ("m1", "m2", "steps")}
    if check_exercise:
        exercise.check(n_steps)
    return worst, exercise
