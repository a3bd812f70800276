"""CPU restatements of the analytic encodings (Frequency, TriangleWave, SphericalHarmonics, Empty: k_encodings.hip) for the tests: no GPU.

Three readings of one recipe, chosen by `mode`:
  "r64"   fp64 throughout with the mathematical constants (pi, N_l^m in double): the function itself.  The second-order tests' truth.
  "r64f"  fp64 arithmetic on the kernels' FLOAT constants ((float)pi, (float)pi / 2, the float-rounded N_l^m): R64 of the per-element
          tests.  What the kernels would give if every operation were exact, so the difference to it is rounding alone.
  "f32"   fp32 in the kernels' operation order (the library is built without floating-point contraction); "half": the same, rounded to
          half where the kernels store a half (Rf32 / Rh).
First order (tests/test_analytic_encodings_per_element.py): values(), dy_dx() / jacobian(), dense_sum(), the per-element Frequency
bounds, the per-column SphericalHarmonics bars and one input set per case (inputs()).  Second order
(tests/test_encoding_second_order.py): _frequency, _trianglewave, _spherical_harmonics, _empty return (y, t, dx) of the second-order pass.

Scope of the input set: finite inputs on which the restated arithmetic is well defined -- |x| <= 256 (so |x| 2^(F+1) < 2^24 for F <= 12
and TriangleWave's (int) cast is defined), x = +-0 or |x| >= 2^-100 (no subnormal intermediate).  Inf, NaN, larger magnitudes and
subnormals are out of scope: nothing here says what the kernels do with them."""
import math

import numpy as np

# sinf / cosf on the device against the correctly rounded value, in float steps: measured over 65536 arguments per row of
# profiles/libm_f32_ulp.txt (rows "sinf" / "cosf": worst 1 and 2) and quoted in profiles/activation_sweep_f32.txt ("K_sinf = 1, K_cosf = 2")
K_SINF, K_COSF = 1, 2
N_ROWS = 512


# ---------------------------------------------------------------------------------------------------- the recipes, restated
def _mode(mode):
    """(compute dtype, rounding applied where the kernels store a value of the encoding's precision)"""
    import torch

    if mode in ("r64", "r64f"):
        return torch.float64, (lambda t: t)
    if mode == "f32":
        return torch.float32, (lambda t: t)
    assert mode == "half"
    return torch.float32, (lambda t: t.half().float())


def _pi(mode):
    return math.pi if mode == "r64" else float(np.float32(math.pi))  # the kernels' constant is a float


def _padded(live, pad, value, first=False):
    import torch

    fill = torch.full((live.shape[0], pad), value, dtype=live.dtype)
    return torch.cat([fill, live] if first else [live, fill], dim=1)


def _frequency(x, v, d, n_frequencies, pad, mode):
    """k_frequency_fwd and k_frequency_bwd_bwd_input.  Output j of dim a: (frequency k, phase) at a * 2F + 2k + phase.
    Returns y, t [n][D * 2F + pad] and dx [n][D]."""
    import torch

    dt, store = _mode(mode)
    PI = _pi(mode)
    x, v = x.to(dt), v.to(dt)
    n, D = x.shape
    F2 = 2 * n_frequencies
    dl = d[:, :D * F2].to(dt).reshape(n, D, F2)
    ys, ts = [None] * F2, [None] * F2
    total = torch.zeros(n, D, dtype=dt)
    for k in range(n_frequencies):
        scaled = x * float(2 ** k)
        scale = float(2 ** k) * PI
        for phase in range(2):
            arg = scaled * PI + phase * (PI / 2)
            ys[2 * k + phase] = store(torch.sin(arg))
            ts[2 * k + phase] = store(scale * torch.cos(arg) * v)
            total = total + dl[:, :, 2 * k + phase] * (-(scale * scale) * torch.sin(arg))
    y = torch.stack(ys, dim=2).reshape(n, D * F2)
    t = torch.stack(ts, dim=2).reshape(n, D * F2)
    return _padded(y, pad, 1.0), _padded(t, pad, 0.0), v * total


def _triangle_val(x, k, dt):
    return x.to(dt) * float(2.0 ** (k - 1)) + k * 0.25


def _trianglewave(x, v, d, n_frequencies, pad, mode):
    """k_trianglewave_fwd and k_trianglewave_bwd_bwd_input: the slope's sign by the kernel's rule (floor(2 val) even: falling)"""
    import torch

    dt, store = _mode(mode)
    x, v = x.to(dt), v.to(dt)
    n, D = x.shape
    ys, ts = [], []
    for k in range(n_frequencies):
        val = _triangle_val(x, k, dt)
        ys.append(store((val - torch.floor(val) - 0.5).abs() * 4 - 1))
        sign = torch.where(torch.floor(val * 2.0).to(torch.int64) % 2 == 0, -torch.ones_like(val), torch.ones_like(val))
        ts.append(store(sign * float(2.0 ** (k + 1)) * v))
    y = torch.stack(ys, dim=2).reshape(n, D * n_frequencies)
    t = torch.stack(ts, dim=2).reshape(n, D * n_frequencies)
    return _padded(y, pad, 1.0), _padded(t, pad, 0.0), torch.zeros(n, D, dtype=dt)


def _sh_norm(l, m, mode):
    ratio = 1.0
    for k in range(l - m + 1, l + m + 1):
        ratio /= k
    value = math.sqrt((2.0 * l + 1.0) / (4.0 * math.pi) * ratio) * (math.sqrt(2.0) if m else 1.0)
    return value if mode == "r64" else float(np.float32(value))


def _spherical_harmonics(p, v, d, degree, pad, mode):
    """sh_eval / sh_eval_dotted line by line: every quantity with its directional derivative along 2 v.  The padding columns come
    first.  Returns y, t [n][pad + degree^2] and dx [n][3]."""
    import torch

    dt, store = _mode(mode)
    x, y, z = [p[:, i].to(dt) * 2.0 - 1.0 for i in range(3)]
    dx, dy, dz = [v[:, i].to(dt) * 2.0 for i in range(3)]
    dl = d[:, pad:].to(dt)
    n = p.shape[0]
    zero, one = torch.zeros(n, dtype=dt), torch.ones(n, dtype=dt)
    values, tangent = [None] * (degree * degree), [None] * (degree * degree)
    gx_, gy_, gz_ = zero, zero, zero
    c, s, cp, sp = one, zero, zero, zero
    c_, s_, cp_, sp_ = zero, zero, zero, zero
    qmm = 1.0
    for m in range(degree):
        if m > 0:
            cp, sp, cp_, sp_ = c, s, c_, s_
            c = x * cp - y * sp
            s = x * sp + y * cp
            c_ = (dx * cp + x * cp_) - (dy * sp + y * sp_)
            s_ = (dx * sp + x * sp_) + (dy * cp + y * cp_)
            qmm = -qmm * (2 * m - 1)
        q2 = q1 = d2 = d1 = zero
        q2_ = q1_ = d2_ = d1_ = zero
        for l in range(m, degree):
            if l == m:
                q, dq, q_, dq_ = qmm * one, zero, zero, zero
            elif l == m + 1:
                q = (2 * m + 1) * z * q1
                dq = (2 * m + 1) * q1
                q_ = (2 * m + 1) * (dz * q1 + z * q1_)
                dq_ = (2 * m + 1) * q1_
            else:
                q = ((2 * l - 1) * z * q1 - (l + m - 1) * q2) / (l - m)
                dq = ((2 * l - 1) * (q1 + z * d1) - (l + m - 1) * d2) / (l - m)
                q_ = ((2 * l - 1) * (dz * q1 + z * q1_) - (l + m - 1) * q2_) / (l - m)
                dq_ = ((2 * l - 1) * (q1_ + (dz * d1 + z * d1_)) - (l + m - 1) * d2_) / (l - m)
            q2, q1, d2, d1 = q1, q, d1, dq
            q2_, q1_, d2_, d1_ = q1_, q_, d1_, dq_
            norm = _sh_norm(l, m, mode)
            nq, ndq, nq_, ndq_ = norm * q, norm * dq, norm * q_, norm * dq_
            base = l * l + l
            if m == 0:
                values[base] = store(nq)
                tangent[base] = store(nq_)
                gz_ = gz_ + dl[:, base] * ndq_
            else:
                values[base + m], values[base - m] = store(nq * c), store(nq * s)
                tangent[base + m], tangent[base - m] = store(nq_ * c + nq * c_), store(nq_ * s + nq * s_)
                gp, gm = dl[:, base + m], dl[:, base - m]
                ncp_, nsp_ = m * (nq_ * cp + nq * cp_), m * (nq_ * sp + nq * sp_)
                gx_ = gx_ + (gp * ncp_ + gm * nsp_)
                gy_ = gy_ + (gp * -nsp_ + gm * ncp_)
                gz_ = gz_ + (gp * (ndq_ * c + ndq * c_) + gm * (ndq_ * s + ndq * s_))
    return (_padded(torch.stack(values, dim=1), pad, 1.0, first=True), _padded(torch.stack(tangent, dim=1), pad, 0.0, first=True),
            torch.stack([2.0 * gx_, 2.0 * gy_, 2.0 * gz_], dim=1))


def _empty(x, v, d, pad, mode):
    import torch

    dt, _ = _mode(mode)
    n = x.shape[0]
    return torch.ones(n, pad, dtype=dt), torch.zeros(n, pad, dtype=dt), torch.zeros(n, x.shape[1], dtype=dt)


def _restate(cfg, x, v, d, pad, mode):
    otype = cfg["otype"]
    if otype == "Frequency":
        return _frequency(x, v, d, cfg["n_frequencies"], pad, mode)
    if otype == "TriangleWave":
        return _trianglewave(x, v, d, cfg["n_frequencies"], pad, mode)
    if otype == "SphericalHarmonics":
        return _spherical_harmonics(x, v, d, cfg["degree"], pad, mode)
    assert otype == "Empty"
    return _empty(x, v, d, pad, mode)


def _width(cfg, n_in):
    return {"Frequency": lambda: n_in * 2 * cfg["n_frequencies"], "TriangleWave": lambda: n_in * cfg["n_frequencies"],
            "SphericalHarmonics": lambda: cfg["degree"] ** 2, "Empty": lambda: 0}[cfg["otype"]]()


def _triangle_inputs(n, n_in, seed):
    """x = (m + 0.37) / 2^16 with integer m: x 2^(k+1) is never an integer for k <= 11, so no sample sits on a kink of any frequency"""
    import torch

    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, 2 ** 16, (n, n_in), generator=g)
    return ((m.double() + 0.37) / 2.0 ** 16).float()


def _half_ulp(value):
    """half of the distance between neighbouring half-precision numbers at |value| (2^-24 apart below 2^-14)"""
    import torch

    exponent = torch.floor(torch.log2(value.abs().clamp_min(2.0 ** -14)))
    return 0.5 * torch.pow(2.0, exponent - 10)


# ---------------------------------------------------------------------------------------------------- first order
def outputs_per_input(cfg):
    """P: the outputs of one input dim of a periodic encoding, adjacent columns a * P .. a * P + P - 1"""
    return 2 * cfg["n_frequencies"] if cfg["otype"] == "Frequency" else cfg["n_frequencies"]


def ulp32(value):
    """the distance between neighbouring floats at |value| (a float64 tensor); 2^-149 at and below the smallest normal"""
    import torch

    _, exponent = torch.frexp(value.abs().double())  # |value| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(value, dtype=torch.float64), (exponent - 1).clamp_min(-126) - 23)


def values(cfg, x, mode, pad=0):
    """The forward pass [n][width + pad]: R64 with mode "r64f", Rf32 with "f32" / "half" """
    import torch

    zeros = torch.zeros(x.shape[0], _width(cfg, x.shape[1]) + pad)
    return _restate(cfg, x, torch.zeros(x.shape), zeros, pad, mode)[0]


def dy_dx(cfg, x, mode):
    """What k_frequency_fwd / k_trianglewave_fwd store as dy_dx [n][D * P]: the derivative of output column a * P + k with respect to
    input a (closed form; TriangleWave: the kernel's sign rule at kinks, every entry +-2^(k+1) exactly)"""
    import torch

    dt, _ = _mode(mode)
    x = x.to(dt)
    n, D = x.shape
    F = cfg["n_frequencies"]
    cols = []
    if cfg["otype"] == "Frequency":
        PI = _pi(mode)
        for k in range(F):
            scaled = x * float(2 ** k)
            for phase in range(2):
                cols.append(float(2 ** k) * PI * torch.cos(scaled * PI + phase * (PI / 2)))
    else:
        assert cfg["otype"] == "TriangleWave"
        for k in range(F):
            val = _triangle_val(x, k, dt)
            falling = torch.floor(val * 2.0).to(torch.int64) % 2 == 0
            cols.append(torch.where(falling, -torch.ones_like(val), torch.ones_like(val)) * float(2.0 ** (k + 1)))
    return torch.stack(cols, dim=2).reshape(n, D * len(cols))


def sh_first_order(p, d, degree, mode):
    """sh_eval's gradient half line by line (k_sh_bwd_input): returns (J [n][degree^2][3], dL_dx [n][3] or None without d).
    J[:, j, :] holds the three products the kernel multiplies dL_dy[j] with, times the 2 of [0, 1]^3 -> [-1, 1]^3; dL_dx accumulates
    them in the kernel's order (m outer, l inner; x and y: (gp A + gm B) added as one term)."""
    import torch

    dt, _ = _mode(mode)
    x, y, z = [p[:, i].to(dt) * 2.0 - 1.0 for i in range(3)]
    n = p.shape[0]
    zero, one = torch.zeros(n, dtype=dt), torch.ones(n, dtype=dt)
    J = [[zero, zero, zero] for _ in range(degree * degree)]
    dl = None if d is None else d.to(dt)
    gx, gy, gz = zero, zero, zero
    c, s, cp, sp = one, zero, zero, zero
    qmm = 1.0
    for m in range(degree):
        if m > 0:
            cp, sp = c, s
            c = x * cp - y * sp
            s = x * sp + y * cp
            qmm = -qmm * (2 * m - 1)
        q2 = q1 = d2 = d1 = zero
        for l in range(m, degree):
            if l == m:
                q, dq = qmm * one, zero
            elif l == m + 1:
                q = (2 * m + 1) * z * q1
                dq = (2 * m + 1) * q1
            else:
                q = ((2 * l - 1) * z * q1 - (l + m - 1) * q2) / (l - m)
                dq = ((2 * l - 1) * (q1 + z * d1) - (l + m - 1) * d2) / (l - m)
            q2, q1, d2, d1 = q1, q, d1, dq
            norm = _sh_norm(l, m, mode)
            nq, ndq = norm * q, norm * dq
            base = l * l + l
            if m == 0:
                J[base] = [zero, zero, ndq]
                if dl is not None:
                    gz = gz + dl[:, base] * ndq
            else:
                xp, xm = nq * float(m) * cp, nq * float(m) * sp
                yp, ym = nq * -float(m) * sp, nq * float(m) * cp
                zp, zm = ndq * c, ndq * s
                J[base + m], J[base - m] = [xp, yp, zp], [xm, ym, zm]
                if dl is not None:
                    gp, gm = dl[:, base + m], dl[:, base - m]
                    gx = gx + (gp * xp + gm * xm)
                    gy = gy + (gp * yp + gm * ym)
                    gz = gz + (gp * zp + gm * zm)
    jac = 2.0 * torch.stack([torch.stack(row, dim=1) for row in J], dim=1)
    return jac, (None if dl is None else torch.stack([2.0 * gx, 2.0 * gy, 2.0 * gz], dim=1))


def sh_jacobian_autograd(p, degree):
    """R64's Jacobian of SphericalHarmonics [n][degree^2][3] by torch.autograd on the fp64 restatement of the VALUES (float constants):
    the hand-written derivative recurrence is not its own judge.  The 2 of [0, 1]^3 -> [-1, 1]^3 comes with the map itself."""
    import torch

    pr = p.double().clone().requires_grad_(True)
    zeros = torch.zeros(p.shape[0], degree * degree)
    y = _spherical_harmonics(pr, torch.zeros_like(p), zeros, degree, 0, "r64f")[0]
    rows = []
    for j in range(degree * degree):
        if not y[:, j].requires_grad:  # degree 0: a constant
            rows.append(torch.zeros_like(pr))
            continue
        (g,) = torch.autograd.grad(y[:, j].sum(), pr, retain_graph=True)
        rows.append(g)
    return torch.stack(rows, dim=1)


def jacobian(cfg, x):
    """R64's full first-order Jacobian J[i, j, a] = d y_j / d x_a in fp64 (no padding columns)"""
    import torch

    if cfg["otype"] == "SphericalHarmonics":
        return sh_jacobian_autograd(x, cfg["degree"])
    n, D = x.shape
    P = outputs_per_input(cfg)
    band = dy_dx(cfg, x, "r64f").reshape(n, D, P)
    J = torch.zeros(n, D * P, D, dtype=torch.float64)
    for a in range(D):
        J[:, a * P:(a + 1) * P, a] = band[:, a]
    return J


def dense_sum(dy, band, P, dt):
    """k_periodic_bwd_input: dL_dx[i, a] = sum_k dy[i, a P + k] band[i, a P + k], one product and one addition per term in ascending k
    (fp32: the kernel's roundings; fp64: the reference sum).  dy [n][D P], band [n][D P], P outputs per input -> [n][D]"""
    import torch

    n = band.shape[0]
    D = band.shape[1] // P
    a, b = dy[:, :D * P].to(dt).reshape(n, D, P), band.to(dt).reshape(n, D, P)
    result = torch.zeros(n, D, dtype=dt)
    for k in range(P):
        result = result + a[:, :, k] * b[:, :, k]
    return result


def frequency_bounds(cfg, x, half):
    """Per-element bounds for Frequency against R64 [n][D * 2F], fp64: (value bound, dy_dx bound, |arg|).

    arg = x 2^k PI_f + phase_f exactly (PI_f = (float)pi, phase_f in {0, PI_f / 2}; x 2^k PI_f is exact in fp64).  The kernel forms it
    with at most two roundings, v PI_f and the sum: |arg_kernel - arg| <= 2^-24 (|v PI_f| + |arg|) <= 2^-24 (2 |arg| + pi / 2)
    <= 2^-23 (|arg| + pi / 2).  |sin'|, |cos'| <= 1 carry that to the result; sinf / cosf are within K_SINF / K_COSF float steps of the
    correctly rounded value, itself half a step from the true one:
      value  |y - R64| <= 2^-23 (|arg| + pi / 2) + (K_SINF + 1/2) ulp32(R64)   (+ half a half-ulp at |R64| where a half is stored)
      dy_dx  2^k PI_f (2^-23 (|arg| + pi / 2) + (K_COSF + 1/2) ulp32(cos arg)) + 2^-24 |ref|   (2^k PI_f is exact; one product rounds)"""
    import torch

    xd = x.double()
    n, D = xd.shape
    F = cfg["n_frequencies"]
    PI = _pi("r64f")
    value, slope, args = [], [], []
    for k in range(F):
        for phase in range(2):
            arg = xd * float(2 ** k) * PI + phase * (PI / 2)
            arg_error = 2.0 ** -23 * (arg.abs() + math.pi / 2)
            y, c = torch.sin(arg), torch.cos(arg)
            bound = arg_error + (K_SINF + 0.5) * ulp32(y)
            if half:
                bound = bound + _half_ulp(y)
            value.append(bound)
            scale = float(2 ** k) * PI
            slope.append(scale * (arg_error + (K_COSF + 0.5) * ulp32(c)) + 2.0 ** -24 * (scale * c).abs())
            args.append(arg.abs())
    shape = lambda cols: torch.stack(cols, dim=2).reshape(n, D * 2 * F)  # noqa: E731
    return shape(value), shape(slope), shape(args)


def dense_bound(dy, J_band, bound_band, P):
    """dL_dx[i, a] = sum_j dy_j J_j over the P outputs of dim a against the fp64 sum: every entry of dy_dx within its bound, P products
    and P additions (the first onto zero is exact) each within 2^-24 of a quantity no larger than sum_j |dy_j J_j|:
      sum_j |dy_j| bound_j + P 2^-24 sum_j |dy_j J_j|      (all fp64; dy [n][D P], J_band, bound_band [n][D P] -> [n][D])"""
    n = J_band.shape[0]
    D = J_band.shape[1] // P
    a = dy[:, :D * P].double().abs().reshape(n, D, P)
    return (a * bound_band.reshape(n, D, P)).sum(2) + P * 2.0 ** -24 * (a * J_band.double().abs().reshape(n, D, P)).sum(2)


SH_MARGIN = 4.0


def column_bar(rf32, r64):
    """The SphericalHarmonics yardstick, per column (any trailing dims count as columns): E_j = max_i |Rf32 - R64| over the rows, and
    the bar SH_MARGIN E_j + ulp32(max_i |R64|) that max_i |ours - R64| has to stay under.  The margin of 4: the kernel may contract
    a b + c and uses the device's division -- each differs from Rf32 by at most one rounding per operation, at most twice the
    restatement's worst-case growth -- and E_j is a realised error on a finite sample, not a worst case: another factor 2.
    Returns (E [cols...], bar [cols...]) in fp64."""
    E = (rf32.double() - r64).abs().amax(dim=0)
    return E, SH_MARGIN * E + ulp32(r64.abs().amax(dim=0))


# ---------------------------------------------------------------------------------------------------- the input set
def _neighbours(values):
    v = np.asarray(values, dtype=np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


def periodic_specials(n_frequencies):
    """Every kink m 2^-(k+1), k < F, for a spread of m on both sides of zero, with both float neighbours of each; +-0, +-1, +-0.5,
    +-255.75 (the largest magnitudes: |x| 2^(F+1) < 2^24 for F <= 12)"""
    kinks = []
    for k in range(n_frequencies):
        for m in (-(2 ** (k + 2)) - 1, -3, -2, -1, 1, 2, 3, 2 ** (k + 2) + 1):
            kinks.append(m * 2.0 ** -(k + 1))
    specials = np.concatenate([_neighbours(kinks), np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 255.75, -255.75], dtype=np.float32)])
    assert np.all(np.abs(specials) <= 256) and np.all((specials == 0) | (np.abs(specials) >= 2.0 ** -100))
    return specials


def inputs(cfg, n_in, seed=31):
    """The one input set of a case, float32 [N_ROWS][n_in], shared by every test of it (see the module docstring for the scope).
    Periodic encodings: the specials (periodic_specials) in the last rows, every one at least once; the rows before them in three
    parts: uniform in [0, 1), uniform in [-4, 4), x = (m + 0.37) / 2^16 (no kink of any frequency k <= 11).
    SphericalHarmonics: points of [0, 1]^3 -- the 8 corners, the 6 face centres, the centre (x = y = z = 0 after the map), 241 unit
    directions d as (d + 1) / 2 (the first six along the axes' neighbours: one component 0 exactly), the rest uniform in [0, 1)^3."""
    import torch

    g = torch.Generator().manual_seed(seed)
    if cfg["otype"] == "SphericalHarmonics":
        assert n_in == 3
        corners = [[a, b, c] for a in (0.0, 1.0) for b in (0.0, 1.0) for c in (0.0, 1.0)]
        faces = [[0.5 + 0.5 * s * (i == a) for i in range(3)] for a in range(3) for s in (-1.0, 1.0)]
        fixed = torch.tensor(corners + faces + [[0.5, 0.5, 0.5]], dtype=torch.float32)
        d = torch.randn(241, 3, generator=g, dtype=torch.float64)
        for i in range(6):
            d[i, i % 3] = 0.0
        d = d / d.norm(dim=1, keepdim=True)
        directions = ((d + 1.0) / 2.0).float()
        rest = torch.rand(N_ROWS - fixed.shape[0] - directions.shape[0], 3, generator=g)
        x = torch.cat([fixed, directions, rest], dim=0)
    else:
        specials = torch.from_numpy(periodic_specials(cfg["n_frequencies"]))
        special_rows = -(-specials.numel() // n_in)
        free = N_ROWS - special_rows
        assert free >= 96, (special_rows, n_in)
        a, b = free * 3 // 8, free * 3 // 8
        unit = torch.rand(a, n_in, generator=g)
        wide = torch.rand(b, n_in, generator=g) * 8.0 - 4.0
        off_kink = _triangle_inputs(free - a - b, n_in, seed)
        slots = torch.arange(special_rows * n_in).reshape(special_rows, n_in)
        x = torch.cat([unit, wide, off_kink, specials[slots % specials.numel()]], dim=0)
        assert bool(((x == 0) | (x.abs() >= 2.0 ** -100)).all()) and float(x.abs().max()) <= 256
    assert x.shape == (N_ROWS, n_in) and x.dtype == torch.float32
    return x
