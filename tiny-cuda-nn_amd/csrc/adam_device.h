// adam_device.h -- one Adam update (optimizers/adam.h:48-119), shared by k_adam, k_adam_prologue (k_misc.hip) and by the slab reduction
// that applies the update to the weights whose gradients it finishes (k_wgrad_reduce_adam, k_mlp.hip).  One source for all, so that every
// route produces the same bits.
#pragma once
#include "tcnn_common.h"

namespace tcnn_amd {

// ---- sqrtf and the division of the effective learning rate, correctly rounded, without the generic expansions' scaling and fix-up.
// The compiler's sqrtf / `/` are correctly rounded for every input: they scale operands that could leave the normal range on the way, and
// put zeros, infinities and NaN right afterwards (16 and 11 vector instructions).  Between the bounds below nothing can leave the normal
// range, so the scaling is the identity and the fix-up has nothing to fix; outside them the callers run the plain expression.
//
// Square root, x in [2^-96, 2^32).  y = v_rsq_f32(x) (1 ulp), s = x * y is sqrt(x) to a few ulp, and one Newton step on the exact residual
// r = fma(-s, s, x) with h = y / 2 gives fma(r, h, s).  That this IS the correctly rounded root is not argued but counted: the root's
// rounding depends on the significand and the exponent's parity alone as long as no intermediate is a denormal or overflows, and the form was
// compared with sqrtf on every pattern of the range (tcnn_adam_math_sweep, tests/test_adam_fast_math.py: 0 mismatches of 2^30; below 2^-100
// the residual becomes a denormal and the form does fail, which is why the lower bound is there).  s lies in [2^-48, 2^16].
constexpr uint32_t ADAM_SQRT_LO = (127u - 96u) << 23, ADAM_SQRT_SPAN = 128u << 23;
// Division n / d, n in [2^-64, 2^64) and d in [2^-48, 2^18): the generic expansion's own sequence -- v_rcp_f32, one Newton step on the
// reciprocal, the quotient and two residual corrections of it -- without v_div_scale_f32 in front and v_div_fmas_f32's scaling /
// v_div_fixup_f32 behind.  The generic expansion is correctly rounded; what its scaling does is multiply an operand by 2^+-64 where an
// intermediate could otherwise leave the normal range, and undo that at the end.  Here none can: the reciprocal lies in (2^-18, 2^48], the
// quotient in (2^-82, 2^112), a residual fma(-d, q, n) is zero or at least n * 2^-24 >= 2^-88, the reciprocal's residual is zero or
// about 2^-24.  On normal numbers rounding commutes with a power of two, so each operation here rounds to the generic expansion's value
// times that power: the same quotient, and v_div_fixup_f32 only replaces quotients of zeros, infinities, NaN and denormals.  (The sweep
// runs every denominator pattern against numerators across the range of learning_rate * debias, and seeded pairs around both ranges'
// edges: 0 mismatches with the plain `/`.)
constexpr uint32_t ADAM_DIV_N_LO = (127u - 64u) << 23, ADAM_DIV_N_SPAN = 128u << 23;
constexpr uint32_t ADAM_DIV_D_LO = (127u - 48u) << 23, ADAM_DIV_D_SPAN = 66u << 23;
// (bits - LO < SPAN as unsigned: negative numbers, NaN, infinities, zeros and denormals all fall outside)
__device__ inline uint32_t adam_sqrt_excess(const float x) { return __float_as_uint(x) - ADAM_SQRT_LO; }
__device__ inline uint32_t adam_div_n_excess(const float n) { return __float_as_uint(n) - ADAM_DIV_N_LO; }
__device__ inline bool adam_div_d_in_range(const float d) { return __float_as_uint(d) - ADAM_DIV_D_LO < ADAM_DIV_D_SPAN; }

__device__ inline float adam_sqrt_fast(const float x) {
	const float y = __builtin_amdgcn_rsqf(x);
	const float s = x * y, h = 0.5f * y;
	return fmaf(fmaf(-s, s, x), h, s);
}
__device__ inline float adam_div_fast(const float n, const float d) {
	float r = __builtin_amdgcn_rcpf(d);
	r = fmaf(fmaf(-d, r, 1.0f), r, r);
	float q = n * r;
	q = fmaf(fmaf(-d, q, n), r, q);
	return fmaf(fmaf(-d, q, n), r, q);
}
// the guarded forms on their own (the math sweep runs exactly these)
__device__ inline float adam_sqrt(const float x) { return adam_sqrt_excess(x) < ADAM_SQRT_SPAN ? adam_sqrt_fast(x) : sqrtf(x); }
__device__ inline float adam_div(const float n, const float d) { return adam_div_n_excess(n) < ADAM_DIV_N_SPAN && adam_div_d_in_range(d) ? adam_div_fast(n, d) : n / d; }

// The launch-constant part of the guard: with 0 <= epsilon <= 2^16, sqrt in [2^-48, 2^16] makes sqrt + epsilon a denominator in [2^-48, 2^17].
__device__ inline bool adam_epsilon_in_range(const AdamArgs& a) { return a.epsilon >= 0.0f && a.epsilon <= 65536.0f; }

// ---- one parameter, in three pieces so that a quad can run the middle one -- learning_rate / (sqrtf(second_moment) + epsilon) -- under
// ONE range test for its four parameters: four branches would cut the quad's instruction stream into pieces that cannot overlap.
// PLAIN: the host found loss_scale an exact power of two (inv_loss_scale_exact) and weight_clipping_magnitude == 0.  Both are tests of launch
// constants that the generic code makes per parameter (and, the division being "cheap" to the compiler, it computes g / loss_scale AND
// g * inv_loss_scale and selects); PLAIN is that code with the two tests decided: no arithmetic is replaced by other arithmetic, so there
// is no input on which it could differ.  (The other options stay in: with both decays zero the decay expression still turns a weight of
// -0 into +0, fminf(fmaxf(x, 0), FLT_MAX) turns NaN into 0, and l2_reg * w is NaN for an infinite weight whatever l2_reg is.)
struct AdamLane {
	float weight_fp, first_moment, second_moment, learning_rate; // (learning_rate: debiased)
	bool updated;
};

// debias: the optimizer's table at min(step + 1, common_step) -- a parameter never has more steps than the optimizer -- which every caller
// loads in front, for skipped parameters too (their result is dropped): no lookup inside a divergent branch.
// G: the type the gradient was loaded as, _Float16 (the trainer's gradient vector) or float (a caller's own fp32 gradients, standalone
// optimizers): the value is taken to float as it is and unscaled the same way -- no rounding in between for either type.
template <bool PLAIN, typename G>
__device__ inline AdamLane adam_front(const AdamArgs& a, const float debias, const bool is_matrix, const G g_in, const float w_fp, const float m1, const float m2) {
	AdamLane l;
	const float g = (float)g_in;
	// loss_scale is a power of two in practice (128): the reciprocal multiply is then exact, i.e. identical to the division
	float gradient = (PLAIN || a.inv_loss_scale_exact) ? g * a.inv_loss_scale : g / a.loss_scale;
	l.updated = is_matrix ? a.optimize_matrix_params != 0 : (a.optimize_non_matrix_params != 0 && gradient != 0);
	l.weight_fp = w_fp;
	if (is_matrix) gradient += a.l2_reg * w_fp;
	const float gradient_sq = gradient * gradient;
	l.first_moment = a.beta1 * m1 + (1 - a.beta1) * gradient;
	l.second_moment = a.beta2 * m2 + (1 - a.beta2) * gradient_sq;
	float learning_rate = a.learning_rate;
	if (!is_matrix) learning_rate *= a.non_matrix_learning_rate_factor;
	l.learning_rate = learning_rate * debias;
	return l;
}

// rate: learning_rate / (sqrtf(second_moment) + epsilon)
// W: the working weights' type, _Float16, or float for an optimizer whose master vector is its working vector (w_h then equals w_fp's new value).
template <bool PLAIN, typename W>
__device__ inline void adam_back(const AdamArgs& a, const AdamLane& l, const float rate, float& w_fp, W& w_h, float& m1, float& m2, uint32_t& step) {
	const float effective_learning_rate = fminf(fmaxf(rate, a.lower_lr_bound), a.upper_lr_bound);
	// weight_decay(rel * lr, abs * lr, w), common_device.h:870-873
	const float decayed_weight = (1 - a.relative_weight_decay * l.learning_rate) * l.weight_fp - copysignf(a.absolute_weight_decay * l.learning_rate, l.weight_fp);
	float new_weight = decayed_weight - effective_learning_rate * l.first_moment;
	if constexpr (!PLAIN) {
		if (a.weight_clipping_magnitude != 0.0f) new_weight = fminf(fmaxf(new_weight, -a.weight_clipping_magnitude), a.weight_clipping_magnitude);
	}
	w_fp = l.updated ? new_weight : l.weight_fp;
	w_h = (W)new_weight; // stored only if updated
	m1 = l.updated ? l.first_moment : m1;
	m2 = l.updated ? l.second_moment : m2;
	step = l.updated ? step + 1 : step;
}

// One parameter, branch-free but for the range test (selects instead of early returns, so that a wave whose lanes disagree about "skipped"
// does not execute the body twice).  `updated` reports whether adam.h:76-84 lets this parameter through.
template <bool PLAIN = false, typename G, typename W>
__device__ inline void adam_one(const AdamArgs& a, const float debias, const bool is_matrix, const G g_in, float& w_fp, W& w_h, float& m1, float& m2, uint32_t& step, bool& updated) {
	const AdamLane l = adam_front<PLAIN>(a, debias, is_matrix, g_in, w_fp, m1, m2);
	float rate;
	if (adam_epsilon_in_range(a) && (adam_sqrt_excess(l.second_moment) | adam_div_n_excess(l.learning_rate)) < ADAM_SQRT_SPAN) rate = adam_div_fast(l.learning_rate, adam_sqrt_fast(l.second_moment) + a.epsilon);
	else rate = l.learning_rate / (sqrtf(l.second_moment) + a.epsilon);
	adam_back<PLAIN>(a, l, rate, w_fp, w_h, m1, m2, step);
	updated = l.updated;
}

// Four parameters: adam_one four times, the range test made once (x, y < 2^30 exactly when x | y < 2^30: the two spans are that power of two).
static_assert(ADAM_SQRT_SPAN == ADAM_DIV_N_SPAN && (ADAM_SQRT_SPAN & (ADAM_SQRT_SPAN - 1)) == 0, "the joint range test ORs the excesses");
template <bool PLAIN, typename G, typename W>
__device__ inline void adam_four(const AdamArgs& a, const float (&debias)[4], const bool (&is_matrix)[4], const G (&g_in)[4], float (&w_fp)[4], W (&w_h)[4], float (&m1)[4], float (&m2)[4],
                                 uint32_t (&step)[4], bool (&updated)[4]) {
	AdamLane l[4];
	uint32_t excess = 0;
#pragma unroll
	for (int e = 0; e < 4; ++e) {
		l[e] = adam_front<PLAIN>(a, debias[e], is_matrix[e], g_in[e], w_fp[e], m1[e], m2[e]);
		excess |= adam_sqrt_excess(l[e].second_moment) | adam_div_n_excess(l[e].learning_rate);
	}
	float rate[4];
	if (adam_epsilon_in_range(a) && excess < ADAM_SQRT_SPAN) {
#pragma unroll
		for (int e = 0; e < 4; ++e) rate[e] = adam_div_fast(l[e].learning_rate, adam_sqrt_fast(l[e].second_moment) + a.epsilon);
	} else {
#pragma unroll
		for (int e = 0; e < 4; ++e) rate[e] = l[e].learning_rate / (sqrtf(l[e].second_moment) + a.epsilon);
	}
#pragma unroll
	for (int e = 0; e < 4; ++e) {
		adam_back<PLAIN>(a, l[e], rate[e], w_fp[e], w_h[e], m1[e], m2[e], step[e]);
		updated[e] = l[e].updated;
	}
}

} // namespace tcnn_amd
