// adam_device.h -- one Adam update (optimizers/adam.h:48-119), shared by k_adam, k_adam_prologue (k_misc.hip) and by the slab reduction
// that applies the update to the weights whose gradients it finishes (k_wgrad_reduce_adam, k_mlp.hip).  One source for all, so that every
// route produces the same bits.
#pragma once
#include "tcnn_common.h"

namespace tcnn_amd {

// One parameter, branch-free (selects instead of early returns, so that a wave whose lanes disagree about "skipped" does not
// execute the body twice).  common_debias = debias_table[common_step]; parameters with their own step count look theirs up.
// `updated` reports whether adam.h:76-84 lets this parameter through.
// debias_of(t): the debiasing factor of step t <= common_step (a lookup in the optimizer's table).
// G: the type the gradient was loaded as, _Float16 (the trainer's gradient vector) or float (a caller's own fp32 gradients, standalone
// optimizers): the value is taken to float as it is and unscaled the same way -- no rounding in between for either type.
// W: the working weights' type, _Float16, or float for an optimizer whose master vector is its working vector (w_h then equals w_fp's new value).
template <typename DebiasOf, typename G, typename W>
__device__ inline void adam_one(const AdamArgs& a, DebiasOf&& debias_of, const float common_debias, const bool is_matrix, const G g_in, float& w_fp, W& w_h,
                                float& m1, float& m2, uint32_t& step, bool& updated) {
	const float g = (float)g_in;
	// loss_scale is a power of two in practice (128): the reciprocal multiply is then exact, i.e. identical to the division
	float gradient = a.inv_loss_scale_exact ? g * a.inv_loss_scale : g / a.loss_scale;
	updated = is_matrix ? a.optimize_matrix_params != 0 : (a.optimize_non_matrix_params != 0 && gradient != 0);
	const float weight_fp = w_fp;
	if (is_matrix) gradient += a.l2_reg * weight_fp;
	const float gradient_sq = gradient * gradient;
	const float first_moment = a.beta1 * m1 + (1 - a.beta1) * gradient;
	const float second_moment = a.beta2 * m2 + (1 - a.beta2) * gradient_sq;
	float learning_rate = a.learning_rate;
	if (!is_matrix) learning_rate *= a.non_matrix_learning_rate_factor;
	const uint32_t current_step = step + 1;
	float debias = common_debias;
	if (updated && current_step != a.common_step) debias = debias_of(min(current_step, a.common_step)); // a parameter never has more steps than the optimizer
	learning_rate *= debias;
	const float effective_learning_rate = fminf(fmaxf(learning_rate / (sqrtf(second_moment) + a.epsilon), a.lower_lr_bound), a.upper_lr_bound);
	// weight_decay(rel * lr, abs * lr, w), common_device.h:870-873
	const float decayed_weight = (1 - a.relative_weight_decay * learning_rate) * weight_fp - copysignf(a.absolute_weight_decay * learning_rate, weight_fp);
	float new_weight = decayed_weight - effective_learning_rate * first_moment;
	if (a.weight_clipping_magnitude != 0.0f) new_weight = fminf(fmaxf(new_weight, -a.weight_clipping_magnitude), a.weight_clipping_magnitude);
	w_fp = updated ? new_weight : weight_fp;
	w_h = (W)new_weight; // stored only if updated
	m1 = updated ? first_moment : m1;
	m2 = updated ? second_moment : m2;
	step = updated ? current_step : step;
}

} // namespace tcnn_amd
