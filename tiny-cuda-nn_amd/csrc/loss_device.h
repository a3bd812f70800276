// loss_device.h -- one element of every loss of src/loss.cu:57-65: the device code shared by the trainer's loss kernels (k_misc.hip)
// and the evaluator for caller-owned predictions (k_loss_eval.hip), so that both compute the same bits.
#pragma once

#include "tcnn_common.h"

namespace tcnn_amd {
namespace {

// ---- loss: l2.h:40-74 / relative_l2.h:40-75 and the other element-wise losses.  One element: the reference's expressions, term for term.
// (row: the sample's padded prediction row -- RelativeL2Luminance reads the pixel's other channels from it)
// P: the predictions' and gradients' type, half_t, or float (Loss<float>: the cast of the gradient is then no rounding)
template <typename P>
__device__ inline void loss_element(const uint32_t type, const float prediction, const float target, const float pdf, const uint32_t n_total, const float loss_scale,
                                    const P* __restrict__ row, const uint32_t dims, float& value_out, P& grad_out) {
	const float difference = prediction - target;
	float value, gradient;
	switch ((LossType)type) {
		case LossType::RelativeL2: { // relative_l2.h:60-73
			const float prediction_sq_plus_epsilon = prediction * prediction + 0.01f;
			value = difference * difference / prediction_sq_plus_epsilon / pdf / n_total;
			gradient = 2 * difference / prediction_sq_plus_epsilon / pdf;
			break;
		}
		case LossType::RelativeL2Luminance: { // relative_l2_luminance.h:40-85: the divisor is the squared luminance of the pixel
			const P* px = row;
			float r = (float)px[0], g = (float)px[1], b = (float)px[2];
			if (dims >= 6) {
				r += (float)px[3];
				g += (float)px[4];
				b += (float)px[5];
			}
			const float luminance = (0.299f * r + 0.587f * g + 0.114f * b);
			const float prediction_sq_plus_epsilon = luminance * luminance + 0.01f;
			value = difference * difference / prediction_sq_plus_epsilon / pdf / n_total;
			gradient = 2 * difference / prediction_sq_plus_epsilon / pdf;
			break;
		}
		case LossType::L1: // l1.h:40-70
			value = fabsf(difference) / pdf / n_total;
			gradient = copysignf(1.0f / pdf, difference);
			break;
		case LossType::RelativeL1: { // relative_l1.h:40-72
			const float scale = 1.0f / (fabsf(prediction) + 1e-2f) / pdf;
			value = fabsf(difference) * scale / n_total;
			gradient = copysignf(scale, difference);
			break;
		}
		case LossType::Mape: { // mape.h:40-73
			const float scale = 1.0f / (fabsf(target) + 1e-2f) / pdf;
			value = fabsf(difference) * scale / n_total;
			gradient = copysignf(scale, difference);
			break;
		}
		case LossType::Smape: { // smape.h:40-73
			const float scale = 1.0f / (0.5f * (fabsf(target) + fabsf(prediction)) + 1e-2f) / pdf;
			value = fabsf(difference) * scale / n_total;
			gradient = copysignf(scale, difference);
			break;
		}
		case LossType::CrossEntropy: { // cross_entropy.h:40-72: the gradient already carries 1 / n_total
			const float factor = -target / pdf / n_total;
			value_out = factor * logf(prediction);
			grad_out = (P)(loss_scale * (factor / prediction));
			return;
		}
		case LossType::Variance: { // variance_is.h:40-72
			const float factor = target * target / pdf / n_total;
			value_out = factor / prediction - factor / pdf;
			grad_out = (P)(loss_scale * (-factor / (prediction * prediction)));
			return;
		}
		default: // L2, l2.h:60-72
			value = difference * difference / pdf / n_total;
			gradient = 2 * difference / pdf;
			break;
	}
	value_out = value;
	grad_out = (P)(loss_scale * gradient / n_total);
}

} // namespace
} // namespace tcnn_amd
