// k_loss_eval.hip -- the losses of src/loss.cu:57-65 on caller-owned predictions: Loss<T>::evaluate (loss.h:41-60) for tensors that are
// not a trainer's -- a renderer's output, a slice of a module's padded output, a C++ caller's own matrix.
//
// One kernel: every element is loss_element (loss_device.h), the expressions the trainer's k_loss / k_loss8 / k_loss4_f32 evaluate, so the
// bits are the trainer's.  What differs is the shape of the work:
//   - each output (values, gradients, the sum) is optional and has its own row stride; columns >= dims of an output row are zeros;
//   - the sum of the values is reduced from registers -- one partial per block, k_reduce_stage2 (k_misc.hip) sums the partials -- so a
//     caller that wants the scalar never stores or re-reads a values matrix.  Fixed grid, fixed order, no floating-point atomics: the
//     sum depends on (n, dims, strides, type) only;
//   - a device-side factor (scale_dev: autograd's incoming gradient, a GradScaler's scale) is multiplied into loss_scale in fp32, ahead
//     of the gradient's one rounding to the prediction type, without the host ever reading it.
// Streaming and launch-bound at the sizes callers have (2^18 x 3: ~6 MB): the point is one or two launches and one rounding.
#include "tcnn_common.h"
#include "loss_device.h"
#include "reduce_device.h"

#include <hip/hip_fp16.h>

#include <algorithm>

namespace tcnn_amd {
namespace {

typedef _Float16 half_t;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

template <typename P> struct PredictionVector;
template <> struct PredictionVector<half_t> { typedef h8 type; };
template <> struct PredictionVector<float> { typedef f4 type; };

struct LossEvalArgs {
	uint32_t type, n, dims, n_total;
	uint32_t width;               // columns a row of work covers: VEC > 1: == p_stride (the prediction as one flat array); VEC == 1: max(dims, output strides)
	uint32_t p_stride, v_stride, g_stride;
	uint32_t v_vector, g_vector;  // VEC > 1: the output's stride is `width` and its base is 16-byte aligned: whole vectors are stored at once
	float loss_scale;
	const float* scale_dev;
	const void* prediction;
	const float* target;
	const float* data_pdf;
	float* values;
	void* gradients;
	float* partials;
};

// VEC consecutive elements of [n][width] per thread and trip of a grid-stride loop.  VEC == 8 (half) / 4 (float): one 16-byte load of
// predictions where the thread's elements lie inside the array (all but the last thread of an array whose size is no multiple of VEC)
// AND the vector's first column holds a value (col < dims): a vector that lies in the padding columns is never loaded -- the caller owns
// rows of dims values, not the padding behind the last one -- and an aligned 16-byte load that starts at a value ends inside the
// 16-byte block that holds that value.  Rows may end anywhere inside the vector (compact rows: stride == dims); (row, col) come from one
// division per trip and are carried along from element to element instead of divided out for each.
template <typename P, int VEC>
__global__ void __launch_bounds__(256) k_loss_eval(const LossEvalArgs a) {
	__shared__ float sm[4];
	const P* __restrict__ predictions = (const P*)a.prediction;
	P* __restrict__ gradients = (P*)a.gradients;
	const float loss_scale = a.scale_dev ? a.loss_scale * *a.scale_dev : a.loss_scale;
	const uint64_t total = (uint64_t)a.n * a.width; // < 2^32 (checked by the caller)
	const uint64_t n_vectors = (total + VEC - 1) / VEC;
	float acc = 0.0f;
	for (uint64_t vi = (uint64_t)blockIdx.x * 256 + threadIdx.x; vi < n_vectors; vi += (uint64_t)gridDim.x * 256) {
		const uint32_t i0 = (uint32_t)(vi * VEC);
		const uint32_t count = (uint32_t)std::min<uint64_t>(VEC, total - i0);
		const bool whole = VEC > 1 && count == VEC;
		uint32_t row = i0 / a.width, col = i0 - row * a.width;
		const bool loaded = whole && col < a.dims;
		typename PredictionVector<P>::type pv = {}; // (VEC == 1: unused)
		if constexpr (VEC > 1) {
			if (loaded) pv = *(const typename PredictionVector<P>::type*)(predictions + i0);
		}
		float v[VEC];
		P g[VEC];
#pragma unroll
		for (int k = 0; k < VEC; ++k) {
			v[k] = 0.0f;
			g[k] = (P)0.0f;
			if ((uint32_t)k < count) {
				if (col < a.dims) {
					const P* prediction_row = predictions + (size_t)row * a.p_stride;
					const uint32_t target_idx = row * a.dims + col;
					const float pdf = a.data_pdf ? a.data_pdf[target_idx] : 1;
					const float prediction = loaded ? (float)pv[k] : (float)prediction_row[col];
					loss_element(a.type, prediction, a.target[target_idx], pdf, a.n_total, loss_scale, prediction_row, a.dims, v[k], g[k]);
					acc += v[k];
				}
				if (a.values && !(whole && a.v_vector) && col < a.v_stride) a.values[(size_t)row * a.v_stride + col] = v[k];
				if (gradients && !(whole && a.g_vector) && col < a.g_stride) gradients[(size_t)row * a.g_stride + col] = g[k];
				if (++col == a.width) {
					col = 0;
					++row;
				}
			}
		}
		if constexpr (VEC > 1) {
			if (whole && a.values && a.v_vector) {
#pragma unroll
				for (int q = 0; q < VEC; q += 4) *(f4*)(a.values + i0 + q) = f4{v[q], v[q + 1], v[q + 2], v[q + 3]};
			}
			if (whole && gradients && a.g_vector) {
				typename PredictionVector<P>::type packed;
#pragma unroll
				for (int k = 0; k < VEC; ++k) packed[k] = g[k];
				*(typename PredictionVector<P>::type*)(gradients + i0) = packed;
			}
		}
	}
	if (a.partials) { // (uniform over the grid)
		const float s = block_sum_256(acc, sm);
		if (threadIdx.x == 0) a.partials[blockIdx.x] = s;
	}
}

template <typename P, int VEC>
void launch(hipStream_t stream, const LossEvalArgs& a, uint32_t blocks) {
	hipLaunchKernelGGL((k_loss_eval<P, VEC>), dim3(blocks), dim3(256), 0, stream, a);
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

} // namespace

void loss_eval_launch(hipStream_t stream, const LossEvalRequest& r) {
	const bool fp32 = r.precision == Precision::Fp32;
	const uint32_t vec = fp32 ? 4 : 8;
	LossEvalArgs a{};
	a.type = (uint32_t)r.type;
	a.n = r.n;
	a.dims = r.dims;
	a.n_total = r.n * r.dims;
	a.p_stride = r.prediction_stride;
	a.v_stride = r.values ? r.values_stride : 0;
	a.g_stride = r.gradients ? r.gradients_stride : 0;
	a.loss_scale = r.loss_scale;
	a.scale_dev = r.scale_dev;
	a.prediction = r.prediction;
	a.target = r.target;
	a.data_pdf = r.data_pdf;
	a.values = r.values;
	a.gradients = r.gradients;
	a.partials = r.loss_sum ? r.partials : nullptr;

	// The vector path walks the prediction as one flat array [n * p_stride]: rows of whole vectors (a padded stride, as k_loss8 /
	// k_loss4_f32), or compact rows.  An output wider than the prediction has padding columns that walk would not reach.
	const bool rows_allow = r.prediction_stride % vec == 0 || r.prediction_stride == r.dims;
	const bool vector = rows_allow && aligned16(r.prediction) && a.v_stride <= r.prediction_stride && a.g_stride <= r.prediction_stride;
	if (vector) {
		a.width = r.prediction_stride;
		a.v_vector = r.values && a.v_stride == a.width && aligned16(r.values);
		a.g_vector = r.gradients && a.g_stride == a.width && aligned16(r.gradients);
	} else {
		a.width = std::max(r.dims, std::max(a.v_stride, a.g_stride));
	}
	const uint64_t total = (uint64_t)r.n * a.width;
	const uint64_t n_vectors = vector ? (total + vec - 1) / vec : total;
	const uint32_t blocks = (uint32_t)std::min<uint64_t>(LOSS_EVAL_MAX_BLOCKS, std::max<uint64_t>((n_vectors + 255) / 256, 1));
	if (vector) {
		if (fp32) launch<float, 4>(stream, a, blocks);
		else launch<half_t, 8>(stream, a, blocks);
	} else {
		if (fp32) launch<float, 1>(stream, a, blocks);
		else launch<half_t, 1>(stream, a, blocks);
	}
	if (a.partials) reduce_partials(stream, blocks, a.partials, r.loss_sum);
}

} // namespace tcnn_amd
