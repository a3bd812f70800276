// k_misc.hip -- streaming kernels around the MLP: OneBlob / Identity encodings, losses, sum reduction, Adam,
// parameter initialisation and dtype plumbing.  All HBM-bound: 16-byte accesses, wave64 reductions.
//
// Replaces (reference, /root/reference/include/tiny-cuda-nn):
//   encodings/oneblob.h:47-164   kernel_one_blob / _backward          -> k_oneblob_fwd / k_oneblob_bwd_input
//   encodings/identity.h:46-85   identity / identity_backward         -> k_identity_fwd / k_identity_bwd_input
//   losses/l2.h:40-74, losses/relative_l2.h:40-75                     -> k_loss
//   reduce_sum.h:52-157          block_reduce + atomicAdd             -> k_reduce_stage1 / k_reduce_stage2 (deterministic)
//   optimizers/adam.h:48-119     adam_step                            -> k_adam
//   random.h:40-55               generate_random_kernel               -> k_random_uniform
//   common_device.h:990-1014     trim_and_cast / cast / cast_from     -> k_trim_and_cast / k_cast_*
#include "tcnn_common.h"
#include "adam_device.h"
#include "grid_fixed.h"
#include "loss_device.h"
#include "mlp_side_jobs.h"
#include "oneblob_device.h"
#include "reduce_device.h"

#include <hip/hip_fp16.h>

#include <cstring>

#include <cmath>
#include <limits>

namespace tcnn_amd {
namespace {

typedef _Float16 half_t;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// OneBlob, definition form of oneblob.h:47-67: bin k = C(l_{k+1}) - C(l_k), C(l) = cdf(l-x) + cdf(l-x-1) + cdf(l-x+1),
// the last bin's right edge is bin 0's left edge + 1 (wrap-around).  One thread per output element (AoS).
template <typename T>
__global__ void __launch_bounds__(256) k_oneblob_fwd(const uint32_t n, const uint32_t n_dims, const uint32_t log2_bins, const MatView x, T* __restrict__ out, const uint32_t out_stride) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / out_stride;
	if (i >= n) return;
	const uint32_t j = gid - i * out_stride;
	const uint32_t n_bins = 1u << log2_bins;
	if (j >= n_dims * n_bins) { // oneblob.h:207-209
		out[gid] = (T)1.0f;
		return;
	}
	const uint32_t dim = j >> log2_bins, bin = j & (n_bins - 1);
	const float xv = x.data[(size_t)i * x.stride_sample + (size_t)dim * x.stride_dim];
	const float nb = (float)n_bins;
	const float lb = scalbnf((float)bin, -(int)log2_bins);
	const float l = quartic_cdf(lb - xv, nb) + quartic_cdf(lb - xv - 1.0f, nb) + quartic_cdf(lb - xv + 1.0f, nb);
	const float rb = scalbnf((float)((bin + 1) & (n_bins - 1)), -(int)log2_bins);
	float r = quartic_cdf(rb - xv, nb) + quartic_cdf(rb - xv - 1.0f, nb) + quartic_cdf(rb - xv + 1.0f, nb);
	if (bin == n_bins - 1) r += 1;
	out[gid] = (T)(r - l);
}

// The same, 8 consecutive bins per thread (n_bins and out_stride multiples of 8): the 9 bin edges are evaluated once each --
// the right edge of bin k IS the left edge of bin k + 1, bit for bit -- and the 8 results leave in one store.  27 cdf evaluations
// for 8 outputs instead of 48: the element-per-thread form took 26 of C2's 84 us per step, ALU-bound.
template <typename T>
__global__ void __launch_bounds__(256) k_oneblob_fwd8(const uint32_t n, const uint32_t n_dims, const uint32_t log2_bins, const MatView x, T* __restrict__ out, const uint32_t out_stride) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t chunks = out_stride / 8;
	const uint32_t i = gid / chunks;
	if (i >= n) return;
	const uint32_t j0 = (gid - i * chunks) * 8;
	const uint32_t n_bins = 1u << log2_bins;
	typedef T vec8 __attribute__((ext_vector_type(8)));
	vec8 v;
	if (j0 >= n_dims * n_bins) { // oneblob.h:207-209
#pragma unroll
		for (int k = 0; k < 8; ++k) v[k] = (T)1.0f;
	} else {
		const uint32_t dim = j0 >> log2_bins, b0 = j0 & (n_bins - 1);
		const float xv = x.data[(size_t)i * x.stride_sample + (size_t)dim * x.stride_dim];
		const float nb = (float)n_bins;
		float edge[9];
#pragma unroll
		for (int k = 0; k < 9; ++k) {
			const float lb = scalbnf((float)((b0 + k) & (n_bins - 1)), -(int)log2_bins);
			edge[k] = quartic_cdf(lb - xv, nb) + quartic_cdf(lb - xv - 1.0f, nb) + quartic_cdf(lb - xv + 1.0f, nb);
		}
		if (b0 + 8 == n_bins) edge[8] += 1; // the last bin's right edge is bin 0's left edge + 1
#pragma unroll
		for (int k = 0; k < 8; ++k) v[k] = (T)(edge[k + 1] - edge[k]);
	}
	*(vec8*)(out + (size_t)i * out_stride + j0) = v;
}

// The same, 8 consecutive bins per thread, for rows that are mostly zeros.  The quartic kernel has radius 1 / n_bins, so for an
// input in [0, 1] only the bins within one bin of x (and of its wrap-around images x +- 1, which fall on the same bins modulo
// n_bins) see anything but saturated cdf values; every other bin is a difference of equal integers, exactly +0.  The n_bins / 8
// threads of a row (consecutive lanes of one wave) share the work on the five bins floor(x n_bins) - 2 .. + 2 -- evaluated in the
// definition form, same operations, same bits -- exchange them with lane shuffles, and every thread stores its 8 bins: 30 cdf
// evaluations per row instead of 27 per 8 bins (k_oneblob_fwd8 was ALU-bound: 14.5 of C2's 60 us), dense 1 KB stores per wave.
// Inputs outside [0, 1] take the general form.  The threads behind the last row write the padding columns (ones, oneblob.h:207-209).
template <typename T, int CPR> // CPR = n_bins / 8 = threads per row, a power of two <= 64
__global__ void __launch_bounds__(256) k_oneblob_fwd_sparse(const uint32_t n, const uint32_t n_dims, const uint32_t log2_bins, const MatView x, T* __restrict__ out, const uint32_t out_stride) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	typedef T vec8 __attribute__((ext_vector_type(8)));
	const uint32_t n_bins = 1u << log2_bins;
	constexpr uint32_t cpr = CPR;
	const uint32_t row_threads = n * n_dims * cpr;
	if (gid >= row_threads) {
		const uint32_t pad_chunks = (out_stride - n_dims * n_bins) >> 3;
		const uint32_t p = gid - row_threads;
		if (pad_chunks == 0 || p >= n * pad_chunks) return;
		const uint32_t i = p / pad_chunks, pc = p - i * pad_chunks;
		vec8 ones;
#pragma unroll
		for (int k = 0; k < 8; ++k) ones[k] = (T)1.0f;
		*(vec8*)(out + (size_t)i * out_stride + n_dims * n_bins + 8 * pc) = ones;
		return;
	}
	const uint32_t r = gid / cpr, j = gid - r * cpr; // row, chunk of 8 bins inside it
	const uint32_t i = r / n_dims, dim = r - i * n_dims;
	const uint32_t b0 = 8 * j;
	const float xv = x.data[(size_t)i * x.stride_sample + (size_t)dim * x.stride_dim];
	const float nb = (float)n_bins;
	auto edge = [&](const uint32_t bin) {
		const float lb = scalbnf((float)(bin & (n_bins - 1)), -(int)log2_bins);
		return quartic_cdf(lb - xv, nb) + quartic_cdf(lb - xv - 1.0f, nb) + quartic_cdf(lb - xv + 1.0f, nb);
	};
	vec8 v;
	if (!(xv >= 0.0f && xv <= 1.0f)) { // general form (k_oneblob_fwd8); the threads of a row agree about this branch
		float e[9];
#pragma unroll
		for (int k = 0; k < 9; ++k) e[k] = edge(b0 + k);
		if (b0 + 8 == n_bins) e[8] += 1;
#pragma unroll
		for (int k = 0; k < 8; ++k) v[k] = (T)(e[k + 1] - e[k]);
	} else {
		const uint32_t centre = (uint32_t)(int)floorf(xv * nb) + n_bins - 2u; // window bin o is (centre + o) mod n_bins, o = 0..4: distinct since n_bins >= 8
		// thread j evaluates the window bins j, j + CPR, ... (every thread the same number of them: a surplus thread repeats bin 4)
		constexpr int PER = (5 + CPR - 1) / CPR;
		float mine[PER];
#pragma unroll
		for (int t = 0; t < PER; ++t) {
			const uint32_t o = min(j + (uint32_t)t * cpr, 4u);
			const uint32_t bin = (centre + o) & (n_bins - 1);
			const float l = edge(bin);
			float rr = edge(bin + 1);
			if (bin == n_bins - 1) rr += 1; // the last bin's right edge is bin 0's left edge + 1
			mine[t] = rr - l;
		}
#pragma unroll
		for (int k = 0; k < 8; ++k) v[k] = (T)0.0f;
#pragma unroll
		for (int o = 0; o < 5; ++o) {
			const float val = CPR == 1 ? mine[o / CPR] : __shfl(mine[o / CPR], o % CPR, CPR);
			const uint32_t d = ((centre + o) & (n_bins - 1)) - b0;
#pragma unroll
			for (int k = 0; k < 8; ++k) v[k] = d == (uint32_t)k ? (T)val : v[k];
		}
	}
	*(vec8*)(out + (size_t)i * out_stride + (size_t)dim * n_bins + b0) = v;
}

template <typename T>
__global__ void __launch_bounds__(128) k_oneblob_bwd_input(const uint32_t n, const uint32_t n_dims, const uint32_t log2_bins, const MatView x, const T* __restrict__ dL_dy, const uint32_t dy_stride, const MatViewMut dL_dx) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_dims;
	if (i >= n) return;
	const uint32_t j = gid - i * n_dims;
	const uint32_t n_bins = 1u << log2_bins;
	const float nb = (float)n_bins;
	const float xv = x.data[(size_t)i * x.stride_sample + (size_t)j * x.stride_dim];
	float result = 0;
	float left = quartic_cdf_deriv(-xv, nb) + quartic_cdf_deriv(-xv - 1.0f, nb) + quartic_cdf_deriv(-xv + 1.0f, nb);
	for (uint32_t k = 0; k < n_bins; ++k) {
		const float rb = scalbnf((float)(k + 1), -(int)log2_bins);
		const float right = quartic_cdf_deriv(rb - xv, nb) + quartic_cdf_deriv(rb - xv - 1.0f, nb) + quartic_cdf_deriv(rb - xv + 1.0f, nb);
		const float deriv = left - right;
		left = right;
		result += (float)dL_dy[(size_t)i * dy_stride + j * n_bins + k] * deriv;
	}
	dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)j * dL_dx.stride_dim] = result;
}

template <typename T>
__global__ void __launch_bounds__(256) k_identity_fwd(const uint32_t n, const uint32_t n_dims, const float scale, const float offset, const MatView x, T* __restrict__ out, const uint32_t out_stride) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / out_stride;
	if (i >= n) return;
	const uint32_t j = gid - i * out_stride;
	out[gid] = j >= n_dims ? (T)1.0f : (T)(x.data[(size_t)i * x.stride_sample + (size_t)j * x.stride_dim] * scale + offset);
}

template <typename T>
__global__ void __launch_bounds__(256) k_identity_bwd_input(const uint32_t n, const uint32_t n_dims, const float scale, const T* __restrict__ dL_dy, const uint32_t dy_stride, const MatViewMut dL_dx) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_dims;
	if (i >= n) return;
	const uint32_t j = gid - i * n_dims;
	dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)j * dL_dx.stride_dim] = (float)(T)((float)dL_dy[(size_t)i * dy_stride + j] * scale);
}

template <typename T>
__global__ void __launch_bounds__(256) k_identity_bwd_bwd_input(const uint32_t n, const uint32_t n_dims, const float scale, const MatView dL_ddLdx, T* __restrict__ dL_ddLdy, const uint32_t dy_stride) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / dy_stride;
	if (i >= n) return;
	const uint32_t j = gid - i * dy_stride;
	dL_ddLdy[gid] = j >= n_dims ? (T)0.0f : (T)(dL_ddLdx.data[(size_t)i * dL_ddLdx.stride_sample + (size_t)j * dL_ddLdx.stride_dim] * scale);
}

// ---- loss: one element is loss_element (loss_device.h), the reference's expressions term for term

// one thread per padded output element (any stride)
template <typename P>
__global__ void __launch_bounds__(256) k_loss(
	const uint32_t type, const uint32_t n_elements, const uint32_t stride, const uint32_t dims, const float loss_scale,
	const P* __restrict__ predictions, const float* __restrict__ targets, float* __restrict__ values, P* __restrict__ gradients, const float* __restrict__ data_pdf
) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_elements) return;
	const uint32_t intra = i % stride;
	const uint32_t inter = i / stride;
	if (intra >= dims) {
		values[i] = 0;
		gradients[i] = (P)0.0f;
		return;
	}
	const uint32_t target_idx = inter * dims + intra;
	const uint32_t n_total = n_elements / stride * dims;
	const float prediction = (float)predictions[i];
	const float pdf = data_pdf ? data_pdf[target_idx] : 1;
	float value;
	P grad;
	loss_element(type, prediction, targets[target_idx], pdf, n_total, loss_scale, predictions + (i - intra), dims, value, grad);
	values[i] = value;
	gradients[i] = grad;
}

// The same for strides that are multiples of 8 (every network's padded output): eight consecutive elements per thread -- one 16-byte load of
// predictions, one 16-byte store of gradients, two of values -- and ONE division by the stride per thread instead of three per element
// (round 5: 20 -> 13 us at 2^18 x 16, the unfused step's loss launch).  Same expressions per element, same bits.
__global__ void __launch_bounds__(256) k_loss8(
	const uint32_t type, const uint32_t n_elements, const uint32_t stride, const uint32_t dims, const uint32_t n_total, const float loss_scale,
	const half_t* __restrict__ predictions, const float* __restrict__ targets, float* __restrict__ values, half_t* __restrict__ gradients, const float* __restrict__ data_pdf
) {
	const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
	if (i0 >= n_elements) return;
	const uint32_t inter = i0 / stride, intra0 = i0 - inter * stride;
	const h8 pv = *(const h8*)(predictions + i0);
	float v[8];
	h8 g;
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		const uint32_t intra = intra0 + k;
		v[k] = 0;
		g[k] = (half_t)0.0f;
		if (intra < dims) {
			const uint32_t target_idx = inter * dims + intra;
			const float pdf = data_pdf ? data_pdf[target_idx] : 1;
			half_t gk;
			loss_element(type, (float)pv[k], targets[target_idx], pdf, n_total, loss_scale, predictions + (i0 - intra0), dims, v[k], gk);
			g[k] = gk;
		}
	}
	*(float4*)(values + i0) = float4{v[0], v[1], v[2], v[3]};
	*(float4*)(values + i0 + 4) = float4{v[4], v[5], v[6], v[7]};
	*(h8*)(gradients + i0) = g;
}

// Float predictions, strides that are multiples of 4 (every network's padded output): four consecutive elements per thread -- one 16-byte
// load of predictions, one 16-byte store of values, one of gradients.  Same expressions per element as k_loss<float>, same bits.
__global__ void __launch_bounds__(256) k_loss4_f32(
	const uint32_t type, const uint32_t n_elements, const uint32_t stride, const uint32_t dims, const uint32_t n_total, const float loss_scale,
	const float* __restrict__ predictions, const float* __restrict__ targets, float* __restrict__ values, float* __restrict__ gradients, const float* __restrict__ data_pdf
) {
	const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
	if (i0 >= n_elements) return;
	const uint32_t inter = i0 / stride, intra0 = i0 - inter * stride;
	const float4 pv4 = *(const float4*)(predictions + i0);
	const float pv[4] = {pv4.x, pv4.y, pv4.z, pv4.w};
	float v[4], g[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const uint32_t intra = intra0 + k;
		v[k] = 0;
		g[k] = 0;
		if (intra < dims) {
			const uint32_t target_idx = inter * dims + intra;
			const float pdf = data_pdf ? data_pdf[target_idx] : 1;
			loss_element(type, pv[k], targets[target_idx], pdf, n_total, loss_scale, predictions + (i0 - intra0), dims, v[k], g[k]);
		}
	}
	*(float4*)(values + i0) = float4{v[0], v[1], v[2], v[3]};
	*(float4*)(gradients + i0) = float4{g[0], g[1], g[2], g[3]};
}

// ---- deterministic two-stage sum: stage 1 = one partial per block (fixed grid), stage 2 = one block sums the partials
__global__ void __launch_bounds__(256) k_reduce_stage1(const size_t n, const float* __restrict__ values, float* __restrict__ partials) {
	__shared__ float sm[4];
	float acc = 0.0f;
	const size_t n4 = n / 4;
	const float4* v4 = (const float4*)values;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
		const float4 v = v4[i];
		acc += (v.x + v.y) + (v.z + v.w);
	}
	if (blockIdx.x == 0 && threadIdx.x < (n & 3)) acc += values[n4 * 4 + threadIdx.x];
	const float s = block_sum_256(acc, sm);
	if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) k_reduce_stage2(const uint32_t n_partials, const float* __restrict__ partials, float* __restrict__ result) {
	__shared__ float sm[4];
	float acc = 0.0f;
	for (uint32_t i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
	const float s = block_sum_256(acc, sm);
	if (threadIdx.x == 0) *result = s;
}

// ---- Adam, adam.h:48-119.  4 parameters per thread, 16-byte accesses; 36 B/param of HBM traffic is the floor.

// debiasing factor of adam.h:97-98
__device__ inline float adam_debias(const float beta1, const float beta2, uint32_t step) { return sqrtf(1 - powf(beta2, (float)step)) / (1 - powf(beta1, (float)step)); }

// table[t] = adam_debias(t) for t in [from, to): the factor depends on (beta1, beta2, t) only.  Evaluating it per parameter
// (two powf, ~300 instructions) made the kernel ALU-bound, and more so with every step: a grid parameter that misses one
// update (zero gradient) has a step count of its own from then on, so after a few dozen steps almost every parameter does.
__global__ void __launch_bounds__(256) k_adam_debias_table(const float beta1, const float beta2, const uint32_t from, const uint32_t to, float* __restrict__ table) {
	const uint32_t t = from + blockIdx.x * blockDim.x + threadIdx.x;
	if (t < to) table[t] = adam_debias(beta1, beta2, t);
}

constexpr int ADAM_Q = 1; // quads (of 4 parameters) per thread, one block-width apart (measured: 1 -> 82 us, 2 -> 84 us, 4 -> 91 us on C3a; occupancy wins)

// QUAD_UNIFORM: n_matrix is a multiple of 4, so the 4 parameters of a quad are all matrix weights or all not
// STEP_T: uint32_t, or uint16_t while every count fits (AdamOptimizer widens the array before one could overflow)
typedef uint16_t adam_u16x4 __attribute__((ext_vector_type(4)));
template <typename STEP_T> __device__ inline uint4 adam_load_steps(const STEP_T* p) {
	if constexpr (sizeof(STEP_T) == 2) {
		const adam_u16x4 v = *(const adam_u16x4*)p;
		return uint4{v[0], v[1], v[2], v[3]};
	} else {
		return *(const uint4*)p;
	}
}
template <typename STEP_T> __device__ inline void adam_store_steps(STEP_T* p, const uint4 v) {
	if constexpr (sizeof(STEP_T) == 2) *(adam_u16x4*)p = adam_u16x4{(uint16_t)v.x, (uint16_t)v.y, (uint16_t)v.z, (uint16_t)v.w};
	else *(uint4*)p = v;
}
// G: the gradients' type, half_t (8-byte quads) or float (16-byte quads: a caller's own fp32 gradients, standalone optimizers)
typedef float f4 __attribute__((ext_vector_type(4)));
template <typename G> struct GradQuad;
template <> struct GradQuad<half_t> { typedef h4 type; };
template <> struct GradQuad<float> { typedef f4 type; };
// W: the working weights' type.  half_t: w is the half copy of w_fp.  float: w_fp is the optimizer's one weight vector -- read once, stored
// once, w is not touched (30 - 32 B/param instead of 32 - 36) -- and G is float.
// debias_table at min(step + 1, common_step) for each of a quad's parameters: requested together, in front of the arithmetic
__device__ inline void adam_load_debias(const float* __restrict__ debias_table, const uint32_t common_step, const uint4 st, float (&debias)[4]) {
	debias[0] = debias_table[min(st.x + 1, common_step)];
	debias[1] = debias_table[min(st.y + 1, common_step)];
	debias[2] = debias_table[min(st.z + 1, common_step)];
	debias[3] = debias_table[min(st.w + 1, common_step)];
}
// one parameter on its own (ragged tails, unaligned ranges, the MLP's weights behind their slab sums)
template <typename STEP_T, typename G, typename W>
__device__ inline void adam_single(const AdamArgs& a, const float* __restrict__ debias_table, const bool is_matrix, const size_t i, const G g, float* __restrict__ w_fp, W* __restrict__ w,
                                   float* __restrict__ m1, float* __restrict__ m2, STEP_T* __restrict__ steps) {
	bool up;
	W wh;
	uint32_t st1 = steps[i];
	adam_one(a, debias_table[min(st1 + 1, a.common_step)], is_matrix, g, w_fp[i], wh, m1[i], m2[i], st1, up);
	steps[i] = (STEP_T)st1;
	if constexpr (sizeof(W) == 2) { if (up) w[i] = wh; }
}

// PLAIN: adam_device.h (a power-of-two loss scale and no weight clipping, found by the host)
template <bool PLAIN, bool QUAD_UNIFORM, typename STEP_T, typename G, typename W>
__global__ void __launch_bounds__(256) k_adam(
	const AdamArgs a, const size_t n, const size_t n_matrix,
	float* __restrict__ w_fp, W* __restrict__ w, const G* __restrict__ g, float* __restrict__ m1, float* __restrict__ m2, STEP_T* __restrict__ steps,
	const float* __restrict__ debias_table
) {
	const size_t base = (size_t)blockIdx.x * (256 * 4 * ADAM_Q) + threadIdx.x * 4;
	// phase 1: the gradients of all quads (8 B each, 16 B for fp32 gradients).  Grid (non-matrix) quads whose 4 gradients are all zero are skipped
	// without touching the other 32 B/param (adam.h:76-79 returns before reading anything else).
	typedef typename GradQuad<G>::type g4;
	g4 gv[ADAM_Q];
	bool live[ADAM_Q];
#pragma unroll
	for (int q = 0; q < ADAM_Q; ++q) {
		const size_t i4 = base + (size_t)q * 1024;
		live[q] = i4 + 4 <= n;
		gv[q] = live[q] ? *(const g4*)(g + i4) : g4{0, 0, 0, 0};
	}
#pragma unroll
	for (int q = 0; q < ADAM_Q; ++q) {
		const size_t i4 = base + (size_t)q * 1024;
		const bool zero = gv[q][0] == (G)0.0f && gv[q][1] == (G)0.0f && gv[q][2] == (G)0.0f && gv[q][3] == (G)0.0f;
		if (live[q] && i4 >= n_matrix && zero) live[q] = false;
	}
	// phase 2: all remaining loads in flight together; the counts first, the debias factors they select right behind them
	float4 wf[ADAM_Q], a1[ADAM_Q], a2[ADAM_Q];
	uint4 st[ADAM_Q];
	float debias[ADAM_Q][4];
#pragma unroll
	for (int q = 0; q < ADAM_Q; ++q) {
		const size_t i4 = base + (size_t)q * 1024;
		if (live[q]) {
			st[q] = adam_load_steps(steps + i4);
			wf[q] = *(const float4*)(w_fp + i4);
			a1[q] = *(const float4*)(m1 + i4);
			a2[q] = *(const float4*)(m2 + i4);
			adam_load_debias(debias_table, a.common_step, st[q], debias[q]);
		}
	}
#pragma unroll
	for (int q = 0; q < ADAM_Q; ++q) {
		const size_t i4 = base + (size_t)q * 1024;
		if (live[q]) {
			W wh[4];
			bool up[4];
			const bool quad_matrix = i4 < n_matrix;
			const bool is_matrix[4] = {QUAD_UNIFORM ? quad_matrix : i4 + 0 < n_matrix, QUAD_UNIFORM ? quad_matrix : i4 + 1 < n_matrix, QUAD_UNIFORM ? quad_matrix : i4 + 2 < n_matrix,
			                           QUAD_UNIFORM ? quad_matrix : i4 + 3 < n_matrix};
			const G gq[4] = {gv[q][0], gv[q][1], gv[q][2], gv[q][3]};
			float w4[4] = {wf[q].x, wf[q].y, wf[q].z, wf[q].w}, f4_[4] = {a1[q].x, a1[q].y, a1[q].z, a1[q].w}, s4[4] = {a2[q].x, a2[q].y, a2[q].z, a2[q].w};
			uint32_t c4[4] = {st[q].x, st[q].y, st[q].z, st[q].w};
			adam_four<PLAIN>(a, debias[q], is_matrix, gq, w4, wh, f4_, s4, c4, up);
			*(float4*)(w_fp + i4) = float4{w4[0], w4[1], w4[2], w4[3]};
			*(float4*)(m1 + i4) = float4{f4_[0], f4_[1], f4_[2], f4_[3]};
			*(float4*)(m2 + i4) = float4{s4[0], s4[1], s4[2], s4[3]};
			adam_store_steps(steps + i4, uint4{c4[0], c4[1], c4[2], c4[3]});
			if constexpr (sizeof(W) == 2) {
				if (up[0] && up[1] && up[2] && up[3]) {
					*(h4*)(w + i4) = h4{wh[0], wh[1], wh[2], wh[3]};
				} else { // skipped parameters keep their half value, whatever it is: only the updated ones are stored
#pragma unroll
					for (int e = 0; e < 4; ++e) if (up[e]) w[i4 + e] = wh[e];
				}
			}
		} else if (i4 < n && i4 + 4 > n) { // ragged tail
			for (size_t i = i4; i < n; ++i) adam_single(a, debias_table, i < n_matrix, i, g[i], w_fp, w, m1, m2, steps);
		}
	}
}

// One parameter per thread, no vector accesses: for parameter ranges that do not start on a 16-byte boundary (a Composite
// optimizer hands its nested optimizers slices at arbitrary offsets, optimizers/composite.h:126-135)
template <typename STEP_T, typename G, typename W>
__global__ void __launch_bounds__(256) k_adam_scalar(
	const AdamArgs a, const size_t n, const size_t n_matrix,
	float* __restrict__ w_fp, W* __restrict__ w, const G* __restrict__ g, float* __restrict__ m1, float* __restrict__ m2, STEP_T* __restrict__ steps,
	const float* __restrict__ debias_table
) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	adam_single(a, debias_table, i < n_matrix, i, g[i], w_fp, w, m1, m2, steps);
}

// ---- pcg32 strided uniform fill, random.h:40-55 (N_TO_GENERATE = 4, thread i advances a copy of the rng by 4 i)
__global__ void __launch_bounds__(128) k_random_uniform(const size_t n, const uint64_t state, const uint64_t inc, float* __restrict__ out, const float lower, const float upper) {
	const uint64_t MULT = 0x5851f42d4c957f2dULL;
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	const size_t n_threads = (size_t)blockDim.x * gridDim.x;
	// advance(4 i)
	uint64_t cur_mult = MULT, cur_plus = inc, acc_mult = 1u, acc_plus = 0u;
	uint64_t delta = (uint64_t)i * 4;
	while (delta > 0) {
		if (delta & 1) {
			acc_mult *= cur_mult;
			acc_plus = acc_plus * cur_mult + cur_plus;
		}
		cur_plus = (cur_mult + 1) * cur_plus;
		cur_mult *= cur_mult;
		delta /= 2;
	}
	uint64_t st = acc_mult * state + acc_plus;
	for (size_t j = 0; j < 4; ++j) {
		const size_t idx = i + n_threads * j;
		if (idx >= n) return;
		const uint64_t old = st;
		st = old * MULT + inc;
		const uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
		const uint32_t rot = (uint32_t)(old >> 59u);
		const uint32_t u = ((xorshifted >> rot) | (xorshifted << ((~rot + 1u) & 31)));
		const float f = __uint_as_float((u >> 9) | 0x3f800000u) - 1.0f;
		out[idx] = f * (upper - lower) + lower;
	}
}

__global__ void __launch_bounds__(256) k_cast_f2h(const size_t n, const float* __restrict__ in, half_t* __restrict__ out) {
	const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
	if (i + 4 <= n) {
		const float4 v = *(const float4*)(in + i);
		*(h4*)(out + i) = h4{(half_t)v.x, (half_t)v.y, (half_t)v.z, (half_t)v.w};
	} else {
		for (size_t k = i; k < n; ++k) out[k] = (half_t)in[k];
	}
}

__global__ void __launch_bounds__(256) k_cast_h2f(const size_t n, const half_t* __restrict__ in, float* __restrict__ out) {
	const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
	if (i + 4 <= n) {
		const h4 v = *(const h4*)(in + i);
		*(float4*)(out + i) = float4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
	} else {
		for (size_t k = i; k < n; ++k) out[k] = (float)in[k];
	}
}

template <typename T>
__global__ void __launch_bounds__(256) k_trim_and_cast(const uint32_t n, const uint32_t in_stride, const uint32_t dims, const T* __restrict__ in, const MatViewMut out) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / dims;
	if (i >= n) return;
	const uint32_t d = gid - i * dims;
	out.data[(size_t)i * out.stride_sample + (size_t)d * out.stride_dim] = (float)in[(size_t)i * in_stride + d];
}

__global__ void __launch_bounds__(256) k_fill_half(const size_t n, half_t* __restrict__ out, const half_t v) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = v;
}

inline uint32_t log2_exact(uint32_t v) {
	uint32_t l = 0;
	while ((1u << l) < v) ++l;
	return l;
}

inline uint32_t blocks_for(uint64_t total, uint32_t threads) {
	const uint64_t b = (total + threads - 1) / threads;
	CHECK_THROW(b < (1ull << 31));
	return (uint32_t)b;
}

} // namespace

void oneblob_forward(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_bins, MatView x, void* out, uint32_t out_stride) {
	const uint64_t total = (uint64_t)n * out_stride;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32));
	const uint32_t lb = log2_exact(n_bins);
	if (n_bins % 8 == 0 && n_bins <= 512 && out_stride % 8 == 0) { // rows of at most 64 threads
		const uint64_t threads = total / 8; // one per 8 outputs, the rows first, then the padding columns
		const dim3 grid(blocks_for(threads, 256));
#define TCNN_ONEBLOB_SPARSE(CPR_) \
		case CPR_: \
			if (fp32) hipLaunchKernelGGL((k_oneblob_fwd_sparse<float, CPR_>), grid, dim3(256), 0, stream, n, n_dims, lb, x, (float*)out, out_stride); \
			else hipLaunchKernelGGL((k_oneblob_fwd_sparse<half_t, CPR_>), grid, dim3(256), 0, stream, n, n_dims, lb, x, (half_t*)out, out_stride); \
			break;
		switch (n_bins / 8) {
			TCNN_ONEBLOB_SPARSE(1) TCNN_ONEBLOB_SPARSE(2) TCNN_ONEBLOB_SPARSE(4) TCNN_ONEBLOB_SPARSE(8)
			TCNN_ONEBLOB_SPARSE(16) TCNN_ONEBLOB_SPARSE(32) TCNN_ONEBLOB_SPARSE(64)
			default: CHECK_THROW(false);
		}
#undef TCNN_ONEBLOB_SPARSE
		return;
	}
	if (n_bins % 8 == 0 && out_stride % 8 == 0) {
		const uint64_t threads = total / 8;
		if (fp32) hipLaunchKernelGGL(k_oneblob_fwd8<float>, dim3(blocks_for(threads, 256)), dim3(256), 0, stream, n, n_dims, lb, x, (float*)out, out_stride);
		else hipLaunchKernelGGL(k_oneblob_fwd8<half_t>, dim3(blocks_for(threads, 256)), dim3(256), 0, stream, n, n_dims, lb, x, (half_t*)out, out_stride);
		return;
	}
	if (fp32) hipLaunchKernelGGL(k_oneblob_fwd<float>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, n_dims, lb, x, (float*)out, out_stride);
	else hipLaunchKernelGGL(k_oneblob_fwd<half_t>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, n_dims, lb, x, (half_t*)out, out_stride);
}

void oneblob_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_bins, MatView x, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	const uint64_t total = (uint64_t)n * n_dims;
	if (total == 0) return;
	const uint32_t lb = log2_exact(n_bins);
	if (fp32) hipLaunchKernelGGL(k_oneblob_bwd_input<float>, dim3(blocks_for(total, 128)), dim3(128), 0, stream, n, n_dims, lb, x, (const float*)dL_dy, dy_stride, dL_dx);
	else hipLaunchKernelGGL(k_oneblob_bwd_input<half_t>, dim3(blocks_for(total, 128)), dim3(128), 0, stream, n, n_dims, lb, x, (const half_t*)dL_dy, dy_stride, dL_dx);
}

void identity_forward(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, float scale, float offset, MatView x, void* out, uint32_t out_stride) {
	const uint64_t total = (uint64_t)n * out_stride;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32));
	if (fp32) hipLaunchKernelGGL(k_identity_fwd<float>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, n_dims, scale, offset, x, (float*)out, out_stride);
	else hipLaunchKernelGGL(k_identity_fwd<half_t>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, n_dims, scale, offset, x, (half_t*)out, out_stride);
}

void identity_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, float scale, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	const uint64_t total = (uint64_t)n * n_dims;
	if (total == 0) return;
	if (fp32) hipLaunchKernelGGL(k_identity_bwd_input<float>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, n_dims, scale, (const float*)dL_dy, dy_stride, dL_dx);
	else hipLaunchKernelGGL(k_identity_bwd_input<half_t>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, n_dims, scale, (const half_t*)dL_dy, dy_stride, dL_dx);
}

void identity_backward_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, float scale, MatView dL_ddLdx, void* dL_ddLdy, uint32_t dy_stride) {
	const uint64_t total = (uint64_t)n * dy_stride;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32));
	if (fp32) hipLaunchKernelGGL(k_identity_bwd_bwd_input<float>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, n_dims, scale, dL_ddLdx, (float*)dL_ddLdy, dy_stride);
	else hipLaunchKernelGGL(k_identity_bwd_bwd_input<half_t>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, n_dims, scale, dL_ddLdx, (half_t*)dL_ddLdy, dy_stride);
}

void loss_evaluate(hipStream_t stream, LossType type, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale,
                   const void* pred_half, const float* target, float* values, void* grads_half, const float* data_pdf, Precision precision) {
	const uint64_t total = (uint64_t)n * stride;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32));
	if (precision == Precision::Fp32) { // (pred_half / grads_half: floats)
		if (stride % 4 == 0 && ((uintptr_t)pred_half | (uintptr_t)values | (uintptr_t)grads_half) % 16 == 0) {
			hipLaunchKernelGGL(k_loss4_f32, dim3(blocks_for(total / 4, 256)), dim3(256), 0, stream, (uint32_t)type, (uint32_t)total, stride, dims, (uint32_t)(total / stride * dims), loss_scale,
			                   (const float*)pred_half, target, values, (float*)grads_half, data_pdf);
			return;
		}
		hipLaunchKernelGGL(k_loss<float>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, (uint32_t)type, (uint32_t)total, stride, dims, loss_scale,
		                   (const float*)pred_half, target, values, (float*)grads_half, data_pdf);
		return;
	}
	if (stride % 8 == 0 && ((uintptr_t)pred_half | (uintptr_t)values | (uintptr_t)grads_half) % 16 == 0) {
		hipLaunchKernelGGL(k_loss8, dim3(blocks_for(total / 8, 256)), dim3(256), 0, stream, (uint32_t)type, (uint32_t)total, stride, dims, (uint32_t)(total / stride * dims), loss_scale,
		                   (const half_t*)pred_half, target, values, (half_t*)grads_half, data_pdf);
		return;
	}
	hipLaunchKernelGGL(k_loss<half_t>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, (uint32_t)type, (uint32_t)total, stride, dims, loss_scale,
	                   (const half_t*)pred_half, target, values, (half_t*)grads_half, data_pdf);
}

void reduce_sum(hipStream_t stream, size_t n, const float* values, float* partials, float* result_dev) {
	uint32_t blocks = blocks_for((n + 3) / 4, 256);
	if (blocks > 1024) blocks = 1024;
	if (blocks == 0) blocks = 1;
	hipLaunchKernelGGL(k_reduce_stage1, dim3(blocks), dim3(256), 0, stream, n, values, partials);
	hipLaunchKernelGGL(k_reduce_stage2, dim3(1), dim3(256), 0, stream, blocks, partials, result_dev);
}

void reduce_partials(hipStream_t stream, uint32_t n_partials, const float* partials, float* result_dev) {
	hipLaunchKernelGGL(k_reduce_stage2, dim3(1), dim3(256), 0, stream, n_partials, partials, result_dev);
}

AdamArgs make_adam_args(const AdamHyper& h, float loss_scale, uint32_t current_step) {
	AdamArgs a;
	a.relative_weight_decay = h.relative_decay;
	a.absolute_weight_decay = h.absolute_decay;
	a.weight_clipping_magnitude = h.clipping_magnitude;
	a.loss_scale = loss_scale;
	a.learning_rate = h.learning_rate;
	a.non_matrix_learning_rate_factor = h.non_matrix_learning_rate_factor;
	a.beta1 = h.beta1;
	a.beta2 = h.beta2;
	a.epsilon = h.epsilon;
	a.lower_lr_bound = 0;
	a.upper_lr_bound = std::numeric_limits<float>::max();
	if (h.adabound) { // adam.h:157-160
		a.lower_lr_bound = 0.1f - 0.1f / ((1 - h.beta2) * (float)current_step + 1);
		a.upper_lr_bound = 0.1f + 0.1f / ((1 - h.beta2) * (float)current_step);
	}
	a.l2_reg = h.l2_reg;
	a.optimize_matrix_params = h.optimize_matrix_params;
	a.optimize_non_matrix_params = h.optimize_non_matrix_params;
	a.common_step = current_step;
	int exponent = 0;
	a.inv_loss_scale_exact = (std::frexp(loss_scale, &exponent) == 0.5f && loss_scale >= 1.0f / 65536 && loss_scale <= 65536.0f) ? 1 : 0;
	a.inv_loss_scale = 1.0f / loss_scale;
	return a;
}

namespace {
// the PLAIN instantiations' condition (adam_device.h): both tests are of launch constants
inline bool adam_args_plain(const AdamArgs& a) { return a.inv_loss_scale_exact != 0 && a.weight_clipping_magnitude == 0.0f; }
__global__ void __launch_bounds__(256) k_adam_widen_steps(const size_t n, const uint16_t* __restrict__ in, uint32_t* __restrict__ out) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = in[i];
}
template <typename STEP_T, typename G, typename W>
void adam_launch(hipStream_t stream, const AdamArgs& a, size_t n, size_t n_matrix, float* w_fp, W* w, const G* g, float* m1, float* m2, STEP_T* steps, const float* debias_table) {
	// the quad kernel reads float4 / 4 step counts / half4 / 4 gradients: every base pointer must allow that (W = float: w is not touched)
	const auto aligned = [](const void* p, size_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; };
	if (!(aligned(w_fp, 16) && aligned(m1, 16) && aligned(m2, 16) && aligned(steps, 4 * sizeof(STEP_T)) && (sizeof(W) == 4 || aligned(w, 8)) && aligned(g, 4 * sizeof(G)))) {
		hipLaunchKernelGGL((k_adam_scalar<STEP_T, G, W>), dim3(blocks_for(n, 256)), dim3(256), 0, stream, a, n, n_matrix, w_fp, w, g, m1, m2, steps, debias_table);
		return;
	}
	const dim3 grid(blocks_for((n + 3) / 4, 256 * ADAM_Q));
	const bool uniform = n_matrix % 4 == 0;
	if (adam_args_plain(a)) {
		if (uniform) hipLaunchKernelGGL((k_adam<true, true, STEP_T, G, W>), grid, dim3(256), 0, stream, a, n, n_matrix, w_fp, w, g, m1, m2, steps, debias_table);
		else hipLaunchKernelGGL((k_adam<true, false, STEP_T, G, W>), grid, dim3(256), 0, stream, a, n, n_matrix, w_fp, w, g, m1, m2, steps, debias_table);
	} else if (uniform) hipLaunchKernelGGL((k_adam<false, true, STEP_T, G, W>), grid, dim3(256), 0, stream, a, n, n_matrix, w_fp, w, g, m1, m2, steps, debias_table);
	else hipLaunchKernelGGL((k_adam<false, false, STEP_T, G, W>), grid, dim3(256), 0, stream, a, n, n_matrix, w_fp, w, g, m1, m2, steps, debias_table);
}
template <typename G, typename W>
void adam_launch_steps(hipStream_t stream, const AdamArgs& a, size_t n, size_t n_matrix, float* w_fp, W* w, const G* g, float* m1, float* m2, void* steps, bool steps16, const float* debias_table) {
	if (steps16) adam_launch<uint16_t, G, W>(stream, a, n, n_matrix, w_fp, w, g, m1, m2, (uint16_t*)steps, debias_table);
	else adam_launch<uint32_t, G, W>(stream, a, n, n_matrix, w_fp, w, g, m1, m2, (uint32_t*)steps, debias_table);
}
} // namespace

void adam_widen_steps(hipStream_t stream, size_t n, const void* steps16, void* steps32) {
	if (n == 0) return;
	hipLaunchKernelGGL(k_adam_widen_steps, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, (const uint16_t*)steps16, (uint32_t*)steps32);
}

void adam_step(hipStream_t stream, const AdamHyper& h, size_t n, size_t n_matrix, float loss_scale, uint32_t current_step,
               float* w_fp, void* w_half, const void* gradients, float* m1, float* m2, void* steps, bool steps16, const float* debias_table, GradientPrecision precision, Precision weight_precision) {
	if (n == 0) return;
	const AdamArgs a = make_adam_args(h, loss_scale, current_step);
	if (weight_precision == Precision::Fp32) {
		CHECK_THROW(precision == GradientPrecision::Fp32);
		adam_launch_steps(stream, a, n, n_matrix, w_fp, (float*)nullptr, (const float*)gradients, m1, m2, steps, steps16, debias_table);
	} else if (precision == GradientPrecision::Fp32) adam_launch_steps(stream, a, n, n_matrix, w_fp, (half_t*)w_half, (const float*)gradients, m1, m2, steps, steps16, debias_table);
	else adam_launch_steps(stream, a, n, n_matrix, w_fp, (half_t*)w_half, (const half_t*)gradients, m1, m2, steps, steps16, debias_table);
}

// ---- Adam with the backward pass's last two reductions in front (AdamPrologue, tcnn_common.h): workgroups [0, n_reduce_blocks) sum the MLP's
// weight-gradient slabs (the order of mlp_reduce_block, mlp_side_jobs.h) and step those weights; the next pro_range_blocks() per shared
// range round the scatter's exact sums into the gradient (what k_grid_scatter_finalize does) and step those parameters; the others are
// k_adam on everything else.  Whoever writes a gradient's final value applies adam_one to it at once.
namespace {
constexpr uint32_t PRO_THREADS = SLAB_REDUCE_ELEMS * SLAB_REDUCE_GROUPS; // 1024
constexpr uint32_t PRO_MAX_BLOCKS_PER_RANGE = 64;
// workgroups of a shared range: one per 1024 quads, at most 64 (k_grid_scatter_finalize's number)
__host__ __device__ inline uint32_t pro_range_blocks(const uint32_t n_elems) { return min(PRO_MAX_BLOCKS_PER_RANGE, max(1u, (n_elems / 4 + PRO_THREADS - 1) / PRO_THREADS)); }

template <bool PLAIN, typename STEP_T>
__device__ inline void adam_quad(const AdamArgs& a, const float* __restrict__ debias_table, const bool quad_matrix, const size_t i4, const h4 gv,
                                 float* __restrict__ w_fp, half_t* __restrict__ w, float* __restrict__ m1, float* __restrict__ m2, STEP_T* __restrict__ steps) {
	// adam.h:76-79: a grid parameter with a zero gradient is left alone -- nothing else of it is read
	if (!quad_matrix && gv[0] == (half_t)0.0f && gv[1] == (half_t)0.0f && gv[2] == (half_t)0.0f && gv[3] == (half_t)0.0f) return;
	const uint4 st = adam_load_steps(steps + i4); // first: the debias factors wait for it alone
	const float4 wf = *(const float4*)(w_fp + i4), a1 = *(const float4*)(m1 + i4), a2 = *(const float4*)(m2 + i4);
	float debias[4];
	adam_load_debias(debias_table, a.common_step, st, debias);
	half_t wh[4];
	bool up[4];
	const bool is_matrix[4] = {quad_matrix, quad_matrix, quad_matrix, quad_matrix};
	const half_t gq[4] = {gv[0], gv[1], gv[2], gv[3]};
	float w4[4] = {wf.x, wf.y, wf.z, wf.w}, f4_[4] = {a1.x, a1.y, a1.z, a1.w}, s4[4] = {a2.x, a2.y, a2.z, a2.w};
	uint32_t c4[4] = {st.x, st.y, st.z, st.w};
	adam_four<PLAIN>(a, debias, is_matrix, gq, w4, wh, f4_, s4, c4, up);
	*(float4*)(w_fp + i4) = float4{w4[0], w4[1], w4[2], w4[3]};
	*(float4*)(m1 + i4) = float4{f4_[0], f4_[1], f4_[2], f4_[3]};
	*(float4*)(m2 + i4) = float4{s4[0], s4[1], s4[2], s4[3]};
	adam_store_steps(steps + i4, uint4{c4[0], c4[1], c4[2], c4[3]});
	if (up[0] && up[1] && up[2] && up[3]) {
		*(h4*)(w + i4) = h4{wh[0], wh[1], wh[2], wh[3]};
	} else { // skipped parameters keep their half value, whatever it is
#pragma unroll
		for (int e = 0; e < 4; ++e) if (up[e]) w[i4 + e] = wh[e];
	}
}

struct PrologueArgs {
	uint32_t n_reduce_blocks, reduce_elems, reduce_slabs;
	int reduce_accumulate;
	const float* slabs;
	const GridScatterRange* ranges;
	uint32_t n_ranges, n_range_blocks; // (the sum of pro_range_blocks over the ranges)
	int accumulate;
	unsigned long long* scratch;
	size_t range_base; // parameter index of the gradient element the ranges' grad_begin counts from
	size_t bulk_begin; // first parameter of the k_adam part (behind the MLP's weights when their slabs are summed here)
};

// (98 scalar registers per wave admit ONE 16-wave workgroup per CU.  Limiting them to 80 -- amdgpu_num_sgpr, two workgroups per CU, the
// 8 waves per SIMD k_adam keeps -- was measured on C3a, same device, three alternations: optimizer 61.0 - 62.5 us against 58.8 - 59.8.)
#ifndef TCNN_PRO_BOUNDS
#define TCNN_PRO_BOUNDS __launch_bounds__(PRO_THREADS)
#endif
#ifndef TCNN_PRO_Q
#define TCNN_PRO_Q 1
#endif
constexpr int PRO_Q = TCNN_PRO_Q; // quads per thread of the k_adam part, one workgroup width apart
template <bool PLAIN, typename STEP_T>
__global__ void TCNN_PRO_BOUNDS k_adam_prologue(const AdamArgs a, const size_t n, const size_t n_matrix, float* __restrict__ w_fp, half_t* __restrict__ w, half_t* __restrict__ g,
                                                               float* __restrict__ m1, float* __restrict__ m2, STEP_T* __restrict__ steps, const float* __restrict__ debias_table, const PrologueArgs p) {
	__shared__ float part[SLAB_REDUCE_GROUPS * SLAB_REDUCE_ELEMS];
	const uint32_t tid = threadIdx.x;
	if (blockIdx.x < p.n_reduce_blocks) {
		// mlp_reduce_block's sum of element i over the slabs, term for term
		const uint32_t e = tid & (SLAB_REDUCE_ELEMS - 1), grp = tid / SLAB_REDUCE_ELEMS;
		const uint32_t i = blockIdx.x * SLAB_REDUCE_ELEMS + e;
		float q[4] = {0, 0, 0, 0};
		if (i < p.reduce_elems) {
			uint32_t k = grp;
			for (; k + 3 * SLAB_REDUCE_GROUPS < p.reduce_slabs; k += 4 * SLAB_REDUCE_GROUPS) {
#pragma unroll
				for (int u = 0; u < 4; ++u) q[u] += p.slabs[(size_t)(k + u * SLAB_REDUCE_GROUPS) * p.reduce_elems + i];
			}
			for (; k < p.reduce_slabs; k += SLAB_REDUCE_GROUPS) q[0] += p.slabs[(size_t)k * p.reduce_elems + i];
		}
		part[grp * SLAB_REDUCE_ELEMS + e] = (q[0] + q[1]) + (q[2] + q[3]);
		__syncthreads();
		if (grp == 0 && i < p.reduce_elems) {
			float s = 0;
#pragma unroll
			for (int gi = 0; gi < SLAB_REDUCE_GROUPS; ++gi) s += part[gi * SLAB_REDUCE_ELEMS + e];
			if (p.reduce_accumulate) s += (float)g[i];
			const half_t gh = (half_t)s;
			g[i] = gh;
			adam_single(a, debias_table, i < n_matrix, i, gh, w_fp, w, m1, m2, steps);
		}
		return;
	}
	const uint32_t b = blockIdx.x - p.n_reduce_blocks;
	if (b < p.n_range_blocks) {
		// k_grid_scatter_finalize's rounding of a shared range, four elements per thread; the scratch is left zero for the next step
		uint32_t ri = 0, first = 0; // which range this workgroup belongs to, and which of the range's workgroups it is
		for (uint32_t nb = pro_range_blocks(p.ranges[0].n_elems); b >= first + nb; nb = pro_range_blocks(p.ranges[ri].n_elems)) { first += nb; ++ri; }
		const GridScatterRange r = p.ranges[ri];
		const uint32_t my = b - first, of = pro_range_blocks(r.n_elems);
		typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
		u64x2* sc = (u64x2*)(p.scratch + r.scratch_begin);
		const size_t g0 = p.range_base + r.grad_begin;
		for (uint32_t quad = my * PRO_THREADS + tid; quad < r.n_elems / 4; quad += of * PRO_THREADS) {
			const u64x2 lo = sc[2 * quad], hi = sc[2 * quad + 1];
			sc[2 * quad] = u64x2{0, 0};
			sc[2 * quad + 1] = u64x2{0, 0};
			long long s[4] = {(long long)lo.x, (long long)lo.y, (long long)hi.x, (long long)hi.y};
			const size_t i4 = g0 + 4 * (size_t)quad;
			if (p.accumulate) {
				const h4 old = *(const h4*)(g + i4);
#pragma unroll
				for (int e = 0; e < 4; ++e) s[e] += half_to_fixed(old[e]);
			}
			const h4 gv = h4{fixed_to_half(s[0]), fixed_to_half(s[1]), fixed_to_half(s[2]), fixed_to_half(s[3])};
			*(h4*)(g + i4) = gv;
			adam_quad<PLAIN>(a, debias_table, i4 < n_matrix, i4, gv, w_fp, w, m1, m2, steps);
		}
		return;
	}
	h4 gv[PRO_Q];
	bool live[PRO_Q];
#pragma unroll
	for (int k = 0; k < PRO_Q; ++k) {
		const size_t i4 = p.bulk_begin + (((size_t)(b - p.n_range_blocks) * PRO_Q + k) * PRO_THREADS + tid) * 4;
		live[k] = i4 < n; // (n - bulk_begin is a multiple of 4: adam_step_with_prologue)
		for (uint32_t r = 0; r < p.n_ranges; ++r) { // the shared ranges have been done above
			const size_t rb = p.range_base + p.ranges[r].grad_begin;
			if (i4 >= rb && i4 < rb + p.ranges[r].n_elems) live[k] = false;
		}
		if (live[k]) gv[k] = *(const h4*)(g + i4);
	}
#pragma unroll
	for (int k = 0; k < PRO_Q; ++k) {
		const size_t i4 = p.bulk_begin + (((size_t)(b - p.n_range_blocks) * PRO_Q + k) * PRO_THREADS + tid) * 4;
		if (live[k]) adam_quad<PLAIN>(a, debias_table, i4 < n_matrix, i4, gv[k], w_fp, w, m1, m2, steps);
	}
}
} // namespace

bool adam_step_with_prologue(hipStream_t stream, const AdamHyper& h, size_t n, size_t n_matrix, float loss_scale, uint32_t current_step,
                             float* w_fp, void* w_half, void* g_half, float* m1, float* m2, void* steps, bool steps16, const float* debias_table, const AdamPrologue& pro) {
	const auto aligned = [](const void* ptr, size_t bytes) { return ((uintptr_t)ptr & (bytes - 1)) == 0; };
	if (n == 0 || !(aligned(w_fp, 16) && aligned(m1, 16) && aligned(m2, 16) && aligned(steps, steps16 ? 8 : 16) && aligned(w_half, 8) && aligned(g_half, 8))) return false;
	PrologueArgs p{};
	p.bulk_begin = 0;
	if (pro.has_reduce) {
		// the MLP's weights are the first parameters and all of the matrix weights: quads must not straddle the end of either
		if (pro.reduce_elems % 4 != 0 || pro.reduce_elems > n || n_matrix % 4 != 0) return false;
		p.n_reduce_blocks = div_round_up(pro.reduce_elems, (uint32_t)SLAB_REDUCE_ELEMS);
		p.reduce_elems = pro.reduce_elems;
		p.reduce_slabs = pro.reduce_slabs;
		p.reduce_accumulate = pro.reduce_accumulate;
		p.slabs = pro.slabs;
		p.bulk_begin = pro.reduce_elems;
	} else if (n_matrix % 4 != 0) return false;
	if ((n - p.bulk_begin) % 4 != 0) return false;
	if (!pro.ranges.empty()) {
		if ((const char*)pro.grad_base < (const char*)g_half || !aligned(pro.scratch, 16)) return false;
		p.range_base = (size_t)((const half_t*)pro.grad_base - (const half_t*)g_half);
		if (p.range_base % 4 != 0) return false;
		for (const GridScatterRange& r : pro.ranges) {
			if (r.grad_begin % 4 != 0 || r.n_elems % 4 != 0 || r.scratch_begin % 2 != 0 || p.range_base + r.grad_begin + r.n_elems > n || p.range_base + r.grad_begin < p.bulk_begin) return false;
		}
		// shared ranges that follow the k_adam part's first parameter without a gap (the coarse levels at the front of the table) are not its
		// business: it starts behind them (its workgroups skip whatever other range they meet)
		for (bool moved = true; moved;) {
			moved = false;
			for (const GridScatterRange& r : pro.ranges) {
				if (r.n_elems && p.range_base + r.grad_begin == p.bulk_begin) { p.bulk_begin += r.n_elems; moved = true; }
			}
		}
		p.ranges = pro.dev_ranges;
		p.n_ranges = (uint32_t)pro.ranges.size();
		for (const GridScatterRange& r : pro.ranges) p.n_range_blocks += pro_range_blocks(r.n_elems);
		p.scratch = (unsigned long long*)pro.scratch;
		p.accumulate = pro.accumulate ? 1 : 0;
	}
	const AdamArgs a = make_adam_args(h, loss_scale, current_step);
	const uint32_t bulk_blocks = div_round_up((uint32_t)((n - p.bulk_begin) / 4), PRO_THREADS * (uint32_t)PRO_Q);
	const dim3 grid(p.n_reduce_blocks + p.n_range_blocks + bulk_blocks);
	if (adam_args_plain(a)) {
		if (steps16) hipLaunchKernelGGL((k_adam_prologue<true, uint16_t>), grid, dim3(PRO_THREADS), 0, stream, a, n, n_matrix, w_fp, (half_t*)w_half, (half_t*)g_half, m1, m2, (uint16_t*)steps, debias_table, p);
		else hipLaunchKernelGGL((k_adam_prologue<true, uint32_t>), grid, dim3(PRO_THREADS), 0, stream, a, n, n_matrix, w_fp, (half_t*)w_half, (half_t*)g_half, m1, m2, (uint32_t*)steps, debias_table, p);
	} else if (steps16) hipLaunchKernelGGL((k_adam_prologue<false, uint16_t>), grid, dim3(PRO_THREADS), 0, stream, a, n, n_matrix, w_fp, (half_t*)w_half, (half_t*)g_half, m1, m2, (uint16_t*)steps, debias_table, p);
	else hipLaunchKernelGGL((k_adam_prologue<false, uint32_t>), grid, dim3(PRO_THREADS), 0, stream, a, n, n_matrix, w_fp, (half_t*)w_half, (half_t*)g_half, m1, m2, (uint32_t*)steps, debias_table, p);
	HIP_CHECK_THROW(hipGetLastError());
	return true;
}

void adam_fill_debias_table(hipStream_t stream, float beta1, float beta2, uint32_t from, uint32_t to, float* table) {
	if (to <= from) return;
	hipLaunchKernelGGL(k_adam_debias_table, dim3(blocks_for(to - from, 256)), dim3(256), 0, stream, beta1, beta2, from, to, table);
}

// ---- the math sweep (adam_math_sweep, tcnn_common.h): adam_device.h's guarded square root and division against the plain expressions
namespace {
__device__ inline uint32_t sweep_hash(const uint32_t v) { // pcg output function on a counter
	const uint32_t s = v * 747796405u + 2891336453u;
	const uint32_t w = ((s >> ((s >> 28u) + 4u)) ^ s) * 277803737u;
	return (w >> 22u) ^ w;
}
__device__ inline void sweep_report(const unsigned long long bad, const unsigned long long first_bad, unsigned long long* __restrict__ out) {
	if (bad) {
		atomicAdd(out, bad);
		atomicMin(out + 1, first_bad);
	}
}
// every bit pattern in [first, first + count)
__global__ void __launch_bounds__(256) k_adam_sweep_sqrt(const uint64_t first, const uint64_t count, unsigned long long* __restrict__ out) {
	unsigned long long bad = 0, first_bad = ~0ull;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
		const uint32_t b = (uint32_t)(first + i);
		const float x = __uint_as_float(b);
		if (__float_as_uint(adam_sqrt(x)) != __float_as_uint(sqrtf(x))) {
			++bad;
			first_bad = min(first_bad, (unsigned long long)b);
		}
	}
	sweep_report(bad, first_bad, out);
}
// every denominator pattern in [first, first + count) against n_numerators numerators whose patterns step evenly from lo_bits to hi_bits
// (the same for every denominator: evenly spread over the binades in between), their low 16 bits hashed
__global__ void __launch_bounds__(256) k_adam_sweep_div_grid(const uint64_t first, const uint64_t count, const uint32_t n_numerators, const uint32_t lo_bits, const uint32_t hi_bits,
                                                             const uint32_t seed, unsigned long long* __restrict__ out) {
	unsigned long long bad = 0, first_bad = ~0ull;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
		const uint32_t db = (uint32_t)(first + i);
		const float d = __uint_as_float(db);
		const uint32_t pitch = (hi_bits - lo_bits) / n_numerators;
		// A denominator outside adam_div's range makes adam_div(n, d) the expression `n / d` itself for every n: comparing that with `n / d`
		// a thousand times is 2 s of divisions that cannot differ.  Such a denominator is visited with the first numerator only.
		const uint32_t n_here = adam_div_d_in_range(d) ? n_numerators : 1u;
		uint32_t lowest = 0xffffffffu;
		for (uint32_t k = 0; k < n_here; ++k) {
			const uint32_t nb = (lo_bits + pitch * k) ^ (sweep_hash(k ^ seed) & 0xffffu);
			const float n = __uint_as_float(nb);
			const bool differs = __float_as_uint(adam_div(n, d)) != __float_as_uint(n / d);
			bad += differs ? 1u : 0u;
			lowest = min(lowest, differs ? nb : 0xffffffffu);
		}
		if (lowest != 0xffffffffu) first_bad = min(first_bad, (unsigned long long)db << 32 | lowest);
	}
	sweep_report(bad, first_bad, out);
}
// `count` seeded pairs around the guard's edges: numerators of 2^-70 .. 2^70, denominators of 2^-54 .. 2^24, a quarter of each negative
__global__ void __launch_bounds__(256) k_adam_sweep_div_pairs(const uint64_t count, const uint32_t seed, unsigned long long* __restrict__ out) {
	unsigned long long bad = 0, first_bad = ~0ull;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
		const uint32_t h1 = sweep_hash((uint32_t)(2 * i) ^ seed), h2 = sweep_hash((uint32_t)(2 * i + 1) ^ seed), h3 = sweep_hash(h1 ^ h2);
		const uint32_t nb = ((127u - 70u + (((h1 >> 23) & 0xffu) * 140u >> 8)) << 23) | (h1 & 0x7fffffu) | ((h3 & 3u) == 0 ? 0x80000000u : 0u);
		const uint32_t db = ((127u - 54u + (((h2 >> 23) & 0xffu) * 78u >> 8)) << 23) | (h2 & 0x7fffffu) | ((h3 & 12u) == 0 ? 0x80000000u : 0u);
		const float n = __uint_as_float(nb), d = __uint_as_float(db);
		if (__float_as_uint(adam_div(n, d)) != __float_as_uint(n / d)) {
			++bad;
			first_bad = min(first_bad, (unsigned long long)db << 32 | nb);
		}
	}
	sweep_report(bad, first_bad, out);
}
} // namespace

void adam_math_sweep(hipStream_t stream, int what, uint64_t first, uint64_t count, uint32_t n_numerators, float numerator_lo, float numerator_hi, uint64_t seed, uint64_t* mismatches,
                     uint64_t* first_bad) {
	CHECK_THROW(what >= 0 && what <= 2 && mismatches != nullptr && first_bad != nullptr);
	CHECK_THROW(what == 2 || first + count <= (1ull << 32));
	uint32_t lo_bits = 0, hi_bits = 0;
	if (what == 1) {
		CHECK_THROW(n_numerators > 0 && numerator_lo > 0.0f && numerator_hi >= numerator_lo && std::isfinite(numerator_hi));
		std::memcpy(&lo_bits, &numerator_lo, 4);
		std::memcpy(&hi_bits, &numerator_hi, 4);
	}
	unsigned long long host[2] = {0ull, ~0ull};
	unsigned long long* out = nullptr;
	HIP_CHECK_THROW(hipMalloc((void**)&out, sizeof(host)));
	hipError_t err = hipMemcpyAsync(out, host, sizeof(host), hipMemcpyHostToDevice, stream);
	if (err == hipSuccess && count) {
		const dim3 grid((uint32_t)std::min<uint64_t>((count + 255) / 256, 8192));
		if (what == 0) hipLaunchKernelGGL(k_adam_sweep_sqrt, grid, dim3(256), 0, stream, first, count, out);
		else if (what == 1) hipLaunchKernelGGL(k_adam_sweep_div_grid, grid, dim3(256), 0, stream, first, count, n_numerators, lo_bits, hi_bits, (uint32_t)seed, out);
		else hipLaunchKernelGGL(k_adam_sweep_div_pairs, grid, dim3(256), 0, stream, count, (uint32_t)seed, out);
		err = hipGetLastError();
	}
	if (err == hipSuccess) err = hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, stream);
	if (err == hipSuccess) err = hipStreamSynchronize(stream);
	(void)hipFree(out);
	HIP_CHECK_THROW(err);
	*mismatches = host[0];
	*first_bad = host[1];
}

namespace {
// optimizers/sgd.h:44-72
template <typename G, typename W>
__global__ void __launch_bounds__(256) k_sgd(const size_t n, const float loss_scale, const float learning_rate, const float l2_reg, float* __restrict__ w_fp, W* __restrict__ w,
                                             const G* __restrict__ g) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float weight_fp = w_fp[i];
	float gradient = (float)g[i] / loss_scale;
	gradient += l2_reg * weight_fp;
	const float new_weight = weight_fp - learning_rate * gradient;
	w_fp[i] = new_weight;
	if constexpr (sizeof(W) == 2) w[i] = (W)new_weight;
}

// optimizers/ema.h:44-78: tmp != nullptr keeps the average in fp32 (full_precision), else it lives in the half weights themselves
template <typename W>
__global__ void __launch_bounds__(256) k_ema(const size_t n, const float decay, const float debias_old, const float debias_new, const W* __restrict__ weights, W* __restrict__ weights_ema,
                                             float* __restrict__ tmp) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float previous = tmp ? tmp[i] : (float)weights_ema[i];
	const float filtered = (previous * decay * debias_old + (float)weights[i] * (1 - decay)) * debias_new;
	if (tmp) tmp[i] = filtered;
	weights_ema[i] = (W)filtered;
}
// optimizers/average.h:44-60: running mean of the last n_samples weight vectors; `current` is the slot the new weights replace
template <typename W>
__global__ void __launch_bounds__(256) k_average_step(const size_t n, const uint32_t n_samples, const W* __restrict__ weights, W* __restrict__ current, W* __restrict__ average) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const W weight = weights[i];
	average[i] = (W)((float)average[i] + ((float)weight - (float)current[i]) / (float)n_samples);
	current[i] = weight;
}
// optimizers/batched.h:44-61: pool (+)= gradient / batch_size_multiplier, restarted with the first gradient of a group
template <typename G>
__global__ void __launch_bounds__(256) k_batched_accumulate(const size_t n, const int first, const uint32_t multiplier, const G* __restrict__ gradients, float* __restrict__ pool) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float v = first ? 0.0f : pool[i];
	v += (float)gradients[i] / (float)multiplier;
	pool[i] = v;
}
// optimizers/novograd.h:44-94.  One workgroup per layer sums the squared gradients (fixed tree: reproducible) and folds the sum
// into the layer's second moment, moment = beta2 moment + (1 - beta2) sum / loss_scale / loss_scale; then the element-wise step.
template <typename G>
__global__ void __launch_bounds__(1024) k_novo_second_moment(const size_t n, const float loss_scale, const float beta2, const G* __restrict__ gradients, float* __restrict__ moment) {
	__shared__ float part[1024];
	float acc = 0.0f;
	for (size_t i = threadIdx.x; i < n; i += 1024) {
		const float g = (float)gradients[i];
		acc += g * g;
	}
	part[threadIdx.x] = acc;
	__syncthreads();
	for (uint32_t stride = 512; stride > 0; stride >>= 1) {
		if (threadIdx.x < stride) part[threadIdx.x] += part[threadIdx.x + stride];
		__syncthreads();
	}
	if (threadIdx.x == 0) *moment = beta2 * *moment + (1 - beta2) * part[0] / loss_scale / loss_scale;
}
template <typename G, typename W>
__global__ void __launch_bounds__(256) k_novo_step(const size_t n, const float relative_weight_decay, const float absolute_weight_decay, const float loss_scale, const float learning_rate,
                                                   const float beta1, const float epsilon, float* __restrict__ weights_fp, W* __restrict__ weights, const G* __restrict__ gradients,
                                                   float* __restrict__ first_moments, const float* __restrict__ layer_second_moment) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float weight_fp = weights_fp[i];
	const float gradient = (float)gradients[i] / loss_scale;
	const float first_moment = beta1 * first_moments[i] + (1 - beta1) * gradient / (sqrtf(*layer_second_moment) + epsilon);
	first_moments[i] = first_moment;
	// weight_decay(rel * lr, abs * lr, w), common_device.h:870-873
	const float decayed_weight = (1 - relative_weight_decay * learning_rate) * weight_fp - copysignf(absolute_weight_decay * learning_rate, weight_fp);
	const float new_weight = decayed_weight - learning_rate * first_moment;
	weights_fp[i] = new_weight;
	if constexpr (sizeof(W) == 2) weights[i] = (W)new_weight;
}
// optimizers/lookahead.h:44-59: slow weights <- slow * (1 - alpha) + fast * alpha, and the fast weights restart from them
template <typename W>
__global__ void __launch_bounds__(256) k_lookahead_step(const size_t n, const float alpha, float* __restrict__ weights_fp, W* __restrict__ weights, W* __restrict__ lookahead) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float new_weight = (float)lookahead[i] * (1.0f - alpha) + weights_fp[i] * alpha;
	weights_fp[i] = new_weight;
	const W h = (W)new_weight;
	lookahead[i] = h;
	if constexpr (sizeof(W) == 2) weights[i] = h;
}
} // namespace

namespace {
// dst[i][dst_col + j] = src[i][src_col + j], j < width (Composite encoding: nested AoS blocks <-> column ranges of the composite row)
template <typename T>
__global__ void __launch_bounds__(256) k_copy_columns(const uint32_t n_elements, const uint32_t width, const T* __restrict__ src, const uint32_t src_stride, const uint32_t src_col,
                                                      T* __restrict__ dst, const uint32_t dst_stride, const uint32_t dst_col) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elements) return;
	const uint32_t i = e / width, j = e - i * width;
	dst[(size_t)i * dst_stride + dst_col + j] = src[(size_t)i * src_stride + src_col + j];
}
} // namespace

void copy_columns(hipStream_t stream, size_t elem_bytes, uint32_t n, const void* src, uint32_t src_stride, uint32_t src_col, void* dst, uint32_t dst_stride, uint32_t dst_col, uint32_t width) {
	const uint64_t total = (uint64_t)n * width;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32) && (elem_bytes == 2 || elem_bytes == 4));
	const dim3 blocks((uint32_t)((total + 255) / 256));
	if (elem_bytes == 2) hipLaunchKernelGGL((k_copy_columns<uint16_t>), blocks, dim3(256), 0, stream, (uint32_t)total, width, (const uint16_t*)src, src_stride, src_col, (uint16_t*)dst, dst_stride, dst_col);
	else hipLaunchKernelGGL((k_copy_columns<uint32_t>), blocks, dim3(256), 0, stream, (uint32_t)total, width, (const uint32_t*)src, src_stride, src_col, (uint32_t*)dst, dst_stride, dst_col);
}

void sgd_step(hipStream_t stream, size_t n, float loss_scale, float learning_rate, float l2_reg, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision, Precision weight_precision) {
	if (n == 0) return;
	if (weight_precision == Precision::Fp32) {
		CHECK_THROW(precision == GradientPrecision::Fp32);
		hipLaunchKernelGGL((k_sgd<float, float>), dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, loss_scale, learning_rate, l2_reg, weights_full_precision, (float*)nullptr, (const float*)gradients);
	} else if (precision == GradientPrecision::Fp32) hipLaunchKernelGGL((k_sgd<float, half_t>), dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, loss_scale, learning_rate, l2_reg, weights_full_precision, (half_t*)weights, (const float*)gradients);
	else hipLaunchKernelGGL((k_sgd<half_t, half_t>), dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, loss_scale, learning_rate, l2_reg, weights_full_precision, (half_t*)weights, (const half_t*)gradients);
}

void average_step(hipStream_t stream, size_t n, uint32_t n_samples, const void* weights, void* current_sample, void* average, Precision weight_precision) {
	if (n == 0) return;
	if (weight_precision == Precision::Fp32) hipLaunchKernelGGL(k_average_step<float>, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, n_samples, (const float*)weights, (float*)current_sample, (float*)average);
	else hipLaunchKernelGGL(k_average_step<half_t>, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, n_samples, (const half_t*)weights, (half_t*)current_sample, (half_t*)average);
}
void batched_accumulate(hipStream_t stream, size_t n, bool first, uint32_t multiplier, const void* gradients, float* pool, GradientPrecision precision) {
	if (n == 0) return;
	if (precision == GradientPrecision::Fp32) hipLaunchKernelGGL(k_batched_accumulate<float>, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, first ? 1 : 0, multiplier, (const float*)gradients, pool);
	else hipLaunchKernelGGL(k_batched_accumulate<half_t>, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, first ? 1 : 0, multiplier, (const half_t*)gradients, pool);
}
void novograd_layer_step(hipStream_t stream, size_t n, float relative_decay, float absolute_decay, float loss_scale, float learning_rate, float beta1, float beta2, float epsilon,
                         float* weights_full_precision, void* weights, const void* gradients, float* first_moments, float* layer_second_moment, GradientPrecision precision, Precision weight_precision) {
	if (n == 0) return;
	if (weight_precision == Precision::Fp32) {
		CHECK_THROW(precision == GradientPrecision::Fp32);
		hipLaunchKernelGGL(k_novo_second_moment<float>, dim3(1), dim3(1024), 0, stream, n, loss_scale, beta2, (const float*)gradients, layer_second_moment);
		hipLaunchKernelGGL((k_novo_step<float, float>), dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, relative_decay, absolute_decay, loss_scale, learning_rate, beta1, epsilon, weights_full_precision,
		                   (float*)nullptr, (const float*)gradients, first_moments, layer_second_moment);
		return;
	}
	if (precision == GradientPrecision::Fp32) {
		hipLaunchKernelGGL(k_novo_second_moment<float>, dim3(1), dim3(1024), 0, stream, n, loss_scale, beta2, (const float*)gradients, layer_second_moment);
		hipLaunchKernelGGL((k_novo_step<float, half_t>), dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, relative_decay, absolute_decay, loss_scale, learning_rate, beta1, epsilon, weights_full_precision,
		                   (half_t*)weights, (const float*)gradients, first_moments, layer_second_moment);
		return;
	}
	hipLaunchKernelGGL(k_novo_second_moment<half_t>, dim3(1), dim3(1024), 0, stream, n, loss_scale, beta2, (const half_t*)gradients, layer_second_moment);
	hipLaunchKernelGGL((k_novo_step<half_t, half_t>), dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, relative_decay, absolute_decay, loss_scale, learning_rate, beta1, epsilon, weights_full_precision,
	                   (half_t*)weights, (const half_t*)gradients, first_moments, layer_second_moment);
}
void lookahead_step(hipStream_t stream, size_t n, float alpha, float* weights_full_precision, void* weights, void* weights_lookahead, Precision weight_precision) {
	if (n == 0) return;
	if (weight_precision == Precision::Fp32) hipLaunchKernelGGL(k_lookahead_step<float>, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, alpha, weights_full_precision, (float*)nullptr, (float*)weights_lookahead);
	else hipLaunchKernelGGL(k_lookahead_step<half_t>, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, alpha, weights_full_precision, (half_t*)weights, (half_t*)weights_lookahead);
}

void ema_step(hipStream_t stream, size_t n, float decay, float debias_old, float debias_new, const void* weights, void* weights_ema, float* tmp, Precision weight_precision) {
	if (n == 0) return;
	if (weight_precision == Precision::Fp32) hipLaunchKernelGGL(k_ema<float>, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, decay, debias_old, debias_new, (const float*)weights, (float*)weights_ema, tmp);
	else hipLaunchKernelGGL(k_ema<half_t>, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, decay, debias_old, debias_new, (const half_t*)weights, (half_t*)weights_ema, tmp);
}

namespace {
void pcg32_advance_host(uint64_t* st, uint64_t delta) {
	const uint64_t MULT = 0x5851f42d4c957f2dULL;
	uint64_t cur_mult = MULT, cur_plus = st[1], acc_mult = 1u, acc_plus = 0u;
	while (delta > 0) {
		if (delta & 1) {
			acc_mult *= cur_mult;
			acc_plus = acc_plus * cur_mult + cur_plus;
		}
		cur_plus = (cur_mult + 1) * cur_plus;
		cur_mult *= cur_mult;
		delta /= 2;
	}
	st[0] = acc_mult * st[0] + acc_plus;
}
} // namespace

void generate_random_uniform(hipStream_t stream, uint64_t* state_inc_host, size_t n, float* out, float lower, float upper) {
	if (n > 0) {
		const size_t n_threads = (n + 3) / 4;
		const uint32_t blocks = blocks_for(n_threads, 128); // n_blocks_linear(n_threads), N_THREADS_LINEAR = 128 (common.h:236-245)
		hipLaunchKernelGGL(k_random_uniform, dim3(blocks), dim3(128), 0, stream, n, state_inc_host[0], state_inc_host[1], out, lower, upper);
	}
	pcg32_advance_host(state_inc_host, (uint64_t)n); // random.h:64
}

void cast_float_to_half(hipStream_t stream, size_t n, const float* in, void* out) {
	if (n == 0) return;
	hipLaunchKernelGGL(k_cast_f2h, dim3(blocks_for((n + 3) / 4, 256)), dim3(256), 0, stream, n, in, (half_t*)out);
}

void cast_half_to_float(hipStream_t stream, size_t n, const void* in, float* out) {
	if (n == 0) return;
	hipLaunchKernelGGL(k_cast_h2f, dim3(blocks_for((n + 3) / 4, 256)), dim3(256), 0, stream, n, (const half_t*)in, out);
}

void trim_and_cast(hipStream_t stream, bool fp32, uint32_t n, uint32_t in_stride, uint32_t dims, const void* in, MatViewMut out) {
	const uint64_t total = (uint64_t)n * dims;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32));
	if (fp32) hipLaunchKernelGGL(k_trim_and_cast<float>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, in_stride, dims, (const float*)in, out);
	else hipLaunchKernelGGL(k_trim_and_cast<half_t>, dim3(blocks_for(total, 256)), dim3(256), 0, stream, n, in_stride, dims, (const half_t*)in, out);
}

void fill_half(hipStream_t stream, size_t n, void* out, float value) {
	if (n == 0) return;
	hipLaunchKernelGGL(k_fill_half, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, (half_t*)out, (half_t)value);
}

} // namespace tcnn_amd
