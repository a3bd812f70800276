// k_grid_max_level.hip -- the grid encodings' max_level cut-off (GridEncoding::set_max_level / set_max_level_gpu, grid_interface.h:101-123).
//
// The reference decides per (sample, level) inside every grid kernel (grid.h:67-90, :237-245, :377-384, :482-490):
//   ml = max_level_gpu ? max_level_gpu[i] : max_level;  m = (ml * num_grid_features) / N_FEATURES_PER_LEVEL
//   forward: level l is off when l >= m + 1e-3f (zeros in its features and in dy_dx)
//   gradients and both second-order kernels: level l is skipped when l > m + 1e-3f
// Here the grid kernels stay as they are and this one kernel zeroes the (sample, level) pairs that are off: in the encoded batch and
// dy_dx after a forward pass (forward rule), in a copy of dL/dy in front of a per-sample backward pass (gradient rule).  The scalar form
// needs no pass over dL/dy: its off levels are a suffix, whose parameter gradients are one contiguous tail (GridEncoding::backward).
#include "tcnn_common.h"

namespace tcnn_amd {
namespace {

// the reference's expressions in fp32, nothing contracted or reordered (NaN: both comparisons false, every level on)
__device__ __forceinline__ bool grid_level_off(uint32_t level, float ml, float n_grid_features, float F, bool gradient_rule) {
	const float threshold = __fadd_rn(__fdiv_rn(__fmul_rn(ml, n_grid_features), F), 1e-3f);
	const float l = (float)level;
	return gradient_rule ? l > threshold : l >= threshold;
}

// one thread per (sample, level): level = level0 + blockIdx.y; the pair's `width` elements start at data + i * sample_stride + level * level_stride.
// Off: per_sample's rule, or (scalar) level >= first_off.  With src: every pair is written, src's elements where the pair is on (a masked
// copy in one pass); without: the pairs that are off are zeroed.
template <typename T, bool PER_SAMPLE>
__global__ void __launch_bounds__(256) k_grid_zero_levels(const uint32_t n, const uint32_t level0, const uint32_t first_off, const uint32_t width, const uint64_t sample_stride, const uint64_t level_stride,
                                                          T* __restrict__ data, const T* __restrict__ src, const float* __restrict__ per_sample, const float n_grid_features,
                                                          const float F, const uint32_t gradient_rule) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t level = level0 + blockIdx.y;
	const bool off = PER_SAMPLE ? grid_level_off(level, per_sample[i], n_grid_features, F, gradient_rule != 0) : level >= first_off;
	const uint64_t at = i * sample_stride + level * level_stride;
	if (src) {
		for (uint32_t k = 0; k < width; ++k) data[at + k] = off ? T(0) : src[at + k];
	} else if (off) {
		for (uint32_t k = 0; k < width; ++k) data[at + k] = T(0);
	}
}

template <typename T>
void launch_zero_levels(hipStream_t stream, uint32_t n, uint32_t n_levels, uint32_t first_off, uint32_t width, uint64_t sample_stride, uint64_t level_stride, void* data,
                        const void* src, const float* per_sample, uint32_t n_grid_features, uint32_t F, bool gradient_rule) {
	const uint32_t level0 = (src || per_sample) ? 0u : first_off; // (zeroing the scalar's suffix: its levels alone)
	const dim3 blocks((n + 255) / 256, n_levels - level0);
	if (per_sample) {
		hipLaunchKernelGGL((k_grid_zero_levels<T, true>), blocks, dim3(256), 0, stream, n, level0, first_off, width, sample_stride, level_stride, (T*)data, (const T*)src, per_sample,
		                   (float)n_grid_features, (float)F, gradient_rule ? 1u : 0u);
	} else {
		hipLaunchKernelGGL((k_grid_zero_levels<T, false>), blocks, dim3(256), 0, stream, n, level0, first_off, width, sample_stride, level_stride, (T*)data, (const T*)src, nullptr,
		                   (float)n_grid_features, (float)F, gradient_rule ? 1u : 0u);
	}
}

} // namespace

void grid_zero_levels(hipStream_t stream, size_t elem_bytes, uint32_t n, uint32_t n_levels, uint32_t level0, uint32_t width, uint64_t sample_stride, uint64_t level_stride,
                      void* data, const void* src, const float* per_sample, uint32_t n_grid_features, uint32_t F, bool gradient_rule) {
	if (n == 0 || width == 0 || n_levels == 0 || (!src && !per_sample && level0 >= n_levels)) return;
	CHECK_THROW(elem_bytes == 2 || elem_bytes == 4);
	if (elem_bytes == 2) launch_zero_levels<uint16_t>(stream, n, n_levels, level0, width, sample_stride, level_stride, data, src, per_sample, n_grid_features, F, gradient_rule);
	else launch_zero_levels<uint32_t>(stream, n, n_levels, level0, width, sample_stride, level_stride, data, src, per_sample, n_grid_features, F, gradient_rule);
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace tcnn_amd
