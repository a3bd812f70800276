// reduce_device.h -- wave64 and 256-thread block sums in a fixed order: the building blocks of the deterministic two-stage sums
// (k_reduce_stage1 / k_reduce_stage2 in k_misc.hip, k_loss_eval in k_loss_eval.hip).
#pragma once

#include "tcnn_common.h"

namespace tcnn_amd {
namespace {

__device__ inline float wave_sum(float v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}

__device__ inline float block_sum_256(float v, float* smem4) {
	v = wave_sum(v);
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	if (lane == 0) smem4[w] = v;
	__syncthreads();
	return smem4[0] + smem4[1] + smem4[2] + smem4[3];
}

} // namespace
} // namespace tcnn_amd
