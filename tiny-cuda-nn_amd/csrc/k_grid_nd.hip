// k_grid_nd.hip -- the grid encoding in 5, 6 and 7 dimensions: the ROLLED kernel form.
//
// Same reference kernels as k_grid.hip / k_grid_bwdbwd.hip (include/tiny-cuda-nn/encodings/grid.h:49-349, :352-650) and the same
// arithmetic, bit for bit.  What differs is the loop shape.  k_grid_fwd unrolls all 2^D corners (times 8 / F levels per thread, plus
// D 2^(D-1) corner pairs for dy/dx): right for 2 - 4 dimensions, 256 VGPRs + 256 AGPRs + 2 KB of scratch per lane at D = 7.  Here
//   * one thread serves ONE (sample, level) pair -- consecutive lanes are consecutive levels of a sample, so a wave's stores into the
//     AoS output [n][stride] stay dense;
//   * the corners are walked in GROUPS of 8: the group loop is rolled, the 8 corners of a group are unrolled, their 8 gathers are
//     issued together and the dependent arithmetic follows in ascending corner order (one fma chain in T, as the reference);
//   * a corner is its D-bit code.  Per dimension the two index terms cell_d * m_d and (cell_d + 1) * m_d (m_d: the hash's prime or
//     the dense stride, uint32 wrap-around included) are computed once per level; a corner's index combines one term per dimension,
//     chosen by a bit test on the code -- registers only, no array is indexed by a run-time value;
//   * dy/dx rolls the gradient dimension too: "the product over the other dimensions" multiplies by one select per dimension.
//
// Compiled with -ffp-contract=off: every fused multiply-add is explicit.
#include "grid_device.h"

namespace tcnn_amd {
namespace {

template <typename T> __device__ inline T nd_fma(T a, T b, T c);
template <> __device__ inline float nd_fma<float>(float a, float b, float c) { return fmaf(a, b, c); }
template <> __device__ inline half_t nd_fma<half_t>(half_t a, half_t b, half_t c) { return __builtin_fmaf16(a, b, c); }

template <typename GT> __device__ inline void nd_atomic_add_pair(GT* p, GT a, GT b);
template <> __device__ inline void nd_atomic_add_pair<half_t>(half_t* p, half_t a, half_t b) { // one global_atomic_pk_add_f16, as k_grid_bwd
	__half2 v;
	v.x = *(const __half*)&a;
	v.y = *(const __half*)&b;
	unsafeAtomicAdd((__half2*)p, v);
}

__device__ inline float nd_smoothstep_2nd_derivative(float v) { return 6.0f - 12.0f * v; } // common_device.h:809-811

constexpr int ND_GROUP = 8; // gathers a lane has in flight

// One (sample, level): the cell, its fractions and the per-dimension index terms.
template <int D>
struct NdCell {
	uint32_t t0[D], t1[D]; // index term of dimension d for corner bit 0 / 1 (Rng hash: the cell coordinates themselves)
	float pos[D], omp[D];  // the fraction (smoothstepped where the grid is) and 1 - it
	uint32_t size, size_mask;
	bool hashed, rng;

	// pos_derivative (nullable): the fractions' first derivatives
	__device__ inline void setup(const GridLevel& lv, const uint32_t* __restrict__ primes, const uint32_t hash_type, const uint32_t interpolation, const float (&xin)[D], float* pos_derivative) {
		size = lv.size, size_mask = lv.size_mask;
		hashed = lv.hashed != 0;
		rng = hashed && hash_type == (uint32_t)HashType::Rng;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			float pd;
			const uint32_t cell = pos_fract(xin[d], lv.scale, interpolation, &pos[d], &pd);
			if (pos_derivative) pos_derivative[d] = pd;
			omp[d] = 1 - pos[d];
			const uint32_t m = rng ? 1u : (hashed ? primes[d] : lv.stride[d]);
			t0[d] = cell * m;
			t1[d] = (cell + 1) * m;
		}
	}

	// grid_index (common_device.h:690-707) of the corner whose bit d says "cell_d + 1"
	__device__ inline uint32_t index(const uint32_t code) const {
		uint32_t index;
		if (rng) { // common_device.h:663-676
			uint64_t step = 0;
#pragma unroll
			for (int d = 0; d < D; ++d) step ^= (uint64_t)((code >> d) & 1u ? t1[d] : t0[d]) << (d * (64 / D));
			index = pcg32_output(pcg32_1337_advanced(step));
		} else {
			uint32_t x = 0, s = 0;
#pragma unroll
			for (int d = 0; d < D; ++d) {
				const uint32_t t = (code >> d) & 1u ? t1[d] : t0[d];
				x ^= t;
				s += t;
			}
			index = hashed ? x : s;
		}
		if (size_mask) return index & size_mask;
		return index >= size ? index % size : index;
	}

	// fp32 product over d = 0 .. D-1 in that order, starting from `first`; dimension `skip` (>= D: none) is left out
	__device__ inline float weight(const uint32_t code, const float first, const uint32_t skip) const {
		float w = first;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const float f = (code >> d) & 1u ? pos[d] : omp[d];
			w = (uint32_t)d == skip ? w : w * f;
		}
		return w;
	}
};

// v[k] without a run-time index.  With masks, not selects: hipcc folds a chain of selects between array elements back into one load
// through a selected ADDRESS, and the array then lives in LDS or scratch.
template <int D> __device__ inline float nd_pick(const float (&v)[D], const uint32_t k) {
	uint32_t r = 0;
#pragma unroll
	for (int d = 0; d < D; ++d) r |= __builtin_bit_cast(uint32_t, v[d]) & (k == (uint32_t)d ? 0xffffffffu : 0u);
	return __builtin_bit_cast(float, r);
}
// the D-bit corner code of pair `idx` (D - 1 bits: the dimensions but `k`, in order) with bit k clear
__device__ inline uint32_t nd_expand(const uint32_t idx, const uint32_t k) {
	const uint32_t lo = idx & ((1u << k) - 1u);
	return lo | ((idx >> k) << (k + 1u));
}

// the sample filter's bit of scatter chunk ch (levels cut into more than 64 chunks have no filter: k_grid_mask_to_bits)
__device__ inline unsigned long long nd_chunk_bit(const uint32_t ch) { return ch < 64u ? 1ull << ch : 0ull; }

template <typename T, int F> __device__ inline T nd_elem(const typename VecOf<T, F>::type& v, int f) {
	if constexpr (F == 1) return v; else return v[f];
}

// ---------------------------------------------------------------------------------------------------------------- forward (grid.h:49-212)
template <typename T, int D, int F>
__global__ void __launch_bounds__(256) k_grid_nd_fwd(
	const GridMeta* __restrict__ meta, const uint32_t n, const MatView x, const T* __restrict__ grid,
	T* __restrict__ out, const uint32_t out_stride, const uint32_t n_slots, float* __restrict__ dy_dx, unsigned long long* __restrict__ chunk_mask
) {
	typedef typename VecOf<T, F>::type vecF;
	static_assert(GRID_FILTER_MAX_CHUNKS == 64, "one mask word per (sample, level)");
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_slots;
	if (i >= n) return;
	const uint32_t level = gid - i * n_slots; // slots behind the levels: the padding features, written as zeros
	const uint32_t n_levels = meta->n_levels;

	T res[F];
#pragma unroll
	for (int f = 0; f < F; ++f) res[f] = (T)0.0f;

	if (level < n_levels) {
		const uint32_t interpolation = meta->interpolation;
		const GridLevel lv = meta->levels[level];
		const T* __restrict__ lgrid = grid + (size_t)lv.offset * F;
		float xin[D], pos_derivative[D];
		load_coords<D>(x, i, xin);
		NdCell<D> c;
		c.setup(lv, meta->primes, meta->hash_type, interpolation, xin, pos_derivative);
		float* __restrict__ dst = dy_dx ? dy_dx + ((size_t)i * n_levels * F + (size_t)level * F) * D : nullptr;

		if (interpolation == (uint32_t)InterpolationType::Nearest) { // grid.h:121-140
			const uint32_t index = c.index(0);
			const vecF v = *(const vecF*)&lgrid[(size_t)index * F];
#pragma unroll
			for (int f = 0; f < F; ++f) res[f] = nd_elem<T, F>(v, f);
			if (chunk_mask) chunk_mask[(size_t)level * n + i] = nd_chunk_bit(scatter_chunk(lv, index));
			if (dst) {
#pragma unroll 1
				for (int k = 0; k < F * D; ++k) dst[k] = 0.0f;
			}
		} else {
			// N-linear interpolation (grid.h:142-169): weight product in fp32 (dim order), cast to T, fma chain in corner order
			unsigned long long touched = 0; // scatter chunks of this level the sample's corners fall into
#pragma unroll 1
			for (uint32_t g = 0; g < (1u << D) / ND_GROUP; ++g) {
				uint32_t index[ND_GROUP];
				vecF v[ND_GROUP];
#pragma unroll
				for (int j = 0; j < ND_GROUP; ++j) index[j] = c.index((g * ND_GROUP) | (uint32_t)j);
#pragma unroll
				for (int j = 0; j < ND_GROUP; ++j) v[j] = *(const vecF*)&lgrid[(size_t)index[j] * F];
				if (chunk_mask) {
#pragma unroll
					for (int j = 0; j < ND_GROUP; ++j) touched |= nd_chunk_bit(scatter_chunk(lv, index[j]));
				}
#pragma unroll
				for (int j = 0; j < ND_GROUP; ++j) {
					float weight = c.weight((g * ND_GROUP) | (uint32_t)j, 1.0f, D);
					// the reference rounds the fp32 weight product to fp32 FIRST and to T afterwards: keep hipcc from folding the
					// last multiply and the conversion into one v_fma_mixlo_f16 (see k_grid.hip)
					asm volatile("" : "+v"(weight));
					const T w = (T)weight;
#pragma unroll
					for (int f = 0; f < F; ++f) res[f] = nd_fma<T>(w, nd_elem<T, F>(v[j], f), res[f]);
				}
			}
			if (chunk_mask) chunk_mask[(size_t)level * n + i] = touched;

			if (dst) { // grid.h:172-211: grad_dim outer, corner pairs inner
#pragma unroll 1
				for (uint32_t gd = 0; gd < D; ++gd) {
					const float pdg = nd_pick<D>(pos_derivative, gd);
					float grads[F];
#pragma unroll
					for (int f = 0; f < F; ++f) grads[f] = 0.0f;
					constexpr int PAIRS = ND_GROUP / 2;
#pragma unroll 1
					for (uint32_t g = 0; g < (1u << (D - 1)) / PAIRS; ++g) {
						vecF vl[PAIRS], vr[PAIRS];
						uint32_t code[PAIRS];
#pragma unroll
						for (int j = 0; j < PAIRS; ++j) {
							code[j] = nd_expand((g * PAIRS) | (uint32_t)j, gd);
							vl[j] = *(const vecF*)&lgrid[(size_t)c.index(code[j]) * F];
							vr[j] = *(const vecF*)&lgrid[(size_t)c.index(code[j] | (1u << gd)) * F];
						}
#pragma unroll
						for (int j = 0; j < PAIRS; ++j) {
							const float weight = c.weight(code[j], lv.scale, gd);
#pragma unroll
							for (int f = 0; f < F; ++f) grads[f] += weight * ((float)nd_elem<T, F>(vr[j], f) - (float)nd_elem<T, F>(vl[j], f)) * pdg;
						}
					}
#pragma unroll
					for (int f = 0; f < F; ++f) dst[f * D + gd] = grads[f];
				}
			}
		}
	}

	if (!out) return;
	T* o = out + (size_t)i * out_stride + (size_t)level * F;
	if (out_stride % F == 0) { // (then level * F + F <= out_stride: n_slots = ceil(out_stride / F))
		vecF v;
		if constexpr (F == 1) v = res[0];
		else {
#pragma unroll
			for (int f = 0; f < F; ++f) v[f] = res[f];
		}
		*(vecF*)o = v;
	} else {
#pragma unroll
		for (int f = 0; f < F; ++f) if (level * F + f < out_stride) o[f] = res[f];
	}
}

// ------------------------------------------------------------------------- parameter gradients, global atomics (grid.h:215-320)
// STOCH: stochastic_interpolation (grid.h:284-298) -- dL/dy with weight 1 onto the one corner drawn per (sample, level)
template <typename T, typename GT, int D, int F, bool STOCH>
__global__ void __launch_bounds__(256) k_grid_nd_bwd(
	const GridMeta* __restrict__ meta, const uint32_t n, const MatView x, const T* __restrict__ dL_dy, const uint32_t dy_stride, GT* __restrict__ grad
) {
	typedef typename VecOf<T, F>::type vecF;
	const uint32_t n_levels = meta->n_levels;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_levels;
	if (i >= n) return;
	const uint32_t level = gid - i * n_levels;
	const uint32_t interpolation = meta->interpolation;
	const GridLevel lv = meta->levels[level];
	GT* __restrict__ lgrad = grad + (size_t)lv.offset * F;

	float xin[D];
	load_coords<D>(x, i, xin);
	NdCell<D> c;
	c.setup(lv, meta->primes, meta->hash_type, interpolation, xin, nullptr);

	const vecF gv = *(const vecF*)&dL_dy[(size_t)i * dy_stride + level * F];
	T g[F];
#pragma unroll
	for (int f = 0; f < F; ++f) g[f] = nd_elem<T, F>(gv, f);

	auto add = [&](const uint32_t code, float weight) { // grid.h:252-255
		GT* p = lgrad + (size_t)c.index(code) * F;
		if constexpr (sizeof(GT) == 2) {
			asm volatile("" : "+v"(weight)); // keep the fp32 rounding of the weight product (see k_grid_nd_fwd)
			const GT w = (GT)weight;
#pragma unroll
			for (int f = 0; f < F; f += 2) nd_atomic_add_pair<GT>(p + f, (GT)(w * (GT)g[f]), (GT)(w * (GT)g[f + 1]));
		} else {
#pragma unroll
			for (int f = 0; f < F; ++f) unsafeAtomicAdd((float*)p + f, weight * (float)g[f]);
		}
	};

	if (interpolation == (uint32_t)InterpolationType::Nearest) {
		add(0, 1.0f);
		return;
	}
	if constexpr (STOCH) { // stochastic_corner (grid_device.h) as a corner code
		const float sample = grid_random_val(i + level * n);
		uint32_t code = 0;
#pragma unroll
		for (int d = 0; d < D; ++d) code |= sample >= c.pos[d] ? 0u : 1u << d;
		add(code, 1.0f);
		return;
	}
#pragma unroll 1
	for (uint32_t g0 = 0; g0 < (1u << D) / ND_GROUP; ++g0) {
#pragma unroll
		for (int j = 0; j < ND_GROUP; ++j) {
			const uint32_t code = (g0 * ND_GROUP) | (uint32_t)j;
			add(code, c.weight(code, 1.0f, D));
		}
	}
}

// ------------------------------------------------------------------------- second order (grid.h:352-650; shapes as k_grid_bwdbwd.hip)
template <int D>
__device__ inline void nd_fractions(const MatView& x, const uint32_t i, const float scale, const uint32_t interpolation, float (&d1)[D], float (&d2)[D]) {
#pragma unroll
	for (int d = 0; d < D; ++d) { // common_device.h:825-838: the derivatives at the un-smoothed fraction
		float p = fmaf(scale, x.data[(size_t)i * x.stride_sample + (size_t)d * x.stride_dim], 0.5f);
		p -= floorf(p);
		if (interpolation == (uint32_t)InterpolationType::Smoothstep) {
			d2[d] = nd_smoothstep_2nd_derivative(p);
			d1[d] = smoothstep_derivative(p);
		} else {
			d2[d] = 0.0f;
			d1[d] = 1.0f;
		}
	}
}

// one thread per (sample, level); grad is accumulated in place
template <typename T, typename GT, int D, int F>
__global__ void __launch_bounds__(256) k_grid_nd_bwdbwd_grid(const GridMeta* __restrict__ meta, const uint32_t n, const MatView x, const MatView dL_ddLdx, const T* __restrict__ dL_dy,
                                                             const uint32_t dy_stride, GT* __restrict__ grad) {
	typedef typename VecOf<T, F>::type vecF;
	const uint32_t n_levels = meta->n_levels;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_levels;
	if (i >= n) return;
	const uint32_t level = gid - i * n_levels;
	const uint32_t interpolation = meta->interpolation;
	if (interpolation == (uint32_t)InterpolationType::Nearest) return; // grid.h:420-423
	const GridLevel lv = meta->levels[level];
	GT* __restrict__ lgrad = grad + (size_t)lv.offset * F;

	float xin[D], d1[D], d2[D];
#pragma unroll
	for (int d = 0; d < D; ++d) xin[d] = x.data[(size_t)i * x.stride_sample + (size_t)d * x.stride_dim];
	NdCell<D> c;
	c.setup(lv, meta->primes, meta->hash_type, interpolation, xin, nullptr);
	nd_fractions<D>(x, i, lv.scale, interpolation, d1, d2);
	const vecF gv = *(const vecF*)&dL_dy[(size_t)i * dy_stride + level * F];
	T g[F];
#pragma unroll
	for (int f = 0; f < F; ++f) g[f] = nd_elem<T, F>(gv, f);

	auto add = [&](const uint32_t code, float weight) { // grid.h:393-396
		GT* p = lgrad + (size_t)c.index(code) * F;
		if constexpr (sizeof(GT) == 2) {
			asm volatile("" : "+v"(weight));
			const GT w = (GT)weight;
#pragma unroll
			for (int f = 0; f < F; f += 2) nd_atomic_add_pair<GT>(p + f, (GT)(w * (GT)g[f]), (GT)(w * (GT)g[f + 1]));
		} else {
#pragma unroll
			for (int f = 0; f < F; ++f) unsafeAtomicAdd((float*)p + f, weight * (float)g[f]);
		}
	};

#pragma unroll 1
	for (uint32_t gd = 0; gd < D; ++gd) {
		const float grad_in = lv.scale * dL_ddLdx.data[(size_t)i * dL_ddLdx.stride_sample + (size_t)gd * dL_ddLdx.stride_dim] * nd_pick<D>(d1, gd);
#pragma unroll 4
		for (uint32_t idx = 0; idx < (1u << (D - 1)); ++idx) {
			const uint32_t code = nd_expand(idx, gd);
			const float weight = c.weight(code, grad_in, gd);
			add(code, -weight);
			add(code | (1u << gd), weight);
		}
	}
}

// one thread per sample: levels, then feature pairs, in order
template <typename T, int D, int F>
__global__ void __launch_bounds__(128) k_grid_nd_bwdbwd_input(const GridMeta* __restrict__ meta, const uint32_t n, const MatView x, const MatView dL_ddLdx, const T* __restrict__ dL_dy,
                                                              const uint32_t dy_stride, const T* __restrict__ grid, const MatViewMut dL_dx) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	constexpr int FT = F < 2 ? F : 2; // N_FEATURES_PER_THREAD (grid.h:998)
	const uint32_t interpolation = meta->interpolation;
	const bool smooth = interpolation == (uint32_t)InterpolationType::Smoothstep;
	float xin[D], v[D];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		xin[d] = x.data[(size_t)i * x.stride_sample + (size_t)d * x.stride_dim];
		v[d] = dL_ddLdx.data[(size_t)i * dL_ddLdx.stride_sample + (size_t)d * dL_ddLdx.stride_dim];
	}
	const uint32_t n_levels = interpolation == (uint32_t)InterpolationType::Nearest ? 0u : meta->n_levels; // grid.h:525-528
#pragma unroll 1
	for (uint32_t gd = 0; gd < D; ++gd) {
		float out = 0.0f;
#pragma unroll 1
		for (uint32_t level = 0; level < n_levels; ++level) {
			const GridLevel lv = meta->levels[level];
			const T* __restrict__ lgrid = grid + (size_t)lv.offset * F;
			float d1[D], d2[D];
			NdCell<D> c;
			c.setup(lv, meta->primes, meta->hash_type, interpolation, xin, nullptr);
			nd_fractions<D>(x, i, lv.scale, interpolation, d1, d2);
			const float d1g = nd_pick<D>(d1, gd);
			const float diag = lv.scale * lv.scale * nd_pick<D>(v, gd) * nd_pick<D>(d2, gd);
#pragma unroll 1
			for (int feature = 0; feature < F; feature += FT) {
				const T* gy = dL_dy + (size_t)i * dy_stride + level * F + feature;
				float gyf[FT];
#pragma unroll
				for (int f = 0; f < FT; ++f) gyf[f] = (float)gy[f];
				auto calc = [&](const uint32_t code, const float weight) { // grid.h:531-541
					const size_t index = (size_t)c.index(code) * F + feature;
					float r = 0;
#pragma unroll
					for (int f = 0; f < FT; ++f) r += (float)lgrid[index + f] * gyf[f] * weight;
					return r;
				};
				float grad_out = 0;
#pragma unroll 1
				for (uint32_t idx = 0; idx < (1u << (D - 1)); ++idx) {
					if (smooth) { // diagonal of the Hessian; zero for linear interpolation
						const uint32_t code = nd_expand(idx, gd);
						const float w = c.weight(code, diag, gd);
						grad_out += calc(code, -w);
						grad_out += calc(code | (1u << gd), w);
					}
#pragma unroll 1
					for (uint32_t og = 0; og < D - 1; ++og) { // mixed part: d(dy/d[other])/d[grad_dim]
						const uint32_t rog = og >= gd ? (og + 1) : og;
						const uint32_t code = nd_expand(idx, rog);
						float w = lv.scale * lv.scale * nd_pick<D>(v, rog) * nd_pick<D>(d1, rog) * d1g;
#pragma unroll
						for (int d = 0; d < D; ++d) { // the dimensions but rog, in order; grad_dim contributes its sign instead of a fraction
							const bool bit = (code >> d) & 1u;
							const float f = (uint32_t)d == gd ? (bit ? 1.0f : -1.0f) : (bit ? c.pos[d] : c.omp[d]);
							w = (uint32_t)d == rog ? w : w * f;
						}
						grad_out += calc(code, -w);
						grad_out += calc(code | (1u << rog), w);
					}
				}
				out += grad_out;
			}
		}
		dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)gd * dL_dx.stride_dim] = out;
	}
}

// ---------------------------------------------------------------------------------------------------------------- launchers
template <typename T, int D>
void nd_launch_fwd(hipStream_t s, uint32_t F, const GridMeta* dm, uint32_t n, MatView x, const void* grid, void* out, uint32_t os, float* dy_dx, uint64_t* cm) {
	const uint32_t n_slots = div_round_up(os, F);
	const uint64_t total = (uint64_t)n * n_slots;
	CHECK_THROW(total < (1ull << 32));
	const dim3 blocks((uint32_t)((total + 255) / 256));
	if (blocks.x == 0) return;
#define TCNN_ND_FWD(F_) hipLaunchKernelGGL((k_grid_nd_fwd<T, D, F_>), blocks, dim3(256), 0, s, dm, n, x, (const T*)grid, (T*)out, os, n_slots, dy_dx, (unsigned long long*)cm)
	switch (F) {
		case 1: TCNN_ND_FWD(1); break;
		case 2: TCNN_ND_FWD(2); break;
		case 4: TCNN_ND_FWD(4); break;
		case 8: TCNN_ND_FWD(8); break;
		default: throw std::runtime_error{"GridEncoding: n_features_per_level must be 1, 2, 4, or 8."};
	}
#undef TCNN_ND_FWD
}

template <typename T, typename GT, int D>
void nd_launch_bwd(hipStream_t s, const GridMeta& m, const GridMeta* dm, uint32_t n, MatView x, const void* dy, uint32_t ds, void* grad, bool st) {
	const uint64_t total = (uint64_t)n * m.n_levels;
	CHECK_THROW(total < (1ull << 32));
	const dim3 blocks((uint32_t)((total + 255) / 256));
	if (blocks.x == 0) return;
#define TCNN_ND_BWD(F_) \
	if (st) hipLaunchKernelGGL((k_grid_nd_bwd<T, GT, D, F_, true>), blocks, dim3(256), 0, s, dm, n, x, (const T*)dy, ds, (GT*)grad); \
	else hipLaunchKernelGGL((k_grid_nd_bwd<T, GT, D, F_, false>), blocks, dim3(256), 0, s, dm, n, x, (const T*)dy, ds, (GT*)grad)
	switch (m.n_features_per_level) {
		case 1:
			if constexpr (sizeof(GT) == 4) { TCNN_ND_BWD(1); }
			else throw std::runtime_error{"GridEncoding: F == 1 accumulates gradients in fp32"};
			break;
		case 2: TCNN_ND_BWD(2); break;
		case 4: TCNN_ND_BWD(4); break;
		case 8: TCNN_ND_BWD(8); break;
		default: throw std::runtime_error{"GridEncoding: n_features_per_level must be 1, 2, 4, or 8."};
	}
#undef TCNN_ND_BWD
}

template <typename T, typename GT, int D>
void nd_launch_bwdbwd(hipStream_t s, const GridMeta& meta, const GridMeta* dm, uint32_t n, MatView x, MatView v, const void* dy, uint32_t ds, const void* grid, void* grad, MatViewMut* dx) {
	const uint32_t F = meta.n_features_per_level;
	if (grad) {
		const uint64_t total = (uint64_t)n * meta.n_levels;
		CHECK_THROW(total < (1ull << 32));
		const dim3 blocks((uint32_t)((total + 255) / 256));
#define TCNN_ND_BB_GRID(F_) hipLaunchKernelGGL((k_grid_nd_bwdbwd_grid<T, GT, D, F_>), blocks, dim3(256), 0, s, dm, n, x, v, (const T*)dy, ds, (GT*)grad)
		switch (F) {
			case 1:
				if constexpr (sizeof(GT) == 4) TCNN_ND_BB_GRID(1);
				else throw std::runtime_error{"GridEncoding: F == 1 accumulates gradients in fp32"};
				break;
			case 2: TCNN_ND_BB_GRID(2); break;
			case 4: TCNN_ND_BB_GRID(4); break;
			case 8: TCNN_ND_BB_GRID(8); break;
			default: throw std::runtime_error{"GridEncoding: n_features_per_level must be 1, 2, 4, or 8."};
		}
#undef TCNN_ND_BB_GRID
	}
	if (dx) {
		const dim3 blocks(div_round_up(n, 128));
#define TCNN_ND_BB_IN(F_) hipLaunchKernelGGL((k_grid_nd_bwdbwd_input<T, D, F_>), blocks, dim3(128), 0, s, dm, n, x, v, (const T*)dy, ds, (const T*)grid, *dx)
		switch (F) {
			case 1: TCNN_ND_BB_IN(1); break;
			case 2: TCNN_ND_BB_IN(2); break;
			case 4: TCNN_ND_BB_IN(4); break;
			case 8: TCNN_ND_BB_IN(8); break;
			default: throw std::runtime_error{"GridEncoding: n_features_per_level must be 1, 2, 4, or 8."};
		}
#undef TCNN_ND_BB_IN
	}
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace

#define TCNN_ND_DIMS(CALL) \
	switch (meta.n_pos_dims) { \
		case 5: { CALL(5); } break; \
		case 6: { CALL(6); } break; \
		case 7: { CALL(7); } break; \
		default: throw std::runtime_error{"GridEncoding: number of input dims must be 2 or 3."}; \
	}

void grid_nd_forward(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, bool fp32, uint32_t n, MatView x, const void* grid, void* out, uint32_t out_stride, float* dy_dx,
                     uint64_t* chunk_mask) {
	const uint32_t F = meta.n_features_per_level;
#define TCNN_ND_CALL_H(D) nd_launch_fwd<half_t, D>(stream, F, dev_meta, n, x, grid, out, out_stride, dy_dx, chunk_mask)
#define TCNN_ND_CALL_F(D) nd_launch_fwd<float, D>(stream, F, dev_meta, n, x, grid, out, out_stride, dy_dx, chunk_mask)
	if (fp32) { TCNN_ND_DIMS(TCNN_ND_CALL_F) } else { TCNN_ND_DIMS(TCNN_ND_CALL_H) }
#undef TCNN_ND_CALL_H
#undef TCNN_ND_CALL_F
}

void grid_nd_backward(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, bool fp32_grad, uint32_t n, MatView x, const void* dL_dy, bool dy_fp32, uint32_t dy_stride, void* grad,
                      bool stochastic) {
#define TCNN_ND_CALL_FF(D) nd_launch_bwd<float, float, D>(stream, meta, dev_meta, n, x, dL_dy, dy_stride, grad, stochastic)
#define TCNN_ND_CALL_HF(D) nd_launch_bwd<half_t, float, D>(stream, meta, dev_meta, n, x, dL_dy, dy_stride, grad, stochastic)
#define TCNN_ND_CALL_HH(D) nd_launch_bwd<half_t, half_t, D>(stream, meta, dev_meta, n, x, dL_dy, dy_stride, grad, stochastic)
	if (dy_fp32) {
		CHECK_THROW(fp32_grad);
		TCNN_ND_DIMS(TCNN_ND_CALL_FF)
	} else if (fp32_grad) {
		TCNN_ND_DIMS(TCNN_ND_CALL_HF)
	} else {
		TCNN_ND_DIMS(TCNN_ND_CALL_HH)
	}
#undef TCNN_ND_CALL_FF
#undef TCNN_ND_CALL_HF
#undef TCNN_ND_CALL_HH
}

void grid_nd_backward_backward_input(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, bool fp32, bool fp32_grad, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy,
                                     uint32_t dy_stride, const void* grid, void* grad, MatViewMut* dL_dx) {
	if (n == 0) return;
#define TCNN_ND_CALL_FF(D) nd_launch_bwdbwd<float, float, D>(stream, meta, dev_meta, n, x, dL_ddLdx, dL_dy, dy_stride, grid, grad, dL_dx)
#define TCNN_ND_CALL_HF(D) nd_launch_bwdbwd<half_t, float, D>(stream, meta, dev_meta, n, x, dL_ddLdx, dL_dy, dy_stride, grid, grad, dL_dx)
#define TCNN_ND_CALL_HH(D) nd_launch_bwdbwd<half_t, half_t, D>(stream, meta, dev_meta, n, x, dL_ddLdx, dL_dy, dy_stride, grid, grad, dL_dx)
	if (fp32) {
		CHECK_THROW(fp32_grad);
		TCNN_ND_DIMS(TCNN_ND_CALL_FF)
	} else if (fp32_grad) {
		TCNN_ND_DIMS(TCNN_ND_CALL_HF)
	} else {
		TCNN_ND_DIMS(TCNN_ND_CALL_HH)
	}
#undef TCNN_ND_CALL_FF
#undef TCNN_ND_CALL_HF
#undef TCNN_ND_CALL_HH
}
#undef TCNN_ND_DIMS

} // namespace tcnn_amd
