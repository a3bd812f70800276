// k_kplanes.hip -- the planar factorisation ("KPlanes"): per level a D-dimensional field is the K = D (D - 1) / 2 dense 2-D feature grids
// over its axis pairs (a, b), a < b, in lexicographic order, multiplied (K-Planes, HexPlane) or summed (tri-planes) per feature.
// Parameters: T [L][K][entries_l][F], entries_l = next_multiple(R_l^2, 8) -- for K = 1 the dense grid's own layout.
//
// A plane is a 2-D DenseGrid level with Linear interpolation: pos_fract on x_a and x_b, the grid's corner order (bit 0: +1 along a, stride 1;
// bit 1: +1 along b, stride R), its weight products and its index rule (uint32 sum, modulo the entry count).  The plane's value P_k[f] is
// the fp32 fmaf chain over the four corners, NOT rounded; y[l F + f] = (T)(P_0[f] op P_1[f] op ...), left to right in fp32, rounded once.
// (One plane, D = 2, in half: the dense grid's own half chain instead, so that KPlanes at D = 2 and the 2-D DenseGrid give the same bits.)
// The four corners are base, base + 1, base + R, base + R + 1 (mod 2^32); where base + R + 1 is inside the plane -- every sample of
// [0, 1)^D but the last cell row -- no corner needs the modulo, and only the others pay for the four integer divisions (corners()).
//
//   k_kplanes_fwd        one thread per (sample, level), consecutive lanes = consecutive levels of a sample (dense AoS rows); all 4 K
//                        indices first, then all gathers (one F-wide load each), then the chains.  The x-neighbours of a corner row are
//                        adjacent entries, but base is odd as often as even: one load for both would be misaligned half the time, so
//                        every corner keeps its own load.
//   k_kplanes_bwd_input  the lookup again from x; a sample's levels on W neighbouring lanes, summed by a fixed-order xor butterfly.
//                        Plane (a, b) feeds x_a and x_b through G_k[f] = dL/dy_f (times the other planes' values for Product).
//   k_kplanes_bwd        dL/dparams, half.  A workgroup owns ALL K planes of one level and a slice of the batch: a thread gathers the
//                        sample's 4 K entries once, forms every P_q and from them every "product of the others" (prefix times suffix, 2 K
//                        multiplies per feature), and then emits all 4 K F contributions (half)(G_k[f] w_corner) as 2^-24 fixed point.
//                        One workgroup per plane would let a plane three times as large stay in LDS, but would gather and chain all K
//                        planes K times over -- and the gathers are what a sample costs.  The level's accumulators live in LDS when
//                        K entries F 8 bytes <= 64 KB (two workgroups per CU), flushed to the global scratch afterwards (non-zeros only);
//                        larger levels add straight into the scratch.  k_kplanes_finalize rounds once and leaves the scratch zero.
//                        Sum reads no parameters at all.
//   k_kplanes_bwd_f32    fp32 modules: float atomicAdd into the gradient (order not fixed).
//   k_kplanes_tangent, k_kplanes_bwdbwd_input, k_kplanes_bwdbwd, k_kplanes_bwdbwd_f32: the second-order pass, each in the work split of
//                        its first-order counterpart above ("second order" below has the function).
//
// D, F and the reduction are compile-time; every array below is indexed by unrolled loop variables only (no scratch, no static LDS).
// Compiled with -ffp-contract=off and without packed fp32 instructions (build.py).
#include "grid_fixed.h"

namespace tcnn_amd {
namespace {

constexpr uint32_t KPLANES_LDS_BYTES = 64 * 1024; // accumulators of one level (all planes) in LDS: two workgroups per CU
constexpr uint32_t KPLANES_BWD_SAMPLES = 4096;    // samples per workgroup of k_kplanes_bwd

// plane k of D dimensions is the axis pair (KPLANES_A[D][k], KPLANES_B[D][k]): lexicographic order.  Only ever read with an unrolled k.
__device__ constexpr int KPLANES_A[5][6] = {{0}, {0}, {0}, {0, 0, 1}, {0, 0, 0, 1, 1, 2}};
__device__ constexpr int KPLANES_B[5][6] = {{0}, {0}, {1}, {1, 2, 2}, {1, 2, 3, 2, 3, 3}};

template <typename T, int F> __device__ inline float kplanes_elem(const typename VecOf<T, F>::type& v, int f) {
	if constexpr (F == 1) return (float)v; else return (float)v[f];
}

// a sample's cell and fractions at one level
template <int D>
struct KPlanesCell {
	float pos[D];
	uint32_t cell[D];

	__device__ inline void setup(const float (&x)[D], const float scale) {
#pragma unroll
		for (int d = 0; d < D; ++d) {
			float derivative;
			cell[d] = pos_fract(x[d], scale, (uint32_t)InterpolationType::Linear, &pos[d], &derivative);
		}
	}
	// the grid's weight product of corner c of plane (a, b): 1 * (x part) * (y part)
	__device__ inline float weight(const int a, const int b, const int c) const {
		return ((c & 1) ? pos[a] : 1 - pos[a]) * ((c & 2) ? pos[b] : 1 - pos[b]);
	}
	// entries of the four corners: (cell_a + c0) + (cell_b + c1) * R in uint32, modulo size (entries >= R + 1 for every R >= 1)
	__device__ inline void corners(const int a, const int b, const uint32_t R, const uint32_t size, uint32_t (&idx)[4]) const {
		const uint32_t base = cell[a] + cell[b] * R;
		if (base < size - R - 1u) {
			idx[0] = base; idx[1] = base + 1u; idx[2] = base + R; idx[3] = base + R + 1u;
		} else {
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				const uint32_t i = base + (uint32_t)(c & 1) + (uint32_t)(c >> 1) * R;
				idx[c] = i >= size ? i % size : i;
			}
		}
	}
};

// gathers of all planes of a level: v[k][c], table = the level's first plane
template <typename T, int D, int F>
__device__ inline void kplanes_gather(const KPlanesCell<D>& cs, const T* __restrict__ table, const uint32_t R, const uint32_t size,
                                      typename VecOf<T, F>::type (&v)[D * (D - 1) / 2][4]) {
	typedef typename VecOf<T, F>::type vecF;
	constexpr int K = D * (D - 1) / 2;
	uint32_t idx[K][4];
#pragma unroll
	for (int k = 0; k < K; ++k) cs.corners(KPLANES_A[D][k], KPLANES_B[D][k], R, size, idx[k]);
#pragma unroll
	for (int k = 0; k < K; ++k) {
#pragma unroll
		for (int c = 0; c < 4; ++c) v[k][c] = *(const vecF*)&table[((size_t)k * size + idx[k][c]) * F];
	}
}

// P[k][f]: the fp32 fma chain over the corners, in corner order
template <typename T, int D, int F>
__device__ inline void kplanes_values(const KPlanesCell<D>& cs, const typename VecOf<T, F>::type (&v)[D * (D - 1) / 2][4], float (&P)[D * (D - 1) / 2][F]) {
	constexpr int K = D * (D - 1) / 2;
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const int a = KPLANES_A[D][k], b = KPLANES_B[D][k];
#pragma unroll
		for (int f = 0; f < F; ++f) P[k][f] = 0.0f;
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			const float w = cs.weight(a, b, c);
#pragma unroll
			for (int f = 0; f < F; ++f) P[k][f] = fmaf(w, kplanes_elem<T, F>(v[k][c], f), P[k][f]);
		}
	}
}

// G[k][f] = dL/dP_k[f]: g[f] for Sum, g[f] times the product of the other planes' values for Product (prefix times suffix)
template <int K, int F, bool PRODUCT>
__device__ inline void kplanes_plane_gradients(const float (&P)[K][F], const float (&g)[F], float (&G)[K][F]) {
	if constexpr (!PRODUCT || K == 1) {
#pragma unroll
		for (int k = 0; k < K; ++k) {
#pragma unroll
			for (int f = 0; f < F; ++f) G[k][f] = g[f];
		}
	} else {
#pragma unroll
		for (int f = 0; f < F; ++f) {
			float suffix[K]; // product of P[q][f], q > k
			suffix[K - 1] = 1.0f;
#pragma unroll
			for (int k = K - 2; k >= 0; --k) suffix[k] = suffix[k + 1] * P[k + 1][f];
			float prefix = 1.0f;
#pragma unroll
			for (int k = 0; k < K; ++k) {
				G[k][f] = g[f] * (prefix * suffix[k]);
				prefix *= P[k][f];
			}
		}
	}
}

template <typename T, int F>
__device__ inline void kplanes_load_dy(const T* __restrict__ dy, const uint32_t dy_stride, float (&g)[F]) {
	typedef typename VecOf<T, F>::type vecF;
	if (dy_stride % F == 0) {
		const vecF gv = *(const vecF*)dy;
#pragma unroll
		for (int f = 0; f < F; ++f) g[f] = kplanes_elem<T, F>(gv, f);
	} else {
#pragma unroll
		for (int f = 0; f < F; ++f) g[f] = (float)dy[f];
	}
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <typename T, int D, int F, bool PRODUCT>
__global__ void __launch_bounds__(256) k_kplanes_fwd(const uint32_t n, const uint32_t n_levels, const KPlanesShape::Levels lv, const MatView x, const T* __restrict__ params,
                                                     T* __restrict__ out, const uint32_t out_stride, const uint32_t n_slots) {
	typedef typename VecOf<T, F>::type vecF;
	constexpr int K = D * (D - 1) / 2;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_slots;
	if (i >= n) return;
	const uint32_t level = gid - i * n_slots; // slots behind the levels write the padding: ones
	float res[F];
#pragma unroll
	for (int f = 0; f < F; ++f) res[f] = 1.0f;
	if (level < n_levels) {
		float xin[D];
		load_coords<D>(x, i, xin);
		KPlanesCell<D> cs;
		cs.setup(xin, lv.scale[level]);
		vecF v[K][4];
		kplanes_gather<T, D, F>(cs, params + (size_t)lv.offset[level] * F, lv.resolution[level], lv.entries[level], v);
		if constexpr (K == 1 && sizeof(T) == 2) {
			// One plane, half: there is nothing to reduce, and the encoding IS a 2-D DenseGrid -- in its arithmetic too, so that the two are
			// interchangeable bit for bit: each fp32 weight product rounded to half, then a half fma chain (k_grid_fwd, which also says why
			// the weight passes through a register barrier).  In fp32 the chain below already is the grid's.
			half_t acc[F];
#pragma unroll
			for (int f = 0; f < F; ++f) acc[f] = (half_t)0.0f;
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				float w = cs.weight(0, 1, c);
				asm volatile("" : "+v"(w));
				const half_t wh = (half_t)w;
#pragma unroll
				for (int f = 0; f < F; ++f) {
					half_t val;
					if constexpr (F == 1) val = v[0][c]; else val = v[0][c][f];
					acc[f] = __builtin_fmaf16(wh, val, acc[f]);
				}
			}
#pragma unroll
			for (int f = 0; f < F; ++f) res[f] = (float)acc[f];
		} else {
			float P[K][F];
			kplanes_values<T, D, F>(cs, v, P);
#pragma unroll
			for (int f = 0; f < F; ++f) res[f] = P[0][f];
#pragma unroll
			for (int k = 1; k < K; ++k) {
#pragma unroll
				for (int f = 0; f < F; ++f) res[f] = PRODUCT ? res[f] * P[k][f] : res[f] + P[k][f];
			}
		}
	}
	T* o = out + (size_t)i * out_stride + (size_t)level * F;
	if (out_stride % F == 0) { // (then level * F + F <= out_stride: n_slots = ceil(out_stride / F))
		vecF w;
		if constexpr (F == 1) w = (T)res[0];
		else {
#pragma unroll
			for (int f = 0; f < F; ++f) w[f] = (T)res[f];
		}
		*(vecF*)o = w;
	} else {
#pragma unroll
		for (int f = 0; f < F; ++f) if (level * F + f < out_stride) o[f] = (T)res[f];
	}
}

// ---------------------------------------------------------------------------------------------------------------- dL/dx
// W lanes per sample (a power of two, <= 64); lane j of a sample takes levels j, j + W, ...
template <typename T, int D, int F, bool PRODUCT>
__global__ void __launch_bounds__(256) k_kplanes_bwd_input(const uint32_t n, const uint32_t n_levels, const KPlanesShape::Levels lv, const MatView x, const T* __restrict__ params,
                                                           const T* __restrict__ dL_dy, const uint32_t dy_stride, const uint32_t W, const MatViewMut dL_dx) {
	typedef typename VecOf<T, F>::type vecF;
	constexpr int K = D * (D - 1) / 2;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / W, j = gid & (W - 1u);
	const bool live = i < n; // (no early return: every lane of the wave takes part in the butterfly)
	float sum[D];
#pragma unroll
	for (int d = 0; d < D; ++d) sum[d] = 0.0f;
	if (live) {
		float xin[D];
		load_coords<D>(x, i, xin);
		for (uint32_t level = j; level < n_levels; level += W) {
			const float scale = lv.scale[level];
			KPlanesCell<D> cs;
			cs.setup(xin, scale);
			vecF v[K][4];
			kplanes_gather<T, D, F>(cs, params + (size_t)lv.offset[level] * F, lv.resolution[level], lv.entries[level], v);
			float g[F], P[K][F], G[K][F];
			kplanes_load_dy<T, F>(dL_dy + (size_t)i * dy_stride + (size_t)level * F, dy_stride, g);
			if constexpr (PRODUCT && K > 1) kplanes_values<T, D, F>(cs, v, P);
			kplanes_plane_gradients<K, F, PRODUCT>(P, g, G);
			float dx[D]; // in cells; times scale below
#pragma unroll
			for (int d = 0; d < D; ++d) dx[d] = 0.0f;
#pragma unroll
			for (int k = 0; k < K; ++k) {
				const int a = KPLANES_A[D][k], b = KPLANES_B[D][k];
				float da = 0.0f; float db = 0.0f;
#pragma unroll
				for (int f = 0; f < F; ++f) {
					const float v0 = kplanes_elem<T, F>(v[k][0], f), v1 = kplanes_elem<T, F>(v[k][1], f), v2 = kplanes_elem<T, F>(v[k][2], f), v3 = kplanes_elem<T, F>(v[k][3], f);
					da = fmaf(G[k][f], fmaf(cs.pos[b], (v3 - v2) - (v1 - v0), v1 - v0), da); // dP/dx_a = (1 - y)(v1 - v0) + y (v3 - v2)
					db = fmaf(G[k][f], fmaf(cs.pos[a], (v3 - v1) - (v2 - v0), v2 - v0), db); // dP/dx_b = (1 - x)(v2 - v0) + x (v3 - v1)
				}
				dx[a] += da;
				dx[b] += db;
			}
#pragma unroll
			for (int d = 0; d < D; ++d) sum[d] = fmaf(scale, dx[d], sum[d]);
		}
	}
	for (uint32_t m = W >> 1; m >= 1; m >>= 1) {
#pragma unroll
		for (int d = 0; d < D; ++d) sum[d] += __shfl_xor(sum[d], (int)m, 64);
	}
	if (live && j == 0) {
#pragma unroll
		for (int d = 0; d < D; ++d) dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)d * dL_dx.stride_dim] = sum[d];
	}
}

// ---------------------------------------------------------------------------------------------------------------- dL/dparams, half
template <int D, int F, bool PRODUCT>
__global__ void __launch_bounds__(256) k_kplanes_bwd(const uint32_t n, const KPlanesShape::Levels lv, const MatView x, const half_t* __restrict__ params,
                                                     const half_t* __restrict__ dL_dy, const uint32_t dy_stride, unsigned long long* __restrict__ scratch, const int in_lds) {
	extern __shared__ __attribute__((aligned(16))) char kplanes_smem[];
	typedef __attribute__((address_space(3))) unsigned long long lds_u64;
	typedef typename VecOf<half_t, F>::type vecF;
	constexpr int K = D * (D - 1) / 2;
	lds_u64* acc = (lds_u64*)kplanes_smem;
	const uint32_t level = blockIdx.y;
	const uint32_t R = lv.resolution[level], size = lv.entries[level];
	const uint32_t entries = K * size * F; // of the level's K planes (in_lds: at most 8192)
	if (((size_t)K * size * F * sizeof(unsigned long long) <= KPLANES_LDS_BYTES) != (in_lds != 0)) return; // the other launch's level
	if (in_lds) {
		for (uint32_t e = threadIdx.x; e < entries; e += blockDim.x) ((unsigned long long*)kplanes_smem)[e] = 0ull;
		__syncthreads();
	}
	const float scale = lv.scale[level];
	const half_t* __restrict__ table = params + (size_t)lv.offset[level] * F;
	unsigned long long* global_acc = scratch + (size_t)lv.offset[level] * F;
	const uint32_t begin = blockIdx.x * KPLANES_BWD_SAMPLES, end = min(n, begin + KPLANES_BWD_SAMPLES);
	for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
		float xin[D];
		load_coords<D>(x, i, xin);
		KPlanesCell<D> cs;
		cs.setup(xin, scale);
		float g[F], P[K][F], G[K][F];
		kplanes_load_dy<half_t, F>(dL_dy + (size_t)i * dy_stride + (size_t)level * F, dy_stride, g);
		if constexpr (PRODUCT && K > 1) { // the other planes' values: formed once per (sample, level)
			vecF v[K][4];
			kplanes_gather<half_t, D, F>(cs, table, R, size, v);
			kplanes_values<half_t, D, F>(cs, v, P);
		}
		kplanes_plane_gradients<K, F, PRODUCT>(P, g, G);
#pragma unroll
		for (int k = 0; k < K; ++k) {
			const int a = KPLANES_A[D][k], b = KPLANES_B[D][k];
			uint32_t idx[4];
			cs.corners(a, b, R, size, idx);
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				const float w = cs.weight(a, b, c);
				const size_t e = ((size_t)k * size + idx[c]) * F;
#pragma unroll
				for (int f = 0; f < F; ++f) {
					const unsigned long long t = (unsigned long long)half_to_fixed_fast((half_t)(G[k][f] * w));
					if (in_lds) __hip_atomic_fetch_add(acc + (uint32_t)e + f, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					else if (t != 0) atomicAdd(global_acc + e + f, t);
				}
			}
		}
	}
	if (in_lds) {
		__syncthreads();
		for (uint32_t e = threadIdx.x; e < entries; e += blockDim.x) {
			const unsigned long long v = ((unsigned long long*)kplanes_smem)[e];
			if (v != 0) atomicAdd(global_acc + e, v);
		}
	}
}

// scratch (exact sums) -> gradients, rounded once; the scratch is left zeroed for the next pass
__global__ void __launch_bounds__(256) k_kplanes_finalize(const size_t n_params, unsigned long long* __restrict__ scratch, half_t* __restrict__ grad, const int accumulate) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_params) return;
	long long s = (long long)scratch[i];
	if (s != 0) scratch[i] = 0;
	if (accumulate) s += half_to_fixed_fast(grad[i]);
	grad[i] = fixed_to_half_fast(s);
}

// ---------------------------------------------------------------------------------------------------------------- dL/dparams, float
__global__ void __launch_bounds__(256) k_kplanes_zero(const size_t n, float* __restrict__ p) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) p[i] = 0.0f;
}

template <int D, int F, bool PRODUCT>
__global__ void __launch_bounds__(256) k_kplanes_bwd_f32(const uint32_t n, const uint32_t n_levels, const KPlanesShape::Levels lv, const MatView x, const float* __restrict__ params,
                                                         const float* __restrict__ dL_dy, const uint32_t dy_stride, float* __restrict__ grad) {
	typedef typename VecOf<float, F>::type vecF;
	constexpr int K = D * (D - 1) / 2;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_levels;
	if (i >= n) return;
	const uint32_t level = gid - i * n_levels;
	const uint32_t R = lv.resolution[level], size = lv.entries[level];
	float xin[D];
	load_coords<D>(x, i, xin);
	KPlanesCell<D> cs;
	cs.setup(xin, lv.scale[level]);
	float g[F], P[K][F], G[K][F];
	kplanes_load_dy<float, F>(dL_dy + (size_t)i * dy_stride + (size_t)level * F, dy_stride, g);
	if constexpr (PRODUCT && K > 1) {
		vecF v[K][4];
		kplanes_gather<float, D, F>(cs, params + (size_t)lv.offset[level] * F, R, size, v);
		kplanes_values<float, D, F>(cs, v, P);
	}
	kplanes_plane_gradients<K, F, PRODUCT>(P, g, G);
	float* __restrict__ table = grad + (size_t)lv.offset[level] * F;
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const int a = KPLANES_A[D][k], b = KPLANES_B[D][k];
		uint32_t idx[4];
		cs.corners(a, b, R, size, idx);
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			const float w = cs.weight(a, b, c);
			const size_t e = ((size_t)k * size + idx[c]) * F;
#pragma unroll
			for (int f = 0; f < F; ++f) atomicAdd(table + e + f, G[k][f] * w);
		}
	}
}

// ---------------------------------------------------------------------------------------------------------------- second order
// kplanes_values for one feature: the same chains, formed where the feature is walked, so that only K values are live beside the gathers
template <typename T, int D, int F>
__device__ inline void kplanes_values_of_feature(const KPlanesCell<D>& cs, const typename VecOf<T, F>::type (&v)[D * (D - 1) / 2][4], const int f, float (&P)[D * (D - 1) / 2]) {
	constexpr int K = D * (D - 1) / 2;
#pragma unroll
	for (int k = 0; k < K; ++k) {
		P[k] = 0.0f;
#pragma unroll
		for (int c = 0; c < 4; ++c) P[k] = fmaf(cs.weight(KPLANES_A[D][k], KPLANES_B[D][k], c), kplanes_elem<T, F>(v[k][c], f), P[k]);
	}
}

// With v = dL_ddLdx and d = dL_dy, Q = <v, J^T d> = sum_f d_f t_f, t = J v the tangent.  Everything below is per (sample, level, feature) in
// fp32, along vs = scale * v (the direction in cells).  A plane is bilinear in its fractions (u_a, u_b): da = dP/du_a, db = dP/du_b (the first
// order's own chains), the mixed derivative dc = (v3 - v2) - (v1 - v0) is the only second one, and T = D_v P = vs_a da + vs_b db.
template <typename T, int D, int F>
__device__ inline void kplanes_derivatives(const KPlanesCell<D>& cs, const float (&vs)[D], const typename VecOf<T, F>::type (&v)[D * (D - 1) / 2][4], const int f,
                                           float (&da)[D * (D - 1) / 2], float (&db)[D * (D - 1) / 2], float (&dc)[D * (D - 1) / 2], float (&t)[D * (D - 1) / 2]) {
	constexpr int K = D * (D - 1) / 2;
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const int a = KPLANES_A[D][k], b = KPLANES_B[D][k];
		const float v0 = kplanes_elem<T, F>(v[k][0], f), v1 = kplanes_elem<T, F>(v[k][1], f), v2 = kplanes_elem<T, F>(v[k][2], f), v3 = kplanes_elem<T, F>(v[k][3], f);
		dc[k] = (v3 - v2) - (v1 - v0);
		da[k] = fmaf(cs.pos[b], dc[k], v1 - v0);
		db[k] = fmaf(cs.pos[a], (v3 - v1) - (v2 - v0), v2 - v0);
		t[k] = fmaf(vs[b], db[k], vs[a] * da[k]);
	}
}

// O[k] = prod_{q != k} P[q], what the other planes put on plane k, and S[k] = D_v O[k] = sum_{q != k} T[q] prod_{m != k, q} P[m].  The pair
// products are never formed, let alone by division (a plane value may be zero): the prefix and suffix products of the first order carry their
// derivatives along v with them, (p, dp) * (P, T) = (p P, dp P + p T) -- 6 K operations per feature and 2 K + 2 live values instead of K^2 / 2.
// Sum, or one plane: O = 1, S = 0.
template <int K, bool PRODUCT>
__device__ inline void kplanes_others(const float (&P)[K], const float (&t)[K], float (&O)[K], float (&S)[K]) {
	if constexpr (!PRODUCT || K == 1) {
#pragma unroll
		for (int k = 0; k < K; ++k) { O[k] = 1.0f; S[k] = 0.0f; }
	} else {
		float suffix[K], dsuffix[K]; // over q > k
		suffix[K - 1] = 1.0f; dsuffix[K - 1] = 0.0f;
#pragma unroll
		for (int k = K - 2; k >= 0; --k) {
			dsuffix[k] = fmaf(dsuffix[k + 1], P[k + 1], suffix[k + 1] * t[k + 1]);
			suffix[k] = suffix[k + 1] * P[k + 1];
		}
		float prefix = 1.0f, dprefix = 0.0f;
#pragma unroll
		for (int k = 0; k < K; ++k) {
			O[k] = prefix * suffix[k];
			S[k] = fmaf(dprefix, suffix[k], prefix * dsuffix[k]);
			dprefix = fmaf(dprefix, P[k], prefix * t[k]);
			prefix *= P[k];
		}
	}
}

// D_v of corner c's weight, along vs: the weight's factor on the other axis times -+vs
template <int D>
__device__ inline float kplanes_weight_derivative(const KPlanesCell<D>& cs, const float (&vs)[D], const int a, const int b, const int c) {
	return fmaf((c & 2) ? vs[b] : -vs[b], (c & 1) ? cs.pos[a] : 1 - cs.pos[a], ((c & 1) ? vs[a] : -vs[a]) * ((c & 2) ? cs.pos[b] : 1 - cs.pos[b]));
}

template <int D>
__device__ inline void kplanes_load_direction(const MatView& v, const uint32_t i, const float scale, float (&vs)[D]) {
	load_coords<D>(v, i, vs);
#pragma unroll
	for (int d = 0; d < D; ++d) vs[d] = scale * vs[d];
}

// the tangent t[l F + f] = sum_k O_k T_k = D_v (P_0 op P_1 op ...): the forward kernel's work split, its reduction carried with its derivative
// along v (Product: the running product as a pair; the sum of the O_k T_k in that association, never through an O_k).  Rounded to T once;
// the slots behind the levels store zeros, not the forward pass's ones.
template <typename T, int D, int F, bool PRODUCT>
__global__ void __launch_bounds__(256) k_kplanes_tangent(const uint32_t n, const uint32_t n_levels, const KPlanesShape::Levels lv, const MatView x, const MatView v_in,
                                                         const T* __restrict__ params, T* __restrict__ out, const uint32_t out_stride, const uint32_t n_slots) {
	typedef typename VecOf<T, F>::type vecF;
	constexpr int K = D * (D - 1) / 2;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_slots;
	if (i >= n) return;
	const uint32_t level = gid - i * n_slots;
	float res[F];
#pragma unroll
	for (int f = 0; f < F; ++f) res[f] = 0.0f;
	if (level < n_levels) {
		const float scale = lv.scale[level];
		float xin[D], vs[D];
		load_coords<D>(x, i, xin);
		kplanes_load_direction<D>(v_in, i, scale, vs);
		KPlanesCell<D> cs;
		cs.setup(xin, scale);
		vecF v[K][4];
		kplanes_gather<T, D, F>(cs, params + (size_t)lv.offset[level] * F, lv.resolution[level], lv.entries[level], v);
#pragma unroll
		for (int f = 0; f < F; ++f) {
			float da[K], db[K], dc[K], t[K], P[K];
			kplanes_derivatives<T, D, F>(cs, vs, v, f, da, db, dc, t);
			if constexpr (PRODUCT && K > 1) kplanes_values_of_feature<T, D, F>(cs, v, f, P);
			float p = 1.0f, dp = t[0];
			if constexpr (PRODUCT && K > 1) p = P[0];
#pragma unroll
			for (int k = 1; k < K; ++k) {
				if constexpr (PRODUCT) { dp = fmaf(dp, P[k], p * t[k]); p *= P[k]; }
				else dp += t[k];
			}
			res[f] = dp;
		}
	}
	T* o = out + (size_t)i * out_stride + (size_t)level * F;
	if (out_stride % F == 0) { // (as k_kplanes_fwd)
		vecF w;
		if constexpr (F == 1) w = (T)res[0];
		else {
#pragma unroll
			for (int f = 0; f < F; ++f) w[f] = (T)res[f];
		}
		*(vecF*)o = w;
	} else {
#pragma unroll
		for (int f = 0; f < F; ++f) if (level * F + f < out_stride) o[f] = (T)res[f];
	}
}

// dQ/dx: k_kplanes_bwd_input's work split and butterfly.  Plane k = (a, b) feeds x_a with d_f (O_k vs_b dc_k + S_k da_k) and x_b with
// d_f (O_k vs_a dc_k + S_k db_k), in cells; times scale per level.  The features are walked one at a time over the gathers the thread
// holds: beside them only one feature's 4 K derivatives, 2 K + 2 prefix / suffix values and O, S are live (kplanes_others).
template <typename T, int D, int F, bool PRODUCT>
__global__ void __launch_bounds__(256) k_kplanes_bwdbwd_input(const uint32_t n, const uint32_t n_levels, const KPlanesShape::Levels lv, const MatView x, const MatView v_in,
                                                              const T* __restrict__ params, const T* __restrict__ dL_dy, const uint32_t dy_stride, const uint32_t W, const MatViewMut dL_dx) {
	typedef typename VecOf<T, F>::type vecF;
	constexpr int K = D * (D - 1) / 2;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / W, j = gid & (W - 1u);
	const bool live = i < n; // (no early return: every lane of the wave takes part in the butterfly)
	float sum[D];
#pragma unroll
	for (int d = 0; d < D; ++d) sum[d] = 0.0f;
	if (live) {
		float xin[D];
		load_coords<D>(x, i, xin);
		for (uint32_t level = j; level < n_levels; level += W) {
			const float scale = lv.scale[level];
			float vs[D];
			kplanes_load_direction<D>(v_in, i, scale, vs);
			KPlanesCell<D> cs;
			cs.setup(xin, scale);
			vecF v[K][4];
			kplanes_gather<T, D, F>(cs, params + (size_t)lv.offset[level] * F, lv.resolution[level], lv.entries[level], v);
			float g[F];
			kplanes_load_dy<T, F>(dL_dy + (size_t)i * dy_stride + (size_t)level * F, dy_stride, g);
			float dx[D]; // in cells; times scale below
#pragma unroll
			for (int d = 0; d < D; ++d) dx[d] = 0.0f;
#pragma unroll
			for (int f = 0; f < F; ++f) {
				float da[K], db[K], dc[K], t[K], P[K], O[K], S[K];
				kplanes_derivatives<T, D, F>(cs, vs, v, f, da, db, dc, t);
				if constexpr (PRODUCT && K > 1) kplanes_values_of_feature<T, D, F>(cs, v, f, P);
				kplanes_others<K, PRODUCT>(P, t, O, S);
#pragma unroll
				for (int k = 0; k < K; ++k) {
					const int a = KPLANES_A[D][k], b = KPLANES_B[D][k];
					if constexpr (PRODUCT && K > 1) {
						dx[a] = fmaf(g[f], fmaf(O[k], vs[b] * dc[k], S[k] * da[k]), dx[a]);
						dx[b] = fmaf(g[f], fmaf(O[k], vs[a] * dc[k], S[k] * db[k]), dx[b]);
					} else {
						dx[a] = fmaf(g[f], vs[b] * dc[k], dx[a]);
						dx[b] = fmaf(g[f], vs[a] * dc[k], dx[b]);
					}
				}
			}
#pragma unroll
			for (int d = 0; d < D; ++d) sum[d] = fmaf(scale, dx[d], sum[d]);
		}
	}
	for (uint32_t m = W >> 1; m >= 1; m >>= 1) {
#pragma unroll
		for (int d = 0; d < D; ++d) sum[d] += __shfl_xor(sum[d], (int)m, 64);
	}
	if (live && j == 0) {
#pragma unroll
		for (int d = 0; d < D; ++d) dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)d * dL_dx.stride_dim] = sum[d];
	}
}

// O[k][f] and S[k][f] of a (sample, level) for the parameter kernels (Product with K > 1 only: the gathers die here)
template <typename T, int D, int F>
__device__ inline void kplanes_others_of_level(const KPlanesCell<D>& cs, const float (&vs)[D], const T* __restrict__ table, const uint32_t R, const uint32_t size,
                                               float (&O)[D * (D - 1) / 2][F], float (&S)[D * (D - 1) / 2][F]) {
	constexpr int K = D * (D - 1) / 2;
	typename VecOf<T, F>::type v[K][4];
	kplanes_gather<T, D, F>(cs, table, R, size, v);
#pragma unroll
	for (int f = 0; f < F; ++f) {
		float da[K], db[K], dc[K], t[K], P[K], Of[K], Sf[K];
		kplanes_derivatives<T, D, F>(cs, vs, v, f, da, db, dc, t);
		kplanes_values_of_feature<T, D, F>(cs, v, f, P);
		kplanes_others<K, true>(P, t, Of, Sf);
#pragma unroll
		for (int k = 0; k < K; ++k) { O[k][f] = Of[k]; S[k][f] = Sf[k]; }
	}
}

// dQ/dparams: (plane k, corner c, feature f) receives d_f (O_k D_v w_c + w_c S_k); Sum: d_f D_v w_c, and no parameter is read.
// Half: k_kplanes_bwd's work split and accumulators (signed 2^-24 fixed point, exact and order-independent; k_kplanes_finalize
// rounds once).  The contributions carry scale (and, through S, scale times the other planes' slopes): one beyond half's range converts to
// +-inf, whose fixed-point form is not defined -- the same limit as the grid's second-order parameter gradient.
template <int D, int F, bool PRODUCT>
__global__ void __launch_bounds__(256) k_kplanes_bwdbwd(const uint32_t n, const KPlanesShape::Levels lv, const MatView x, const MatView v_in, const half_t* __restrict__ params,
                                                        const half_t* __restrict__ dL_dy, const uint32_t dy_stride, unsigned long long* __restrict__ scratch, const int in_lds) {
	extern __shared__ __attribute__((aligned(16))) char kplanes_smem[];
	typedef __attribute__((address_space(3))) unsigned long long lds_u64;
	constexpr int K = D * (D - 1) / 2;
	lds_u64* acc = (lds_u64*)kplanes_smem;
	const uint32_t level = blockIdx.y;
	const uint32_t R = lv.resolution[level], size = lv.entries[level];
	const uint32_t entries = K * size * F; // of the level's K planes (in_lds: at most 8192)
	if (((size_t)K * size * F * sizeof(unsigned long long) <= KPLANES_LDS_BYTES) != (in_lds != 0)) return; // the other launch's level
	if (in_lds) {
		for (uint32_t e = threadIdx.x; e < entries; e += blockDim.x) ((unsigned long long*)kplanes_smem)[e] = 0ull;
		__syncthreads();
	}
	const float scale = lv.scale[level];
	const half_t* __restrict__ table = params + (size_t)lv.offset[level] * F;
	unsigned long long* global_acc = scratch + (size_t)lv.offset[level] * F;
	const uint32_t begin = blockIdx.x * KPLANES_BWD_SAMPLES, end = min(n, begin + KPLANES_BWD_SAMPLES);
	for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
		float xin[D], vs[D];
		load_coords<D>(x, i, xin);
		kplanes_load_direction<D>(v_in, i, scale, vs);
		KPlanesCell<D> cs;
		cs.setup(xin, scale);
		float g[F], O[K][F], S[K][F];
		kplanes_load_dy<half_t, F>(dL_dy + (size_t)i * dy_stride + (size_t)level * F, dy_stride, g);
		if constexpr (PRODUCT && K > 1) kplanes_others_of_level<half_t, D, F>(cs, vs, table, R, size, O, S);
#pragma unroll
		for (int k = 0; k < K; ++k) {
			const int a = KPLANES_A[D][k], b = KPLANES_B[D][k];
			uint32_t idx[4];
			cs.corners(a, b, R, size, idx);
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				const float w = cs.weight(a, b, c), dw = kplanes_weight_derivative<D>(cs, vs, a, b, c);
				const size_t e = ((size_t)k * size + idx[c]) * F;
#pragma unroll
				for (int f = 0; f < F; ++f) {
					float contribution;
					if constexpr (PRODUCT && K > 1) contribution = g[f] * fmaf(O[k][f], dw, w * S[k][f]); else contribution = g[f] * dw;
					const unsigned long long t = (unsigned long long)half_to_fixed_fast((half_t)contribution);
					if (in_lds) __hip_atomic_fetch_add(acc + (uint32_t)e + f, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					else if (t != 0) atomicAdd(global_acc + e + f, t);
				}
			}
		}
	}
	if (in_lds) {
		__syncthreads();
		for (uint32_t e = threadIdx.x; e < entries; e += blockDim.x) {
			const unsigned long long v = ((unsigned long long*)kplanes_smem)[e];
			if (v != 0) atomicAdd(global_acc + e, v);
		}
	}
}

// dQ/dparams, float: one thread per (sample, level), float atomicAdd into the gradient (order not fixed)
template <int D, int F, bool PRODUCT>
__global__ void __launch_bounds__(256) k_kplanes_bwdbwd_f32(const uint32_t n, const uint32_t n_levels, const KPlanesShape::Levels lv, const MatView x, const MatView v_in,
                                                            const float* __restrict__ params, const float* __restrict__ dL_dy, const uint32_t dy_stride, float* __restrict__ grad) {
	constexpr int K = D * (D - 1) / 2;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_levels;
	if (i >= n) return;
	const uint32_t level = gid - i * n_levels;
	const uint32_t R = lv.resolution[level], size = lv.entries[level];
	const float scale = lv.scale[level];
	float xin[D], vs[D];
	load_coords<D>(x, i, xin);
	kplanes_load_direction<D>(v_in, i, scale, vs);
	KPlanesCell<D> cs;
	cs.setup(xin, scale);
	float g[F], O[K][F], S[K][F];
	kplanes_load_dy<float, F>(dL_dy + (size_t)i * dy_stride + (size_t)level * F, dy_stride, g);
	if constexpr (PRODUCT && K > 1) kplanes_others_of_level<float, D, F>(cs, vs, params + (size_t)lv.offset[level] * F, R, size, O, S);
	float* __restrict__ table = grad + (size_t)lv.offset[level] * F;
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const int a = KPLANES_A[D][k], b = KPLANES_B[D][k];
		uint32_t idx[4];
		cs.corners(a, b, R, size, idx);
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			const float w = cs.weight(a, b, c), dw = kplanes_weight_derivative<D>(cs, vs, a, b, c);
			const size_t e = ((size_t)k * size + idx[c]) * F;
#pragma unroll
			for (int f = 0; f < F; ++f) {
				if constexpr (PRODUCT && K > 1) atomicAdd(table + e + f, g[f] * fmaf(O[k][f], dw, w * S[k][f])); else atomicAdd(table + e + f, g[f] * dw);
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------------------------- launches
uint32_t blocks_for(uint64_t threads) {
	CHECK_THROW(threads < (1ull << 32));
	return (uint32_t)((threads + 255) / 256);
}

size_t n_params_of(const KPlanesShape& p) {
	const uint32_t last = p.n_levels - 1, K = p.n_dims * (p.n_dims - 1) / 2;
	return ((size_t)p.levels.offset[last] + (size_t)K * p.levels.entries[last]) * p.n_features_per_level;
}

template <typename T, int D, int F, bool PRODUCT>
void launch_fwd(hipStream_t s, const KPlanesShape& p, uint32_t n, MatView x, const void* params, void* out, uint32_t out_stride) {
	const uint32_t n_slots = div_round_up(out_stride, (uint32_t)F);
	hipLaunchKernelGGL((k_kplanes_fwd<T, D, F, PRODUCT>), dim3(blocks_for((uint64_t)n * n_slots)), dim3(256), 0, s, n, p.n_levels, p.levels, x, (const T*)params, (T*)out, out_stride, n_slots);
}

template <typename T, int D, int F, bool PRODUCT>
void launch_bwd_input(hipStream_t s, const KPlanesShape& p, uint32_t n, MatView x, const void* params, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	uint32_t W = 1;
	while (W < p.n_levels && W < 64) W *= 2;
	hipLaunchKernelGGL((k_kplanes_bwd_input<T, D, F, PRODUCT>), dim3(blocks_for((uint64_t)n * W)), dim3(256), 0, s, n, p.n_levels, p.levels, x, (const T*)params, (const T*)dL_dy, dy_stride, W,
	                   dL_dx);
}

template <int D, int F, bool PRODUCT>
void launch_bwd(hipStream_t s, const KPlanesShape& p, bool fp32, uint32_t n, MatView x, const void* params, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad,
                bool accumulate) {
	constexpr uint32_t K = D * (D - 1) / 2;
	const size_t n_params = n_params_of(p);
	if (fp32) {
		if (!accumulate) hipLaunchKernelGGL(k_kplanes_zero, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (float*)grad);
		if (n > 0) hipLaunchKernelGGL((k_kplanes_bwd_f32<D, F, PRODUCT>), dim3(blocks_for((uint64_t)n * p.n_levels)), dim3(256), 0, s, n, p.n_levels, p.levels, x, (const float*)params,
		                              (const float*)dL_dy, dy_stride, (float*)grad);
		return;
	}
	if (n > 0) {
		// One launch for the levels whose planes fit the LDS (it asks for the largest of them) and one for the rest; in each the other
		// levels' workgroups return at once.
		size_t lds_bytes = 0;
		bool any_global = false;
		for (uint32_t l = 0; l < p.n_levels; ++l) {
			const size_t bytes = (size_t)K * p.levels.entries[l] * F * sizeof(uint64_t);
			if (bytes <= KPLANES_LDS_BYTES) lds_bytes = std::max(lds_bytes, bytes);
			else any_global = true;
		}
		const dim3 grid(div_round_up(n, KPLANES_BWD_SAMPLES), p.n_levels);
		if (lds_bytes > 0) hipLaunchKernelGGL((k_kplanes_bwd<D, F, PRODUCT>), grid, dim3(256), (uint32_t)lds_bytes, s, n, p.levels, x, (const half_t*)params, (const half_t*)dL_dy, dy_stride,
		                                      (unsigned long long*)scratch, 1);
		if (any_global) hipLaunchKernelGGL((k_kplanes_bwd<D, F, PRODUCT>), grid, dim3(256), 0, s, n, p.levels, x, (const half_t*)params, (const half_t*)dL_dy, dy_stride,
		                                   (unsigned long long*)scratch, 0);
	}
	hipLaunchKernelGGL(k_kplanes_finalize, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (unsigned long long*)scratch, (half_t*)grad, accumulate ? 1 : 0);
}

template <typename T, int D, int F, bool PRODUCT>
void launch_tangent(hipStream_t s, const KPlanesShape& p, uint32_t n, MatView x, MatView v, const void* params, void* t, uint32_t t_stride) {
	const uint32_t n_slots = div_round_up(t_stride, (uint32_t)F);
	hipLaunchKernelGGL((k_kplanes_tangent<T, D, F, PRODUCT>), dim3(blocks_for((uint64_t)n * n_slots)), dim3(256), 0, s, n, p.n_levels, p.levels, x, v, (const T*)params, (T*)t, t_stride, n_slots);
}

template <typename T, int D, int F, bool PRODUCT>
void launch_bwdbwd_input(hipStream_t s, const KPlanesShape& p, uint32_t n, MatView x, MatView v, const void* params, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	uint32_t W = 1;
	while (W < p.n_levels && W < 64) W *= 2;
	hipLaunchKernelGGL((k_kplanes_bwdbwd_input<T, D, F, PRODUCT>), dim3(blocks_for((uint64_t)n * W)), dim3(256), 0, s, n, p.n_levels, p.levels, x, v, (const T*)params, (const T*)dL_dy,
	                   dy_stride, W, dL_dx);
}

// (launch_bwd's split of the levels between LDS and global accumulators, its zeroing and its finalize pass)
template <int D, int F, bool PRODUCT>
void launch_bwdbwd(hipStream_t s, const KPlanesShape& p, bool fp32, uint32_t n, MatView x, MatView v, const void* params, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad,
                   bool accumulate) {
	constexpr uint32_t K = D * (D - 1) / 2;
	const size_t n_params = n_params_of(p);
	if (fp32) {
		if (!accumulate) hipLaunchKernelGGL(k_kplanes_zero, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (float*)grad);
		if (n > 0) hipLaunchKernelGGL((k_kplanes_bwdbwd_f32<D, F, PRODUCT>), dim3(blocks_for((uint64_t)n * p.n_levels)), dim3(256), 0, s, n, p.n_levels, p.levels, x, v, (const float*)params,
		                              (const float*)dL_dy, dy_stride, (float*)grad);
		return;
	}
	if (n > 0) {
		size_t lds_bytes = 0;
		bool any_global = false;
		for (uint32_t l = 0; l < p.n_levels; ++l) {
			const size_t bytes = (size_t)K * p.levels.entries[l] * F * sizeof(uint64_t);
			if (bytes <= KPLANES_LDS_BYTES) lds_bytes = std::max(lds_bytes, bytes);
			else any_global = true;
		}
		const dim3 grid(div_round_up(n, KPLANES_BWD_SAMPLES), p.n_levels);
		if (lds_bytes > 0) hipLaunchKernelGGL((k_kplanes_bwdbwd<D, F, PRODUCT>), grid, dim3(256), (uint32_t)lds_bytes, s, n, p.levels, x, v, (const half_t*)params, (const half_t*)dL_dy, dy_stride,
		                                      (unsigned long long*)scratch, 1);
		if (any_global) hipLaunchKernelGGL((k_kplanes_bwdbwd<D, F, PRODUCT>), grid, dim3(256), 0, s, n, p.levels, x, v, (const half_t*)params, (const half_t*)dL_dy, dy_stride,
		                                   (unsigned long long*)scratch, 0);
	}
	hipLaunchKernelGGL(k_kplanes_finalize, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (unsigned long long*)scratch, (half_t*)grad, accumulate ? 1 : 0);
}

// run CALL with the compile-time <D, F, PRODUCT> of the shape (one plane: the reductions coincide, Sum's code serves both)
#define TCNN_KPLANES_F(D_, P_, CALL) \
	switch (p.n_features_per_level) { \
		case 1: { constexpr int D = D_, F = 1; constexpr bool PRODUCT = P_; CALL; } break; \
		case 2: { constexpr int D = D_, F = 2; constexpr bool PRODUCT = P_; CALL; } break; \
		case 4: { constexpr int D = D_, F = 4; constexpr bool PRODUCT = P_; CALL; } break; \
		case 8: { constexpr int D = D_, F = 8; constexpr bool PRODUCT = P_; CALL; } break; \
		default: throw std::runtime_error{"KPlanes: n_features_per_level must be 1, 2, 4 or 8"}; \
	}
#define TCNN_KPLANES_DISPATCH(CALL) \
	switch (p.n_dims) { \
		case 2: TCNN_KPLANES_F(2, false, CALL) break; \
		case 3: if (p.product) { TCNN_KPLANES_F(3, true, CALL) } else { TCNN_KPLANES_F(3, false, CALL) } break; \
		case 4: if (p.product) { TCNN_KPLANES_F(4, true, CALL) } else { TCNN_KPLANES_F(4, false, CALL) } break; \
		default: throw std::runtime_error{"KPlanes: n_dims_to_encode must be 2 to 4"}; \
	}

} // namespace

void kplanes_forward(hipStream_t stream, const KPlanesShape& p, bool fp32, uint32_t n, MatView x, const void* params, void* out, uint32_t out_stride) {
	if (n == 0 || out_stride == 0) return;
	CHECK_THROW(out_stride >= p.n_levels * p.n_features_per_level);
	if (fp32) { TCNN_KPLANES_DISPATCH((launch_fwd<float, D, F, PRODUCT>(stream, p, n, x, params, out, out_stride))) }
	else { TCNN_KPLANES_DISPATCH((launch_fwd<half_t, D, F, PRODUCT>(stream, p, n, x, params, out, out_stride))) }
	HIP_CHECK_THROW(hipGetLastError());
}

void kplanes_backward_input(hipStream_t stream, const KPlanesShape& p, bool fp32, uint32_t n, MatView x, const void* params, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	if (n == 0) return;
	if (fp32) { TCNN_KPLANES_DISPATCH((launch_bwd_input<float, D, F, PRODUCT>(stream, p, n, x, params, dL_dy, dy_stride, dL_dx))) }
	else { TCNN_KPLANES_DISPATCH((launch_bwd_input<half_t, D, F, PRODUCT>(stream, p, n, x, params, dL_dy, dy_stride, dL_dx))) }
	HIP_CHECK_THROW(hipGetLastError());
}

void kplanes_backward(hipStream_t stream, const KPlanesShape& p, bool fp32, uint32_t n, MatView x, const void* params, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad,
                      bool accumulate) {
	TCNN_KPLANES_DISPATCH((launch_bwd<D, F, PRODUCT>(stream, p, fp32, n, x, params, dL_dy, dy_stride, scratch, grad, accumulate)))
	HIP_CHECK_THROW(hipGetLastError());
}

void kplanes_tangent(hipStream_t stream, const KPlanesShape& p, bool fp32, uint32_t n, MatView x, MatView v, const void* params, void* t, uint32_t t_stride) {
	if (n == 0 || t_stride == 0) return;
	CHECK_THROW(t_stride >= p.n_levels * p.n_features_per_level);
	if (fp32) { TCNN_KPLANES_DISPATCH((launch_tangent<float, D, F, PRODUCT>(stream, p, n, x, v, params, t, t_stride))) }
	else { TCNN_KPLANES_DISPATCH((launch_tangent<half_t, D, F, PRODUCT>(stream, p, n, x, v, params, t, t_stride))) }
	HIP_CHECK_THROW(hipGetLastError());
}

void kplanes_backward_backward_input(hipStream_t stream, const KPlanesShape& p, bool fp32, uint32_t n, MatView x, MatView v, const void* params, const void* dL_dy, uint32_t dy_stride,
                                     MatViewMut* dL_dx, uint64_t* scratch, void* grad, bool accumulate) {
	if (dL_dx && n > 0) {
		if (fp32) { TCNN_KPLANES_DISPATCH((launch_bwdbwd_input<float, D, F, PRODUCT>(stream, p, n, x, v, params, dL_dy, dy_stride, *dL_dx))) }
		else { TCNN_KPLANES_DISPATCH((launch_bwdbwd_input<half_t, D, F, PRODUCT>(stream, p, n, x, v, params, dL_dy, dy_stride, *dL_dx))) }
	}
	if (grad) { TCNN_KPLANES_DISPATCH((launch_bwdbwd<D, F, PRODUCT>(stream, p, fp32, n, x, v, params, dL_dy, dy_stride, scratch, grad, accumulate))) }
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace tcnn_amd
