// k_permuto.hip -- the permutohedral-lattice hash encoding ("PermutoGrid"): per level the input is scaled, elevated onto the hyperplane
// sum(E) = 0 of R^(D+1), and interpolated linearly on the lattice SIMPLEX that holds it -- D + 1 vertices, where a cubic grid cell has
// 2^D corners (Adams, Baek, Davis: "Fast high-dimensional filtering using the permutohedral lattice", 2010; the lookup of section 3).
// Parameters: T [L][2^log2_T][F], level-major; a vertex's first D key components go through the grid's coherent-prime hash.
//
// The lookup (permuto_simplex) is written without a single array that a run-time value indexes: the recipe's b[D - rank[i]] += d becomes
// "the residuals sorted by rank", s[k] = sum_i (rank[i] == k ? d_i : 0) over compile-time i and k, and b[r] = s[D - r] - s[D + 1 - r]
// (b[0] = s[D] + (1 - s[0])) -- the same additions the recipe makes, O(D^2) selects on registers, no scratch and no LDS.
//
//   k_permuto_fwd        one thread per (sample, level), consecutive lanes = consecutive levels of a sample (dense AoS rows); all D + 1
//                        indices first, then all gathers, then one fp32 fma chain in ascending vertex order, rounded to T once.
//   k_permuto_bwd_input  the same lookup again from x (nothing but x is kept from the forward pass); a sample's levels sit on W
//                        neighbouring lanes (W: the power of two >= L, at most 64; more levels than lanes are looped), and the sum
//                        over levels is a fixed-order xor butterfly over those W lanes.  One store per sample, no atomics.
//   k_permuto_bwd        dL/dparams, half: a workgroup owns one level and a slice of the batch; every contribution (half)(dL/dy * b) is
//                        added exactly as 2^-24 fixed point -- into a 64-bit table in LDS when the level fits (T F 8 bytes <= 64 KB: two
//                        workgroups per CU in gfx950's 160 KB), flushed to the global scratch afterwards, else straight into the global
//                        scratch.  k_permuto_finalize rounds each sum once and leaves the scratch zero.  Integer adds: any order, same bits.
//   k_permuto_bwd_f32    fp32 modules: float atomicAdd into the gradient itself (order not fixed, as on the fp32 grid route).
// Second order ("second_order": true).  b is affine in x inside a simplex, so the Hessian term is zero: what is left of <v, J^T d> is
// beta = db/dx . v (PermutoSimplex::weight_tangent: the elevation of v, sorted by the ranks the lookup already has).
//   k_permuto_tangent    k_permuto_fwd's split; simplex, indices and gathers once, then a rolled loop over any number of directions.
//   k_permuto_bwdbwd     k_permuto_bwd with beta in place of b (signed contributions, the same exact sums); k_permuto_bwdbwd_f32 likewise.
//
// Compiled with -ffp-contract=off: every fused multiply-add is explicit.
#include "grid_fixed.h"

namespace tcnn_amd {
namespace {

constexpr uint32_t PERMUTO_LDS_BYTES = 64 * 1024;  // accumulators of one level in LDS: two workgroups per CU
constexpr uint32_t PERMUTO_BWD_SAMPLES = 4096;     // samples per workgroup of k_permuto_bwd

// 1 / sqrt((i + 1) (i + 2)), rounded to float
__device__ constexpr float PERMUTO_SF[GRID_MAX_DIMS] = {0.70710678118654752f, 0.40824829046386302f, 0.28867513459481288f, 0.22360679774997897f,
                                                        0.18257418583505537f, 0.15430334996209191f, 0.13363062095621219f};

// The simplex of the lattice that holds p = x * scale: rem0 (the remainder-0 point, after the fix-up), rank (a permutation of 0 .. D)
// and the barycentric weights b of its D + 1 vertices.
template <int D>
struct PermutoSimplex {
	static constexpr int N = D + 1;
	int rem0[N], rank[N];
	float b[N];

	__device__ inline void setup(const float (&x)[D], const float scale) {
		constexpr float inv = 1.0f / (float)N;
		float E[N];
		float sm = 0.0f;
#pragma unroll
		for (int i = D; i >= 1; --i) { // elevate
			const float cf = (x[i - 1] * scale) * PERMUTO_SF[i - 1];
			E[i] = sm - (float)i * cf;
			sm += cf;
		}
		E[0] = sm;
		int sum = 0;
		float delta[N];
#pragma unroll
		for (int i = 0; i < N; ++i) { // the nearest remainder-0 point
			const float v = E[i] * inv, up = ceilf(v), down = floorf(v);
			const float c = (up * (float)N - E[i] < E[i] - down * (float)N) ? up : down;
			const float r0 = c * (float)N;
			rem0[i] = (int)r0;
			sum += (int)c;
			delta[i] = E[i] - r0;
			rank[i] = 0;
		}
#pragma unroll
		for (int i = 0; i < N; ++i) {
#pragma unroll
			for (int j = i + 1; j < N; ++j) {
				const bool lt = delta[i] < delta[j];
				rank[i] += lt ? 1 : 0;
				rank[j] += lt ? 0 : 1;
			}
		}
		float s[N]; // the residuals / (D + 1), sorted by rank
#pragma unroll
		for (int k = 0; k < N; ++k) s[k] = 0.0f;
#pragma unroll
		for (int i = 0; i < N; ++i) { // fix-up: back onto the hyperplane
			const bool dec = sum > 0 && rank[i] >= N - sum, inc = sum < 0 && rank[i] < -sum;
			const int shift = inc ? N : (dec ? -N : 0);
			rem0[i] += shift;
			rank[i] += sum + shift;
			const float d = (E[i] - (float)rem0[i]) * inv;
#pragma unroll
			for (int k = 0; k < N; ++k) s[k] += rank[i] == k ? d : 0.0f;
		}
		b[0] = s[D] + (1.0f - s[0]);
#pragma unroll
		for (int r = 1; r < N; ++r) b[r] = s[D - r] - s[N - r];
	}

	// table entry of vertex r (compile-time in every caller): key_i = rem0_i + r, minus D + 1 where rank_i > D - r; int32 -> uint32 wraps
	__device__ inline uint32_t index(const int r, const uint32_t mask) const {
		uint32_t h = 0;
#pragma unroll
		for (int i = 0; i < D; ++i) h ^= (uint32_t)(rem0[i] + r - (rank[i] > D - r ? N : 0)) * GRID_COHERENT_PRIMES[i];
		return h & mask;
	}

	// dL/dx of this level from c[r] = dL/d b[r]: b is affine in E inside the simplex (1 / (D + 1) per E component where the value walk
	// has d), E is linear in x (the transpose of the elevation), and p = x * scale
	__device__ inline void input_gradient(const float (&c)[N], const float scale, float (&dx)[D]) const {
		constexpr float inv = 1.0f / (float)N;
		float cs[N]; // dL/d d_i for the component of rank k
		cs[0] = c[D] - c[0];
#pragma unroll
		for (int k = 1; k < N; ++k) cs[k] = c[D - k] - c[N - k];
		float pre = 0.0f; // sum of dL/dE_i over i < j
#pragma unroll
		for (int i = 0; i < N; ++i) {
			float dE = 0.0f;
#pragma unroll
			for (int k = 0; k < N; ++k) dE += rank[i] == k ? cs[k] : 0.0f;
			dE *= inv;
			if (i >= 1) dx[i - 1] = (scale * PERMUTO_SF[i - 1]) * (pre - (float)i * dE);
			pre += dE;
		}
	}

	// beta[r] = d b[r] / dx along v inside this simplex: setup()'s elevation applied to the direction (no rounding, no rem0), sorted by
	// the ranks after the fix-up, and the additions setup() makes for b without its 1 -.  The beta sum to zero.
	__device__ inline void weight_tangent(const float (&v)[D], const float scale, float (&beta)[N]) const {
		constexpr float inv = 1.0f / (float)N;
		float Ep[N];
		float sm = 0.0f;
#pragma unroll
		for (int i = D; i >= 1; --i) {
			const float cf = (v[i - 1] * scale) * PERMUTO_SF[i - 1];
			Ep[i] = sm - (float)i * cf;
			sm += cf;
		}
		Ep[0] = sm;
		float s[N];
#pragma unroll
		for (int k = 0; k < N; ++k) s[k] = 0.0f;
#pragma unroll
		for (int i = 0; i < N; ++i) {
			const float d = Ep[i] * inv;
#pragma unroll
			for (int k = 0; k < N; ++k) s[k] += rank[i] == k ? d : 0.0f;
		}
		beta[0] = s[D] - s[0];
#pragma unroll
		for (int r = 1; r < N; ++r) beta[r] = s[D - r] - s[N - r];
	}
};

template <typename T, int F> __device__ inline float permuto_elem(const typename VecOf<T, F>::type& v, int f) {
	if constexpr (F == 1) return (float)v; else return (float)v[f];
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <typename T, int D, int F>
__global__ void __launch_bounds__(256) k_permuto_fwd(const uint32_t n, const uint32_t n_levels, const uint32_t log2_T, const PermutoShape::Scales scales, const MatView x,
                                                     const T* __restrict__ params, T* __restrict__ out, const uint32_t out_stride, const uint32_t n_slots) {
	typedef typename VecOf<T, F>::type vecF;
	constexpr int N = D + 1;
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
		PermutoSimplex<D> sx;
		sx.setup(xin, scales.v[level]);
		const T* __restrict__ table = params + (((size_t)level << log2_T) * F);
		const uint32_t mask = (1u << log2_T) - 1u;
		uint32_t index[N];
		vecF v[N];
#pragma unroll
		for (int r = 0; r < N; ++r) index[r] = sx.index(r, mask);
#pragma unroll
		for (int r = 0; r < N; ++r) v[r] = *(const vecF*)&table[(size_t)index[r] * F];
#pragma unroll
		for (int f = 0; f < F; ++f) res[f] = 0.0f;
#pragma unroll
		for (int r = 0; r < N; ++r) {
#pragma unroll
			for (int f = 0; f < F; ++f) res[f] = fmaf(sx.b[r], permuto_elem<T, F>(v[r], f), res[f]);
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
template <typename T, int D, int F>
__global__ void __launch_bounds__(256) k_permuto_bwd_input(const uint32_t n, const uint32_t n_levels, const uint32_t log2_T, const PermutoShape::Scales scales, const MatView x,
                                                           const T* __restrict__ params, const T* __restrict__ dL_dy, const uint32_t dy_stride, const uint32_t W,
                                                           const MatViewMut dL_dx) {
	typedef typename VecOf<T, F>::type vecF;
	constexpr int N = D + 1;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / W, j = gid & (W - 1u);
	const bool live = i < n; // (no early return: every lane of the wave takes part in the butterfly)
	float sum[D];
#pragma unroll
	for (int d = 0; d < D; ++d) sum[d] = 0.0f;
	if (live) {
		float xin[D];
		load_coords<D>(x, i, xin);
		const uint32_t mask = (1u << log2_T) - 1u;
		for (uint32_t level = j; level < n_levels; level += W) {
			const float scale = scales.v[level];
			PermutoSimplex<D> sx;
			sx.setup(xin, scale);
			const T* __restrict__ table = params + (((size_t)level << log2_T) * F);
			const T* __restrict__ dy = dL_dy + (size_t)i * dy_stride + (size_t)level * F;
			uint32_t index[N];
			vecF v[N];
#pragma unroll
			for (int r = 0; r < N; ++r) index[r] = sx.index(r, mask);
#pragma unroll
			for (int r = 0; r < N; ++r) v[r] = *(const vecF*)&table[(size_t)index[r] * F];
			float g[F];
#pragma unroll
			for (int f = 0; f < F; ++f) g[f] = (float)dy[f];
			float c[N];
#pragma unroll
			for (int r = 0; r < N; ++r) {
				c[r] = 0.0f;
#pragma unroll
				for (int f = 0; f < F; ++f) c[r] = fmaf(g[f], permuto_elem<T, F>(v[r], f), c[r]);
			}
			float dx[D];
			sx.input_gradient(c, scale, dx);
#pragma unroll
			for (int d = 0; d < D; ++d) sum[d] += dx[d];
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
template <int D, int F>
__global__ void __launch_bounds__(256) k_permuto_bwd(const uint32_t n, const uint32_t log2_T, const PermutoShape::Scales scales, const MatView x, const half_t* __restrict__ dL_dy,
                                                     const uint32_t dy_stride, unsigned long long* __restrict__ scratch, const int in_lds) {
	extern __shared__ __attribute__((aligned(16))) char permuto_smem[];
	typedef __attribute__((address_space(3))) unsigned long long lds_u64;
	typedef typename VecOf<half_t, F>::type vecF;
	constexpr int N = D + 1;
	lds_u64* acc = (lds_u64*)permuto_smem;
	const uint32_t level = blockIdx.y;
	const uint32_t entries = (1u << log2_T) * F, mask = (1u << log2_T) - 1u;
	if (in_lds) {
		for (uint32_t e = threadIdx.x; e < entries; e += blockDim.x) ((unsigned long long*)permuto_smem)[e] = 0ull;
		__syncthreads();
	}
	const float scale = scales.v[level];
	unsigned long long* global_acc = scratch + (((size_t)level << log2_T) * F);
	const uint32_t begin = blockIdx.x * PERMUTO_BWD_SAMPLES, end = min(n, begin + PERMUTO_BWD_SAMPLES);
	for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
		float xin[D];
		load_coords<D>(x, i, xin);
		PermutoSimplex<D> sx;
		sx.setup(xin, scale);
		const half_t* __restrict__ dy = dL_dy + (size_t)i * dy_stride + (size_t)level * F;
		float g[F];
		if (dy_stride % F == 0) {
			const vecF gv = *(const vecF*)dy;
#pragma unroll
			for (int f = 0; f < F; ++f) g[f] = permuto_elem<half_t, F>(gv, f);
		} else {
#pragma unroll
			for (int f = 0; f < F; ++f) g[f] = (float)dy[f];
		}
#pragma unroll
		for (int r = 0; r < N; ++r) {
			const uint32_t e = sx.index(r, mask) * F;
#pragma unroll
			for (int f = 0; f < F; ++f) {
				const unsigned long long c = (unsigned long long)half_to_fixed_fast((half_t)(g[f] * sx.b[r]));
				if (in_lds) __hip_atomic_fetch_add(acc + e + f, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				else if (c != 0) atomicAdd(global_acc + e + f, c);
			}
		}
	}
	if (in_lds) {
		__syncthreads();
		for (uint32_t e = threadIdx.x; e < entries; e += blockDim.x) {
			const unsigned long long v = ((unsigned long long*)permuto_smem)[e];
			if (v != 0) atomicAdd(global_acc + e, v);
		}
	}
}

// scratch (exact sums) -> gradients, rounded once; the scratch is left zeroed for the next pass
__global__ void __launch_bounds__(256) k_permuto_finalize(const size_t n_params, unsigned long long* __restrict__ scratch, half_t* __restrict__ grad, const int accumulate) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_params) return;
	long long s = (long long)scratch[i];
	if (s != 0) scratch[i] = 0;
	if (accumulate) s += half_to_fixed_fast(grad[i]);
	grad[i] = fixed_to_half_fast(s);
}

// ---------------------------------------------------------------------------------------------------------------- dL/dparams, float
__global__ void __launch_bounds__(256) k_permuto_zero(const size_t n, float* __restrict__ p) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) p[i] = 0.0f;
}

template <int D, int F>
__global__ void __launch_bounds__(256) k_permuto_bwd_f32(const uint32_t n, const uint32_t n_levels, const uint32_t log2_T, const PermutoShape::Scales scales, const MatView x,
                                                         const float* __restrict__ dL_dy, const uint32_t dy_stride, float* __restrict__ grad) {
	constexpr int N = D + 1;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_levels;
	if (i >= n) return;
	const uint32_t level = gid - i * n_levels;
	float xin[D];
	load_coords<D>(x, i, xin);
	PermutoSimplex<D> sx;
	sx.setup(xin, scales.v[level]);
	float* __restrict__ table = grad + (((size_t)level << log2_T) * F);
	const float* __restrict__ dy = dL_dy + (size_t)i * dy_stride + (size_t)level * F;
	const uint32_t mask = (1u << log2_T) - 1u;
	float g[F];
#pragma unroll
	for (int f = 0; f < F; ++f) g[f] = dy[f];
#pragma unroll
	for (int r = 0; r < N; ++r) {
		const size_t e = (size_t)sx.index(r, mask) * F;
#pragma unroll
		for (int f = 0; f < F; ++f) atomicAdd(table + e + f, g[f] * sx.b[r]);
	}
}

// ---------------------------------------------------------------------------------------------------------------- tangent, n_t directions
// k_permuto_fwd's split.  The simplex is set up, the D + 1 indices formed and the D + 1 gathers issued ONCE; the rolled loop over the
// directions keeps the ranks and the gathered vectors in registers and adds, per direction, the elevation of v and O(D^2) selects.
// Direction t is v.data + t * v_next through v's strides; its result goes to the buffer t * t_next bytes behind `out`.
template <typename T, int D, int F>
__global__ void __launch_bounds__(256) k_permuto_tangent(const uint32_t n, const uint32_t n_levels, const uint32_t log2_T, const PermutoShape::Scales scales, const MatView x,
                                                         const MatView v, const uint32_t v_next, const uint32_t n_t, const T* __restrict__ params, T* __restrict__ out,
                                                         const uint32_t out_stride, const size_t t_next, const uint32_t n_slots, const int vector_stores) {
	typedef typename VecOf<T, F>::type vecF;
	constexpr int N = D + 1;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_slots;
	if (i >= n) return;
	const uint32_t level = gid - i * n_slots; // slots behind the levels write the padding: zeros
	const bool live = level < n_levels;
	const float scale = live ? scales.v[level] : 0.0f;
	PermutoSimplex<D> sx;
	vecF val[N];
	if (live) {
		float xin[D];
		load_coords<D>(x, i, xin);
		sx.setup(xin, scale);
		const T* __restrict__ table = params + (((size_t)level << log2_T) * F);
		const uint32_t mask = (1u << log2_T) - 1u;
		uint32_t index[N];
#pragma unroll
		for (int r = 0; r < N; ++r) index[r] = sx.index(r, mask);
#pragma unroll
		for (int r = 0; r < N; ++r) val[r] = *(const vecF*)&table[(size_t)index[r] * F];
	}
	const size_t o_first = (size_t)i * out_stride + (size_t)level * F;
#pragma unroll 1
	for (uint32_t t = 0; t < n_t; ++t) {
		float res[F];
#pragma unroll
		for (int f = 0; f < F; ++f) res[f] = 0.0f;
		if (live) {
			float vin[D], beta[N];
			load_coords<D>(MatView{v.data + (size_t)t * v_next, v.stride_sample, v.stride_dim}, i, vin);
			sx.weight_tangent(vin, scale, beta);
#pragma unroll
			for (int r = 0; r < N; ++r) {
#pragma unroll
				for (int f = 0; f < F; ++f) res[f] = fmaf(beta[r], permuto_elem<T, F>(val[r], f), res[f]);
			}
		}
		T* o = (T*)((char*)out + (size_t)t * t_next) + o_first;
		if (vector_stores) { // (out_stride % F == 0, so level * F + F <= out_stride, and every buffer starts on a multiple of F elements)
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
}

// ---------------------------------------------------------------------------------------------------------------- d<v, J^T dL/dy>/dparams, half
// k_permuto_bwd with beta = weight_tangent(v) in place of b: the same split, accumulators, exact signed sums and k_permuto_finalize.
template <int D, int F>
__global__ void __launch_bounds__(256) k_permuto_bwdbwd(const uint32_t n, const uint32_t log2_T, const PermutoShape::Scales scales, const MatView x, const MatView v,
                                                        const half_t* __restrict__ dL_dy, const uint32_t dy_stride, unsigned long long* __restrict__ scratch, const int in_lds) {
	extern __shared__ __attribute__((aligned(16))) char permuto_smem[];
	typedef __attribute__((address_space(3))) unsigned long long lds_u64;
	typedef typename VecOf<half_t, F>::type vecF;
	constexpr int N = D + 1;
	lds_u64* acc = (lds_u64*)permuto_smem;
	const uint32_t level = blockIdx.y;
	const uint32_t entries = (1u << log2_T) * F, mask = (1u << log2_T) - 1u;
	if (in_lds) {
		for (uint32_t e = threadIdx.x; e < entries; e += blockDim.x) ((unsigned long long*)permuto_smem)[e] = 0ull;
		__syncthreads();
	}
	const float scale = scales.v[level];
	unsigned long long* global_acc = scratch + (((size_t)level << log2_T) * F);
	const uint32_t begin = blockIdx.x * PERMUTO_BWD_SAMPLES, end = min(n, begin + PERMUTO_BWD_SAMPLES);
	for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
		float xin[D], vin[D], beta[N];
		load_coords<D>(x, i, xin);
		load_coords<D>(v, i, vin);
		PermutoSimplex<D> sx;
		sx.setup(xin, scale);
		sx.weight_tangent(vin, scale, beta);
		const half_t* __restrict__ dy = dL_dy + (size_t)i * dy_stride + (size_t)level * F;
		float g[F];
		if (dy_stride % F == 0) {
			const vecF gv = *(const vecF*)dy;
#pragma unroll
			for (int f = 0; f < F; ++f) g[f] = permuto_elem<half_t, F>(gv, f);
		} else {
#pragma unroll
			for (int f = 0; f < F; ++f) g[f] = (float)dy[f];
		}
#pragma unroll
		for (int r = 0; r < N; ++r) {
			const uint32_t e = sx.index(r, mask) * F;
#pragma unroll
			for (int f = 0; f < F; ++f) {
				const unsigned long long c = (unsigned long long)half_to_fixed_fast((half_t)(g[f] * beta[r]));
				if (in_lds) __hip_atomic_fetch_add(acc + e + f, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				else if (c != 0) atomicAdd(global_acc + e + f, c);
			}
		}
	}
	if (in_lds) {
		__syncthreads();
		for (uint32_t e = threadIdx.x; e < entries; e += blockDim.x) {
			const unsigned long long s = ((unsigned long long*)permuto_smem)[e];
			if (s != 0) atomicAdd(global_acc + e, s);
		}
	}
}

// fp32 modules: k_permuto_bwd_f32's split, float atomicAdd of dL/dy_f * beta_r
template <int D, int F>
__global__ void __launch_bounds__(256) k_permuto_bwdbwd_f32(const uint32_t n, const uint32_t n_levels, const uint32_t log2_T, const PermutoShape::Scales scales, const MatView x,
                                                            const MatView v, const float* __restrict__ dL_dy, const uint32_t dy_stride, float* __restrict__ grad) {
	constexpr int N = D + 1;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_levels;
	if (i >= n) return;
	const uint32_t level = gid - i * n_levels;
	const float scale = scales.v[level];
	float xin[D], vin[D], beta[N];
	load_coords<D>(x, i, xin);
	load_coords<D>(v, i, vin);
	PermutoSimplex<D> sx;
	sx.setup(xin, scale);
	sx.weight_tangent(vin, scale, beta);
	float* __restrict__ table = grad + (((size_t)level << log2_T) * F);
	const float* __restrict__ dy = dL_dy + (size_t)i * dy_stride + (size_t)level * F;
	const uint32_t mask = (1u << log2_T) - 1u;
	float g[F];
#pragma unroll
	for (int f = 0; f < F; ++f) g[f] = dy[f];
#pragma unroll
	for (int r = 0; r < N; ++r) {
		const size_t e = (size_t)sx.index(r, mask) * F;
#pragma unroll
		for (int f = 0; f < F; ++f) atomicAdd(table + e + f, g[f] * beta[r]);
	}
}

// ---------------------------------------------------------------------------------------------------------------- launches
uint32_t blocks_for(uint64_t threads) {
	CHECK_THROW(threads < (1ull << 32));
	return (uint32_t)((threads + 255) / 256);
}

template <typename T, int D, int F>
void launch_fwd(hipStream_t s, const PermutoShape& p, uint32_t n, MatView x, const void* params, void* out, uint32_t out_stride) {
	const uint32_t n_slots = div_round_up(out_stride, (uint32_t)F);
	hipLaunchKernelGGL((k_permuto_fwd<T, D, F>), dim3(blocks_for((uint64_t)n * n_slots)), dim3(256), 0, s, n, p.n_levels, p.log2_hashmap_size, p.scales, x, (const T*)params, (T*)out,
	                   out_stride, n_slots);
}

template <typename T, int D, int F>
void launch_bwd_input(hipStream_t s, const PermutoShape& p, uint32_t n, MatView x, const void* params, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	uint32_t W = 1;
	while (W < p.n_levels && W < 64) W *= 2;
	hipLaunchKernelGGL((k_permuto_bwd_input<T, D, F>), dim3(blocks_for((uint64_t)n * W)), dim3(256), 0, s, n, p.n_levels, p.log2_hashmap_size, p.scales, x, (const T*)params,
	                   (const T*)dL_dy, dy_stride, W, dL_dx);
}

template <int D, int F>
void launch_bwd(hipStream_t s, const PermutoShape& p, bool fp32, uint32_t n, MatView x, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad, bool accumulate) {
	const size_t n_params = ((size_t)p.n_levels << p.log2_hashmap_size) * F;
	if (fp32) {
		if (!accumulate) hipLaunchKernelGGL(k_permuto_zero, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (float*)grad);
		if (n > 0) hipLaunchKernelGGL((k_permuto_bwd_f32<D, F>), dim3(blocks_for((uint64_t)n * p.n_levels)), dim3(256), 0, s, n, p.n_levels, p.log2_hashmap_size, p.scales, x,
		                              (const float*)dL_dy, dy_stride, (float*)grad);
		return;
	}
	if (n > 0) {
		const size_t lds_bytes = ((size_t)F << p.log2_hashmap_size) * sizeof(uint64_t);
		const bool in_lds = lds_bytes <= PERMUTO_LDS_BYTES;
		hipLaunchKernelGGL((k_permuto_bwd<D, F>), dim3(div_round_up(n, PERMUTO_BWD_SAMPLES), p.n_levels), dim3(256), in_lds ? (uint32_t)lds_bytes : 0u, s, n, p.log2_hashmap_size,
		                   p.scales, x, (const half_t*)dL_dy, dy_stride, (unsigned long long*)scratch, in_lds ? 1 : 0);
	}
	hipLaunchKernelGGL(k_permuto_finalize, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (unsigned long long*)scratch, (half_t*)grad, accumulate ? 1 : 0);
}

template <typename T, int D, int F>
void launch_tangent(hipStream_t s, const PermutoShape& p, uint32_t n, MatView x, MatView v, uint32_t v_next, uint32_t n_t, const void* params, void* t, uint32_t t_stride, size_t t_next) {
	const uint32_t n_slots = div_round_up(t_stride, (uint32_t)F);
	const bool vector_stores = t_stride % F == 0 && t_next % (F * sizeof(T)) == 0;
	hipLaunchKernelGGL((k_permuto_tangent<T, D, F>), dim3(blocks_for((uint64_t)n * n_slots)), dim3(256), 0, s, n, p.n_levels, p.log2_hashmap_size, p.scales, x, v, v_next, n_t,
	                   (const T*)params, (T*)t, t_stride, t_next, n_slots, vector_stores ? 1 : 0);
}

template <int D, int F>
void launch_bwdbwd(hipStream_t s, const PermutoShape& p, bool fp32, uint32_t n, MatView x, MatView v, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad, bool accumulate) {
	const size_t n_params = ((size_t)p.n_levels << p.log2_hashmap_size) * F;
	if (fp32) {
		if (!accumulate) hipLaunchKernelGGL(k_permuto_zero, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (float*)grad);
		if (n > 0) hipLaunchKernelGGL((k_permuto_bwdbwd_f32<D, F>), dim3(blocks_for((uint64_t)n * p.n_levels)), dim3(256), 0, s, n, p.n_levels, p.log2_hashmap_size, p.scales, x, v,
		                              (const float*)dL_dy, dy_stride, (float*)grad);
		return;
	}
	if (n > 0) {
		const size_t lds_bytes = ((size_t)F << p.log2_hashmap_size) * sizeof(uint64_t);
		const bool in_lds = lds_bytes <= PERMUTO_LDS_BYTES;
		hipLaunchKernelGGL((k_permuto_bwdbwd<D, F>), dim3(div_round_up(n, PERMUTO_BWD_SAMPLES), p.n_levels), dim3(256), in_lds ? (uint32_t)lds_bytes : 0u, s, n, p.log2_hashmap_size,
		                   p.scales, x, v, (const half_t*)dL_dy, dy_stride, (unsigned long long*)scratch, in_lds ? 1 : 0);
	}
	hipLaunchKernelGGL(k_permuto_finalize, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (unsigned long long*)scratch, (half_t*)grad, accumulate ? 1 : 0);
}

// run `body` with the compile-time <D, F> of the shape
#define TCNN_PERMUTO_F(D_, CALL) \
	switch (p.n_features_per_level) { \
		case 1: { constexpr int D = D_, F = 1; CALL; } break; \
		case 2: { constexpr int D = D_, F = 2; CALL; } break; \
		case 4: { constexpr int D = D_, F = 4; CALL; } break; \
		case 8: { constexpr int D = D_, F = 8; CALL; } break; \
		default: throw std::runtime_error{"PermutoGrid: n_features_per_level must be 1, 2, 4 or 8"}; \
	}
#define TCNN_PERMUTO_DISPATCH(CALL) \
	switch (p.n_dims) { \
		case 2: TCNN_PERMUTO_F(2, CALL) break; \
		case 3: TCNN_PERMUTO_F(3, CALL) break; \
		case 4: TCNN_PERMUTO_F(4, CALL) break; \
		case 5: TCNN_PERMUTO_F(5, CALL) break; \
		case 6: TCNN_PERMUTO_F(6, CALL) break; \
		case 7: TCNN_PERMUTO_F(7, CALL) break; \
		default: throw std::runtime_error{"PermutoGrid: n_dims_to_encode must be 2 to 7"}; \
	}

} // namespace

void permuto_forward(hipStream_t stream, const PermutoShape& p, bool fp32, uint32_t n, MatView x, const void* params, void* out, uint32_t out_stride) {
	if (n == 0 || out_stride == 0) return;
	CHECK_THROW(out_stride >= p.n_levels * p.n_features_per_level);
	if (fp32) { TCNN_PERMUTO_DISPATCH((launch_fwd<float, D, F>(stream, p, n, x, params, out, out_stride))) }
	else { TCNN_PERMUTO_DISPATCH((launch_fwd<half_t, D, F>(stream, p, n, x, params, out, out_stride))) }
	HIP_CHECK_THROW(hipGetLastError());
}

void permuto_backward_input(hipStream_t stream, const PermutoShape& p, bool fp32, uint32_t n, MatView x, const void* params, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	if (n == 0) return;
	if (fp32) { TCNN_PERMUTO_DISPATCH((launch_bwd_input<float, D, F>(stream, p, n, x, params, dL_dy, dy_stride, dL_dx))) }
	else { TCNN_PERMUTO_DISPATCH((launch_bwd_input<half_t, D, F>(stream, p, n, x, params, dL_dy, dy_stride, dL_dx))) }
	HIP_CHECK_THROW(hipGetLastError());
}

void permuto_backward(hipStream_t stream, const PermutoShape& p, bool fp32, uint32_t n, MatView x, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad, bool accumulate) {
	TCNN_PERMUTO_DISPATCH((launch_bwd<D, F>(stream, p, fp32, n, x, dL_dy, dy_stride, scratch, grad, accumulate)))
	HIP_CHECK_THROW(hipGetLastError());
}

void permuto_tangent(hipStream_t stream, const PermutoShape& p, bool fp32, uint32_t n, MatView x, MatView v, uint32_t v_next, uint32_t n_tangents, const void* params, void* t,
                     uint32_t t_stride, size_t t_next) {
	if (n == 0 || t_stride == 0 || n_tangents == 0) return;
	CHECK_THROW(t_stride >= p.n_levels * p.n_features_per_level && t_next % (fp32 ? 4 : 2) == 0);
	if (fp32) { TCNN_PERMUTO_DISPATCH((launch_tangent<float, D, F>(stream, p, n, x, v, v_next, n_tangents, params, t, t_stride, t_next))) }
	else { TCNN_PERMUTO_DISPATCH((launch_tangent<half_t, D, F>(stream, p, n, x, v, v_next, n_tangents, params, t, t_stride, t_next))) }
	HIP_CHECK_THROW(hipGetLastError());
}

void permuto_backward_backward(hipStream_t stream, const PermutoShape& p, bool fp32, uint32_t n, MatView x, MatView v, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch,
                               void* grad, bool accumulate) {
	TCNN_PERMUTO_DISPATCH((launch_bwdbwd<D, F>(stream, p, fp32, n, x, v, dL_dy, dy_stride, scratch, grad, accumulate)))
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace tcnn_amd
