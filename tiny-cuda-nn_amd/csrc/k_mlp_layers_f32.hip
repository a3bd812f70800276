// k_mlp_layers_f32.hip -- the layer-by-layer MLP path in full precision: the network of the reference's build without
// TCNN_HALF_PRECISION (common.h:99-123: network_precision_t = float, CutlassMLP<float>), here a choice per module
// (Network{json, Precision::Fp32}).  The fp32 form of k_mlp_layers.hip: one GEMM launch per layer, activations and gradients are
// row-major float matrices [n][width], the weights are read from the fp32 parameter vector as they are (no half copy, no
// fragment images).
//
// Numerical contract (tests/test_fp32_network.py holds it, bit for bit against std::fmaf on the CPU):
//   * every output element of a layer product is ONE fp32 accumulator that starts at +0;
//   * it receives the products in ascending k, one fmaf each: acc = fmaf(a[k], b[k], acc), k = 0, 1, ..., K - 1
//     (v_mfma_f32_16x16x4_f32 is exactly that chain over its four k, lane group l >> 4 holding k = l >> 4);
//   * no split-K, no second accumulator summed in at the end; K steps past the matrix are not multiplied at all;
//   * latency is hidden across a wave's 16 output tiles (16 independent chains per k step), never within one element's chain.
// The epilogues work in fp32 with no rounding other than fp32's own (-ffp-contract=off: a product and a sum are two roundings):
//   forward        Y[s][r] = a(z), z = sum_c X[s][c] W[r][c]; z is stored as well where asked for (Sine, layers with curvature)
//   backward data  G[s][c] = a'(.) sum_r D[s][r] Wt[c][r], a' from the stored output (activation_bwd), from the pre-activation for Sine
//   second order   the three products of second_order_epilogue (k_mlp_layers.hip) with float in place of half_t
//
// k_layer_gemm_f32 keeps the half kernel's tiling -- 256 threads, a workgroup tile of BO outputs x BS samples (64 x 256 for layers of
// at most 64 outputs, else 128 x 128), K staged through LDS 32 deep with 16-byte loads, the next stage's loads in flight in
// registers while this one is multiplied, two barriers per stage -- so the shapes that cross a boundary are the same.  An LDS row
// is 32 + 4 floats: the 16 rows a 16x16x4 operand read touches start 36 floats apart, which are 16 different multiples of 4 banks,
// and the four k of a lane group fill the banks between them: one conflict-free 4-byte read per operand and k step.
//
// Weight gradients dW[r][c] = sum_s D[s][r] X[s][c] (k_wgrad_f32): panels of at most 128 x 128; a workgroup multiplies chunks of
// 32 samples (chunk b, b + grid, ... in ascending order) into an fp32 slab of its own and k_wgrad_reduce_f32 adds the slabs in
// ascending order: no atomics, the same inputs give the same bits; Overwrite stores the sum, Accumulate adds it to what is there.
#include "mlp_device.h"

namespace tcnn_amd {
namespace {

constexpr uint32_t LF_BK = 32;          // K per staged step (eight 16x16x4 k-steps)
constexpr uint32_t LF_LDK = LF_BK + 4;  // floats per LDS row

struct LayerGemmArgsF32 {
	const float* x;   // [n][ldx], columns 0..k-1 read
	const float* w;   // [rows][k]
	float* y;         // [n][ldy], columns 0..rows-1 written
	float* pre;       // as LayerGemmArgs::pre
	const float* aux; // as LayerGemmArgs::aux
	uint32_t n, ldx, k, rows, ldy, act, mode;
	const float* aux2; // as LayerGemmArgs::aux2
};

__device__ inline f4 mfma_f32(const float a, const float b, const f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// second_order_epilogue of k_mlp_layers.hip on floats
__device__ inline f4 second_order_epilogue_f32(const LayerGemmArgsF32& a, const size_t at, const f4 acc) {
	f4 x = f4{0, 0, 0, 0}, v;
	f4 d1 = f4{1, 1, 1, 1};
	if (a.act != (uint32_t)Activation::None) {
		x = *(const f4*)(a.aux + at);
		for (int r = 0; r < 4; ++r) d1[r] = act_d1(a.act, x[r]);
	}
	if (a.mode == LG_TANGENT) {
		if (a.pre) {
			const f4 g = *(const f4*)(a.aux2 + at);
			f4 c;
			for (int r = 0; r < 4; ++r) c[r] = act_d2(a.act, x[r]) * g[r] * acc[r];
			*(f4*)(a.pre + at) = c;
		}
		for (int r = 0; r < 4; ++r) v[r] = d1[r] * acc[r];
	} else if (a.mode == LG_BWD_KEEP) {
		if (a.pre) *(f4*)(a.pre + at) = acc;
		for (int r = 0; r < 4; ++r) v[r] = d1[r] * acc[r];
	} else { // LG_CURVATURE
		f4 c = f4{0, 0, 0, 0};
		if (a.aux2) c = *(const f4*)(a.aux2 + at);
		for (int r = 0; r < 4; ++r) v[r] = c[r] + d1[r] * acc[r];
	}
	return v;
}

// WO x WS waves, each TO x TS tiles of 16 outputs x 16 samples
template <int WO, int WS, int TO, int TS, bool SECOND = false>
__global__ void __launch_bounds__(256) k_layer_gemm_f32(const LayerGemmArgsF32 a) {
	static_assert(WO * WS == 4, "four waves");
	constexpr uint32_t BO = WO * TO * 16, BS = WS * TS * 16;
	constexpr uint32_t PW = BO * (LF_BK / 4) / 256, PX = BS * (LF_BK / 4) / 256; // 16-byte pieces per thread
	static_assert(PW * 256 == BO * (LF_BK / 4) && PX * 256 == BS * (LF_BK / 4), "whole pieces per thread");
	__shared__ __attribute__((aligned(16))) float Ws[BO * LF_LDK];
	__shared__ __attribute__((aligned(16))) float Xs[BS * LF_LDK];

	const uint32_t n_ob = (a.rows + BO - 1) / BO;
	const uint32_t ob = blockIdx.x % n_ob, sb = blockIdx.x / n_ob; // consecutive workgroups share the sample rows (L2)
	const uint32_t o0 = ob * BO;
	const size_t s0 = (size_t)sb * BS;
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t wo = wave % WO, ws = wave / WO;
	const uint32_t o_wave = o0 + wo * TO * 16;

	f4 wv[PW], xv[PX];
	const f4 zero = f4{0, 0, 0, 0};
	auto fetch = [&](const uint32_t k0) {
#pragma unroll
		for (uint32_t i = 0; i < PW; ++i) {
			const uint32_t p = tid + i * 256, row = p >> 3, k = k0 + (p & 7) * 4, o = o0 + row;
			wv[i] = (o < a.rows && k < a.k) ? *(const f4*)(a.w + (size_t)o * a.k + k) : zero; // rows past the matrix, k past its columns: zeros
		}
#pragma unroll
		for (uint32_t i = 0; i < PX; ++i) {
			const uint32_t p = tid + i * 256, row = p >> 3, k = k0 + (p & 7) * 4;
			xv[i] = k < a.k ? *(const f4*)(a.x + (s0 + row) * a.ldx + k) : zero; // (n is a multiple of BS: every sample row exists)
		}
	};

	f4 acc[TO][TS];
#pragma unroll
	for (int i = 0; i < TO; ++i)
#pragma unroll
		for (int j = 0; j < TS; ++j) acc[i][j] = f4{0, 0, 0, 0};

	fetch(0);
	for (uint32_t k0 = 0; k0 < a.k; k0 += LF_BK) {
#pragma unroll
		for (uint32_t i = 0; i < PW; ++i) {
			const uint32_t p = tid + i * 256;
			*(f4*)(Ws + (p >> 3) * LF_LDK + (p & 7) * 4) = wv[i];
		}
#pragma unroll
		for (uint32_t i = 0; i < PX; ++i) {
			const uint32_t p = tid + i * 256;
			*(f4*)(Xs + (p >> 3) * LF_LDK + (p & 7) * 4) = xv[i];
		}
		__syncthreads();
		if (k0 + LF_BK < a.k) fetch(k0 + LF_BK); // in flight while this step is multiplied
		const uint32_t k_steps = min(LF_BK, a.k - k0) / 4; // (k is a multiple of 16: whole steps; those past the matrix are not multiplied)
		// 16x16x4 operands: lane l holds row (l & 15), k = 4 kk + (l >> 4) of its tile; ascending kk = ascending k in every chain
#pragma unroll
		for (uint32_t kk = 0; kk < LF_BK / 4; ++kk) {
			if (kk >= k_steps) break;
			float af[TO], bf[TS];
#pragma unroll
			for (int i = 0; i < TO; ++i) af[i] = Ws[(wo * TO * 16 + i * 16 + (lane & 15)) * LF_LDK + 4 * kk + (lane >> 4)];
#pragma unroll
			for (int j = 0; j < TS; ++j) bf[j] = Xs[(ws * TS * 16 + j * 16 + (lane & 15)) * LF_LDK + 4 * kk + (lane >> 4)];
#pragma unroll
			for (int i = 0; i < TO; ++i) {
				if (o_wave + i * 16 >= a.rows) continue; // wave-uniform: output tiles past the matrix are not computed
#pragma unroll
				for (int j = 0; j < TS; ++j) acc[i][j] = mfma_f32(af[i], bf[j], acc[i][j]);
			}
		}
		__syncthreads();
	}

	// D[row = output 4 (l >> 4) + r][col = sample l & 15]: 4 consecutive outputs of one sample, one 16-byte store
#pragma unroll
	for (int i = 0; i < TO; ++i) {
		const uint32_t o = o_wave + i * 16 + 4 * (lane >> 4);
		if (o_wave + i * 16 >= a.rows) continue;
#pragma unroll
		for (int j = 0; j < TS; ++j) {
			const size_t at = (s0 + ws * TS * 16 + j * 16 + (lane & 15)) * a.ldy + o;
			if constexpr (SECOND) {
				*(f4*)(a.y + at) = second_order_epilogue_f32(a, at, acc[i][j]);
			} else {
				f4 v = acc[i][j];
				if (a.mode == LG_FWD) {
					if (a.pre) *(f4*)(a.pre + at) = v;
#pragma unroll
					for (int r = 0; r < 4; ++r) v[r] = activation_fwd(a.act, v[r]);
				} else if (a.act != (uint32_t)Activation::None) {
					const f4 f = *(const f4*)(a.aux + at);
					if (a.act == (uint32_t)Activation::Sine) { // from the stored pre-activation, as in the half kernel
#pragma unroll
						for (int r = 0; r < 4; ++r) v[r] = v[r] * cosf(f[r]);
					} else {
#pragma unroll
						for (int r = 0; r < 4; ++r) v[r] = activation_bwd(a.act, v[r], f[r]);
					}
				}
				*(f4*)(a.y + at) = v;
			}
		}
	}
}

__global__ void __launch_bounds__(256) k_layer_delta_f32(const uint32_t n_elems, const uint32_t act, const float* __restrict__ g, const float* __restrict__ aux, float* __restrict__ delta) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elems) return;
	delta[i] = act_d1(act, aux[i]) * g[i];
}

__global__ void __launch_bounds__(256) k_layer_transpose_f32(const uint32_t rows, const uint32_t cols, const float* __restrict__ w, float* __restrict__ wt) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x; // wt element (c, r) = i: c = i / rows
	if (i >= rows * cols) return;
	const uint32_t c = i / rows, r = i - c * rows;
	wt[i] = w[(size_t)r * cols + c];
}

__global__ void __launch_bounds__(256) k_act_bwd_output_f32(const uint32_t n_elems, const uint32_t act, const float* __restrict__ dL_dout, const float* __restrict__ out, float* __restrict__ result) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elems) return;
	result[i] = activation_bwd(act, dL_dout[i], out[i]);
}

// ---- weight gradients
constexpr uint32_t WF_CHUNK = 32;      // samples per staged chunk
constexpr uint32_t WF_MAX = 128;       // a panel is at most WF_MAX x WF_MAX
constexpr uint32_t WF_MAX_SLABS = 256; // workgroups (= slabs) per panel
constexpr uint32_t WF_MAX_JOBS = 16;   // panels per launch
// floats per LDS row of a chunk: = 16 modulo 64, so that the four sample rows of a 16x16x4 operand read fall into four different groups of 16 banks
__host__ __device__ inline uint32_t wf_pitch(const uint32_t width) { return width + ((80u - (width & 63u)) & 63u); }
constexpr uint32_t WF_MAX_PITCH = 144; // wf_pitch(128), the largest for widths up to WF_MAX

struct WgradJobF32 {
	const float* dO; // [n][ldo], the panel's `rows` columns
	const float* In; // [n][ldi], the panel's `cols` columns
	float* slabs;    // [grid][rows][cols]
	float* grad;     // [rows][ldg]
	uint32_t ldo, ldi, ldg, rows, cols;
};
struct WgradJobsF32 { WgradJobF32 job[WF_MAX_JOBS]; };

// blockIdx.y: the panel; blockIdx.x: the slab.  A wave owns tiles wave, wave + 4, ... of the panel's (rows / 16) x (cols / 16) tiles.
__global__ void __launch_bounds__(256) k_wgrad_f32(const uint32_t n, const WgradJobsF32 jobs) {
	__shared__ __attribute__((aligned(16))) float P[WF_CHUNK * WF_MAX_PITCH];
	__shared__ __attribute__((aligned(16))) float Q[WF_CHUNK * WF_MAX_PITCH];
	const float* __restrict__ dO = jobs.job[blockIdx.y].dO;
	const float* __restrict__ In = jobs.job[blockIdx.y].In;
	const uint32_t ldo = jobs.job[blockIdx.y].ldo, ldi = jobs.job[blockIdx.y].ldi;
	const uint32_t rows = jobs.job[blockIdx.y].rows, cols = jobs.job[blockIdx.y].cols;
	const uint32_t rp = wf_pitch(rows), cp = wf_pitch(cols);
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t q = lane >> 4, li = lane & 15;
	const uint32_t tc = cols / 16, n_tiles = (rows / 16) * tc;
	constexpr int TILES = (WF_MAX / 16) * (WF_MAX / 16) / 4; // per wave

	// where this thread's 16-byte pieces of a chunk come from and go to (at most 4 per operand; rows, cols <= WF_MAX)
	const uint32_t pr = rows / 4, pc = cols / 4; // pieces per sample row
	uint32_t p_src[4], p_dst[4], q_src[4], q_dst[4];
#pragma unroll
	for (uint32_t i = 0; i < 4; ++i) {
		const uint32_t p = tid + i * 256;
		const uint32_t sp = p / pr, cpp = (p - sp * pr) * 4, sq = p / pc, cq = (p - sq * pc) * 4;
		p_src[i] = sp * ldo + cpp, p_dst[i] = sp * rp + cpp;
		q_src[i] = sq * ldi + cq, q_dst[i] = sq * cp + cq;
	}
	const uint32_t n_p = WF_CHUNK * pr, n_q = WF_CHUNK * pc;
	f4 pv[4], qv[4];
	auto fetch = [&](const uint32_t ch) {
		const float* d = dO + (size_t)ch * WF_CHUNK * ldo;
		const float* x = In + (size_t)ch * WF_CHUNK * ldi;
#pragma unroll
		for (uint32_t i = 0; i < 4; ++i) {
			if (tid + i * 256 < n_p) pv[i] = *(const f4*)(d + p_src[i]);
			if (tid + i * 256 < n_q) qv[i] = *(const f4*)(x + q_src[i]);
		}
	};

	uint32_t tile_at[TILES]; // 16 ti | 16 tj << 16
	f4 acc[TILES];
#pragma unroll
	for (int u = 0; u < TILES; ++u) {
		const uint32_t t = wave + 4 * u, ti = t / tc, tj = t - ti * tc;
		tile_at[u] = (16 * ti) | ((16 * tj) << 16);
		acc[u] = f4{0, 0, 0, 0};
	}

	const uint32_t n_chunks = n / WF_CHUNK;
	if (blockIdx.x < n_chunks) fetch(blockIdx.x);
	for (uint32_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
#pragma unroll
		for (uint32_t i = 0; i < 4; ++i) {
			if (tid + i * 256 < n_p) *(f4*)(P + p_dst[i]) = pv[i];
			if (tid + i * 256 < n_q) *(f4*)(Q + q_dst[i]) = qv[i];
		}
		__syncthreads();
		if (ch + gridDim.x < n_chunks) fetch(ch + gridDim.x); // in flight while this chunk is multiplied
		// A[row = l & 15][k = l >> 4] = dO[sample 4 kk + (l >> 4)][16 ti + (l & 15)], B[k][col] = In[the same sample][16 tj + (l & 15)]
#pragma unroll 2
		for (uint32_t kk = 0; kk < WF_CHUNK / 4; ++kk) {
			const uint32_t s = 4 * kk + q;
#pragma unroll
			for (int u = 0; u < TILES; ++u) {
				if (wave + 4 * u >= n_tiles) continue; // wave-uniform
				acc[u] = mfma_f32(P[s * rp + (tile_at[u] & 0xffffu) + li], Q[s * cp + (tile_at[u] >> 16) + li], acc[u]);
			}
		}
		__syncthreads();
	}
	// D[row = 4 (l >> 4) + r][col = l & 15] of tile (ti, tj)
	float* slab = jobs.job[blockIdx.y].slabs + (size_t)blockIdx.x * rows * cols;
#pragma unroll
	for (int u = 0; u < TILES; ++u) {
		if (wave + 4 * u >= n_tiles) continue;
#pragma unroll
		for (int r = 0; r < 4; ++r) slab[(size_t)((tile_at[u] & 0xffffu) + 4 * q + r) * cols + (tile_at[u] >> 16) + li] = acc[u][r];
	}
}

// grad (=|+=) slab 0 + slab 1 + ..., added in that order
__global__ void __launch_bounds__(256) k_wgrad_reduce_f32(const uint32_t n_slabs, const WgradJobsF32 jobs, const int accumulate) {
	const uint32_t rows = jobs.job[blockIdx.y].rows, cols = jobs.job[blockIdx.y].cols, ldg = jobs.job[blockIdx.y].ldg;
	const uint32_t n_elems = rows * cols;
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elems) return;
	const float* __restrict__ slabs = jobs.job[blockIdx.y].slabs + i;
	float sum = slabs[0];
	for (uint32_t k = 1; k < n_slabs; ++k) sum += slabs[(size_t)k * n_elems];
	const uint32_t r = i / cols, c = i - r * cols;
	float* g = jobs.job[blockIdx.y].grad + (size_t)r * ldg + c;
	*g = accumulate ? *g + sum : sum;
}

inline uint32_t wgrad_grid_f32(const uint32_t n) { return std::max(1u, std::min(n / WF_CHUNK, WF_MAX_SLABS)); }

template <bool SECOND>
void launch_layer_gemm_f32(hipStream_t stream, const LayerGemmArgsF32& a) {
	CHECK_THROW(a.n % BATCH_SIZE_GRANULARITY == 0);
	CHECK_THROW(a.rows % 16 == 0 && a.k % 16 == 0 && a.rows > 0 && a.k > 0);
	CHECK_THROW(a.ldx % 4 == 0 && a.ldx >= a.k && a.ldy % 4 == 0 && a.ldy >= a.rows);
	if (a.n == 0) return;
	if (a.rows <= 64) { // narrow layers (the padded output layer): 64 outputs x 256 samples per workgroup
		const uint32_t blocks = (a.n / 256) * div_round_up(a.rows, 64);
		hipLaunchKernelGGL((k_layer_gemm_f32<1, 4, 4, 4, SECOND>), dim3(blocks), dim3(256), 0, stream, a);
	} else {            // 128 outputs x 128 samples, waves 2 x 2 of 64 x 64
		const uint32_t blocks = (a.n / 128) * div_round_up(a.rows, 128);
		hipLaunchKernelGGL((k_layer_gemm_f32<2, 2, 4, 4, SECOND>), dim3(blocks), dim3(256), 0, stream, a);
	}
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace

void mlp_layer_forward_f32(hipStream_t stream, uint32_t n, const float* x, uint32_t ldx, const float* w, uint32_t rows, uint32_t cols, uint32_t activation, float* y, uint32_t ldy, float* pre) {
	LayerGemmArgsF32 a{x, w, y, pre, nullptr, n, ldx, cols, rows, ldy, activation, LG_FWD, nullptr};
	launch_layer_gemm_f32<false>(stream, a);
}

void mlp_layer_backward_f32(hipStream_t stream, uint32_t n, const float* dL_dout, uint32_t ldo, const float* wt, uint32_t rows, uint32_t cols, uint32_t activation, const float* aux,
                            float* dL_din, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	LayerGemmArgsF32 a{dL_dout, wt, dL_din, nullptr, aux, n, ldo, rows, cols, ldi, activation, LG_BWD, nullptr};
	launch_layer_gemm_f32<false>(stream, a);
}

void mlp_layer_tangent_f32(hipStream_t stream, uint32_t n, const float* u_in, uint32_t ldu, const float* w, uint32_t rows, uint32_t cols, uint32_t activation, const float* aux,
                           const float* g, float* u_out, float* r_out, uint32_t ldy) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	CHECK_THROW(!r_out || (g && aux));
	LayerGemmArgsF32 a{u_in, w, u_out, r_out, aux, n, ldu, cols, rows, ldy, activation, LG_TANGENT, g};
	launch_layer_gemm_f32<true>(stream, a);
}

void mlp_layer_backward_keep_f32(hipStream_t stream, uint32_t n, const float* d_out, uint32_t ldo, const float* wt, uint32_t rows, uint32_t cols, uint32_t activation, const float* aux,
                                 float* g_in, float* d_in, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	LayerGemmArgsF32 a{d_out, wt, d_in, g_in, aux, n, ldo, rows, cols, ldi, activation, LG_BWD_KEEP, nullptr};
	launch_layer_gemm_f32<true>(stream, a);
}

void mlp_layer_curvature_backward_f32(hipStream_t stream, uint32_t n, const float* p_out, uint32_t ldo, const float* wt, uint32_t rows, uint32_t cols, uint32_t activation,
                                      const float* aux, const float* r_in, float* p_in, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	LayerGemmArgsF32 a{p_out, wt, p_in, nullptr, aux, n, ldo, rows, cols, ldi, activation, LG_CURVATURE, r_in};
	launch_layer_gemm_f32<true>(stream, a);
}

void mlp_layer_delta_f32(hipStream_t stream, size_t n_elems, uint32_t activation, const float* g, const float* aux, float* delta) {
	if (n_elems == 0) return;
	CHECK_THROW(n_elems < (1ull << 32));
	hipLaunchKernelGGL(k_layer_delta_f32, dim3(div_round_up((uint32_t)n_elems, 256u)), dim3(256), 0, stream, (uint32_t)n_elems, activation, g, aux, delta);
	HIP_CHECK_THROW(hipGetLastError());
}

void mlp_layer_transpose_f32(hipStream_t stream, uint32_t rows, uint32_t cols, const float* w, float* wt) {
	const uint32_t total = rows * cols;
	if (total == 0) return;
	hipLaunchKernelGGL(k_layer_transpose_f32, dim3(div_round_up(total, 256)), dim3(256), 0, stream, rows, cols, w, wt);
	HIP_CHECK_THROW(hipGetLastError());
}

void mlp_activation_backward_output_f32(hipStream_t stream, size_t n_elems, uint32_t activation, const float* dL_dout, const float* out, float* result) {
	if (n_elems == 0) return;
	CHECK_THROW(n_elems < (1ull << 32));
	hipLaunchKernelGGL(k_act_bwd_output_f32, dim3(div_round_up((uint32_t)n_elems, 256u)), dim3(256), 0, stream, (uint32_t)n_elems, activation, dL_dout, out, result);
	HIP_CHECK_THROW(hipGetLastError());
}

size_t wgrad_panels_workspace_floats_f32(const WgradPanel* panels, uint32_t count, uint32_t n) {
	size_t total = 0;
	for (uint32_t i = 0; i < count; ++i) total += (size_t)wgrad_grid_f32(n) * panels[i].rows * panels[i].cols;
	return total;
}

void mlp_wgrad_panels_f32(hipStream_t stream, uint32_t n, const WgradPanel* panels, uint32_t count, bool accumulate, float* workspace) {
	CHECK_THROW(n % WF_CHUNK == 0);
	if (n == 0) return;
	const uint32_t grid = wgrad_grid_f32(n);
	size_t at = 0;
	for (uint32_t i = 0; i < count; i += WF_MAX_JOBS) {
		WgradJobsF32 jobs{};
		const uint32_t n_jobs = std::min(WF_MAX_JOBS, count - i);
		uint32_t max_elems = 0;
		for (uint32_t j = 0; j < n_jobs; ++j) {
			const WgradPanel& p = panels[i + j];
			CHECK_THROW(p.rows % 16 == 0 && p.cols % 16 == 0 && p.rows > 0 && p.cols > 0 && p.rows <= WF_MAX && p.cols <= WF_MAX);
			CHECK_THROW(p.ldo % 4 == 0 && p.ldi % 4 == 0 && !p.dO_tiled && !p.In_tiled);
			jobs.job[j] = WgradJobF32{(const float*)p.dO, (const float*)p.In, workspace + at, (float*)p.grad, p.ldo, p.ldi, p.ldg, p.rows, p.cols};
			at += (size_t)grid * p.rows * p.cols;
			max_elems = std::max(max_elems, p.rows * p.cols);
		}
		hipLaunchKernelGGL(k_wgrad_f32, dim3(grid, n_jobs), dim3(256), 0, stream, n, jobs);
		hipLaunchKernelGGL(k_wgrad_reduce_f32, dim3(div_round_up(max_elems, 256u), n_jobs), dim3(256), 0, stream, grid, jobs, accumulate ? 1 : 0);
		HIP_CHECK_THROW(hipGetLastError());
	}
}

} // namespace tcnn_amd
