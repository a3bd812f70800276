// k_mlp_layers.hip -- the layer-by-layer MLP path (cutlass_mlp.cu:39-300 of the reference): one GEMM launch per layer, activations
// round-trip through memory as row-major half matrices [n][width] (sample-major, the layout of the network's input and output).
//
// It serves the CutlassMLP shapes the fused kernels (k_mlp.hip, k_train*.hip) are not specialised for -- any width that is a multiple
// of 16 up to 1024, zero hidden layers, Sine -- and, under TCNN_AMD_MLP_LAYERWISE=1, every other shape (A/B runs).
//
// Both products are NT GEMMs (k contiguous in both operands):
//   forward        Y[s][r]  = act((half) sum_c X[s][c] W[r][c])
//   backward data  G[s][c]  = act'((half) sum_r D[s][r] Wt[c][r]),   Wt = W^T, transposed once per backward pass (k_layer_transpose)
// k_layer_gemm: 256 threads, a workgroup tile of BO outputs x BS samples, K staged through LDS 32 deep with 16-byte loads (the next
// K step's loads in flight in registers while this one is multiplied; two barriers per step), v_mfma_f32_16x16x32_f16 with fp32
// accumulation.  A = the weight tile (outputs on the rows), B = the activation tile (samples on the columns), so a lane ends up with
// 4 consecutive outputs of one sample: one 8-byte store per tile.  The epilogue rounds to half and then applies the activation, the
// rounding convention of the fused kernels and of the oracle.  No atomics: the same inputs give the same bits.
//
// The second-order pass (Network::second_order_*, model.h) runs three more products of the same shape through the same main loop
// (k_layer_gemm<..., SECOND = true>), with derivatives a', a'' evaluated in fp32 from a stored half matrix `aux` -- the layer's
// pre-activation z, or its output for None / ReLU / LeakyReLU (same sign) -- and one rounding to half per stored matrix:
//   tangent         U[s][r] = a'(z) acc,  R[s][r] = a''(z) G[s][r] acc          acc = sum_c Uin[s][c] W[r][c]   (z' = acc is never stored)
//   backward, keep  G[s][c] = (half) acc,  D[s][c] = a'(z) G[s][c]              acc = sum_r Din[s][r] Wt[c][r]  (G before the derivative, D after)
//   curvature       P[s][c] = R[s][c] + a'(z) acc                               acc = sum_r Pin[s][r] Wt[c][r]  (P may overwrite R)
#include "mlp_device.h"

namespace tcnn_amd {
namespace {

constexpr uint32_t LG_BK = 32;          // K per staged step (one 16x16x32 k-step)
constexpr uint32_t LG_LDK = LG_BK + 8;  // halfs per LDS row: 16 bytes of padding break the power-of-two row stride

struct LayerGemmArgs {
	const half_t* x;   // [n][ldx], columns 0..k-1 read
	const half_t* w;   // [rows][k]
	half_t* y;         // [n][ldy], columns 0..rows-1 written
	half_t* pre;       // forward, optional: the half pre-activation, [n][ldy]
	const half_t* aux; // backward: forward output (or the pre-activation for Sine) of the layer whose input gradient y is, [n][ldy]
	uint32_t n, ldx, k, rows, ldy, act, mode;
	// second-order modes: aux = what a', a'' are taken from (act_d1); aux2 = G (tangent) or R (curvature), optional; pre = R (tangent)
	// or G (backward, keep), optional; all [n][ldy]
	const half_t* aux2;
};

// the second-order epilogues on one 4-output piece of the accumulator (what y gets is returned; R or G go to a.pre on the way)
__device__ inline h4 second_order_epilogue(const LayerGemmArgs& a, const size_t at, const f4 acc) {
	h4 x = h4{0, 0, 0, 0}, v;
	f4 d1 = f4{1, 1, 1, 1};
	if (a.act != (uint32_t)Activation::None) {
		x = *(const h4*)(a.aux + at);
		for (int r = 0; r < 4; ++r) d1[r] = act_d1(a.act, (float)x[r]);
	}
	if (a.mode == LG_TANGENT) {
		if (a.pre) {
			const h4 g = *(const h4*)(a.aux2 + at);
			h4 c;
			for (int r = 0; r < 4; ++r) c[r] = (half_t)(act_d2(a.act, (float)x[r]) * (float)g[r] * acc[r]);
			*(h4*)(a.pre + at) = c;
		}
		for (int r = 0; r < 4; ++r) v[r] = (half_t)(d1[r] * acc[r]);
	} else if (a.mode == LG_BWD_KEEP) {
		for (int r = 0; r < 4; ++r) v[r] = (half_t)acc[r];
		if (a.pre) *(h4*)(a.pre + at) = v;
		for (int r = 0; r < 4; ++r) v[r] = (half_t)(d1[r] * (float)v[r]);
	} else { // LG_CURVATURE
		h4 c = h4{0, 0, 0, 0};
		if (a.aux2) c = *(const h4*)(a.aux2 + at);
		for (int r = 0; r < 4; ++r) v[r] = (half_t)((float)c[r] + d1[r] * acc[r]);
	}
	return v;
}

// WO x WS waves, each TO x TS tiles of 16 outputs x 16 samples
template <int WO, int WS, int TO, int TS, bool SECOND = false>
__global__ void __launch_bounds__(256) k_layer_gemm(const LayerGemmArgs a) {
	static_assert(WO * WS == 4, "four waves");
	constexpr uint32_t BO = WO * TO * 16, BS = WS * TS * 16;
	constexpr uint32_t PW = BO * (LG_BK / 8) / 256, PX = BS * (LG_BK / 8) / 256; // 16-byte pieces per thread
	static_assert(PW * 256 == BO * (LG_BK / 8) && PX * 256 == BS * (LG_BK / 8), "whole pieces per thread");
	__shared__ __attribute__((aligned(16))) half_t Ws[BO * LG_LDK];
	__shared__ __attribute__((aligned(16))) half_t Xs[BS * LG_LDK];

	const uint32_t n_ob = (a.rows + BO - 1) / BO;
	const uint32_t ob = blockIdx.x % n_ob, sb = blockIdx.x / n_ob; // consecutive workgroups share the sample rows (L2)
	const uint32_t o0 = ob * BO;
	const size_t s0 = (size_t)sb * BS;
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t wo = wave % WO, ws = wave / WO;
	const uint32_t o_wave = o0 + wo * TO * 16;

	h8 wv[PW], xv[PX];
	const h8 zero = h8{0, 0, 0, 0, 0, 0, 0, 0};
	auto fetch = [&](const uint32_t k0) {
#pragma unroll
		for (uint32_t i = 0; i < PW; ++i) {
			const uint32_t p = tid + i * 256, row = p >> 2, k = k0 + (p & 3) * 8, o = o0 + row;
			wv[i] = (o < a.rows && k < a.k) ? *(const h8*)(a.w + (size_t)o * a.k + k) : zero; // rows past the matrix, k past its columns: zeros
		}
#pragma unroll
		for (uint32_t i = 0; i < PX; ++i) {
			const uint32_t p = tid + i * 256, row = p >> 2, k = k0 + (p & 3) * 8;
			xv[i] = k < a.k ? *(const h8*)(a.x + (s0 + row) * a.ldx + k) : zero; // (n is a multiple of BS: every sample row exists)
		}
	};

	f4 acc[TO][TS];
#pragma unroll
	for (int i = 0; i < TO; ++i)
#pragma unroll
		for (int j = 0; j < TS; ++j) acc[i][j] = f4{0, 0, 0, 0};

	fetch(0);
	for (uint32_t k0 = 0; k0 < a.k; k0 += LG_BK) {
#pragma unroll
		for (uint32_t i = 0; i < PW; ++i) {
			const uint32_t p = tid + i * 256;
			*(h8*)(Ws + (p >> 2) * LG_LDK + (p & 3) * 8) = wv[i];
		}
#pragma unroll
		for (uint32_t i = 0; i < PX; ++i) {
			const uint32_t p = tid + i * 256;
			*(h8*)(Xs + (p >> 2) * LG_LDK + (p & 3) * 8) = xv[i];
		}
		__syncthreads();
		if (k0 + LG_BK < a.k) fetch(k0 + LG_BK); // in flight while this step is multiplied
		// 16x16x32 operands: lane l holds row (l & 15), k = 8 (l >> 4) .. + 7 of its tile -- one 16-byte LDS read each
		h8 af[TO], bf[TS];
#pragma unroll
		for (int i = 0; i < TO; ++i) af[i] = *(const h8*)(Ws + (wo * TO * 16 + i * 16 + (lane & 15)) * LG_LDK + 8 * (lane >> 4));
#pragma unroll
		for (int j = 0; j < TS; ++j) bf[j] = *(const h8*)(Xs + (ws * TS * 16 + j * 16 + (lane & 15)) * LG_LDK + 8 * (lane >> 4));
#pragma unroll
		for (int i = 0; i < TO; ++i) {
			if (o_wave + i * 16 >= a.rows) continue; // wave-uniform: output tiles past the matrix are not computed
#pragma unroll
			for (int j = 0; j < TS; ++j) acc[i][j] = mfma(af[i], bf[j], acc[i][j]);
		}
		__syncthreads();
	}

	// D[row = output 4 (l >> 4) + r][col = sample l & 15]
#pragma unroll
	for (int i = 0; i < TO; ++i) {
		const uint32_t o = o_wave + i * 16 + 4 * (lane >> 4);
		if (o_wave + i * 16 >= a.rows) continue;
#pragma unroll
		for (int j = 0; j < TS; ++j) {
			const size_t at = (s0 + ws * TS * 16 + j * 16 + (lane & 15)) * a.ldy + o;
			if constexpr (SECOND) {
				*(h4*)(a.y + at) = second_order_epilogue(a, at, acc[i][j]);
			} else {
				h4 v;
#pragma unroll
				for (int r = 0; r < 4; ++r) v[r] = (half_t)acc[i][j][r];
				if (a.mode == LG_FWD) {
					if (a.pre) *(h4*)(a.pre + at) = v;
#pragma unroll
					for (int r = 0; r < 4; ++r) v[r] = activation_fwd(a.act, v[r]);
				} else if (a.act != (uint32_t)Activation::None) {
					const h4 f = *(const h4*)(a.aux + at);
					if (a.act == (uint32_t)Activation::Sine) { // cutlass_mlp.cu:101-113, common_device.h:190-193: from the stored pre-activation
#pragma unroll
						for (int r = 0; r < 4; ++r) v[r] = v[r] * (half_t)cosf((float)f[r]);
					} else {
#pragma unroll
						for (int r = 0; r < 4; ++r) v[r] = activation_bwd(a.act, v[r], f[r]);
					}
				}
				*(h4*)(a.y + at) = v;
			}
		}
	}
}

// D = a'(aux) G, element by element: the output layer's step of the first-order data pass
__global__ void __launch_bounds__(256) k_layer_delta(const uint32_t n_elems, const uint32_t act, const half_t* __restrict__ g, const half_t* __restrict__ aux, half_t* __restrict__ delta) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elems) return;
	delta[i] = (half_t)(act_d1(act, (float)aux[i]) * (float)g[i]);
}

// dst += src for [n][dims] float views
__global__ void __launch_bounds__(256) k_add_input_gradient(const uint32_t n, const uint32_t dims, const MatView src, const MatViewMut dst) {
	const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
	const uint32_t i = gid / dims;
	if (i >= n) return;
	const uint32_t j = gid - i * dims;
	dst.data[(size_t)i * dst.stride_sample + (size_t)j * dst.stride_dim] += src.data[(size_t)i * src.stride_sample + (size_t)j * src.stride_dim];
}

__global__ void __launch_bounds__(256) k_layer_transpose(const uint32_t rows, const uint32_t cols, const half_t* __restrict__ w, half_t* __restrict__ wt) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x; // wt element (c, r) = i: c = i / rows
	if (i >= rows * cols) return;
	const uint32_t c = i / rows, r = i - c * rows;
	wt[i] = w[(size_t)r * cols + c];
}

template <bool SECOND>
void launch_layer_gemm(hipStream_t stream, const LayerGemmArgs& a) {
	CHECK_THROW(a.n % BATCH_SIZE_GRANULARITY == 0);
	CHECK_THROW(a.rows % 16 == 0 && a.k % 16 == 0 && a.rows > 0 && a.k > 0);
	CHECK_THROW(a.ldx % 8 == 0 && a.ldx >= a.k && a.ldy % 4 == 0 && a.ldy >= a.rows);
	if (a.n == 0) return;
	if (a.rows <= 64) { // narrow layers (the padded output layer): 64 outputs x 256 samples per workgroup
		const uint32_t blocks = (a.n / 256) * div_round_up(a.rows, 64);
		hipLaunchKernelGGL((k_layer_gemm<1, 4, 4, 4, SECOND>), dim3(blocks), dim3(256), 0, stream, a);
	} else {            // 128 outputs x 128 samples, waves 2 x 2 of 64 x 64
		const uint32_t blocks = (a.n / 128) * div_round_up(a.rows, 128);
		hipLaunchKernelGGL((k_layer_gemm<2, 2, 4, 4, SECOND>), dim3(blocks), dim3(256), 0, stream, a);
	}
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace

void mlp_layer_forward(hipStream_t stream, uint32_t n, const void* x, uint32_t ldx, const void* w, uint32_t rows, uint32_t cols, uint32_t activation, void* y, uint32_t ldy,
                       void* pre) {
	LayerGemmArgs a{(const half_t*)x, (const half_t*)w, (half_t*)y, (half_t*)pre, nullptr, n, ldx, cols, rows, ldy, activation, LG_FWD, nullptr};
	launch_layer_gemm<false>(stream, a);
}

void mlp_layer_backward(hipStream_t stream, uint32_t n, const void* dL_dout, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols, uint32_t activation, const void* aux,
                        void* dL_din, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	LayerGemmArgs a{(const half_t*)dL_dout, (const half_t*)wt, (half_t*)dL_din, nullptr, (const half_t*)aux, n, ldo, rows, cols, ldi, activation, LG_BWD, nullptr};
	launch_layer_gemm<false>(stream, a);
}

void mlp_layer_tangent(hipStream_t stream, uint32_t n, const void* u_in, uint32_t ldu, const void* w, uint32_t rows, uint32_t cols, uint32_t activation, const void* aux, const void* g,
                       void* u_out, void* r_out, uint32_t ldy) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	CHECK_THROW(!r_out || (g && aux));
	LayerGemmArgs a{(const half_t*)u_in, (const half_t*)w, (half_t*)u_out, (half_t*)r_out, (const half_t*)aux, n, ldu, cols, rows, ldy, activation, LG_TANGENT, (const half_t*)g};
	launch_layer_gemm<true>(stream, a);
}

void mlp_layer_backward_keep(hipStream_t stream, uint32_t n, const void* d_out, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols, uint32_t activation, const void* aux,
                             void* g_in, void* d_in, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	LayerGemmArgs a{(const half_t*)d_out, (const half_t*)wt, (half_t*)d_in, (half_t*)g_in, (const half_t*)aux, n, ldo, rows, cols, ldi, activation, LG_BWD_KEEP, nullptr};
	launch_layer_gemm<true>(stream, a);
}

void mlp_layer_curvature_backward(hipStream_t stream, uint32_t n, const void* p_out, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols, uint32_t activation, const void* aux,
                                  const void* r_in, void* p_in, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	LayerGemmArgs a{(const half_t*)p_out, (const half_t*)wt, (half_t*)p_in, nullptr, (const half_t*)aux, n, ldo, rows, cols, ldi, activation, LG_CURVATURE, (const half_t*)r_in};
	launch_layer_gemm<true>(stream, a);
}

void mlp_layer_delta(hipStream_t stream, size_t n_elems, uint32_t activation, const void* g, const void* aux, void* delta) {
	if (n_elems == 0) return;
	CHECK_THROW(n_elems < (1ull << 32));
	hipLaunchKernelGGL(k_layer_delta, dim3(div_round_up((uint32_t)n_elems, 256u)), dim3(256), 0, stream, (uint32_t)n_elems, activation, (const half_t*)g, (const half_t*)aux, (half_t*)delta);
	HIP_CHECK_THROW(hipGetLastError());
}

void add_input_gradient(hipStream_t stream, uint32_t n, uint32_t dims, MatView src, MatViewMut dst) {
	const uint64_t total = (uint64_t)n * dims;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32));
	hipLaunchKernelGGL(k_add_input_gradient, dim3(div_round_up((uint32_t)total, 256u)), dim3(256), 0, stream, n, dims, src, dst);
	HIP_CHECK_THROW(hipGetLastError());
}

void mlp_layer_transpose(hipStream_t stream, uint32_t rows, uint32_t cols, const void* w, void* wt) {
	const uint32_t total = rows * cols;
	if (total == 0) return;
	hipLaunchKernelGGL(k_layer_transpose, dim3(div_round_up(total, 256)), dim3(256), 0, stream, rows, cols, (const half_t*)w, (half_t*)wt);
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace tcnn_amd
