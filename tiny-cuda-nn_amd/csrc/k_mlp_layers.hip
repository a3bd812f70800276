// k_mlp_layers.hip -- the layer-by-layer MLP path (cutlass_mlp.cu:39-300 of the reference): one GEMM launch per layer, activations
// round-trip through memory as row-major matrices [n][width] (sample-major, the layout of the network's input and output) of the
// network's precision T: half_t, or float for the network of the reference's build without TCNN_HALF_PRECISION (common.h:99-123:
// network_precision_t = float, CutlassMLP<float>), here a choice per module (Network{json, Precision::Fp32}), whose weights are read
// from the fp32 parameter vector as they are (no half copy, no fragment images).
//
// In half it serves the CutlassMLP shapes the fused kernels (k_mlp.hip, k_train*.hip) are not specialised for -- any width that is a
// multiple of 16 up to 1024, zero hidden layers, Sine -- and, under TCNN_AMD_MLP_LAYERWISE=1, every other shape (A/B runs).
//
// Both products are NT GEMMs (k contiguous in both operands):
//   forward        Y[s][r]  = act((T) sum_c X[s][c] W[r][c])                 the pre-activation is stored as well where asked for
//   backward data  G[s][c]  = act'((T) sum_r D[s][r] Wt[c][r]),   Wt = W^T, transposed once per backward pass (k_layer_transpose);
//                  act' from the stored output (activation_bwd), from the pre-activation for Sine
// k_layer_gemm: 256 threads, a workgroup tile of BO outputs x BS samples (64 x 256 for layers of at most 64 outputs, else 128 x 128, in
// either precision, so the shapes that cross a boundary are the same), K staged through LDS 32 deep with 16-byte loads (the next K
// step's loads in flight in registers while this one is multiplied; two barriers per step), MFMA with fp32 accumulation
// (LayerElem<T>).  A = the weight tile (outputs on the rows), B = the activation tile (samples on the columns), so a lane ends
// up with 4 consecutive outputs of one sample: one store per tile.  The epilogue rounds to T -- in half the rounding convention of the
// fused kernels and of the oracle: round, then apply the activation; in fp32 no rounding other than fp32's own (-ffp-contract=off: a
// product and a sum are two roundings) -- and every (T) / (float) cast below is no operation at all for T = float.  No atomics: the
// same inputs give the same bits.
//
// The second-order pass (Network::second_order_*, model.h) runs three more products of the same shape through the same main loop
// (k_layer_gemm<..., SECOND = true>), with derivatives a', a'' evaluated in fp32 from a stored matrix `aux` -- the layer's
// pre-activation z, or its output for None / ReLU / LeakyReLU (same sign) -- and one rounding to T per stored matrix:
//   tangent         U[s][r] = a'(z) acc,  R[s][r] = a''(z) G[s][r] acc          acc = sum_c Uin[s][c] W[r][c]   (z' = acc is never stored)
//   backward, keep  G[s][c] = (T) acc,  D[s][c] = a'(z) G[s][c]                 acc = sum_r Din[s][r] Wt[c][r]  (G before the derivative, D after)
//   curvature       P[s][c] = R[s][c] + a'(z) acc                               acc = sum_r Pin[s][r] Wt[c][r]  (P may overwrite R)
#include "mlp_device.h"

namespace tcnn_amd {
namespace {

constexpr uint32_t LG_BK = 32; // K per staged step

// What differs between the two element types of the layer GEMM: the 16-byte piece a thread moves, the LDS row, and how one staged K
// step is multiplied -- in K_STEPS MFMA k-steps, each from one LDS read per operand tile (read: lane l's part of the 16 rows from
// `row` on of a staged tile) and one mfma per tile pair.  The loops over k-steps and tiles are the kernel's: its accumulators never leave
// its frame (handed to a function by reference they compile to other instruction streams, profiles/layer_path_refactor.txt).
template <typename T> struct LayerElem;

template <> struct LayerElem<half_t> {
	typedef h8 piece;   // 16 bytes of a row
	typedef h4 out4;    // a lane's 4 consecutive outputs of one sample: one 8-byte store
	typedef h8 operand; // of one v_mfma_f32_16x16x32_f16: the whole stage
	static constexpr uint32_t PIECE = 8;
	static constexpr uint32_t LDK = LG_BK + 8; // halfs per LDS row: 16 bytes of padding break the power-of-two row stride
	static constexpr uint32_t K_STEPS = 1;
	static __device__ inline uint32_t k_steps(const uint32_t /*k_left*/) { return 1; } // K past the matrix was staged as zeros and is multiplied
	// 16x16x32 operands: lane l holds row (l & 15), k = 8 (l >> 4) .. + 7 of its tile -- one 16-byte LDS read each
	static __device__ inline h8 read(const half_t* tile, const uint32_t row, const uint32_t /*kk*/, const uint32_t lane) { return *(const h8*)(tile + (row + (lane & 15)) * LDK + 8 * (lane >> 4)); }
	static __device__ inline f4 multiply(const h8 a, const h8 b, const f4 c) { return mfma(a, b, c); }
};

// Numerical contract of the fp32 instantiation (tests/test_fp32_network.py holds it, bit for bit against std::fmaf on the CPU):
//   * every output element of a layer product is ONE fp32 accumulator that starts at +0;
//   * it receives the products in ascending k, one fmaf each: acc = fmaf(a[k], b[k], acc), k = 0, 1, ..., K - 1
//     (v_mfma_f32_16x16x4_f32 is exactly that chain over its four k, lane group l >> 4 holding k = l >> 4);
//   * no split-K, no second accumulator summed in at the end; K steps past the matrix are not multiplied at all;
//   * latency is hidden across a wave's 16 output tiles (16 independent chains per k step), never within one element's chain.
template <> struct LayerElem<float> {
	typedef f4 piece;
	typedef f4 out4;       // one 16-byte store
	typedef float operand; // of one v_mfma_f32_16x16x4_f32
	static constexpr uint32_t PIECE = 4;
	// floats per LDS row: the 16 rows a 16x16x4 operand read touches start 36 floats apart, which are 16 different multiples of 4 banks,
	// and the four k of a lane group fill the banks between them: one conflict-free 4-byte read per operand and k step
	static constexpr uint32_t LDK = LG_BK + 4;
	static constexpr uint32_t K_STEPS = LG_BK / 4; // up to eight 16x16x4 k-steps
	// k_left: what is left of the matrix' K from this stage on (k is a multiple of 16: whole steps; those past the matrix are not multiplied)
	static __device__ inline uint32_t k_steps(const uint32_t k_left) { return min(LG_BK, k_left) / 4; }
	// 16x16x4 operands: lane l holds row (l & 15), k = 4 kk + (l >> 4) of its tile; ascending kk = ascending k in every chain
	static __device__ inline float read(const float* tile, const uint32_t row, const uint32_t kk, const uint32_t lane) { return tile[(row + (lane & 15)) * LDK + 4 * kk + (lane >> 4)]; }
	static __device__ inline f4 multiply(const float a, const float b, const f4 c) { return mfma_f32(a, b, c); }
};

template <typename T>
struct LayerGemmArgs {
	const T* x;   // [n][ldx], columns 0..k-1 read
	const T* w;   // [rows][k]
	T* y;         // [n][ldy], columns 0..rows-1 written
	T* pre;       // forward, optional: the pre-activation, [n][ldy]
	const T* aux; // backward: forward output (or the pre-activation for Sine) of the layer whose input gradient y is, [n][ldy]
	uint32_t n, ldx, k, rows, ldy, act, mode;
	// second-order modes: aux = what a', a'' are taken from (act_d1); aux2 = G (tangent) or R (curvature), optional; pre = R (tangent)
	// or G (backward, keep), optional; all [n][ldy]
	const T* aux2;
};

// the second-order epilogues on one 4-output piece of the accumulator (what y gets is returned; R or G go to a.pre on the way)
template <typename T>
__device__ inline typename LayerElem<T>::out4 second_order_epilogue(const LayerGemmArgs<T>& a, const size_t at, const f4 acc) {
	typedef typename LayerElem<T>::out4 T4;
	T4 x = T4{0, 0, 0, 0}, v;
	f4 d1 = f4{1, 1, 1, 1};
	if (a.act != (uint32_t)Activation::None) {
		x = *(const T4*)(a.aux + at);
		for (int r = 0; r < 4; ++r) d1[r] = act_d1(a.act, (float)x[r]);
	}
	if (a.mode == LG_TANGENT) {
		if (a.pre) {
			const T4 g = *(const T4*)(a.aux2 + at);
			T4 c;
			for (int r = 0; r < 4; ++r) c[r] = (T)(act_d2(a.act, (float)x[r]) * (float)g[r] * acc[r]);
			*(T4*)(a.pre + at) = c;
		}
		for (int r = 0; r < 4; ++r) v[r] = (T)(d1[r] * acc[r]);
	} else if (a.mode == LG_BWD_KEEP) {
		for (int r = 0; r < 4; ++r) v[r] = (T)acc[r];
		if (a.pre) *(T4*)(a.pre + at) = v;
		for (int r = 0; r < 4; ++r) v[r] = (T)(d1[r] * (float)v[r]);
	} else { // LG_CURVATURE
		T4 c = T4{0, 0, 0, 0};
		if (a.aux2) c = *(const T4*)(a.aux2 + at);
		for (int r = 0; r < 4; ++r) v[r] = (T)((float)c[r] + d1[r] * acc[r]);
	}
	return v;
}

// WO x WS waves, each TO x TS tiles of 16 outputs x 16 samples
template <typename T, int WO, int WS, int TO, int TS, bool SECOND = false>
__global__ void __launch_bounds__(256) k_layer_gemm(const LayerGemmArgs<T> a) {
	typedef LayerElem<T> E;
	typedef typename E::piece piece;
	typedef typename E::out4 T4;
	static_assert(WO * WS == 4, "four waves");
	constexpr uint32_t BO = WO * TO * 16, BS = WS * TS * 16;
	constexpr uint32_t RP = LG_BK / E::PIECE;                          // 16-byte pieces per staged row
	constexpr uint32_t PW = BO * RP / 256, PX = BS * RP / 256; // and per thread
	static_assert(PW * 256 == BO * RP && PX * 256 == BS * RP, "whole pieces per thread");
	__shared__ __attribute__((aligned(16))) T Ws[BO * E::LDK];
	__shared__ __attribute__((aligned(16))) T Xs[BS * E::LDK];

	const uint32_t n_ob = (a.rows + BO - 1) / BO;
	const uint32_t ob = blockIdx.x % n_ob, sb = blockIdx.x / n_ob; // consecutive workgroups share the sample rows (L2)
	const uint32_t o0 = ob * BO;
	const size_t s0 = (size_t)sb * BS;
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t wo = wave % WO, ws = wave / WO;
	const uint32_t o_wave = o0 + wo * TO * 16;

	piece wv[PW], xv[PX];
	const piece zero = piece{};
	auto fetch = [&](const uint32_t k0) {
#pragma unroll
		for (uint32_t i = 0; i < PW; ++i) {
			const uint32_t p = tid + i * 256, row = p / RP, k = k0 + (p % RP) * E::PIECE, o = o0 + row;
			wv[i] = (o < a.rows && k < a.k) ? *(const piece*)(a.w + (size_t)o * a.k + k) : zero; // rows past the matrix, k past its columns: zeros
		}
#pragma unroll
		for (uint32_t i = 0; i < PX; ++i) {
			const uint32_t p = tid + i * 256, row = p / RP, k = k0 + (p % RP) * E::PIECE;
			xv[i] = k < a.k ? *(const piece*)(a.x + (s0 + row) * a.ldx + k) : zero; // (n is a multiple of BS: every sample row exists)
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
			*(piece*)(Ws + (p / RP) * E::LDK + (p % RP) * E::PIECE) = wv[i];
		}
#pragma unroll
		for (uint32_t i = 0; i < PX; ++i) {
			const uint32_t p = tid + i * 256;
			*(piece*)(Xs + (p / RP) * E::LDK + (p % RP) * E::PIECE) = xv[i];
		}
		__syncthreads();
		if (k0 + LG_BK < a.k) fetch(k0 + LG_BK); // in flight while this step is multiplied
		const uint32_t k_steps = E::k_steps(a.k - k0);
#pragma unroll
		for (uint32_t kk = 0; kk < E::K_STEPS; ++kk) {
			if (kk >= k_steps) break;
			typename E::operand af[TO], bf[TS];
#pragma unroll
			for (int i = 0; i < TO; ++i) af[i] = E::read(Ws, wo * TO * 16 + i * 16, kk, lane);
#pragma unroll
			for (int j = 0; j < TS; ++j) bf[j] = E::read(Xs, ws * TS * 16 + j * 16, kk, lane);
#pragma unroll
			for (int i = 0; i < TO; ++i) {
				if (o_wave + i * 16 >= a.rows) continue; // wave-uniform: output tiles past the matrix are not computed
#pragma unroll
				for (int j = 0; j < TS; ++j) acc[i][j] = E::multiply(af[i], bf[j], acc[i][j]);
			}
		}
		__syncthreads();
	}

	// D[row = output 4 (l >> 4) + r][col = sample l & 15]: 4 consecutive outputs of one sample
#pragma unroll
	for (int i = 0; i < TO; ++i) {
		const uint32_t o = o_wave + i * 16 + 4 * (lane >> 4);
		if (o_wave + i * 16 >= a.rows) continue;
#pragma unroll
		for (int j = 0; j < TS; ++j) {
			const size_t at = (s0 + ws * TS * 16 + j * 16 + (lane & 15)) * a.ldy + o;
			if constexpr (SECOND) {
				*(T4*)(a.y + at) = second_order_epilogue(a, at, acc[i][j]);
			} else {
				T4 v;
#pragma unroll
				for (int r = 0; r < 4; ++r) v[r] = (T)acc[i][j][r];
				if (a.mode == LG_FWD) {
					if (a.pre) *(T4*)(a.pre + at) = v;
#pragma unroll
					for (int r = 0; r < 4; ++r) v[r] = activation_fwd(a.act, v[r]);
				} else if (a.act != (uint32_t)Activation::None) {
					const T4 f = *(const T4*)(a.aux + at);
					if (a.act == (uint32_t)Activation::Sine) { // cutlass_mlp.cu:101-113, common_device.h:190-193: from the stored pre-activation
#pragma unroll
						for (int r = 0; r < 4; ++r) v[r] = v[r] * (T)cosf((float)f[r]);
					} else {
#pragma unroll
						for (int r = 0; r < 4; ++r) v[r] = activation_bwd(a.act, v[r], f[r]);
					}
				}
				*(T4*)(a.y + at) = v;
			}
		}
	}
}

// D = a'(aux) G, element by element: the output layer's step of the first-order data pass
template <typename T>
__global__ void __launch_bounds__(256) k_layer_delta(const uint32_t n_elems, const uint32_t act, const T* __restrict__ g, const T* __restrict__ aux, T* __restrict__ delta) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elems) return;
	delta[i] = (T)(act_d1(act, (float)aux[i]) * (float)g[i]);
}

// kernel_activation_backward_output (common_device.h:748): dL/d(pre-activation output) from the forward OUTPUT values
template <typename T>
__global__ void __launch_bounds__(256) k_act_bwd_output(const uint32_t n_elems, const uint32_t act, const T* __restrict__ dL_dout, const T* __restrict__ out, T* __restrict__ result) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elems) return;
	result[i] = activation_bwd(act, dL_dout[i], out[i]);
}

// dst += src for [n][dims] float views
__global__ void __launch_bounds__(256) k_add_input_gradient(const uint32_t n, const uint32_t dims, const MatView src, const MatViewMut dst) {
	const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
	const uint32_t i = gid / dims;
	if (i >= n) return;
	const uint32_t j = gid - i * dims;
	dst.data[(size_t)i * dst.stride_sample + (size_t)j * dst.stride_dim] += src.data[(size_t)i * src.stride_sample + (size_t)j * src.stride_dim];
}

template <typename T>
__global__ void __launch_bounds__(256) k_layer_transpose(const uint32_t rows, const uint32_t cols, const T* __restrict__ w, T* __restrict__ wt) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x; // wt element (c, r) = i: c = i / rows
	if (i >= rows * cols) return;
	const uint32_t c = i / rows, r = i - c * rows;
	wt[i] = w[(size_t)r * cols + c];
}

template <bool SECOND, typename T>
void launch_layer_gemm_of(hipStream_t stream, const LayerGemmArgs<T>& a) {
	CHECK_THROW(a.n % BATCH_SIZE_GRANULARITY == 0);
	CHECK_THROW(a.rows % 16 == 0 && a.k % 16 == 0 && a.rows > 0 && a.k > 0);
	CHECK_THROW(a.ldx % LayerElem<T>::PIECE == 0 && a.ldx >= a.k && a.ldy % 4 == 0 && a.ldy >= a.rows); // rows of x start at a whole 16-byte piece
	if (a.n == 0) return;
	if (a.rows <= 64) { // narrow layers (the padded output layer): 64 outputs x 256 samples per workgroup
		const uint32_t blocks = (a.n / 256) * div_round_up(a.rows, 64);
		hipLaunchKernelGGL((k_layer_gemm<T, 1, 4, 4, 4, SECOND>), dim3(blocks), dim3(256), 0, stream, a);
	} else {            // 128 outputs x 128 samples, waves 2 x 2 of 64 x 64
		const uint32_t blocks = (a.n / 128) * div_round_up(a.rows, 128);
		hipLaunchKernelGGL((k_layer_gemm<T, 2, 2, 4, 4, SECOND>), dim3(blocks), dim3(256), 0, stream, a);
	}
	HIP_CHECK_THROW(hipGetLastError());
}

// the operands in the order of LayerGemmArgs, typed by `precision`.  Half is named first: the order of instantiation is the order of the kernels
// in the code object, and where these 240 KB kernels lie moves their time by percents (profiles/layer_path_refactor.txt, section 5)
template <bool SECOND>
void launch_layer_gemm(hipStream_t stream, Precision precision, const void* x, const void* w, void* y, void* pre, const void* aux, uint32_t n, uint32_t ldx, uint32_t k, uint32_t rows,
                       uint32_t ldy, uint32_t act, uint32_t mode, const void* aux2) {
	if (precision == Precision::Fp16) {
		launch_layer_gemm_of<SECOND>(stream, LayerGemmArgs<half_t>{(const half_t*)x, (const half_t*)w, (half_t*)y, (half_t*)pre, (const half_t*)aux, n, ldx, k, rows, ldy, act, mode, (const half_t*)aux2});
	} else {
		launch_layer_gemm_of<SECOND>(stream, LayerGemmArgs<float>{(const float*)x, (const float*)w, (float*)y, (float*)pre, (const float*)aux, n, ldx, k, rows, ldy, act, mode, (const float*)aux2});
	}
}

} // namespace

void mlp_layer_forward(hipStream_t stream, Precision precision, uint32_t n, const void* x, uint32_t ldx, const void* w, uint32_t rows, uint32_t cols, uint32_t activation, void* y,
                       uint32_t ldy, void* pre) {
	launch_layer_gemm<false>(stream, precision, x, w, y, pre, nullptr, n, ldx, cols, rows, ldy, activation, LG_FWD, nullptr);
}

void mlp_layer_backward(hipStream_t stream, Precision precision, uint32_t n, const void* dL_dout, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols, uint32_t activation,
                        const void* aux, void* dL_din, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	launch_layer_gemm<false>(stream, precision, dL_dout, wt, dL_din, nullptr, aux, n, ldo, rows, cols, ldi, activation, LG_BWD, nullptr);
}

void mlp_layer_tangent(hipStream_t stream, Precision precision, uint32_t n, const void* u_in, uint32_t ldu, const void* w, uint32_t rows, uint32_t cols, uint32_t activation,
                       const void* aux, const void* g, void* u_out, void* r_out, uint32_t ldy) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	CHECK_THROW(!r_out || (g && aux));
	launch_layer_gemm<true>(stream, precision, u_in, w, u_out, r_out, aux, n, ldu, cols, rows, ldy, activation, LG_TANGENT, g);
}

void mlp_layer_backward_keep(hipStream_t stream, Precision precision, uint32_t n, const void* d_out, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols, uint32_t activation,
                             const void* aux, void* g_in, void* d_in, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	launch_layer_gemm<true>(stream, precision, d_out, wt, d_in, g_in, aux, n, ldo, rows, cols, ldi, activation, LG_BWD_KEEP, nullptr);
}

void mlp_layer_curvature_backward(hipStream_t stream, Precision precision, uint32_t n, const void* p_out, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols,
                                  uint32_t activation, const void* aux, const void* r_in, void* p_in, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	launch_layer_gemm<true>(stream, precision, p_out, wt, p_in, nullptr, aux, n, ldo, rows, cols, ldi, activation, LG_CURVATURE, r_in);
}

void mlp_layer_delta(hipStream_t stream, Precision precision, size_t n_elems, uint32_t activation, const void* g, const void* aux, void* delta) {
	if (n_elems == 0) return;
	CHECK_THROW(n_elems < (1ull << 32));
	const dim3 grid(div_round_up((uint32_t)n_elems, 256u));
	if (precision == Precision::Fp16) hipLaunchKernelGGL(k_layer_delta<half_t>, grid, dim3(256), 0, stream, (uint32_t)n_elems, activation, (const half_t*)g, (const half_t*)aux, (half_t*)delta);
	else hipLaunchKernelGGL(k_layer_delta<float>, grid, dim3(256), 0, stream, (uint32_t)n_elems, activation, (const float*)g, (const float*)aux, (float*)delta);
	HIP_CHECK_THROW(hipGetLastError());
}

// fully_fused_mlp.cu:757-762: the output activation's transfer, computed once in front of a backward pass
void mlp_activation_backward_output(hipStream_t stream, Precision precision, size_t n_elems, uint32_t activation, const void* dL_dout, const void* out, void* result) {
	if (n_elems == 0) return;
	CHECK_THROW(n_elems < (1ull << 32));
	const dim3 grid(div_round_up((uint32_t)n_elems, 256u));
	if (precision == Precision::Fp16) hipLaunchKernelGGL(k_act_bwd_output<half_t>, grid, dim3(256), 0, stream, (uint32_t)n_elems, activation, (const half_t*)dL_dout, (const half_t*)out, (half_t*)result);
	else hipLaunchKernelGGL(k_act_bwd_output<float>, grid, dim3(256), 0, stream, (uint32_t)n_elems, activation, (const float*)dL_dout, (const float*)out, (float*)result);
	HIP_CHECK_THROW(hipGetLastError());
}

void add_input_gradient(hipStream_t stream, uint32_t n, uint32_t dims, MatView src, MatViewMut dst) {
	const uint64_t total = (uint64_t)n * dims;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32));
	hipLaunchKernelGGL(k_add_input_gradient, dim3(div_round_up((uint32_t)total, 256u)), dim3(256), 0, stream, n, dims, src, dst);
	HIP_CHECK_THROW(hipGetLastError());
}

void mlp_layer_transpose(hipStream_t stream, Precision precision, uint32_t rows, uint32_t cols, const void* w, void* wt) {
	const uint32_t total = rows * cols;
	if (total == 0) return;
	if (precision == Precision::Fp16) hipLaunchKernelGGL(k_layer_transpose<half_t>, dim3(div_round_up(total, 256)), dim3(256), 0, stream, rows, cols, (const half_t*)w, (half_t*)wt);
	else hipLaunchKernelGGL(k_layer_transpose<float>, dim3(div_round_up(total, 256)), dim3(256), 0, stream, rows, cols, (const float*)w, (float*)wt);
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace tcnn_amd
