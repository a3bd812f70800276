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
#include "mlp_device.h"

namespace tcnn_amd {
namespace {

constexpr uint32_t LG_BK = 32;          // K per staged step (one 16x16x32 k-step)
constexpr uint32_t LG_LDK = LG_BK + 8;  // halfs per LDS row: 16 bytes of padding break the power-of-two row stride

enum : uint32_t { LG_FWD = 0, LG_BWD = 1 };

struct LayerGemmArgs {
	const half_t* x;   // [n][ldx], columns 0..k-1 read
	const half_t* w;   // [rows][k]
	half_t* y;         // [n][ldy], columns 0..rows-1 written
	half_t* pre;       // forward, optional: the half pre-activation, [n][ldy]
	const half_t* aux; // backward: forward output (or the pre-activation for Sine) of the layer whose input gradient y is, [n][ldy]
	uint32_t n, ldx, k, rows, ldy, act, mode;
};

// WO x WS waves, each TO x TS tiles of 16 outputs x 16 samples
template <int WO, int WS, int TO, int TS>
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

__global__ void __launch_bounds__(256) k_layer_transpose(const uint32_t rows, const uint32_t cols, const half_t* __restrict__ w, half_t* __restrict__ wt) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x; // wt element (c, r) = i: c = i / rows
	if (i >= rows * cols) return;
	const uint32_t c = i / rows, r = i - c * rows;
	wt[i] = w[(size_t)r * cols + c];
}

void launch_layer_gemm(hipStream_t stream, const LayerGemmArgs& a) {
	CHECK_THROW(a.n % BATCH_SIZE_GRANULARITY == 0);
	CHECK_THROW(a.rows % 16 == 0 && a.k % 16 == 0 && a.rows > 0 && a.k > 0);
	CHECK_THROW(a.ldx % 8 == 0 && a.ldx >= a.k && a.ldy % 4 == 0 && a.ldy >= a.rows);
	if (a.n == 0) return;
	if (a.rows <= 64) { // narrow layers (the padded output layer): 64 outputs x 256 samples per workgroup
		const uint32_t blocks = (a.n / 256) * div_round_up(a.rows, 64);
		hipLaunchKernelGGL((k_layer_gemm<1, 4, 4, 4>), dim3(blocks), dim3(256), 0, stream, a);
	} else {            // 128 outputs x 128 samples, waves 2 x 2 of 64 x 64
		const uint32_t blocks = (a.n / 128) * div_round_up(a.rows, 128);
		hipLaunchKernelGGL((k_layer_gemm<2, 2, 4, 4>), dim3(blocks), dim3(256), 0, stream, a);
	}
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace

void mlp_layer_forward(hipStream_t stream, uint32_t n, const void* x, uint32_t ldx, const void* w, uint32_t rows, uint32_t cols, uint32_t activation, void* y, uint32_t ldy,
                       void* pre) {
	LayerGemmArgs a{(const half_t*)x, (const half_t*)w, (half_t*)y, (half_t*)pre, nullptr, n, ldx, cols, rows, ldy, activation, LG_FWD};
	launch_layer_gemm(stream, a);
}

void mlp_layer_backward(hipStream_t stream, uint32_t n, const void* dL_dout, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols, uint32_t activation, const void* aux,
                        void* dL_din, uint32_t ldi) {
	CHECK_THROW(activation == (uint32_t)Activation::None || aux != nullptr);
	LayerGemmArgs a{(const half_t*)dL_dout, (const half_t*)wt, (half_t*)dL_din, nullptr, (const half_t*)aux, n, ldo, rows, cols, ldi, activation, LG_BWD};
	launch_layer_gemm(stream, a);
}

void mlp_layer_transpose(hipStream_t stream, uint32_t rows, uint32_t cols, const void* w, void* wt) {
	const uint32_t total = rows * cols;
	if (total == 0) return;
	hipLaunchKernelGGL(k_layer_transpose, dim3(div_round_up(total, 256)), dim3(256), 0, stream, rows, cols, (const half_t*)w, (half_t*)wt);
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace tcnn_amd
