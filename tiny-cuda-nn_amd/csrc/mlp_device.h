// mlp_device.h -- device helpers shared by the MLP kernels (k_mlp.hip, k_train.hip): MFMA wrappers, activations
// (common_device.h:102-160, 241-297 of the reference), fragment k-orders, transposing LDS read, dL/dx store.
#pragma once

#include "tcnn_common.h"

#include <hip/hip_fp16.h>

namespace tcnn_amd {

// the fp32 weight gradients (k_mlp_layers_f32.hip) behind wgrad_panels_workspace_floats / mlp_wgrad_panels (k_mlp.hip), which hand Precision::Fp32 on
size_t wgrad_panels_workspace_floats_f32(const WgradPanel* panels, uint32_t count, uint32_t n);
void mlp_wgrad_panels_f32(hipStream_t stream, uint32_t n, const WgradPanel* panels, uint32_t count, bool accumulate, float* workspace);

namespace {

typedef _Float16 half_t;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr float K_ACT = 10.0f;

__device__ inline float logistic(float x) { return 1.0f / (1.0f + expf(-x)); }

// expf where a cancellation magnifies its last bit: 1 - expf(-10 y) in Softplus' for small outputs y, 1 - 2 s in Sigmoid'' for small z.  The
// reference's results come from a correctly rounded expf; ocml's is one ulp off for 5 % of the arguments, which these differences turn into 2
// and 8 half steps.  Below 2^-6 the series 1 + x + x^2/2 + .. + x^5/120, its low part carried beside 1 + x, is correctly rounded but for one
// argument in 40 000; elsewhere expf's last bit is far below half precision.
__device__ inline float expf_near_zero(float x) {
	if (!(fabsf(x) < 0x1p-6f)) return expf(x);
	const float lo = x * x * (0.5f + x * (1.0f / 6 + x * (1.0f / 24 + x * (1.0f / 120))));
	const float s = 1.0f + x;
	const float e = x - (s - 1.0f); // exact: what 1 + x rounded away
	return s + (e + lo);
}

// common_device.h:102-160, applied to the fp16-rounded accumulator like the reference's warp_activation.  T: the network's precision --
// half_t, or float for the full-precision layers (k_mlp_layers.hip), where every (T) below is no rounding at all
template <typename T>
__device__ inline T activation_fwd(uint32_t act, T pre) {
	const float x = (float)pre;
	switch (act) {
		case (uint32_t)Activation::ReLU: return x > 0.0f ? pre : (T)0.0f;
		case (uint32_t)Activation::LeakyReLU: return pre * (T)(x > 0.0f ? 1.0f : 0.01f);
		case (uint32_t)Activation::Exponential: return (T)expf(x);
		case (uint32_t)Activation::Sine: return (T)sinf(x);
		case (uint32_t)Activation::Sigmoid: return (T)logistic(x);
		case (uint32_t)Activation::Squareplus: { const float y = x * K_ACT; return (T)(0.5f * (y + sqrtf(y * y + 4)) / K_ACT); }
		case (uint32_t)Activation::Softplus: return (T)(logf(expf(x * K_ACT) + 1.0f) / K_ACT);
		case (uint32_t)Activation::Tanh: return (T)tanhf(x);
		default: return pre;
	}
}

// common_device.h:241-297: derivative from the forward OUTPUT
template <typename T>
__device__ inline T activation_bwd(uint32_t act, T grad, T fwd) {
	const float y = (float)fwd;
	switch (act) {
		case (uint32_t)Activation::ReLU: return y > 0.0f ? grad : grad * (T)0.0f;
		case (uint32_t)Activation::LeakyReLU: return grad * (T)(y > 0.0f ? 1.0f : 0.01f);
		case (uint32_t)Activation::Exponential: return grad * fwd;
		case (uint32_t)Activation::Sigmoid: return grad * (T)(fwd * (T)(1.0f - y));
		case (uint32_t)Activation::Squareplus: { const float t = y * K_ACT; return grad * (T)(t * t / (t * t + 1)); }
		case (uint32_t)Activation::Softplus: return grad * (T)(1.0f - expf_near_zero(-y * K_ACT));
		case (uint32_t)Activation::Tanh: return grad * (T)(1.0f - (y * y));
		default: return grad; // None; Sine is unsupported from outputs (common_device.h:261-265)
	}
}

// a'(z) and a''(z) in fp32 (the functions of activation_fwd), for the layer-by-layer kernels of either precision (k_mlp_layers.hip).
// x: the stored pre-activation; for ReLU / LeakyReLU the stored output serves as well (same sign), and None takes no argument at all.
__device__ inline float act_d1(const uint32_t act, const float x) {
	switch (act) {
		case (uint32_t)Activation::ReLU: return x > 0.0f ? 1.0f : 0.0f;
		case (uint32_t)Activation::LeakyReLU: return x > 0.0f ? 1.0f : 0.01f;
		case (uint32_t)Activation::Exponential: return expf(x);
		case (uint32_t)Activation::Sine: return cosf(x);
		case (uint32_t)Activation::Sigmoid: { const float s = 1.0f / (1.0f + expf_near_zero(-x)); return s * (1.0f - s); }
		case (uint32_t)Activation::Squareplus: { const float y = x * K_ACT; return 0.5f * (1.0f + y / sqrtf(y * y + 4)); }
		case (uint32_t)Activation::Softplus: return logistic(x * K_ACT);
		case (uint32_t)Activation::Tanh: { const float t = tanhf(x); return 1.0f - t * t; }
		default: return 1.0f;
	}
}
__device__ inline float act_d2(const uint32_t act, const float x) {
	switch (act) {
		case (uint32_t)Activation::Exponential: return expf(x);
		case (uint32_t)Activation::Sine: return -sinf(x);
		case (uint32_t)Activation::Sigmoid: { const float s = 1.0f / (1.0f + expf_near_zero(-x)); return s * (1.0f - s) * (1.0f - 2.0f * s); }
		case (uint32_t)Activation::Squareplus: { const float y = x * K_ACT, q = y * y + 4; return 2.0f * K_ACT / (q * sqrtf(q)); }
		case (uint32_t)Activation::Softplus: { const float s = logistic(x * K_ACT); return K_ACT * s * (1.0f - s); }
		case (uint32_t)Activation::Tanh: { const float t = tanhf(x); return -2.0f * t * (1.0f - t * t); }
		default: return 0.0f; // None, ReLU, LeakyReLU: piecewise linear
	}
}

// what a layer GEMM of the layer-by-layer path computes (its epilogue), in either precision
enum : uint32_t { LG_FWD = 0, LG_BWD = 1, LG_TANGENT = 2, LG_BWD_KEEP = 3, LG_CURVATURE = 4 };

template <int ACT> __device__ inline half_t act_fwd_t(uint32_t act, half_t v) {
	if constexpr (ACT == (int)Activation::ReLU) return v > (half_t)0.0f ? v : (half_t)0.0f;
	else if constexpr (ACT == (int)Activation::None) return v;
	else return activation_fwd(act, v);
}
template <int ACT> __device__ inline half_t act_bwd_t(uint32_t act, half_t g, half_t fwd) {
	if constexpr (ACT == (int)Activation::ReLU) return fwd > (half_t)0.0f ? g : g * (half_t)0.0f;
	else if constexpr (ACT == (int)Activation::None) return g;
	else return activation_bwd(act, g, fwd);
}

__device__ inline f4 mfma(h8 a, h8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
// k = 16: A lane l holds A[row = l & 15][k = 4 (l >> 4) + j], B lane l holds B[k = 4 (l >> 4) + j][col = l & 15], j = 0..3
__device__ inline f4 mfma16(h4 a, h4 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
// k = 4 in fp32: lane l holds A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15]; one fmaf per k, in ascending k
__device__ inline f4 mfma_f32(const float a, const float b, const f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// k index of element j of a chained-layer fragment
__host__ __device__ inline uint32_t k_chain(uint32_t s, uint32_t q, uint32_t j) { return 32 * s + 16 * (j >> 2) + 4 * q + (j & 3); }
__host__ __device__ inline uint32_t k_natural(uint32_t s, uint32_t q, uint32_t j) { return 32 * s + 8 * q + j; }

typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

__device__ inline h4 lds_read_tr(const half_t* p) {
	fp16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((fp16x4 __attribute__((address_space(3)))*)p);
	return __builtin_bit_cast(h4, v);
}

// loads / stores at 32-bit byte offsets from wave-uniform bases (saddr + voffset addressing; the plans cap n)
template <typename V> __device__ inline V ld32(const void* base, const uint32_t byte_off) { return *(const V*)((const char*)base + byte_off); }
template <typename V> __device__ inline void st32(void* base, const uint32_t byte_off, const V v) { *(V*)((char*)base + byte_off) = v; }
// the same as a streaming store, for data nobody on the GPU reads soon (the step's outputs: out, dL_doutput, L): it leaves this
// XCD's L2 as it is written instead of waiting there, dirty, for the write-back at the end of the kernel.  NOT for the scatter
// records: measured on C3a, streamed records cost the scatter 10 us (it finds them in the caches otherwise) for 1.4 us gained here.
template <typename V> __device__ inline void st32_stream(void* base, const uint32_t byte_off, const V v) {
	typedef uint32_t nt2 __attribute__((ext_vector_type(2)));
	typedef uint32_t nt4 __attribute__((ext_vector_type(4)));
	char* p = (char*)base + byte_off;
	if constexpr (sizeof(V) == 16) __builtin_nontemporal_store(__builtin_bit_cast(nt4, v), (nt4*)p);
	else if constexpr (sizeof(V) == 8) __builtin_nontemporal_store(__builtin_bit_cast(nt2, v), (nt2*)p);
	else if constexpr (sizeof(V) == 4) __builtin_nontemporal_store(__builtin_bit_cast(uint32_t, v), (uint32_t*)p);
	else __builtin_nontemporal_store(__builtin_bit_cast(uint16_t, v), (uint16_t*)p);
}

// ---- the forward chain's arguments and pieces (k_mlp_fwd in k_mlp.hip, k_mlp_input_grad in k_mlp_input_grad.hip)
struct FwdArgs {
	const half_t* x;      // [n][in_width], or level planes [in_width / F][n][F] when x_plane_f = F > 0; unused with x_f32
	half_t* out;          // optional [n][out_width]
	half_t* hidden;       // optional [n_hidden][n][width]
	const h8* image;      // forward fragments
	uint32_t n;
	uint32_t x_plane_f;
	// fused Identity encoding (identity.h:46-66): feature k = (half)(x[k] * scale + offset) for k < x_f32_dims, 1 for the padding
	MatView x_f32;        // data == nullptr: not used
	uint32_t x_f32_dims;
	float x_scale, x_offset;
	// fused OneBlob encoding (oneblob.h:47-67): x_f32 holds the coordinates, feature dim * n_bins + bin; 0 = off
	uint32_t oneblob_log2;
	// fused trim_and_cast (common_device.h:990-1002): float output of the first out_f32_dims outputs
	MatViewMut out_f32;   // data == nullptr: not used
	uint32_t out_f32_dims;
};

// 8 consecutive input features k0..k0+7 of one sample: the B operand of layer 0
__device__ inline h8 load_mlp_input(const FwdArgs& a, const uint32_t in_w, const uint32_t sample, const uint32_t k0) {
	if (a.x_f32.data) {
		h8 v;
		if (a.x_f32.stride_dim == 1 && (a.x_f32.stride_sample & 3u) == 0 && k0 + 8 <= a.x_f32_dims) { // two 16-byte loads
			const float4* p = (const float4*)(a.x_f32.data + (size_t)sample * a.x_f32.stride_sample + k0);
			const float4 lo = p[0], hi = p[1];
			v[0] = (half_t)(lo.x * a.x_scale + a.x_offset); v[1] = (half_t)(lo.y * a.x_scale + a.x_offset);
			v[2] = (half_t)(lo.z * a.x_scale + a.x_offset); v[3] = (half_t)(lo.w * a.x_scale + a.x_offset);
			v[4] = (half_t)(hi.x * a.x_scale + a.x_offset); v[5] = (half_t)(hi.y * a.x_scale + a.x_offset);
			v[6] = (half_t)(hi.z * a.x_scale + a.x_offset); v[7] = (half_t)(hi.w * a.x_scale + a.x_offset);
			return v;
		}
#pragma unroll
		for (int j = 0; j < 8; ++j) {
			const uint32_t k = k0 + j;
			v[j] = k < a.x_f32_dims ? (half_t)(a.x_f32.data[(size_t)sample * a.x_f32.stride_sample + (size_t)k * a.x_f32.stride_dim] * a.x_scale + a.x_offset) : (half_t)1.0f;
		}
		return v;
	}
	if (a.x_plane_f == 2) {
		uint4 v;
		v.x = *(const uint32_t*)(a.x + ((size_t)(k0 / 2 + 0) * a.n + sample) * 2);
		v.y = *(const uint32_t*)(a.x + ((size_t)(k0 / 2 + 1) * a.n + sample) * 2);
		v.z = *(const uint32_t*)(a.x + ((size_t)(k0 / 2 + 2) * a.n + sample) * 2);
		v.w = *(const uint32_t*)(a.x + ((size_t)(k0 / 2 + 3) * a.n + sample) * 2);
		return __builtin_bit_cast(h8, v);
	}
	if (a.x_plane_f == 4) {
		const uint2 lo = *(const uint2*)(a.x + ((size_t)(k0 / 4) * a.n + sample) * 4);
		const uint2 hi = *(const uint2*)(a.x + ((size_t)(k0 / 4 + 1) * a.n + sample) * 4);
		uint4 v;
		v.x = lo.x; v.y = lo.y; v.z = hi.x; v.w = hi.y;
		return __builtin_bit_cast(h8, v);
	}
	if (a.x_plane_f == 8) return *(const h8*)(a.x + ((size_t)(k0 / 8) * a.n + sample) * 8);
	return *(const h8*)(a.x + (size_t)sample * in_w + k0);
}

// pack NB accumulator column blocks of T row tiles into chained B fragments (KS k-steps), applying the activation
// (activate_pack_inlined: for callers that cannot afford the call -- acc and hf are passed by reference, and where the compiler keeps
// activate_pack as a function of its own both arrays live in scratch)
template <int T, int KS, int NB, int ACT>
__device__ __forceinline__ void activate_pack_inlined(const f4 (&acc)[T][NB], h8 (&hf)[KS][NB], uint32_t act) {
#pragma unroll
	for (int s = 0; s < KS; ++s) {
#pragma unroll
		for (int b = 0; b < NB; ++b) {
			h8 v;
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				v[r] = act_fwd_t<ACT>(act, (half_t)acc[2 * s][b][r]);
				if (2 * s + 1 < T) v[4 + r] = act_fwd_t<ACT>(act, (half_t)acc[(2 * s + 1 < T) ? 2 * s + 1 : 0][b][r]);
				else v[4 + r] = (half_t)0.0f;
			}
			hf[s][b] = v;
		}
	}
}
template <int T, int KS, int NB, int ACT>
__device__ inline void activate_pack(const f4 (&acc)[T][NB], h8 (&hf)[KS][NB], uint32_t act) { activate_pack_inlined<T, KS, NB, ACT>(acc, hf, act); }

// Store 4 consecutive input-gradient features k0..k0+3 of sample s.  AoS: one 8-byte store.  Level planes (what the grid
// scatter reads with unit stride): feature k lives at ((k / F) * n + s) * F + k % F.
__device__ inline void store_dx(half_t* base, uint32_t plane_f, uint32_t n, uint32_t in_w, uint32_t s, uint32_t k0, h4 v) {
	typedef _Float16 h2 __attribute__((ext_vector_type(2)));
	if (plane_f == 0) {
		*(h4*)(base + (size_t)s * in_w + k0) = v;
	} else if (plane_f == 2) {
		*(h2*)(base + ((size_t)(k0 / 2) * n + s) * 2) = h2{v[0], v[1]};
		*(h2*)(base + ((size_t)(k0 / 2 + 1) * n + s) * 2) = h2{v[2], v[3]};
	} else if (plane_f >= 4) {
		*(h4*)(base + ((size_t)(k0 / plane_f) * n + s) * plane_f + (k0 % plane_f)) = v;
	} else {
#pragma unroll
		for (int r = 0; r < 4; ++r) base[(size_t)(k0 + r) * n + s] = v[r];
	}
}

// "Records" for the grid scatter (k_grid_scatter.hip): 16-byte records = the sample's D coordinates (floats) followed by
// gradients (halves), so that the scatter fetches everything it needs about a hit with ONE load.  Requires 4 D + 2 F <= 16.
//   D = 2, F = 2: float4 rec[level / 2][n] = {x, y, gradients of the even level, gradients of the odd level} (two levels share a record)
//   D = 3, F = 2: float4 rec[level][n]     = {x, y, z, gradients}
//   D = 2, F = 4: float4 rec[level][n]     = {x, y, gradients}
// v = features k0..k0+3 of sample s (k0 a multiple of 4).
__device__ inline void store_dx_record(half_t* base, uint32_t F, uint32_t D, uint32_t n, uint32_t s, uint32_t k0, h4 v, const float* xs) {
	typedef uint32_t u4 __attribute__((ext_vector_type(4)));
	typedef _Float16 h2 __attribute__((ext_vector_type(2)));
	u4* recs = (u4*)base;
	const uint32_t x0 = __builtin_bit_cast(uint32_t, xs[0]), x1 = __builtin_bit_cast(uint32_t, xs[1]), x2 = __builtin_bit_cast(uint32_t, xs[2]);
	const uint32_t lo = __builtin_bit_cast(uint32_t, (h2{v[0], v[1]})), hi = __builtin_bit_cast(uint32_t, (h2{v[2], v[3]}));
	if (F == 2 && D == 3) {
		recs[(size_t)(k0 / 2) * n + s] = u4{x0, x1, x2, lo};
		recs[(size_t)(k0 / 2 + 1) * n + s] = u4{x0, x1, x2, hi};
	} else { // F == 2, D == 2: levels k0 / 2 and k0 / 2 + 1 = pair k0 / 4;  F == 4, D == 2: level k0 / 4
		recs[(size_t)(k0 / 4) * n + s] = u4{x0, x1, lo, hi};
	}
}


// ---- L2 / RelativeL2 inside the fused training kernels (losses/l2.h:40-74, relative_l2.h:40-75):
//     value = d^2 / (p^2 + 0.01) / pdf / n_total,   dL/dy = (half)(loss_scale * (2 d / (p^2 + 0.01) / pdf) / n_total),   d = p - target.
// Floating point, so its bar is the north-star tolerance, not bit equality with the reference's order of operations: ONE reciprocal
// (v_rcp_f32 refined by one Newton step) serves value and gradient, and the two divisions by n_total are multiplications by constants
// computed once per kernel -- 13 dependent instructions where four IEEE divisions were ~100 (the loss was 940 of a wave's 5.9 k clocks
// per trip in k_mlp_train_r32).  Against the reference's order (the oracle; k_loss keeps it): values within 4 ulp, >= 99.9 % of the half
// gradients identical and the rest one half-ulp apart (tests/test_losses.py::test_fused_loss_against_the_exact_order).
struct LossScales { float inv_n_total, scale_over_n; };
__device__ inline LossScales loss_scales(const uint32_t n_total, const float loss_scale) { return LossScales{1.0f / (float)n_total, loss_scale / (float)n_total}; }
template <bool RELATIVE>
__device__ inline void loss_l2_fused(const float prediction, const float target, const LossScales& k, float& value, half_t& grad, const bool has_pdf = false, const float pdf = 1.0f) {
	const float d = prediction - target;
	float dr = d; // d / (p^2 + 0.01) / pdf
	if constexpr (RELATIVE) {
		const float q = __builtin_fmaf(prediction, prediction, 0.01f);
		const float r0 = __builtin_amdgcn_rcpf(q);
		dr = d * __builtin_fmaf(r0, __builtin_fmaf(-q, r0, 1.0f), r0);
	}
	if (has_pdf) dr = dr / pdf; // (uniform; relative_l2.h:66-70: an optional importance-sampling density)
	value = d * dr * k.inv_n_total;
	grad = (half_t)((dr + dr) * k.scale_over_n);
}

} // namespace
} // namespace tcnn_amd
