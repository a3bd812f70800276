// k_encodings.hip -- parameter-free encodings beside OneBlob / Identity: Frequency, TriangleWave, SphericalHarmonics.
//
// Replaces (reference, /root/reference/include/tiny-cuda-nn):
//   encodings/frequency.h:44-101           frequency_encoding / _backward        -> k_frequency_fwd, k_periodic_bwd_input
//   encodings/triangle_wave.h:44-107       triangle_wave_encoding / _backward    -> k_trianglewave_fwd, k_periodic_bwd_input
//   encodings/spherical_harmonics.h:44-108 kernel_sh / kernel_sh_backward, common_device.h:339-700 sh_enc / sh_enc_grad
//                                                                                -> k_sh_fwd, k_sh_bwd_input
// Also here: k_oneblob_tangent, the OneBlob encoding's tangent for input_jvp (no counterpart in the reference; the encoding's other
// kernels are in k_misc.hip).
// All streaming, AoS output [n][out_stride] (padding = 1).  The reference hard-codes the 64 spherical-harmonic polynomials
// of degree <= 8 and their 192 partial derivatives (generated from the recurrences of Sloan, "Stupid Spherical Harmonics
// Tricks", appendix A1); here the same polynomials are evaluated through those recurrences (see the oracle's sh_eval): identical
// functions of (x, y, z), summed in another floating-point order (~1e-7 relative).  Frequency: sinf / cosf instead of the
// reference's __sinf / __cosf hardware approximations.
#include "tcnn_common.h"
#include "oneblob_device.h" // k_oneblob_tangent: the OneBlob kernel's derivative, as k_misc.hip's k_oneblob_bwd_input forms it

#include <hip/hip_fp16.h>

#include <cmath>

namespace tcnn_amd {
namespace {

typedef _Float16 half_t;

struct ShNorms { float v[64]; }; // N_l^m at [l * 8 + m]

template <typename T>
__global__ void __launch_bounds__(256) k_frequency_fwd(const uint32_t n_elements, const uint32_t n_frequencies, const uint32_t n_dims, const uint32_t out_stride, const MatView x,
                                                       T* __restrict__ out, float* __restrict__ dy_dx) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elements) return;
	const uint32_t fan_out_encoded = n_dims * n_frequencies * 2;
	const uint32_t i = e / out_stride, j = e - i * out_stride;
	if (j >= fan_out_encoded) {
		out[e] = (T)1.0f;
		return;
	}
	const float PI = 3.14159265358979323846f;
	const uint32_t feature = j / (n_frequencies * 2);
	const uint32_t log2_frequency = (j / 2) % n_frequencies;
	const float phase_shift = (j % 2) * (PI / 2);
	const float v = scalbnf(x.data[(size_t)i * x.stride_sample + (size_t)feature * x.stride_dim], (int)log2_frequency);
	const float input = v * PI + phase_shift;
	out[e] = (T)sinf(input);
	if (dy_dx) dy_dx[(size_t)i * fan_out_encoded + j] = scalbnf(1.0f, (int)log2_frequency) * PI * cosf(input);
}

template <typename T>
__global__ void __launch_bounds__(256) k_trianglewave_fwd(const uint32_t n_elements, const uint32_t n_frequencies, const uint32_t n_dims, const uint32_t out_stride, const MatView x,
                                                          T* __restrict__ out, float* __restrict__ dy_dx) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elements) return;
	const uint32_t fan_out_encoded = n_dims * n_frequencies;
	const uint32_t i = e / out_stride, j = e - i * out_stride;
	if (j >= fan_out_encoded) {
		out[e] = (T)1.0f;
		return;
	}
	const uint32_t feature = j / n_frequencies;
	const int log2_frequency = (int)(j - feature * n_frequencies);
	const float v = scalbnf(x.data[(size_t)i * x.stride_sample + (size_t)feature * x.stride_dim], log2_frequency - 1);
	const float val = v + log2_frequency * 0.25f;
	out[e] = (T)(fabsf(val - floorf(val) - 0.5f) * 4 - 1);
	if (dy_dx) dy_dx[(size_t)i * fan_out_encoded + j] = scalbnf((int)floorf(val * 2.0f) % 2 == 0 ? -1.0f : 1.0f, log2_frequency + 1);
}

template <typename T>
__global__ void __launch_bounds__(256) k_periodic_bwd_input(const uint32_t n_elements, const uint32_t n_dims, const uint32_t outputs_per_input, const T* __restrict__ dL_dy,
                                                            const uint32_t dy_stride, const float* __restrict__ dy_dx, const MatViewMut dL_dx) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elements) return;
	const uint32_t i = e / n_dims, j = e - i * n_dims;
	float result = 0;
	for (uint32_t k = 0; k < outputs_per_input; ++k) result += (float)dL_dy[(size_t)i * dy_stride + j * outputs_per_input + k] * dy_dx[((size_t)i * n_dims + j) * outputs_per_input + k];
	dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)j * dL_dx.stride_dim] = result;
}

// Second-order pass of Frequency, one thread per (sample, input dim): with arg as in k_frequency_fwd (recomputed from x),
//   tangent  t_j   = (2^k pi cos(arg)) v_a         -- the product the forward kernel stores as dy_dx, times v_a
//   Hessian  dL_dx = v_a sum_j d_j (-(2^k pi)^2 sin(arg))
// over the 2 n_frequencies outputs j of dim a in ascending order.  The thread of the last dim also zeroes the row's padding columns.
template <typename T>
__global__ void __launch_bounds__(256) k_frequency_bwd_bwd_input(const uint32_t n_elements, const uint32_t n_frequencies, const uint32_t n_dims, const uint32_t dy_stride, const MatView x,
                                                                 const MatView v, const T* __restrict__ dL_dy, T* __restrict__ dL_ddLdy, const MatViewMut dL_dx) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elements) return;
	const uint32_t i = e / n_dims, a = e - i * n_dims;
	const float PI = 3.14159265358979323846f;
	const float xa = x.data[(size_t)i * x.stride_sample + (size_t)a * x.stride_dim];
	const float va = v.data[(size_t)i * v.stride_sample + (size_t)a * v.stride_dim];
	const size_t row = (size_t)i * dy_stride, first = (size_t)a * n_frequencies * 2;
	float sum = 0;
	for (uint32_t k = 0; k < n_frequencies; ++k) {
		const float scaled = scalbnf(xa, (int)k);
		const float scale = scalbnf(1.0f, (int)k) * PI;
		for (uint32_t phase = 0; phase < 2; ++phase) {
			const float input = scaled * PI + phase * (PI / 2);
			const size_t j = row + first + 2 * k + phase;
			if (dL_ddLdy) dL_ddLdy[j] = (T)(scale * cosf(input) * va);
			if (dL_dx.data) sum += (float)dL_dy[j] * (-(scale * scale) * sinf(input));
		}
	}
	if (dL_dx.data) dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)a * dL_dx.stride_dim] = va * sum;
	if (dL_ddLdy && a == n_dims - 1) {
		for (uint32_t j = n_dims * n_frequencies * 2; j < dy_stride; ++j) dL_ddLdy[row + j] = (T)0.0f;
	}
}

// TriangleWave is piecewise linear: the tangent is the forward kernel's dy_dx (its own sign rule) times v_a, zero in the padding
template <typename T>
__global__ void __launch_bounds__(256) k_trianglewave_bwd_bwd_input(const uint32_t n_elements, const uint32_t n_frequencies, const uint32_t n_dims, const uint32_t dy_stride, const MatView x,
                                                                    const MatView v, T* __restrict__ dL_ddLdy) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elements) return;
	const uint32_t i = e / dy_stride, j = e - i * dy_stride;
	if (j >= n_dims * n_frequencies) {
		dL_ddLdy[e] = (T)0.0f;
		return;
	}
	const uint32_t feature = j / n_frequencies;
	const int log2_frequency = (int)(j - feature * n_frequencies);
	const float scaled = scalbnf(x.data[(size_t)i * x.stride_sample + (size_t)feature * x.stride_dim], log2_frequency - 1);
	const float val = scaled + log2_frequency * 0.25f;
	const float slope = scalbnf((int)floorf(val * 2.0f) % 2 == 0 ? -1.0f : 1.0f, log2_frequency + 1);
	dL_ddLdy[e] = (T)(slope * v.data[(size_t)i * v.stride_sample + (size_t)feature * v.stride_dim]);
}

// all degree^2 values (values != nullptr) and / or the gradient against dL_dy at one point; same operation order as the oracle's sh_eval
template <typename T>
__device__ inline void sh_eval(const uint32_t degree, const ShNorms& norms, const float x, const float y, const float z, T* __restrict__ values, const T* __restrict__ dL_dy, float (&grad)[3]) {
	float gx = 0, gy = 0, gz = 0;
	float c = 1, s = 0, cp = 0, sp = 0;
	float qmm = 1;
	for (uint32_t m = 0; m < degree; ++m) {
		if (m > 0) {
			cp = c;
			sp = s;
			c = x * cp - y * sp;
			s = x * sp + y * cp;
			qmm = -qmm * (float)(2 * m - 1);
		}
		float q2 = 0, q1 = 0, d2 = 0, d1 = 0;
		for (uint32_t l = m; l < degree; ++l) {
			float q, dq;
			if (l == m) { q = qmm; dq = 0; }
			else if (l == m + 1) { q = (float)(2 * m + 1) * z * q1; dq = (float)(2 * m + 1) * q1; }
			else {
				q = ((float)(2 * l - 1) * z * q1 - (float)(l + m - 1) * q2) / (float)(l - m);
				dq = ((float)(2 * l - 1) * (q1 + z * d1) - (float)(l + m - 1) * d2) / (float)(l - m);
			}
			q2 = q1; q1 = q; d2 = d1; d1 = dq;
			const float nq = norms.v[l * 8 + m] * q, ndq = norms.v[l * 8 + m] * dq;
			const uint32_t base = l * l + l;
			if (m == 0) {
				if (values) values[base] = (T)nq;
				if (dL_dy) gz += (float)dL_dy[base] * ndq;
			} else {
				if (values) { values[base + m] = (T)(nq * c); values[base - m] = (T)(nq * s); }
				if (dL_dy) {
					const float gp = (float)dL_dy[base + m], gm = (float)dL_dy[base - m];
					gx += gp * (nq * (float)m * cp) + gm * (nq * (float)m * sp);
					gy += gp * (nq * -(float)m * sp) + gm * (nq * (float)m * cp);
					gz += gp * (ndq * c) + gm * (ndq * s);
				}
			}
		}
	}
	grad[0] = gx; grad[1] = gy; grad[2] = gz;
}

template <typename T>
__global__ void __launch_bounds__(128) k_sh_fwd(const uint32_t n, const uint32_t degree, const uint32_t n_to_pad, const ShNorms norms, const MatView x, T* __restrict__ out, const uint32_t out_stride) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	T* o = out + (size_t)i * out_stride;
	for (uint32_t j = 0; j < n_to_pad; ++j) o[j] = (T)1.0f; // the padding columns come first (spherical_harmonics.h:58-64)
	float unused[3];
	const float* p = x.data + (size_t)i * x.stride_sample;
	sh_eval<T>(degree, norms, p[0] * 2.f - 1.f, p[x.stride_dim] * 2.f - 1.f, p[2 * (size_t)x.stride_dim] * 2.f - 1.f, o + n_to_pad, nullptr, unused);
}

template <typename T>
__global__ void __launch_bounds__(128) k_sh_bwd_input(const uint32_t n, const uint32_t degree, const uint32_t n_to_pad, const ShNorms norms, const MatView x, const T* __restrict__ dL_dy,
                                                      const uint32_t dy_stride, const MatViewMut dL_dx) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float g[3];
	const float* p = x.data + (size_t)i * x.stride_sample;
	sh_eval<T>(degree, norms, p[0] * 2.f - 1.f, p[x.stride_dim] * 2.f - 1.f, p[2 * (size_t)x.stride_dim] * 2.f - 1.f, (T*)nullptr, dL_dy + (size_t)i * dy_stride + n_to_pad, g);
	// times 2: [0, 1]^3 -> [-1, 1]^3 (spherical_harmonics.h:100-104)
	for (int d = 0; d < 3; ++d) dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)d * dL_dx.stride_dim] = 2.0f * g[d];
}

// sh_eval with a dotted twin (the directional derivative along (dx, dy, dz)) of every quantity: the twins of the values are the
// tangent, the twins of the gradient accumulators are the Hessian applied to the direction.  Same loops and operation order as
// sh_eval; each twin is the product / quotient rule applied to its line, terms in the order of the line's factors.
template <typename T>
__device__ inline void sh_eval_dotted(const uint32_t degree, const ShNorms& norms, const float x, const float y, const float z, const float dx, const float dy, const float dz,
                                      T* __restrict__ tangent, const T* __restrict__ dL_dy, float (&hess)[3]) {
	float gx_ = 0, gy_ = 0, gz_ = 0;
	float c = 1, s = 0, cp = 0, sp = 0;
	float c_ = 0, s_ = 0, cp_ = 0, sp_ = 0;
	float qmm = 1;
	for (uint32_t m = 0; m < degree; ++m) {
		if (m > 0) {
			cp = c; sp = s; cp_ = c_; sp_ = s_;
			c = x * cp - y * sp;
			s = x * sp + y * cp;
			c_ = (dx * cp + x * cp_) - (dy * sp + y * sp_);
			s_ = (dx * sp + x * sp_) + (dy * cp + y * cp_);
			qmm = -qmm * (float)(2 * m - 1);
		}
		float q2 = 0, q1 = 0, d2 = 0, d1 = 0;
		float q2_ = 0, q1_ = 0, d2_ = 0, d1_ = 0;
		for (uint32_t l = m; l < degree; ++l) {
			float q, dq, q_, dq_;
			if (l == m) { q = qmm; dq = 0; q_ = 0; dq_ = 0; }
			else if (l == m + 1) {
				q = (float)(2 * m + 1) * z * q1; dq = (float)(2 * m + 1) * q1;
				q_ = (float)(2 * m + 1) * (dz * q1 + z * q1_); dq_ = (float)(2 * m + 1) * q1_;
			} else {
				q = ((float)(2 * l - 1) * z * q1 - (float)(l + m - 1) * q2) / (float)(l - m);
				dq = ((float)(2 * l - 1) * (q1 + z * d1) - (float)(l + m - 1) * d2) / (float)(l - m);
				q_ = ((float)(2 * l - 1) * (dz * q1 + z * q1_) - (float)(l + m - 1) * q2_) / (float)(l - m);
				dq_ = ((float)(2 * l - 1) * (q1_ + (dz * d1 + z * d1_)) - (float)(l + m - 1) * d2_) / (float)(l - m);
			}
			q2 = q1; q1 = q; d2 = d1; d1 = dq;
			q2_ = q1_; q1_ = q_; d2_ = d1_; d1_ = dq_;
			const float norm = norms.v[l * 8 + m];
			const float nq = norm * q, ndq = norm * dq, nq_ = norm * q_, ndq_ = norm * dq_;
			const uint32_t base = l * l + l;
			if (m == 0) {
				if (tangent) tangent[base] = (T)nq_;
				if (dL_dy) gz_ += (float)dL_dy[base] * ndq_;
			} else {
				if (tangent) { tangent[base + m] = (T)(nq_ * c + nq * c_); tangent[base - m] = (T)(nq_ * s + nq * s_); }
				if (dL_dy) {
					const float gp = (float)dL_dy[base + m], gm = (float)dL_dy[base - m];
					const float ncp_ = (float)m * (nq_ * cp + nq * cp_), nsp_ = (float)m * (nq_ * sp + nq * sp_);
					gx_ += gp * ncp_ + gm * nsp_;
					gy_ += gp * -nsp_ + gm * ncp_;
					gz_ += gp * (ndq_ * c + ndq * c_) + gm * (ndq_ * s + ndq * s_);
				}
			}
		}
	}
	hess[0] = gx_; hess[1] = gy_; hess[2] = gz_;
}

// one thread per sample: the direction is 2 v ([0, 1]^3 -> [-1, 1]^3), so the value twins are t = J v as they stand and the
// gradient twins take the 2 of k_sh_bwd_input: dL_dx = 2 (H 2v) = 4 (sum_j d_j Hess Y_j) v.  The padding columns come first: zero.
template <typename T>
__global__ void __launch_bounds__(128) k_sh_bwd_bwd_input(const uint32_t n, const uint32_t degree, const uint32_t n_to_pad, const ShNorms norms, const MatView x, const MatView v,
                                                          const T* __restrict__ dL_dy, T* __restrict__ dL_ddLdy, const uint32_t dy_stride, const MatViewMut dL_dx) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	T* t = dL_ddLdy ? dL_ddLdy + (size_t)i * dy_stride : nullptr;
	if (t) {
		for (uint32_t j = 0; j < n_to_pad; ++j) t[j] = (T)0.0f;
	}
	float h[3];
	const float* p = x.data + (size_t)i * x.stride_sample;
	const float* pv = v.data + (size_t)i * v.stride_sample;
	sh_eval_dotted<T>(degree, norms, p[0] * 2.f - 1.f, p[x.stride_dim] * 2.f - 1.f, p[2 * (size_t)x.stride_dim] * 2.f - 1.f, pv[0] * 2.f, pv[v.stride_dim] * 2.f, pv[2 * (size_t)v.stride_dim] * 2.f,
	                  t ? t + n_to_pad : nullptr, dL_dx.data ? dL_dy + (size_t)i * dy_stride + n_to_pad : nullptr, h);
	if (dL_dx.data) {
		for (int d = 0; d < 3; ++d) dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)d * dL_dx.stride_dim] = 2.0f * h[d];
	}
}

ShNorms make_norms(uint32_t degree) {
	ShNorms n{};
	for (uint32_t l = 0; l < degree; ++l) {
		for (uint32_t m = 0; m <= l; ++m) {
			double ratio = 1.0; // (l - m)! / (l + m)!
			for (uint32_t k = l - m + 1; k <= l + m; ++k) ratio /= (double)k;
			n.v[l * 8 + m] = (float)(std::sqrt((2.0 * l + 1.0) / (4.0 * 3.14159265358979323846) * ratio) * (m ? std::sqrt(2.0) : 1.0));
		}
	}
	return n;
}

} // namespace

void periodic_forward(hipStream_t stream, bool triangle, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_frequencies, MatView x, void* out, uint32_t out_stride, float* dy_dx) {
	const uint64_t total = (uint64_t)n * out_stride;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32));
	const dim3 blocks((uint32_t)((total + 255) / 256));
#define TCNN_PER(K, T) hipLaunchKernelGGL((K<T>), blocks, dim3(256), 0, stream, (uint32_t)total, n_frequencies, n_dims, out_stride, x, (T*)out, dy_dx)
	if (triangle) { if (fp32) TCNN_PER(k_trianglewave_fwd, float); else TCNN_PER(k_trianglewave_fwd, half_t); }
	else { if (fp32) TCNN_PER(k_frequency_fwd, float); else TCNN_PER(k_frequency_fwd, half_t); }
#undef TCNN_PER
}

void periodic_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, uint32_t outputs_per_input, const void* dL_dy, uint32_t dy_stride, const float* dy_dx, MatViewMut dL_dx) {
	const uint64_t total = (uint64_t)n * n_dims;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32));
	const dim3 blocks((uint32_t)((total + 255) / 256));
	if (fp32) hipLaunchKernelGGL((k_periodic_bwd_input<float>), blocks, dim3(256), 0, stream, (uint32_t)total, n_dims, outputs_per_input, (const float*)dL_dy, dy_stride, dy_dx, dL_dx);
	else hipLaunchKernelGGL((k_periodic_bwd_input<half_t>), blocks, dim3(256), 0, stream, (uint32_t)total, n_dims, outputs_per_input, (const half_t*)dL_dy, dy_stride, dy_dx, dL_dx);
}

void sh_forward(hipStream_t stream, bool fp32, uint32_t n, uint32_t degree, MatView x, void* out, uint32_t out_stride) {
	if (n == 0) return;
	CHECK_THROW(degree >= 1 && degree <= 8 && out_stride >= degree * degree);
	const ShNorms norms = make_norms(degree);
	const uint32_t n_to_pad = out_stride - degree * degree;
	if (fp32) hipLaunchKernelGGL((k_sh_fwd<float>), dim3(div_round_up(n, 128)), dim3(128), 0, stream, n, degree, n_to_pad, norms, x, (float*)out, out_stride);
	else hipLaunchKernelGGL((k_sh_fwd<half_t>), dim3(div_round_up(n, 128)), dim3(128), 0, stream, n, degree, n_to_pad, norms, x, (half_t*)out, out_stride);
}

void sh_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t degree, MatView x, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	if (n == 0) return;
	CHECK_THROW(degree >= 1 && degree <= 8 && dy_stride >= degree * degree);
	const ShNorms norms = make_norms(degree);
	const uint32_t n_to_pad = dy_stride - degree * degree;
	if (fp32) hipLaunchKernelGGL((k_sh_bwd_input<float>), dim3(div_round_up(n, 128)), dim3(128), 0, stream, n, degree, n_to_pad, norms, x, (const float*)dL_dy, dy_stride, dL_dx);
	else hipLaunchKernelGGL((k_sh_bwd_input<half_t>), dim3(div_round_up(n, 128)), dim3(128), 0, stream, n, degree, n_to_pad, norms, x, (const half_t*)dL_dy, dy_stride, dL_dx);
}

void periodic_backward_backward_input(hipStream_t stream, bool triangle, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_frequencies, MatView x, MatView dL_ddLdx, const void* dL_dy,
                                       void* dL_ddLdy, uint32_t dy_stride, MatViewMut* dL_dx) {
	if (triangle) {
		const uint64_t total = (uint64_t)n * dy_stride;
		if (total == 0 || !dL_ddLdy) return;
		CHECK_THROW(total < (1ull << 32));
		const dim3 blocks((uint32_t)((total + 255) / 256));
		if (fp32) hipLaunchKernelGGL((k_trianglewave_bwd_bwd_input<float>), blocks, dim3(256), 0, stream, (uint32_t)total, n_frequencies, n_dims, dy_stride, x, dL_ddLdx, (float*)dL_ddLdy);
		else hipLaunchKernelGGL((k_trianglewave_bwd_bwd_input<half_t>), blocks, dim3(256), 0, stream, (uint32_t)total, n_frequencies, n_dims, dy_stride, x, dL_ddLdx, (half_t*)dL_ddLdy);
		return;
	}
	const uint64_t total = (uint64_t)n * n_dims;
	if (total == 0 || (!dL_ddLdy && !dL_dx)) return;
	CHECK_THROW(total < (1ull << 32) && (uint64_t)n * dy_stride < (1ull << 32));
	CHECK_THROW(!dL_dx || dL_dy != nullptr);
	const MatViewMut dx = dL_dx ? *dL_dx : MatViewMut{nullptr, 0u, 0u};
	const dim3 blocks((uint32_t)((total + 255) / 256));
	if (fp32) hipLaunchKernelGGL((k_frequency_bwd_bwd_input<float>), blocks, dim3(256), 0, stream, (uint32_t)total, n_frequencies, n_dims, dy_stride, x, dL_ddLdx, (const float*)dL_dy, (float*)dL_ddLdy, dx);
	else hipLaunchKernelGGL((k_frequency_bwd_bwd_input<half_t>), blocks, dim3(256), 0, stream, (uint32_t)total, n_frequencies, n_dims, dy_stride, x, dL_ddLdx, (const half_t*)dL_dy, (half_t*)dL_ddLdy, dx);
}

void sh_backward_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t degree, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy, uint32_t dy_stride, MatViewMut* dL_dx) {
	if (n == 0 || (!dL_ddLdy && !dL_dx)) return;
	CHECK_THROW(degree >= 1 && degree <= 8 && dy_stride >= degree * degree);
	CHECK_THROW(!dL_dx || dL_dy != nullptr);
	const ShNorms norms = make_norms(degree);
	const uint32_t n_to_pad = dy_stride - degree * degree;
	const MatViewMut dx = dL_dx ? *dL_dx : MatViewMut{nullptr, 0u, 0u};
	if (fp32) hipLaunchKernelGGL((k_sh_bwd_bwd_input<float>), dim3(div_round_up(n, 128)), dim3(128), 0, stream, n, degree, n_to_pad, norms, x, dL_ddLdx, (const float*)dL_dy, (float*)dL_ddLdy, dy_stride, dx);
	else hipLaunchKernelGGL((k_sh_bwd_bwd_input<half_t>), dim3(div_round_up(n, 128)), dim3(128), 0, stream, n, degree, n_to_pad, norms, x, dL_ddLdx, (const half_t*)dL_dy, (half_t*)dL_ddLdy, dy_stride, dx);
}

namespace {
// composite.h:47-133, one thread per element of the reduced output: the nested values are combined in fp32 in nesting order
template <typename T, bool PRODUCT>
__global__ void __launch_bounds__(256) k_composite_reduce_fwd(const size_t n_elems, const uint32_t n_nested, const T* __restrict__ in, T* __restrict__ out) {
	const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elems) return;
	float result = PRODUCT ? 1.0f : 0.0f;
	for (uint32_t k = 0; k < n_nested; ++k) {
		const float v = (float)in[(size_t)k * n_elems + e];
		if (PRODUCT) result *= v; else result += v;
	}
	out[e] = (T)result;
}

template <typename T, bool PRODUCT>
__global__ void __launch_bounds__(256) k_composite_reduce_bwd(const size_t n_elems, const uint32_t n_nested, const T* __restrict__ in, const T* __restrict__ dL_dout, T* __restrict__ dL_din) {
	const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elems) return;
	const T passed = dL_dout[e];
	for (uint32_t k = 0; k < n_nested; ++k) {
		if (!PRODUCT) {
			dL_din[(size_t)k * n_elems + e] = passed; // :83-86
		} else { // :118-131: the product of the OTHER factors, multiplied up in nesting order (no division)
			float result = (float)passed;
			for (uint32_t l = 0; l + 1 < n_nested; ++l) result *= (float)in[(size_t)(l < k ? l : l + 1) * n_elems + e];
			dL_din[(size_t)k * n_elems + e] = (T)result;
		}
	}
}
// Second-order pass of the Product reduction, one thread per element: with the nested values y_i (`in`), their tangents t_i and d = dL_dout,
//   dL_ddLdout = sum_i t_i P_i,  P_i = prod_{k != i} y_k
//   q_k        = d sum_{i != k} t_i prod_{m not in {i, k}} y_m   (dS/dy_k: what the first-order pass of nested k receives)
// Sums and products in fp32, in nesting order (no division), one rounding per stored value.  Either output may be null.
template <typename T>
__global__ void __launch_bounds__(256) k_composite_reduce_bwd_bwd(const size_t n_elems, const uint32_t n_nested, const T* __restrict__ in, const T* __restrict__ tangents,
                                                                  const T* __restrict__ dL_dout, T* __restrict__ dL_ddLdout, T* __restrict__ q) {
	const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elems) return;
	if (dL_ddLdout) {
		float total = 0;
		for (uint32_t i = 0; i < n_nested; ++i) {
			float term = (float)tangents[(size_t)i * n_elems + e];
			for (uint32_t m = 0; m < n_nested; ++m) {
				if (m != i) term *= (float)in[(size_t)m * n_elems + e];
			}
			total += term;
		}
		dL_ddLdout[e] = (T)total;
	}
	if (q) {
		const float d = (float)dL_dout[e];
		for (uint32_t k = 0; k < n_nested; ++k) {
			float total = 0;
			for (uint32_t i = 0; i < n_nested; ++i) {
				if (i == k) continue;
				float term = (float)tangents[(size_t)i * n_elems + e];
				for (uint32_t m = 0; m < n_nested; ++m) {
					if (m != i && m != k) term *= (float)in[(size_t)m * n_elems + e];
				}
				total += term;
			}
			q[(size_t)k * n_elems + e] = (T)(d * total);
		}
	}
}
} // namespace

void composite_reduce_backward_backward(hipStream_t stream, bool fp32, size_t n_elems, uint32_t n_nested, const void* in, const void* tangents, const void* dL_dout, void* dL_ddLdout, void* q) {
	if (n_elems == 0 || (!dL_ddLdout && !q)) return;
	CHECK_THROW(!q || dL_dout != nullptr);
	const dim3 grid((uint32_t)((n_elems + 255) / 256));
	if (fp32) hipLaunchKernelGGL((k_composite_reduce_bwd_bwd<float>), grid, dim3(256), 0, stream, n_elems, n_nested, (const float*)in, (const float*)tangents, (const float*)dL_dout, (float*)dL_ddLdout, (float*)q);
	else hipLaunchKernelGGL((k_composite_reduce_bwd_bwd<_Float16>), grid, dim3(256), 0, stream, n_elems, n_nested, (const _Float16*)in, (const _Float16*)tangents, (const _Float16*)dL_dout, (_Float16*)dL_ddLdout, (_Float16*)q);
}

void composite_reduce_forward(hipStream_t stream, bool fp32, bool product, size_t n_elems, uint32_t n_nested, const void* in, void* out) {
	if (n_elems == 0) return;
	const dim3 grid((uint32_t)((n_elems + 255) / 256));
	if (fp32) {
		if (product) hipLaunchKernelGGL((k_composite_reduce_fwd<float, true>), grid, dim3(256), 0, stream, n_elems, n_nested, (const float*)in, (float*)out);
		else hipLaunchKernelGGL((k_composite_reduce_fwd<float, false>), grid, dim3(256), 0, stream, n_elems, n_nested, (const float*)in, (float*)out);
	} else {
		if (product) hipLaunchKernelGGL((k_composite_reduce_fwd<_Float16, true>), grid, dim3(256), 0, stream, n_elems, n_nested, (const _Float16*)in, (_Float16*)out);
		else hipLaunchKernelGGL((k_composite_reduce_fwd<_Float16, false>), grid, dim3(256), 0, stream, n_elems, n_nested, (const _Float16*)in, (_Float16*)out);
	}
}

void composite_reduce_backward(hipStream_t stream, bool fp32, bool product, size_t n_elems, uint32_t n_nested, const void* in, const void* dL_dout, void* dL_din) {
	if (n_elems == 0) return;
	const dim3 grid((uint32_t)((n_elems + 255) / 256));
	if (fp32) {
		if (product) hipLaunchKernelGGL((k_composite_reduce_bwd<float, true>), grid, dim3(256), 0, stream, n_elems, n_nested, (const float*)in, (const float*)dL_dout, (float*)dL_din);
		else hipLaunchKernelGGL((k_composite_reduce_bwd<float, false>), grid, dim3(256), 0, stream, n_elems, n_nested, (const float*)in, (const float*)dL_dout, (float*)dL_din);
	} else {
		if (product) hipLaunchKernelGGL((k_composite_reduce_bwd<_Float16, true>), grid, dim3(256), 0, stream, n_elems, n_nested, (const _Float16*)in, (const _Float16*)dL_dout, (_Float16*)dL_din);
		else hipLaunchKernelGGL((k_composite_reduce_bwd<_Float16, false>), grid, dim3(256), 0, stream, n_elems, n_nested, (const _Float16*)in, (const _Float16*)dL_dout, (_Float16*)dL_din);
	}
}

namespace {
// The OneBlob encoding's tangent J v (input_jvp; the encoding has no second-order pass and needs none for this).  One thread per element of
// the padded row: column d * n_bins + b holds (T)(v[d] * k'), where k' = (derivative of C at bin b's left edge) - (at its right edge) is
// formed from the very expressions k_oneblob_bwd_input (k_misc.hip) walks through bin by bin -- its `left` of bin b is its `right` of
// bin b - 1, evaluated at scalbnf(b, -log2_bins), and at bin 0 it reads -x where this reads 0 - x: the quartic squares its argument and
// (+-0) +- 1 is +-1 either way, so every k' has that kernel's bits.  One rounding of the fp32 product; the padding columns are exactly zero.
template <typename T>
__global__ void __launch_bounds__(256) k_oneblob_tangent(const uint32_t n_elements, const uint32_t n_dims, const uint32_t log2_bins, const uint32_t t_stride, const MatView x, const MatView v,
                                                         T* __restrict__ t) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n_elements) return;
	const uint32_t i = e / t_stride, j = e - i * t_stride;
	const uint32_t d = j >> log2_bins, b = j & ((1u << log2_bins) - 1);
	if (d >= n_dims) {
		t[e] = (T)0.0f;
		return;
	}
	const float nb = (float)(1u << log2_bins);
	const float xv = x.data[(size_t)i * x.stride_sample + (size_t)d * x.stride_dim];
	const float lb = scalbnf((float)b, -(int)log2_bins), rb = scalbnf((float)(b + 1), -(int)log2_bins);
	const float left = quartic_cdf_deriv(lb - xv, nb) + quartic_cdf_deriv(lb - xv - 1.0f, nb) + quartic_cdf_deriv(lb - xv + 1.0f, nb);
	const float right = quartic_cdf_deriv(rb - xv, nb) + quartic_cdf_deriv(rb - xv - 1.0f, nb) + quartic_cdf_deriv(rb - xv + 1.0f, nb);
	const float deriv = left - right;
	// the fp32 product as a value of its own: contracted with the conversion into one fused multiply-add onto +0 (v_fma_mixlo_f16), a
	// negative v times k' = 0 would come out as +0 instead of the product's -0
	float product = v.data[(size_t)i * v.stride_sample + (size_t)d * v.stride_dim] * deriv;
	asm volatile("" : "+v"(product));
	t[e] = (T)product;
}
} // namespace

void oneblob_tangent(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_bins, MatView x, MatView v, void* t, uint32_t t_stride) {
	const uint64_t total = (uint64_t)n * t_stride;
	if (total == 0) return;
	CHECK_THROW(total < (1ull << 32) && n_bins > 0 && (n_bins & (n_bins - 1)) == 0 && t_stride >= n_dims * n_bins && x.data && v.data && t);
	uint32_t lb = 0;
	while ((1u << lb) < n_bins) ++lb;
	const dim3 blocks((uint32_t)((total + 255) / 256));
	if (fp32) hipLaunchKernelGGL((k_oneblob_tangent<float>), blocks, dim3(256), 0, stream, (uint32_t)total, n_dims, lb, t_stride, x, v, (float*)t);
	else hipLaunchKernelGGL((k_oneblob_tangent<half_t>), blocks, dim3(256), 0, stream, (uint32_t)total, n_dims, lb, t_stride, x, v, (half_t*)t);
}

} // namespace tcnn_amd
