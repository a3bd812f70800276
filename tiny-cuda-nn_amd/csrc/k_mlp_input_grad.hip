// k_mlp_input_grad.hip -- d output[dim] / d (MLP input) at inference in ONE kernel (object.h:342-366 input_gradient, for the fused fp16 MLP).
//
// What Network::forward + Network::backward(GradientMode::Ignore) compute from a one-hot dL/dy, without their traffic: k_mlp_fwd stores
// every hidden activation, k_mlp_bwd reads them back and writes dhidden for a weight-gradient product that never runs.  The lane layout
// of a forward result tile (lane & 15 = sample, 4 (lane >> 4) + r = feature) is the layout in which k_mlp_bwd reads the stored
// activation (16 c + 4 q), so a wave keeps every layer's activated halves in registers, seeds the one-hot on the output tile it has
// just computed and runs the backward chain on what it kept.  It stores dL/d(MLP input), and the output where asked for.
//
// Same bits as the two kernels: every accumulator receives the matrix instructions of k_mlp_fwd / k_mlp_bwd in their ascending k-step
// order from +0, a sample's column of a product does not depend on its neighbours (so NB is free), the halves kept are the halves
// k_mlp_fwd stores, and the output activation's derivative is activation_bwd on the half output, as k_act_bwd_output applies it to every
// padded column in front of k_mlp_bwd.
//
// NH (hidden layers) is a template parameter: `kept` indexed by a run-time layer number would live in scratch.
#include "mlp_input_grad_device.h" // pack_layer, layer_base / frag_at, Layer<l>, nb_of: shared with k_mlp_input_jacobian.hip

namespace tcnn_amd {
namespace {

struct InputGradArgs {
	FwdArgs f;            // x / x_f32 / planes, out (optional), image = forward fragments, n; hidden and out_f32 unused
	const h8* image_bwd;  // backward fragments
	half_t* dL_dx;        // [n][in_width], or level planes when dx_plane_f > 0
	uint32_t dx_plane_f;
	uint32_t dim;         // the output column differentiated (< out_width)
	half_t seed;          // (half)backprop_scale
};

template <int W, int NB, int ACT, int NH>
__global__ void __launch_bounds__(256) k_mlp_input_grad(const MlpDesc d, const InputGradArgs a) {
	static_assert(NH >= 1 && NH <= 4, "the layer chains below are written out for 1 .. 4 hidden layers");
	constexpr int T = W / 16;
	constexpr int KS = (T + 1) / 2;
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t c = lane & 15, q = lane >> 4;
	const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
	const uint32_t n_iters = a.f.n / (16 * NB);
	const uint32_t in_w = d.in_width, out_w = d.out_width;
	const h8* imgf = a.f.image;
	const h8* imgb = a.image_bwd;
	const uint32_t lane16 = lane * 16;

	for (uint32_t it = wave; it < n_iters; it += n_waves) {
		const uint32_t s0 = it * 16 * NB;
		f4 acc[T][NB];
		h8 kept[NH][KS][NB]; // the activated halves of every hidden layer: what k_mlp_fwd stores and k_mlp_bwd reads back

		// ---- forward, layer 0: B operand from memory, natural k order (k_mlp_fwd)
#pragma unroll
		for (int t = 0; t < T; ++t)
#pragma unroll
			for (int b = 0; b < NB; ++b) acc[t][b] = f4{0, 0, 0, 0};
		{
			const uint32_t ks0 = d.layers[0].ks_fwd;
			const char* img = layer_base(imgf, d.layers[0].fwd_off);
			for (uint32_t s = 0; s < ks0; ++s) {
				h8 bf[NB];
				const uint32_t k0 = 32 * s + 8 * q;
#pragma unroll
				for (int b = 0; b < NB; ++b) {
					if (k0 < in_w) bf[b] = load_mlp_input(a.f, in_w, s0 + 16 * b + c, k0);
					else bf[b] = h8{0, 0, 0, 0, 0, 0, 0, 0};
				}
#pragma unroll
				for (int t = 0; t < T; ++t) {
					const h8 af = frag_at(img, lane16, t * ks0 + s);
#pragma unroll
					for (int b = 0; b < NB; ++b) acc[t][b] = mfma(af, bf[b], acc[t][b]);
				}
			}
		}
		pack_layer<T, KS, NB, ACT>(acc, kept[0], d.activation);

		// ---- forward, hidden layers 1 .. NH - 1: chained in registers, one weight fragment ahead
auto forward_layer = [&](auto layer) {
			constexpr int l = decltype(layer)::value;
			const char* img = layer_base(imgf, d.layers[l].fwd_off);
			auto frag_of = [&](const int i) -> h8 { return frag_at(img, lane16, (i % T) * KS + i / T); };
			h8 af[2];
			af[0] = frag_of(0);
#pragma unroll
			for (int i = 0; i < KS * T; ++i) {
				const int s = i / T, t = i % T;
				if (i + 1 < KS * T) af[(i + 1) & 1] = frag_of(i + 1);
#pragma unroll
				for (int b = 0; b < NB; ++b) acc[t][b] = mfma(af[i & 1], kept[l - 1][s][b], s == 0 ? f4{0, 0, 0, 0} : acc[t][b]);
			}
			pack_layer<T, KS, NB, ACT>(acc, kept[l], d.activation);
		};
		if constexpr (NH > 1) forward_layer(Layer<1>{});
		if constexpr (NH > 2) forward_layer(Layer<2>{});
		if constexpr (NH > 3) forward_layer(Layer<3>{});

		// ---- output tiles, two per k-step of Wout^T dY: the output (stored if asked for), the one-hot seed through the output activation's
		// derivative, and that k-step's products into dH_last -- tile by tile, so that no array is indexed by the run-time output width
#pragma unroll
		for (int t = 0; t < T; ++t)
#pragma unroll
			for (int b = 0; b < NB; ++b) acc[t][b] = f4{0, 0, 0, 0};
		{
			const MlpLayer Lo = d.layers[d.n_layers - 1];
			const uint32_t kso = Lo.ks_bwd;
			const char* imgo = layer_base(imgf, Lo.fwd_off);
			const char* imgt = layer_base(imgb, Lo.bwd_off);
			for (uint32_t s = 0; s < kso; ++s) {
				h8 bf[NB];
#pragma unroll
				for (int half = 0; half < 2; ++half) {
					const uint32_t to = 2 * s + half;
					if (16 * to < out_w) { // wave-uniform
						f4 o[NB];
#pragma unroll
						for (int ks = 0; ks < KS; ++ks) {
							const h8 af = frag_at(imgo, lane16, to * KS + ks);
#pragma unroll
							for (int b = 0; b < NB; ++b) o[b] = mfma(af, kept[NH - 1][ks][b], ks == 0 ? f4{0, 0, 0, 0} : o[b]);
						}
						const uint32_t j0 = 16 * to + 4 * q;
#pragma unroll
						for (int b = 0; b < NB; ++b) {
							h4 v;
#pragma unroll
							for (int r = 0; r < 4; ++r) v[r] = activation_fwd(d.output_activation, (half_t)o[b][r]);
							if (a.f.out) *(h4*)(a.f.out + (size_t)(s0 + 16 * b + c) * out_w + j0) = v;
#pragma unroll
							for (int r = 0; r < 4; ++r) {
								half_t g = j0 + r == a.dim ? a.seed : (half_t)0.0f;
								if (d.output_activation != (uint32_t)Activation::None) g = activation_bwd(d.output_activation, g, v[r]);
								bf[b][4 * half + r] = g;
							}
						}
					} else {
#pragma unroll
						for (int b = 0; b < NB; ++b)
#pragma unroll
							for (int r = 0; r < 4; ++r) bf[b][4 * half + r] = (half_t)0.0f;
					}
				}
#pragma unroll
				for (int t = 0; t < T; ++t) {
					const h8 af = frag_at(imgt, lane16, t * kso + s);
#pragma unroll
					for (int b = 0; b < NB; ++b) acc[t][b] = mfma(af, bf[b], acc[t][b]);
				}
			}
		}

		// ---- backward chain on the kept halves (k_mlp_bwd): dH_l = act'(H_l) (W_{l+1}^T dH_{l+1})
		h8 hf[KS][NB];
auto backward_layer = [&](auto layer) {
			constexpr int l = decltype(layer)::value;
#pragma unroll
			for (int t = 0; t < T; ++t)
#pragma unroll
				for (int b = 0; b < NB; ++b)
#pragma unroll
					for (int r = 0; r < 4; ++r) hf[t / 2][b][(t & 1) * 4 + r] = act_bwd_t<ACT>(d.activation, (half_t)acc[t][b][r], kept[l][t / 2][b][(t & 1) * 4 + r]);
			if constexpr (T & 1) {
#pragma unroll
				for (int b = 0; b < NB; ++b)
#pragma unroll
					for (int r = 0; r < 4; ++r) hf[KS - 1][b][4 + r] = (half_t)0.0f;
			}
			if constexpr (l > 0) {
				const char* img = layer_base(imgb, d.layers[l].bwd_off);
#pragma unroll
				for (int t = 0; t < T; ++t)
#pragma unroll
					for (int b = 0; b < NB; ++b) acc[t][b] = f4{0, 0, 0, 0};
				auto frag_of = [&](const int i) -> h8 { return frag_at(img, lane16, (i % T) * KS + i / T); };
				h8 af[2];
				af[0] = frag_of(0);
#pragma unroll
				for (int i = 0; i < KS * T; ++i) {
					const int s = i / T, t = i % T;
					if (i + 1 < KS * T) af[(i + 1) & 1] = frag_of(i + 1);
#pragma unroll
					for (int b = 0; b < NB; ++b) acc[t][b] = mfma(af[i & 1], hf[s][b], acc[t][b]);
				}
			}
		};
		if constexpr (NH > 3) backward_layer(Layer<3>{});
		if constexpr (NH > 2) backward_layer(Layer<2>{});
		if constexpr (NH > 1) backward_layer(Layer<1>{});
		backward_layer(Layer<0>{});

		// ---- dX = W0^T dH_0, in_width / 16 row tiles
		{
			const char* img = layer_base(imgb, d.layers[0].bwd_off);
			for (uint32_t ti = 0; ti < in_w / 16; ++ti) {
				f4 o[NB];
#pragma unroll
				for (int b = 0; b < NB; ++b) o[b] = f4{0, 0, 0, 0};
#pragma unroll
				for (int s = 0; s < KS; ++s) {
					const h8 af = frag_at(img, lane16, ti * KS + s);
#pragma unroll
					for (int b = 0; b < NB; ++b) o[b] = mfma(af, hf[s][b], o[b]);
				}
#pragma unroll
				for (int b = 0; b < NB; ++b) {
					const h4 v = h4{(half_t)o[b][0], (half_t)o[b][1], (half_t)o[b][2], (half_t)o[b][3]};
					store_dx(a.dL_dx, a.dx_plane_f, a.f.n, in_w, s0 + 16 * b + c, 16 * ti + 4 * q, v);
				}
			}
		}
	}
}

template <typename T>
__global__ void __launch_bounds__(256) k_one_hot(const size_t n_elems, const uint32_t width, const uint32_t dim, const float scale, T* __restrict__ out) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elems) return;
	out[i] = (uint32_t)(i % width) == dim ? (T)scale : (T)0.0f;
}

__global__ void __launch_bounds__(256) k_rescale(const size_t n_elems, const uint32_t dims, const float mult, const MatViewMut m) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elems) return;
	const size_t s = i / dims, j = i - s * dims;
	m.data[s * m.stride_sample + j * m.stride_dim] *= mult;
}

// the instantiations: widths 16 .. 128, 1 .. MLP_INPUT_GRAD_MAX_HIDDEN hidden layers, ReLU | run-time activation, NB as the two-pass kernels have it (nb_of)
template <int W, int NH>
void launch_act(hipStream_t stream, const MlpDesc& d, const InputGradArgs& a, const MlpInputGradPlan& p) {
	constexpr int NB = nb_of(W, NH);
	CHECK_THROW(p.nb == (uint32_t)NB);
	if (p.relu) hipLaunchKernelGGL((k_mlp_input_grad<W, NB, (int)Activation::ReLU, NH>), dim3(p.grid), dim3(256), 0, stream, d, a);
	else hipLaunchKernelGGL((k_mlp_input_grad<W, NB, -1, NH>), dim3(p.grid), dim3(256), 0, stream, d, a);
}

template <int W>
void launch_depth(hipStream_t stream, const MlpDesc& d, const InputGradArgs& a, const MlpInputGradPlan& p) {
	static_assert(MLP_INPUT_GRAD_MAX_HIDDEN == 4, "one case per instantiated depth");
	switch (d.n_hidden) {
		case 1: return launch_act<W, 1>(stream, d, a, p);
		case 2: return launch_act<W, 2>(stream, d, a, p);
		case 3: return launch_act<W, 3>(stream, d, a, p);
		case 4: return launch_act<W, 4>(stream, d, a, p);
		default: throw std::runtime_error{"mlp_input_gradient: no kernel for this depth"};
	}
}

} // namespace

void input_gradient_one_hot(hipStream_t stream, Precision precision, uint32_t n, uint32_t width, uint32_t dim, float backprop_scale, void* d_doutput) {
	const size_t n_elems = (size_t)n * width;
	if (n_elems == 0) return;
	CHECK_THROW(n_elems < (1ull << 39));
	const dim3 grid((uint32_t)((n_elems + 255) / 256));
	if (precision == Precision::Fp16) hipLaunchKernelGGL(k_one_hot<half_t>, grid, dim3(256), 0, stream, n_elems, width, dim, backprop_scale, (half_t*)d_doutput);
	else hipLaunchKernelGGL(k_one_hot<float>, grid, dim3(256), 0, stream, n_elems, width, dim, backprop_scale, (float*)d_doutput);
	HIP_CHECK_THROW(hipGetLastError());
}

void input_gradient_rescale(hipStream_t stream, uint32_t n, uint32_t dims, float mult, MatViewMut d_dinput) {
	const size_t n_elems = (size_t)n * dims;
	if (n_elems == 0) return;
	hipLaunchKernelGGL(k_rescale, dim3((uint32_t)((n_elems + 255) / 256)), dim3(256), 0, stream, n_elems, dims, mult, d_dinput);
	HIP_CHECK_THROW(hipGetLastError());
}

MlpInputGradPlan mlp_input_gradient_plan(const MlpDesc& d, bool layerwise, uint32_t n) {
	MlpInputGradPlan p;
	if (layerwise || d.n_frags_fwd == 0 || d.n_frags_bwd == 0) return p; // no fragment images: fp32, Sine, zero hidden layers, other widths, TCNN_AMD_MLP_LAYERWISE=1
	if (d.width != 16 && d.width != 32 && d.width != 64 && d.width != 128) return p; // (256: see nb_of)
	if (d.n_hidden < 1 || d.n_hidden > MLP_INPUT_GRAD_MAX_HIDDEN) return p;
	const uint32_t nb = (uint32_t)nb_of((int)d.width, (int)d.n_hidden);
	if (n == 0 || n % (16 * nb) != 0) return p;
	const bool relu = d.activation == (uint32_t)Activation::ReLU;
	const uint32_t wgs = div_round_up(n / (16 * nb), 4u); // four waves per workgroup, one trip each up to 8 workgroups per CU (k_mlp.hip mlp_grid)
	// Measured (DESIGN.md "input_gradient"): 128 x 4 ReLU at 2^20 rows takes 0.901 ms fused against 0.904 ms in two passes -- no gain beyond the
	// spread between boxes, so this class keeps the two passes: 128 wide, the compiled ReLU form, 3 or 4 hidden layers, a full machine (the
	// grid at its cap: 2^18 rows and up).  Below that the one launch instead of five decides, and the run-time form gains 20 % at any size.
	if (d.width == 128 && relu && d.n_hidden >= 3 && wgs >= 256 * 8) return p;
	p.fused = true;
	p.nb = nb;
	p.relu = relu;
	p.grid = std::min<uint32_t>(wgs, 256 * 8);
	snprintf(p.name, sizeof(p.name), "k_mlp_input_grad<%u,%u,%u>/%s", d.width, nb, d.n_hidden, p.relu ? "relu" : "act");
	return p;
}

void mlp_input_gradient(hipStream_t stream, const MlpDesc& d, const MlpInputGradPlan& p, const void* image, uint32_t n, const MlpIo& io, uint32_t dim, float backprop_scale,
                        void* dL_dx, uint32_t dx_plane_features) {
	CHECK_THROW(p.fused && p.nb > 0 && n % (16 * p.nb) == 0 && n % BATCH_SIZE_GRANULARITY == 0);
	CHECK_THROW(dim < d.out_width && dL_dx != nullptr);
	CHECK_THROW((io.x_half != nullptr || io.x_f32.data != nullptr) && io.x_oneblob_bins == 0 && io.out_f32.data == nullptr);
	if (n == 0) return;
	InputGradArgs a{};
	a.f = FwdArgs{(const half_t*)io.x_half, (half_t*)io.out_half, nullptr, (const h8*)image, n, io.x_plane_features, io.x_f32, io.x_f32_dims, io.x_scale, io.x_offset, 0u, MatViewMut{}, 0u};
	a.image_bwd = (const h8*)((const char*)image + (size_t)d.n_frags_fwd * 1024);
	a.dL_dx = (half_t*)dL_dx;
	a.dx_plane_f = dx_plane_features;
	a.dim = dim;
	a.seed = (half_t)backprop_scale;
	switch (d.width) {
		case 16: launch_depth<16>(stream, d, a, p); break;
		case 32: launch_depth<32>(stream, d, a, p); break;
		case 64: launch_depth<64>(stream, d, a, p); break;
		case 128: launch_depth<128>(stream, d, a, p); break;
		default: throw std::runtime_error{"mlp_input_gradient: no kernel for this width"};
	}
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace tcnn_amd
