// k_mlp_input_jacobian.hip -- d output[d_k] / d (MLP input) for K output columns at inference in ONE kernel: k_mlp_input_grad
// (k_mlp_input_grad.hip) with the forward chain shared.  Per wave and 16 NB samples the forward chain runs once and every hidden layer's
// activated halves stay in registers (`kept`, live across the backward chain in k_mlp_input_grad already); then, for each of the K dims,
// the output-tile section (output products, output activation, the seed on row d_k through activation_bwd, Wout^T dY by k-step), the
// backward chain on the kept halves and the store into buffer k.  The output is stored with the first dim only.  Recomputing the output
// tiles per dim costs out_width / 16 * KS matrix instructions and keeps the register picture of k_mlp_input_grad.
//
// Same bits as K launches of k_mlp_input_grad: every accumulator of a dim's pass receives that kernel's matrix instructions from +0 in
// the same ascending order, on the same kept halves; nothing of one dim's pass reaches the next but `kept`, which no pass writes.
#include "mlp_input_grad_device.h"

namespace tcnn_amd {
namespace {

struct InputJacobianArgs {
	FwdArgs f;            // x / x_f32 / planes, out (optional), image = forward fragments, n; hidden and out_f32 unused
	const h8* image_bwd;  // backward fragments
	half_t* dL_dx;        // n_dims buffers, one behind the other, each [n][in_width] or level planes when dx_plane_f > 0
	uint32_t dx_plane_f;
	uint32_t n_dims;      // 1 .. MLP_INPUT_JACOBIAN_MAX_DIMS
	half_t seed;          // (half)backprop_scale
	uint32_t dims[MLP_INPUT_JACOBIAN_MAX_DIMS]; // the output columns differentiated (< out_width)
};

template <int KS, int NB>
__device__ __forceinline__ void opaque(h8 (&hf)[KS][NB]) {
#pragma unroll
	for (int s = 0; s < KS; ++s)
#pragma unroll
		for (int b = 0; b < NB; ++b) asm volatile("" : "+v"(hf[s][b]));
}

template <int W, int NB, int ACT, int NH>
__global__ void __launch_bounds__(256) k_mlp_input_jacobian(const MlpDesc d, const InputJacobianArgs a) {
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
	const size_t dx_elems = (size_t)a.f.n * in_w; // one dim's buffer

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

		// ---- one pass per dim on the kept halves (a run-time loop: the dims are the kernel's arguments)
		for (uint32_t k = 0; k < a.n_dims; ++k) {
			const uint32_t dim = a.dims[k];
			half_t* const out = k == 0 ? a.f.out : nullptr;
			half_t* const dx = a.dL_dx + k * dx_elems;
			// Nothing computed from `kept` may count as invariant in this loop: left alone, the compiler hoists every act'(kept) of the backward
			// chain and the output tiles out of it and keeps them across it -- for ReLU one lane mask (an SGPR pair) per kept register, 301
			// SGPRs spilled at 32 x 4; for the run-time form a derivative per kept half, 1688 bytes of scratch at 32 x 4.  So each layer's kept
			// halves pass through an empty asm statement (no instruction) where a dim's pass first reads them: here and in backward_layer.
			opaque(kept[NH - 1]);

			// output tiles, two per k-step of Wout^T dY: the output (stored if asked for), the one-hot seed through the output activation's
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
								if (out) *(h4*)(out + (size_t)(s0 + 16 * b + c) * out_w + j0) = v;
#pragma unroll
								for (int r = 0; r < 4; ++r) {
									half_t g = j0 + r == dim ? a.seed : (half_t)0.0f;
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

			// backward chain on the kept halves (k_mlp_bwd): dH_l = act'(H_l) (W_{l+1}^T dH_{l+1})
			h8 hf[KS][NB];
auto backward_layer = [&](auto layer) {
				constexpr int l = decltype(layer)::value;
				if constexpr (l < NH - 1) opaque(kept[l]);
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

			// dX = W0^T dH_0, in_width / 16 row tiles, into buffer k
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
						store_dx(dx, a.dx_plane_f, a.f.n, in_w, s0 + 16 * b + c, 16 * ti + 4 * q, v);
					}
				}
			}
		}
	}
}

// the instantiations of k_mlp_input_grad: widths 16 .. 128, 1 .. MLP_INPUT_GRAD_MAX_HIDDEN hidden layers, ReLU | run-time activation, its NB
template <int W, int NH>
void launch_act(hipStream_t stream, const MlpDesc& d, const InputJacobianArgs& a, const MlpInputGradPlan& p) {
	constexpr int NB = nb_of(W, NH);
	CHECK_THROW(p.nb == (uint32_t)NB);
	if (p.relu) hipLaunchKernelGGL((k_mlp_input_jacobian<W, NB, (int)Activation::ReLU, NH>), dim3(p.grid), dim3(256), 0, stream, d, a);
	else hipLaunchKernelGGL((k_mlp_input_jacobian<W, NB, -1, NH>), dim3(p.grid), dim3(256), 0, stream, d, a);
}

template <int W>
void launch_depth(hipStream_t stream, const MlpDesc& d, const InputJacobianArgs& a, const MlpInputGradPlan& p) {
	static_assert(MLP_INPUT_GRAD_MAX_HIDDEN == 4, "one case per instantiated depth");
	switch (d.n_hidden) {
		case 1: return launch_act<W, 1>(stream, d, a, p);
		case 2: return launch_act<W, 2>(stream, d, a, p);
		case 3: return launch_act<W, 3>(stream, d, a, p);
		case 4: return launch_act<W, 4>(stream, d, a, p);
		default: throw std::runtime_error{"mlp_input_jacobian: no kernel for this depth"};
	}
}

} // namespace

MlpInputGradPlan mlp_input_jacobian_plan(const MlpDesc& d, bool layerwise, uint32_t n, uint32_t n_dims) {
	MlpInputGradPlan p;
	if (n_dims == 0) return p;
	if (layerwise || d.n_frags_fwd == 0 || d.n_frags_bwd == 0) return p; // no fragment images: fp32, Sine, zero hidden layers, other widths, TCNN_AMD_MLP_LAYERWISE=1
	if (d.width != 16 && d.width != 32 && d.width != 64 && d.width != 128) return p; // (256: see nb_of)
	if (d.n_hidden < 1 || d.n_hidden > MLP_INPUT_GRAD_MAX_HIDDEN) return p;
	const uint32_t nb = (uint32_t)nb_of((int)d.width, (int)d.n_hidden);
	if (n == 0 || n % (16 * nb) != 0) return p;
	const bool relu = d.activation == (uint32_t)Activation::ReLU;
	const uint32_t wgs = div_round_up(n / (16 * nb), 4u); // four waves per workgroup, one trip each up to 8 workgroups per CU (k_mlp.hip mlp_grid)
	// Measured (DESIGN.md "input_jacobian"; tools/bench_input_jacobian.py): the classes in which the fused kernel is not faster than the
	// Jacobian's own two-pass route by more than 3 %, the spread between boxes, keep the two passes.
	// The run-time activation form with more workgroups than CUs: its backward chain runs at one wave per SIMD (up to 423 registers),
	// k_mlp_bwd's does not, and every further dim adds a backward chain but no forward chain.  ACT_MAX_DIMS[width][depth] is the largest
	// n_dims at which the fused kernel measured faster (2^18 rows; 0: never, ~0u: at every n_dims measured, 1 .. 16).  With one workgroup
	// per CU or fewer (measured at 2^15 and 2^16 rows) one launch instead of 1 + 2 n_dims decides, at every n_dims.
	static constexpr uint32_t ANY = ~0u;
	static constexpr uint32_t ACT_MAX_DIMS[4][MLP_INPUT_GRAD_MAX_HIDDEN] = {
		{ANY, ANY, ANY, 0}, // 16 wide, 1 .. 4 hidden layers
		{ANY, ANY, 1, 0},   // 32
		{3, 2, 2, 2},       // 64
		{2, 1, 1, 1},       // 128
	};
	const uint32_t wi = d.width == 16 ? 0 : d.width == 32 ? 1 : d.width == 64 ? 2 : 3;
	if (!relu && wgs > 256 && n_dims > ACT_MAX_DIMS[wi][d.n_hidden - 1]) return p;
	// The ReLU form is faster in every class measured (1.20 to 1.64 at 3 dims, 1.10 to 1.48 at 16; 2^18 rows) but one: 128 x 2 at 2^20 rows
	// took 5.02 ms against 5.07 and 5.01 against 5.17 at 16 dims (1.011, 1.033), 1.041 at 8 dims, 1.08 to 1.13 at 3.
	if (relu && d.width == 128 && d.n_hidden == 2 && n >= (1u << 20) && n_dims > 8) return p;
	p.fused = true;
	p.nb = nb;
	p.relu = relu;
	p.grid = std::min<uint32_t>(wgs, 256 * 8);
	snprintf(p.name, sizeof(p.name), "k_mlp_input_jacobian<%u,%u,%u>/%s", d.width, nb, d.n_hidden, p.relu ? "relu" : "act");
	return p;
}

void mlp_input_jacobian(hipStream_t stream, const MlpDesc& d, const MlpInputGradPlan& p, const void* image, uint32_t n, const MlpIo& io, const uint32_t* dims, uint32_t n_dims,
                        float backprop_scale, void* dL_dx, uint32_t dx_plane_features) {
	CHECK_THROW(p.fused && p.nb > 0 && n % (16 * p.nb) == 0 && n % BATCH_SIZE_GRANULARITY == 0);
	CHECK_THROW(dims != nullptr && n_dims > 0 && dL_dx != nullptr);
	CHECK_THROW((io.x_half != nullptr || io.x_f32.data != nullptr) && io.x_oneblob_bins == 0 && io.out_f32.data == nullptr);
	for (uint32_t k = 0; k < n_dims; ++k) CHECK_THROW(dims[k] < d.out_width);
	if (n == 0) return;
	InputJacobianArgs a{};
	a.f = FwdArgs{(const half_t*)io.x_half, (half_t*)io.out_half, nullptr, (const h8*)image, n, io.x_plane_features, io.x_f32, io.x_f32_dims, io.x_scale, io.x_offset, 0u, MatViewMut{}, 0u};
	a.image_bwd = (const h8*)((const char*)image + (size_t)d.n_frags_fwd * 1024);
	a.dx_plane_f = dx_plane_features;
	a.seed = (half_t)backprop_scale;
	for (uint32_t k0 = 0; k0 < n_dims; k0 += MLP_INPUT_JACOBIAN_MAX_DIMS) { // more dims than a launch carries: further launches, each with its own forward chain
		a.n_dims = std::min(n_dims - k0, MLP_INPUT_JACOBIAN_MAX_DIMS);
		for (uint32_t k = 0; k < a.n_dims; ++k) a.dims[k] = dims[k0 + k];
		a.dL_dx = (half_t*)dL_dx + (size_t)k0 * n * d.in_width;
		if (k0 > 0) a.f.out = nullptr; // the first launch has stored it
		switch (d.width) {
			case 16: launch_depth<16>(stream, d, a, p); break;
			case 32: launch_depth<32>(stream, d, a, p); break;
			case 64: launch_depth<64>(stream, d, a, p); break;
			case 128: launch_depth<128>(stream, d, a, p); break;
			default: throw std::runtime_error{"mlp_input_jacobian: no kernel for this width"};
		}
		HIP_CHECK_THROW(hipGetLastError());
	}
}

} // namespace tcnn_amd
