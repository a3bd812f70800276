// k_mlp_input_jvp.hip -- J(x) v for every output column of the fused fp16 MLP along TT input directions, in ONE kernel (input_jvp).
//
// Forward mode: a tangent chain u_k = a_k'(z_k) (.) (W_k u_{k-1}) multiplies by the same weight fragments in the same order as the forward
// chain h_k = a_k(z_k), z_k = half(W_k h_{k-1}).  So every fragment is read once per layer and feeds the forward matrix instructions and
// then those of the TT tangent chains; a' is read from the pre-activation the wave has just rounded, and nothing is kept across layers but
// the live B operands (hf, uf) -- no transposed image, no stored activation, no kept halves per layer as k_mlp_input_grad needs them.
//
// The forward chain is k_mlp_input_grad's (k_mlp_fwd's): every forward accumulator receives the same matrix instructions in the same
// ascending k-step order from +0, so the output has inference's bits.  Every tangent accumulator starts at +0 too and takes its k-steps in
// ascending order; u = (half)(a'(z) acc) is the one rounding per layer, a' in fp32 (act_d1) from the half pre-activation z -- for ReLU /
// LeakyReLU that is the sign of the half output.  A sample's columns of every product do not depend on its neighbours, so its rows do not
// depend on where in the batch it sits, nor on NB.  The layer-by-layer pass (k_layer_gemm, LG_TANGENT) computes the same values in another
// k-order: the two routes are held to the same accuracy bar, not to each other's bits.
//
// NH (hidden layers) and TT are template parameters: every array below is indexed by compile-time numbers only and lives in registers.
#include "mlp_input_grad_device.h" // layer_base / frag_at, Layer<l>, nb_of: shared with k_mlp_input_grad.hip and k_mlp_input_jacobian.hip

namespace tcnn_amd {
namespace {

struct InputJvpArgs {
	FwdArgs f;              // x / x_f32 / planes, out (optional), image = forward fragments, n; hidden and out_f32 unused
	const half_t* t_half;   // n_t buffers of [n][in_width] half rows one behind the other, or
	MatView t_f32;          // data != nullptr: float [n][..] rows of n_t x f.x_f32_dims values, read as (half)(v * f.x_scale), zero in the padding
	half_t* jvp;            // tangent j of sample s at jvp[s * jvp_stride + j * out_width]
	uint32_t jvp_stride;
	uint32_t n_t;           // tangents of this launch, 1 .. TT: the chains above it run on zeros and store nothing
};

// 8 consecutive features k0 .. k0 + 7 of tangent j of one sample: the B operand of a tangent chain's layer 0
__device__ inline h8 load_tangent(const InputJvpArgs& a, const uint32_t in_w, const uint32_t j, const uint32_t sample, const uint32_t k0) {
	if (a.t_f32.data) {
		h8 v;
		const float* row = a.t_f32.data + (size_t)sample * a.t_f32.stride_sample + (size_t)j * a.f.x_f32_dims;
#pragma unroll
		for (int i = 0; i < 8; ++i) v[i] = k0 + i < a.f.x_f32_dims ? (half_t)(row[k0 + i] * a.f.x_scale) : (half_t)0.0f;
		return v;
	}
	return *(const h8*)(a.t_half + ((size_t)j * a.f.n + sample) * in_w + k0);
}

// one layer's accumulators to the next layer's B operands: z = (half)acc, h = a(z) into hf as activate_pack_inlined packs it, and
// u = (half)(a'(z) tacc) into uf in the same positions
template <int T, int KS, int NB, int TT, int ACT>
__device__ __forceinline__ void pack_jvp_inlined(const f4 (&acc)[T][NB], const f4 (&tacc)[TT][T][NB], h8 (&hf)[KS][NB], h8 (&uf)[TT][KS][NB], const uint32_t act) {
#pragma unroll
	for (int s = 0; s < KS; ++s) {
#pragma unroll
		for (int b = 0; b < NB; ++b) {
#pragma unroll
			for (int half = 0; half < 2; ++half) {
				const int t = 2 * s + half;
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					if (t < T) {
						const int tt = t < T ? t : 0;
						const half_t z = (half_t)acc[tt][b][r];
						hf[s][b][4 * half + r] = act_fwd_t<ACT>(act, z);
						float d1;
						if constexpr (ACT == (int)Activation::ReLU) d1 = z > (half_t)0.0f ? 1.0f : 0.0f;
						else d1 = act_d1(act, (float)z);
#pragma unroll
						for (int j = 0; j < TT; ++j) uf[j][s][b][4 * half + r] = (half_t)(d1 * tacc[j][tt][b][r]);
					} else {
						hf[s][b][4 * half + r] = (half_t)0.0f;
#pragma unroll
						for (int j = 0; j < TT; ++j) uf[j][s][b][4 * half + r] = (half_t)0.0f;
					}
				}
			}
		}
	}
}
// the run-time activation, chosen once per layer with the switch outside the loops (pack_layer in mlp_input_grad_device.h says why)
template <int T, int KS, int NB, int TT, int ACT>
__device__ __forceinline__ void pack_jvp(const f4 (&acc)[T][NB], const f4 (&tacc)[TT][T][NB], h8 (&hf)[KS][NB], h8 (&uf)[TT][KS][NB], const uint32_t act) {
	if constexpr (ACT != -1) {
		pack_jvp_inlined<T, KS, NB, TT, ACT>(acc, tacc, hf, uf, act);
	} else {
		switch (act) {
			case (uint32_t)Activation::ReLU: pack_jvp_inlined<T, KS, NB, TT, -1>(acc, tacc, hf, uf, (uint32_t)Activation::ReLU); break;
			case (uint32_t)Activation::LeakyReLU: pack_jvp_inlined<T, KS, NB, TT, -1>(acc, tacc, hf, uf, (uint32_t)Activation::LeakyReLU); break;
			case (uint32_t)Activation::Exponential: pack_jvp_inlined<T, KS, NB, TT, -1>(acc, tacc, hf, uf, (uint32_t)Activation::Exponential); break;
			case (uint32_t)Activation::Sigmoid: pack_jvp_inlined<T, KS, NB, TT, -1>(acc, tacc, hf, uf, (uint32_t)Activation::Sigmoid); break;
			case (uint32_t)Activation::Squareplus: pack_jvp_inlined<T, KS, NB, TT, -1>(acc, tacc, hf, uf, (uint32_t)Activation::Squareplus); break;
			case (uint32_t)Activation::Softplus: pack_jvp_inlined<T, KS, NB, TT, -1>(acc, tacc, hf, uf, (uint32_t)Activation::Softplus); break;
			case (uint32_t)Activation::Tanh: pack_jvp_inlined<T, KS, NB, TT, -1>(acc, tacc, hf, uf, (uint32_t)Activation::Tanh); break;
			default: pack_jvp_inlined<T, KS, NB, TT, -1>(acc, tacc, hf, uf, (uint32_t)Activation::None); break; // None (a Sine network has no fragment images: never here)
		}
	}
}

template <int W, int NB, int ACT, int NH, int TT>
__global__ void __launch_bounds__(256) k_mlp_input_jvp(const MlpDesc d, const InputJvpArgs a) {
	static_assert(NH >= 1 && NH <= 4, "the layer chain below is written out for 1 .. 4 hidden layers");
	static_assert(TT >= 1 && TT <= (int)MLP_INPUT_JVP_MAX_TT, "tangent chains per launch");
	constexpr int T = W / 16;
	constexpr int KS = (T + 1) / 2;
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t c = lane & 15, q = lane >> 4;
	const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
	const uint32_t n_iters = a.f.n / (16 * NB);
	const uint32_t in_w = d.in_width, out_w = d.out_width;
	const h8* imgf = a.f.image;
	const uint32_t lane16 = lane * 16;

	for (uint32_t it = wave; it < n_iters; it += n_waves) {
		const uint32_t s0 = it * 16 * NB;
		f4 acc[T][NB], tacc[TT][T][NB];
		h8 hf[KS][NB], uf[TT][KS][NB]; // the live B operands: the activated halves and the tangents of the layer below

		// ---- layer 0: B operands from memory, natural k order (k_mlp_fwd)
#pragma unroll
		for (int t = 0; t < T; ++t)
#pragma unroll
			for (int b = 0; b < NB; ++b) {
				acc[t][b] = f4{0, 0, 0, 0};
#pragma unroll
				for (int j = 0; j < TT; ++j) tacc[j][t][b] = f4{0, 0, 0, 0};
			}
		{
			const uint32_t ks0 = d.layers[0].ks_fwd;
			const char* img = layer_base(imgf, d.layers[0].fwd_off);
			for (uint32_t s = 0; s < ks0; ++s) {
				h8 bf[NB], tf[TT][NB];
				const uint32_t k0 = 32 * s + 8 * q;
#pragma unroll
				for (int b = 0; b < NB; ++b) {
					if (k0 < in_w) bf[b] = load_mlp_input(a.f, in_w, s0 + 16 * b + c, k0);
					else bf[b] = h8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
					for (int j = 0; j < TT; ++j) {
						if (k0 < in_w && (uint32_t)j < a.n_t) tf[j][b] = load_tangent(a, in_w, j, s0 + 16 * b + c, k0);
						else tf[j][b] = h8{0, 0, 0, 0, 0, 0, 0, 0};
					}
				}
#pragma unroll
				for (int t = 0; t < T; ++t) {
					const h8 af = frag_at(img, lane16, t * ks0 + s);
#pragma unroll
					for (int b = 0; b < NB; ++b) {
						acc[t][b] = mfma(af, bf[b], acc[t][b]);
#pragma unroll
						for (int j = 0; j < TT; ++j) tacc[j][t][b] = mfma(af, tf[j][b], tacc[j][t][b]);
					}
				}
			}
		}
		pack_jvp<T, KS, NB, TT, ACT>(acc, tacc, hf, uf, d.activation);

		// ---- hidden layers 1 .. NH - 1: chained in registers, one weight fragment ahead; a fragment feeds 1 + TT chains
auto hidden_layer = [&](auto layer) {
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
				for (int b = 0; b < NB; ++b) {
					acc[t][b] = mfma(af[i & 1], hf[s][b], s == 0 ? f4{0, 0, 0, 0} : acc[t][b]);
#pragma unroll
					for (int j = 0; j < TT; ++j) tacc[j][t][b] = mfma(af[i & 1], uf[j][s][b], s == 0 ? f4{0, 0, 0, 0} : tacc[j][t][b]);
				}
			}
			pack_jvp<T, KS, NB, TT, ACT>(acc, tacc, hf, uf, d.activation);
		};
		if constexpr (NH > 1) hidden_layer(Layer<1>{});
		if constexpr (NH > 2) hidden_layer(Layer<2>{});
		if constexpr (NH > 3) hidden_layer(Layer<3>{});

		// ---- output layer, tile by tile (the output width is a run-time number): the output, stored if asked for, and the tangents
		{
			const MlpLayer Lo = d.layers[d.n_layers - 1];
			const char* imgo = layer_base(imgf, Lo.fwd_off);
			for (uint32_t to = 0; 16 * to < out_w; ++to) {
				f4 o[NB], ot[TT][NB];
#pragma unroll
				for (int ks = 0; ks < KS; ++ks) {
					const h8 af = frag_at(imgo, lane16, to * KS + ks);
#pragma unroll
					for (int b = 0; b < NB; ++b) {
						o[b] = mfma(af, hf[ks][b], ks == 0 ? f4{0, 0, 0, 0} : o[b]);
#pragma unroll
						for (int j = 0; j < TT; ++j) ot[j][b] = mfma(af, uf[j][ks][b], ks == 0 ? f4{0, 0, 0, 0} : ot[j][b]);
					}
				}
				const uint32_t j0 = 16 * to + 4 * q;
#pragma unroll
				for (int b = 0; b < NB; ++b) {
					const size_t sample = s0 + 16 * b + c;
					h4 z, v;
					f4 d1;
#pragma unroll
					for (int r = 0; r < 4; ++r) {
						z[r] = (half_t)o[b][r];
						v[r] = activation_fwd(d.output_activation, z[r]);
						d1[r] = act_d1(d.output_activation, (float)z[r]);
					}
					if (a.f.out) *(h4*)(a.f.out + sample * out_w + j0) = v;
#pragma unroll
					for (int j = 0; j < TT; ++j) {
						if ((uint32_t)j < a.n_t) {
							const h4 u = h4{(half_t)(d1[0] * ot[j][b][0]), (half_t)(d1[1] * ot[j][b][1]), (half_t)(d1[2] * ot[j][b][2]), (half_t)(d1[3] * ot[j][b][3])};
							*(h4*)(a.jvp + sample * a.jvp_stride + (size_t)j * out_w + j0) = u;
						}
					}
				}
			}
		}
	}
}

// Column blocks per wave.  One tangent chain: nb_of's, as the input-gradient kernels.  Three: the 4 NB T accumulator registers of a forward
// and three tangent chains and the 4 NB KS operand registers of each must stay within the 512 of a wave -- at 64 and 128 wide with nb_of's
// NB the compiler put 60 to 650 bytes per lane into scratch (every instantiation of both forms), with half of it none does.
constexpr int nb_jvp(int W, int NH, int TT) { return TT == 1 || W < 64 ? nb_of(W, NH) : nb_of(W, NH) / 2; }

// the instantiations: widths 16 .. 128, 1 .. MLP_INPUT_GRAD_MAX_HIDDEN hidden layers, ReLU | run-time activation, TT = 1 | 3
template <int W, int NH, int TT>
void launch_act(hipStream_t stream, const MlpDesc& d, const InputJvpArgs& a, const MlpInputJvpPlan& p) {
	constexpr int NB = nb_jvp(W, NH, TT);
	CHECK_THROW(p.nb == (uint32_t)NB && a.n_t >= 1 && a.n_t <= (uint32_t)TT);
	if (p.relu) hipLaunchKernelGGL((k_mlp_input_jvp<W, NB, (int)Activation::ReLU, NH, TT>), dim3(p.grid), dim3(256), 0, stream, d, a);
	else hipLaunchKernelGGL((k_mlp_input_jvp<W, NB, -1, NH, TT>), dim3(p.grid), dim3(256), 0, stream, d, a);
}

template <int W, int TT>
void launch_depth(hipStream_t stream, const MlpDesc& d, const InputJvpArgs& a, const MlpInputJvpPlan& p) {
	static_assert(MLP_INPUT_GRAD_MAX_HIDDEN == 4, "one case per instantiated depth");
	switch (d.n_hidden) {
		case 1: return launch_act<W, 1, TT>(stream, d, a, p);
		case 2: return launch_act<W, 2, TT>(stream, d, a, p);
		case 3: return launch_act<W, 3, TT>(stream, d, a, p);
		case 4: return launch_act<W, 4, TT>(stream, d, a, p);
		default: throw std::runtime_error{"mlp_input_jvp: no kernel for this depth"};
	}
}

template <int TT>
void launch_width(hipStream_t stream, const MlpDesc& d, const InputJvpArgs& a, const MlpInputJvpPlan& p) {
	switch (d.width) {
		case 16: return launch_depth<16, TT>(stream, d, a, p);
		case 32: return launch_depth<32, TT>(stream, d, a, p);
		case 64: return launch_depth<64, TT>(stream, d, a, p);
		case 128: return launch_depth<128, TT>(stream, d, a, p);
		default: throw std::runtime_error{"mlp_input_jvp: no kernel for this width"};
	}
}

} // namespace

MlpInputJvpPlan mlp_input_jvp_plan(const MlpDesc& d, bool layerwise, uint32_t n, uint32_t n_tangents) {
	MlpInputJvpPlan p;
	if (n_tangents == 0) return p;
	if (layerwise || d.n_frags_fwd == 0) return p; // no fragment images: fp32, Sine, zero hidden layers, other widths, TCNN_AMD_MLP_LAYERWISE=1
	if (d.width != 16 && d.width != 32 && d.width != 64 && d.width != 128) return p; // (256: see nb_of)
	if (d.n_hidden < 1 || d.n_hidden > MLP_INPUT_GRAD_MAX_HIDDEN) return p;
	const uint32_t tt = n_tangents == 1 ? 1u : MLP_INPUT_JVP_MAX_TT; // two tangents: one launch of the three-chain form, the third chain on zeros
	const uint32_t nb = (uint32_t)nb_jvp((int)d.width, (int)d.n_hidden, (int)tt);
	if (n == 0 || n % (16 * nb) != 0) return p;
	const uint32_t wgs = div_round_up(n / (16 * nb), 4u); // four waves per workgroup, one trip each up to 8 workgroups per CU (k_mlp.hip mlp_grid)
	// Measured (DESIGN.md "input_jvp / The plan rule"; tools/bench_input_jvp.py; profiles/input_jvp_bench.txt section 2): in every class
	// instantiated here the kernel is faster than input_jvp's own two-pass route by far more than 3 %, the spread between boxes -- the
	// smallest gain is 1.31 (Softplus 32 x 1, one tangent, 2^18 rows) -- so no class keeps the two passes.
	p.fused = true;
	p.nb = nb;
	p.relu = d.activation == (uint32_t)Activation::ReLU;
	p.tt = tt;
	p.grid = std::min<uint32_t>(wgs, 256 * 8);
	snprintf(p.name, sizeof(p.name), "k_mlp_input_jvp<%u,%u,%u,%u>/%s", d.width, nb, d.n_hidden, p.tt, p.relu ? "relu" : "act");
	return p;
}

void mlp_input_jvp(hipStream_t stream, const MlpDesc& d, const MlpInputJvpPlan& p, const void* image, uint32_t n, const MlpIo& io, const void* tangents, MatView tangents_f32,
                   uint32_t n_tangents, void* jvp, uint32_t jvp_stride) {
	CHECK_THROW(p.fused && p.nb > 0 && (p.tt == 1 || p.tt == MLP_INPUT_JVP_MAX_TT) && n % (16 * p.nb) == 0 && n % BATCH_SIZE_GRANULARITY == 0);
	CHECK_THROW(n_tangents > 0 && jvp != nullptr && jvp_stride >= n_tangents * d.out_width && jvp_stride % 4 == 0);
	CHECK_THROW((io.x_half != nullptr || io.x_f32.data != nullptr) && io.x_oneblob_bins == 0 && io.out_f32.data == nullptr);
	CHECK_THROW((tangents != nullptr) != (tangents_f32.data != nullptr)); // one form
	if (tangents_f32.data) CHECK_THROW(io.x_f32.data != nullptr && tangents_f32.stride_dim == 1 && tangents_f32.stride_sample >= n_tangents * io.x_f32_dims);
	if (n == 0) return;
	InputJvpArgs a{};
	a.f = FwdArgs{(const half_t*)io.x_half, (half_t*)io.out_half, nullptr, (const h8*)image, n, io.x_plane_features, io.x_f32, io.x_f32_dims, io.x_scale, io.x_offset, 0u, MatViewMut{}, 0u};
	a.jvp_stride = jvp_stride;
	for (uint32_t t0 = 0; t0 < n_tangents; t0 += p.tt) { // more tangents than a launch carries: further launches, each with its own forward chain
		a.n_t = std::min(n_tangents - t0, p.tt);
		a.t_half = tangents ? (const half_t*)tangents + (size_t)t0 * n * d.in_width : nullptr;
		a.t_f32 = tangents_f32;
		if (tangents_f32.data) a.t_f32.data = tangents_f32.data + (size_t)t0 * io.x_f32_dims;
		a.jvp = (half_t*)jvp + (size_t)t0 * d.out_width;
		if (t0 > 0) a.f.out = nullptr; // the first launch has stored it
		if (p.tt == 1) launch_width<1>(stream, d, a, p);
		else launch_width<(int)MLP_INPUT_JVP_MAX_TT>(stream, d, a, p);
		HIP_CHECK_THROW(hipGetLastError());
	}
}

} // namespace tcnn_amd
