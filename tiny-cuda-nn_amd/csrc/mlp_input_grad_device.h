// mlp_input_grad_device.h -- the three devices that keep k_mlp_input_grad (k_mlp_input_grad.hip) and k_mlp_input_jacobian
// (k_mlp_input_jacobian.hip) out of scratch, and the column blocks per wave both are instantiated with.
#pragma once
#include "mlp_device.h"

namespace tcnn_amd {
namespace {

// The run-time activation, chosen ONCE per layer and not per element: with the switch outside the loops every
// case is the straight-line code of a compiled form, and inlined by force, so that acc and the packed halves are never passed by
// address (as a function of its own, activate_pack puts both into scratch: k_mlp_fwd's run-time form has 400 bytes of it).  Same functions on the same values.
template <int T, int KS, int NB, int ACT>
__device__ __forceinline__ void pack_layer(const f4 (&acc)[T][NB], h8 (&hf)[KS][NB], const uint32_t act) {
	if constexpr (ACT != -1) {
		activate_pack_inlined<T, KS, NB, ACT>(acc, hf, act);
	} else {
		switch (act) {
			case (uint32_t)Activation::ReLU: activate_pack_inlined<T, KS, NB, -1>(acc, hf, (uint32_t)Activation::ReLU); break;
			case (uint32_t)Activation::LeakyReLU: activate_pack_inlined<T, KS, NB, -1>(acc, hf, (uint32_t)Activation::LeakyReLU); break;
			case (uint32_t)Activation::Exponential: activate_pack_inlined<T, KS, NB, -1>(acc, hf, (uint32_t)Activation::Exponential); break;
			case (uint32_t)Activation::Sigmoid: activate_pack_inlined<T, KS, NB, -1>(acc, hf, (uint32_t)Activation::Sigmoid); break;
			case (uint32_t)Activation::Squareplus: activate_pack_inlined<T, KS, NB, -1>(acc, hf, (uint32_t)Activation::Squareplus); break;
			case (uint32_t)Activation::Softplus: activate_pack_inlined<T, KS, NB, -1>(acc, hf, (uint32_t)Activation::Softplus); break;
			case (uint32_t)Activation::Tanh: activate_pack_inlined<T, KS, NB, -1>(acc, hf, (uint32_t)Activation::Tanh); break;
			default: activate_pack_inlined<T, KS, NB, -1>(acc, hf, (uint32_t)Activation::None); break; // None (a Sine network has no fragment images: never here)
		}
	}
}

// A layer's fragments, as 32-bit byte offsets from the layer's wave-uniform base (saddr + voffset addressing).  The base goes through an
// empty asm statement once per trip and layer: with every layer written out, the compiler otherwise computes all of their fragments'
// 64-bit addresses once, in front of the sample loop, and keeps them there -- two registers per fragment, more than 500 at 128 x 4.
__device__ inline const char* layer_base(const h8* image, const uint32_t first_frag) {
	const char* p = (const char*)image + (size_t)first_frag * 1024;
	asm volatile("" : "+s"(p));
	return p;
}
__device__ inline h8 frag_at(const char* base, const uint32_t lane16, const uint32_t index) { return ld32<h8>(base, lane16 + index * 1024); }

template <int L> struct Layer { static constexpr int value = L; }; // a compile-time layer number: kept[l] is a register, never an address

// NB as the two-pass kernels have it (one column block at 128 wide reads every weight fragment twice as often per sample: 128 x 4 at 2^20
// rows took 1.04 ms against the two passes' 0.91).  256 wide is not instantiated: its 64 accumulators and 32 kept registers per layer
// leave room for one hidden layer.
constexpr int nb_of(int W, int) { return W >= 128 ? 2 : 4; }

} // namespace
} // namespace tcnn_amd
