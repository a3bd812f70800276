// mlp_batched.h -- what BatchedMlpModel (model.h) calls of k_mlp_batched.hip: K small networks of one shape in one launch, each on its
// own rows [offsets[k], offsets[k + 1]) of the batch (DESIGN.md "BatchedMLP").
#pragma once

#include "tcnn_common.h"

namespace tcnn_amd {

constexpr uint32_t BMLP_MAX_WIDTH = 64;          // of the padded input, the hidden layers and the padded output
constexpr uint32_t BMLP_LDS_LIMIT = 144 * 1024;  // bytes of LDS one workgroup of the backward kernel may use
constexpr uint32_t BMLP_CHUNK = 512;             // rows whose weight-gradient sum one workgroup forms in one piece (the unit of the fixed summation order)
constexpr uint32_t BMLP_STAGE_BYTES = 2 * 2 * 64 * 72 * 2; // backward: two buffers of {dZ, A} [64 rows][64 + 8] halves

struct BmlpLayer {
	uint32_t rows, cols; // fan_out, fan_in
	uint32_t w_off;      // element offset inside ONE network's parameters (and inside its fp32 gradient accumulators)
	uint32_t lds_off;    // element offset of the matrix in LDS, rows (cols + 8) halves apart
};
struct BmlpDesc {
	uint32_t n_networks, in_dims, in_width, width, out_width, n_layers, activation, output_activation;
	uint32_t n_params;   // of one network
	uint32_t lds_halves; // of one network's weights in LDS
	BmlpLayer layers[MAX_MLP_LAYERS];
};

// `net`: one network's description (Network::desc(), in_width the padded input width)
inline BmlpDesc bmlp_desc(const MlpDesc& net, uint32_t n_networks, uint32_t in_dims) {
	BmlpDesc d{};
	d.n_networks = n_networks;
	d.in_dims = in_dims;
	d.in_width = net.in_width;
	d.width = net.width;
	d.out_width = net.out_width;
	d.n_layers = net.n_layers;
	d.activation = net.activation;
	d.output_activation = net.output_activation;
	uint32_t lds = 0;
	for (uint32_t l = 0; l < net.n_layers; ++l) {
		d.layers[l] = BmlpLayer{net.layers[l].rows, net.layers[l].cols, net.layers[l].w_off, lds};
		lds += net.layers[l].rows * (net.layers[l].cols + 8);
		d.n_params = net.layers[l].w_off + net.layers[l].rows * net.layers[l].cols;
	}
	d.lds_halves = lds;
	return d;
}
// LDS of a workgroup: the forward kernel holds W in half; the backward kernel W, the staging buffers and dW in fp32
inline size_t bmlp_forward_lds_bytes(const BmlpDesc& d) { return (size_t)d.lds_halves * 2; }
inline size_t bmlp_backward_lds_bytes(const BmlpDesc& d) { return (size_t)d.lds_halves * 2 + BMLP_STAGE_BYTES + (size_t)d.n_params * 4; }
// fp32 partial sums [slot][n_params] for networks whose rows span more than one chunk.  Without offsets the split is equal and the host
// knows whether any does; with offsets it cannot, and 2 floor(n / BMLP_CHUNK) slots hold every split of n rows.
inline size_t bmlp_partial_floats(const BmlpDesc& d, uint32_t n, bool has_offsets) {
	if (!has_offsets && n / d.n_networks <= BMLP_CHUNK) return 0;
	return (size_t)(2 * (n / BMLP_CHUNK) + 2) * d.n_params;
}

// x: the module's float input [n][in_dims]; out: [n][out_width] half; hidden (optional): [n_layers - 1][n][width] half, post-activation.
// offsets: n_networks + 1 ascending row indices in device memory, or nullptr for the equal split (n % n_networks == 0)
void bmlp_forward(hipStream_t stream, const BmlpDesc& d, uint32_t n, const uint32_t* offsets, MatView x, const void* params, void* out, void* hidden);
// dL_dinput (optional): float [n][in_dims]; gradients (mode != Ignore): half [n_networks][n_params]; partials: bmlp_partial_floats() floats
void bmlp_backward(hipStream_t stream, const BmlpDesc& d, uint32_t n, const uint32_t* offsets, MatView x, const void* hidden, const void* out, const void* dL_dout,
                   const void* params, const MatViewMut* dL_dinput, void* gradients, GradientMode mode, float* partials);

// ---- second order (DESIGN.md "BatchedMLP: second-order pass and tangent"): the gradients of S = <v, dL/dinput>, per network on its rows
constexpr uint32_t BMLP_TANGENT_GROUP = 3; // tangent chains that run beside the forward chain in one launch of k_bmlp_tangent

__host__ __device__ inline bool bmlp_curved(uint32_t act) { // a'' != 0 somewhere
	return act != (uint32_t)Activation::None && act != (uint32_t)Activation::ReLU && act != (uint32_t)Activation::LeakyReLU;
}
inline bool bmlp_any_curvature(const BmlpDesc& d) { return bmlp_curved(d.activation) || bmlp_curved(d.output_activation); }
// what the up pass leaves for the down pass, per kind: [n_layers - 1][n][width] like `hidden`, then [n][out_width] for the last layer
inline size_t bmlp_second_order_halves(const BmlpDesc& d, uint32_t n) { return (size_t)n * ((d.n_layers - 1) * d.width + d.out_width); }

// The up pass.  v: the first of n_tangents (1 .. BMLP_TANGENT_GROUP) directions [n][in_dims] floats, the next one v_next floats behind it.
// jvp (optional): tangent t's u_K at jvp[row * jvp_ld + t * out_width ..]; out (optional): the forward output, inference()'s bits.
// u, z, c (all or none, n_tangents == 1, bmlp_second_order_halves() halves each): u_1 .. u_{K-1} in the hidden slots; z_k of every layer
// with an activation; c_k = a_k''(z_k) z'_k of every layer with curvature.
void bmlp_tangent(hipStream_t stream, const BmlpDesc& d, uint32_t n, const uint32_t* offsets, MatView x, MatView v, uint32_t v_next, uint32_t n_tangents, const void* params,
                  void* jvp, uint32_t jvp_ld, void* out, void* u, void* z, void* c);
// The down pass, on what bmlp_tangent left.  dL_dinput (optional) is written only where the network has curvature (else it is zero: the
// caller's to clear); gradients / mode / partials as bmlp_backward.
void bmlp_backward_second(hipStream_t stream, const BmlpDesc& d, uint32_t n, const uint32_t* offsets, MatView x, MatView v, const void* hidden, const void* dL_dout, const void* params,
                          const void* u, const void* z, const void* c, const MatViewMut* dL_dinput, void* gradients, GradientMode mode, float* partials);

} // namespace tcnn_amd
