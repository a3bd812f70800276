// k_mlp_batched.hip -- BatchedMLP: K networks of one shape in one launch, network k on rows [offsets[k], offsets[k + 1]) (DESIGN.md "BatchedMLP").
//
// Grid: K x S workgroups of 4 waves (+ BM_ZERO_BLOCKS that write +0 to the rows no network owns).  Workgroup (k, s) copies network k's
// weights into LDS once -- row-major, rows (cols + 8) halves apart, so that the 16 rows a fragment read touches fall into different banks --
// and keeps them there for all its tiles.  Every product is out^T = W x^T with v_mfma_f32_16x16x32_f16: A = 16 rows of W (two 8-byte LDS
// reads per lane, k in the chained order k_chain), B = the activations of 16 samples, which never leave the registers between layers:
// lane (q, c) holds neurons 4 q + r of sample c in every accumulator block, which is the B fragment of the next layer in chained k order.
//
// Backward: one kernel.  Per round of 64 rows (16 per wave) and layer, from the last to the first:
//   stage   dZ_l and A_{l-1} of the wave's 16 rows into LDS, [row][neuron] (two buffers, so one barrier per layer is enough)
//   dW_l    wave w owns the 16x16 blocks w, w + 4, .. of dW_l: both operands come transposed out of the stage (lds_read_tr), the fp32
//           block lives in LDS between rounds in accumulator order (one 16-byte read and write per lane, no conflicts)
//   dA      = W_l^T dZ_l, W read transposed from the SAME LDS copy (lds_read_tr); times the activation's derivative it is dZ_{l-1}
// The weight gradients are summed in an order fixed by the segment alone: rows in chunks of BMLP_CHUNK from the segment's start, inside a
// chunk round by round through the MFMA accumulator, chunks in ascending order (k_bmlp_reduce when a segment has several).  So they are the
// same bits on every run, for every S, and for the same segment inside any batch.
//
// Second order (further down): k_bmlp_tangent runs the forward chain and up to three tangent chains side by side, k_bmlp_bwd2 is the
// backward kernel with a second chain for the curvature terms; the same grid, weight copy, stage buffers and summation order.
#include "mlp_batched.h"
#include "mlp_device.h"

namespace tcnn_amd {
namespace {

constexpr uint32_t BM_THREADS = 256, BM_WAVES = 4;
constexpr int BM_T = 2;                  // forward: 16-row tiles per wave and trip, so that a weight fragment read serves two MFMAs
constexpr uint32_t BM_ZERO_BLOCKS = 16;  // workgroups behind the K x S that clear the rows no network owns
constexpr uint32_t BM_ROUND = 64;        // backward: rows per workgroup and round
constexpr uint32_t BM_LD = 72;           // halves between staged rows: 64 + 8
constexpr uint32_t BM_STAGE = 2 * BM_ROUND * BM_LD; // halves of one stage buffer {dZ, A}
static_assert(2 * BM_STAGE * 2 == BMLP_STAGE_BYTES, "stage buffers");

struct Segment { uint32_t begin, end; };
// clamped to [0, n] and to begin <= end, whatever the array holds: no row outside the batch is ever touched
__device__ inline Segment segment_of(const BmlpDesc& d, const uint32_t* offsets, const uint32_t n, const uint32_t k) {
	uint32_t b, e;
	if (offsets) {
		b = offsets[k];
		e = offsets[k + 1];
	} else {
		const uint32_t per = n / d.n_networks;
		b = k * per;
		e = b + per;
	}
	e = min(e, n);
	b = min(b, e);
	return Segment{b, e};
}

// rows before offsets[0] and from offsets[K] on belong to no network: f(row, column) for every element of theirs
template <typename F>
__device__ inline void for_unowned(const BmlpDesc& d, const uint32_t* offsets, const uint32_t n, const uint32_t z, const uint32_t width, F f) {
	const uint32_t first = offsets ? min(offsets[0], n) : 0u;
	const uint32_t last = offsets ? max(first, min(offsets[d.n_networks], n)) : (n / d.n_networks) * d.n_networks;
	const uint64_t total = (uint64_t)(first + (n - last)) * width;
	for (uint64_t i = (uint64_t)z * BM_THREADS + threadIdx.x; i < total; i += (uint64_t)BM_ZERO_BLOCKS * BM_THREADS) {
		const uint32_t r = (uint32_t)(i / width), col = (uint32_t)(i % width);
		f(r < first ? r : last + (r - first), col);
	}
}

// network k's matrices -> LDS, 16 bytes per load
__device__ inline void load_weights(const BmlpDesc& d, const half_t* __restrict__ params_k, half_t* W) {
	for (uint32_t l = 0; l < d.n_layers; ++l) {
		const BmlpLayer L = d.layers[l];
		const uint32_t per_row = L.cols / 8, total = L.rows * per_row;
		for (uint32_t i = threadIdx.x; i < total; i += BM_THREADS) {
			const uint32_t r = i / per_row, c8 = i % per_row;
			*(uint4*)(W + L.lds_off + r * (L.cols + 8) + c8 * 8) = *(const uint4*)(params_k + L.w_off + r * L.cols + c8 * 8);
		}
	}
}

__device__ inline h8 join(const h4 lo, const h4 hi) { return h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}; }
__device__ inline h4 zero4() { return h4{(half_t)0.0f, (half_t)0.0f, (half_t)0.0f, (half_t)0.0f}; }

// B fragment s (chained k order) of the padded input of one row: the Identity encoding's cast, ones in the padding, zeros past the width
// and for rows outside the segment
__device__ inline h8 load_input(const BmlpDesc& d, const MatView& x, const uint32_t row, const bool valid, const uint32_t s, const uint32_t q) {
	h8 v;
#pragma unroll
	for (int j = 0; j < 8; ++j) {
		const uint32_t f = k_chain(s, q, j);
		half_t e = (half_t)0.0f;
		if (valid && f < d.in_width) e = f < d.in_dims ? (half_t)x.data[(size_t)row * x.stride_sample + (size_t)f * x.stride_dim] : (half_t)1.0f;
		v[j] = e;
	}
	return v;
}
// the same of a half matrix [.][stride] with `width` columns in use
__device__ inline h8 load_rows(const half_t* __restrict__ base, const uint32_t stride, const uint32_t width, const uint32_t row, const bool valid, const uint32_t s, const uint32_t q) {
	h4 lo = zero4(), hi = zero4();
	if (valid && 32 * s + 4 * q < width) lo = *(const h4*)(base + (size_t)row * stride + 32 * s + 4 * q);
	if (valid && 32 * s + 16 + 4 * q < width) hi = *(const h4*)(base + (size_t)row * stride + 32 * s + 16 + 4 * q);
	return join(lo, hi);
}

// ---------------------------------------------------------------------------------------------------------------- forward / inference
template <bool STORE_HIDDEN>
__global__ void __launch_bounds__(BM_THREADS) k_bmlp_fwd(const BmlpDesc d, const uint32_t S, const uint32_t n, const uint32_t* __restrict__ offsets, const MatView x,
                                                         const half_t* __restrict__ params, half_t* __restrict__ out, half_t* __restrict__ hidden) {
	extern __shared__ __attribute__((aligned(16))) half_t W[];
	if (blockIdx.x >= d.n_networks * S) {
		for_unowned(d, offsets, n, blockIdx.x - d.n_networks * S, d.out_width, [&](uint32_t row, uint32_t col) { out[(size_t)row * d.out_width + col] = (half_t)0.0f; });
		return;
	}
	const uint32_t k = blockIdx.x / S, s_wg = blockIdx.x % S;
	const Segment seg = segment_of(d, offsets, n, k);
	const uint32_t n_tiles = (seg.end - seg.begin + 16 * BM_T - 1) / (16 * BM_T);
	if (s_wg * BM_WAVES >= n_tiles) return; // an empty segment, or no tile for this workgroup
	load_weights(d, params + (size_t)k * d.n_params, W);
	__syncthreads();

	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
	for (uint32_t t = s_wg * BM_WAVES + wave; t < n_tiles; t += S * BM_WAVES) {
		uint32_t row[BM_T];
		bool valid[BM_T];
		h8 hf[BM_T][2];
#pragma unroll
		for (int u = 0; u < BM_T; ++u) {
			row[u] = seg.begin + (t * BM_T + u) * 16 + c;
			valid[u] = row[u] < seg.end;
#pragma unroll
			for (int s = 0; s < 2; ++s) hf[u][s] = load_input(d, x, row[u], valid[u], s, q);
		}
		for (uint32_t l = 0; l < d.n_layers; ++l) {
			const BmlpLayer L = d.layers[l];
			const half_t* Wl = W + L.lds_off + c * (L.cols + 8) + 4 * q;
			const uint32_t nb = L.rows / 16;
			f4 acc[BM_T][4];
#pragma unroll
			for (int b = 0; b < 4; ++b) {
#pragma unroll
				for (int u = 0; u < BM_T; ++u) acc[u][b] = f4{0.0f, 0.0f, 0.0f, 0.0f};
				if ((uint32_t)b < nb) {
#pragma unroll
					for (int s = 0; s < 2; ++s) {
						if (32u * s < L.cols) {
							const half_t* p = Wl + b * 16 * (L.cols + 8) + 32 * s;
							const h8 af = join(*(const h4*)p, 32u * s + 16 < L.cols ? *(const h4*)(p + 16) : zero4());
#pragma unroll
							for (int u = 0; u < BM_T; ++u) acc[u][b] = mfma(af, hf[u][s], acc[u][b]);
						}
					}
				}
			}
			const bool last = l + 1 == d.n_layers;
			const uint32_t act = last ? d.output_activation : d.activation;
#pragma unroll
			for (int u = 0; u < BM_T; ++u) {
				h4 y[4];
#pragma unroll
				for (int b = 0; b < 4; ++b) {
#pragma unroll
					for (int r = 0; r < 4; ++r) y[b][r] = (uint32_t)b < nb ? activation_fwd<half_t>(act, (half_t)acc[u][b][r]) : (half_t)0.0f;
					if ((uint32_t)b < nb && valid[u]) {
						if (last) *(h4*)(out + (size_t)row[u] * d.out_width + 16 * b + 4 * q) = y[b];
						else if (STORE_HIDDEN) *(h4*)(hidden + ((size_t)l * n + row[u]) * d.width + 16 * b + 4 * q) = y[b];
					}
				}
				hf[u][0] = join(y[0], y[1]);
				hf[u][1] = join(y[2], y[3]);
			}
		}
	}
}

// --------------------------------------------------------------------------------------------------------------------------- backward
__device__ inline void store_gradient(half_t* g, const float sum, const bool accumulate) { *g = (half_t)(accumulate ? (float)*g + sum : sum); }

// The fp32 weight-gradient blocks in LDS, in accumulator order; wave w owns blocks w, w + 4, .. of every layer (nobody else ever touches
// them: no barrier).
__device__ inline void clear_accumulators(const BmlpDesc& d, float* accs, const uint32_t wave, const uint32_t lane) {
	for (uint32_t l = 0; l < d.n_layers; ++l) {
		const uint32_t n_blocks = d.layers[l].rows * d.layers[l].cols / 256;
		for (uint32_t bi = wave; bi < n_blocks; bi += BM_WAVES) *(f4*)(accs + d.layers[l].w_off + bi * 256 + lane * 4) = f4{0.0f, 0.0f, 0.0f, 0.0f};
	}
}
// acc + Zs^T As over the round's 64 staged rows, for the 16x16 block (rb, cb): both operands come transposed out of the stage
__device__ inline f4 staged_product(const half_t* Zs, const half_t* As, const uint32_t rb, const uint32_t cb, const uint32_t lane, f4 acc) {
	const uint32_t c = lane & 15, q = lane >> 4, tr_row = c >> 2, tr_col = 4 * (c & 3);
#pragma unroll
	for (int ks = 0; ks < 2; ++ks) {
		const uint32_t r = 32 * ks + 8 * q + tr_row;
		const h8 af = join(lds_read_tr(Zs + r * BM_LD + 16 * rb + tr_col), lds_read_tr(Zs + (r + 4) * BM_LD + 16 * rb + tr_col));
		const h8 bf = join(lds_read_tr(As + r * BM_LD + 16 * cb + tr_col), lds_read_tr(As + (r + 4) * BM_LD + 16 * cb + tr_col));
		acc = mfma(af, bf, acc);
	}
	return acc;
}
// the end of a chunk.  A segment of one chunk (slot == nullptr): rounded and stored (or added) here; else the chunk's fp32 sum goes to
// its slot for k_bmlp_reduce
__device__ inline void flush_chunk(const BmlpDesc& d, const float* accs, const uint32_t wave, const uint32_t lane, float* slot, half_t* gk, const bool accumulate) {
	const uint32_t c = lane & 15, q = lane >> 4;
	for (uint32_t l = 0; l < d.n_layers; ++l) {
		const BmlpLayer L = d.layers[l];
		const uint32_t nbc = L.cols / 16, n_blocks = (L.rows / 16) * nbc;
		for (uint32_t bi = wave; bi < n_blocks; bi += BM_WAVES) {
			const f4 acc = *(const f4*)(accs + L.w_off + bi * 256 + lane * 4);
			const uint32_t at = L.w_off + (16 * (bi / nbc) + 4 * q) * L.cols + 16 * (bi % nbc) + c;
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				if (!slot) store_gradient(gk + at + r * L.cols, acc[r], accumulate);
				else slot[at + r * L.cols] = acc[r];
			}
		}
	}
}
// one row's staged operand: the fragments' elements at their neurons' columns
__device__ inline void stage_row(half_t* row_at_4q, const h8 (&f)[2]) {
#pragma unroll
	for (int s = 0; s < 2; ++s) {
		*(h4*)(row_at_4q + 32 * s) = h4{f[s][0], f[s][1], f[s][2], f[s][3]};
		*(h4*)(row_at_4q + 32 * s + 16) = h4{f[s][4], f[s][5], f[s][6], f[s][7]};
	}
}

template <bool WGRAD>
__global__ void __launch_bounds__(BM_THREADS) k_bmlp_bwd(const BmlpDesc d, const uint32_t S, const uint32_t n, const uint32_t* __restrict__ offsets, const MatView x,
                                                         const half_t* __restrict__ hidden, const half_t* __restrict__ out, const half_t* __restrict__ dy,
                                                         const half_t* __restrict__ params, const MatViewMut dx, half_t* __restrict__ grads, const uint32_t accumulate,
                                                         float* __restrict__ partials) {
	extern __shared__ __attribute__((aligned(16))) half_t lds[];
	half_t* W = lds;
	half_t* stage = W + d.lds_halves;
	float* accs = (float*)(stage + 2 * BM_STAGE);
	if (blockIdx.x >= d.n_networks * S) {
		if (dx.data) for_unowned(d, offsets, n, blockIdx.x - d.n_networks * S, d.in_dims, [&](uint32_t row, uint32_t col) { dx.data[(size_t)row * dx.stride_sample + (size_t)col * dx.stride_dim] = 0.0f; });
		return;
	}
	const uint32_t k = blockIdx.x / S, s_wg = blockIdx.x % S;
	const Segment seg = segment_of(d, offsets, n, k);
	const uint32_t n_chunks = (seg.end - seg.begin + BMLP_CHUNK - 1) / BMLP_CHUNK;
	if (n_chunks == 0) { // an empty network: +0 under Overwrite, nothing under Accumulate
		if (WGRAD && s_wg == 0 && !accumulate) {
			for (uint32_t i = threadIdx.x; i < d.n_params; i += BM_THREADS) grads[(size_t)k * d.n_params + i] = (half_t)0.0f;
		}
		return;
	}
	if (s_wg >= n_chunks) return;
	load_weights(d, params + (size_t)k * d.n_params, W);
	__syncthreads();

	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
	const uint32_t tr_row = c >> 2, tr_col = 4 * (c & 3); // lds_read_tr: lane c names row c / 4, columns 4 (c % 4).. and receives column c of the 4 rows
	uint32_t phase = 0;
	for (uint32_t ch = s_wg; ch < n_chunks; ch += S) {
		const uint32_t chunk_begin = seg.begin + ch * BMLP_CHUNK, chunk_end = min(chunk_begin + BMLP_CHUNK, seg.end);
		if (WGRAD) clear_accumulators(d, accs, wave, lane);
		for (uint32_t r0 = chunk_begin; r0 < chunk_end; r0 += BM_ROUND) {
			const uint32_t row = r0 + 16 * wave + c;
			const bool valid = row < chunk_end;
			h8 g[2];
#pragma unroll
			for (int s = 0; s < 2; ++s) {
				g[s] = load_rows(dy, d.out_width, d.out_width, row, valid, s, q);
				if (d.output_activation != (uint32_t)Activation::None) {
					const h8 y = load_rows(out, d.out_width, d.out_width, row, valid, s, q);
#pragma unroll
					for (int j = 0; j < 8; ++j) g[s][j] = valid && k_chain(s, q, j) < d.out_width ? activation_bwd<half_t>(d.output_activation, g[s][j], y[j]) : (half_t)0.0f;
				}
			}
			for (uint32_t l = d.n_layers - 1;; --l) {
				const BmlpLayer L = d.layers[l];
				h8 av[2]; // A_{l-1}: the layer's input
#pragma unroll
				for (int s = 0; s < 2; ++s) av[s] = l == 0 ? load_input(d, x, row, valid, s, q) : load_rows(hidden + (size_t)(l - 1) * n * d.width, d.width, d.width, row, valid, s, q);
				if (WGRAD) {
					half_t* Zs = stage + phase * BM_STAGE;
					half_t* As = Zs + BM_ROUND * BM_LD;
					half_t* zrow = Zs + (16 * wave + c) * BM_LD + 4 * q;
					half_t* arow = As + (16 * wave + c) * BM_LD + 4 * q;
#pragma unroll
					for (int s = 0; s < 2; ++s) {
						*(h4*)(zrow + 32 * s) = h4{g[s][0], g[s][1], g[s][2], g[s][3]};
						*(h4*)(zrow + 32 * s + 16) = h4{g[s][4], g[s][5], g[s][6], g[s][7]};
						*(h4*)(arow + 32 * s) = h4{av[s][0], av[s][1], av[s][2], av[s][3]};
						*(h4*)(arow + 32 * s + 16) = h4{av[s][4], av[s][5], av[s][6], av[s][7]};
					}
					__syncthreads();
					const uint32_t nbc = L.cols / 16, n_blocks = (L.rows / 16) * nbc;
					for (uint32_t bi = wave; bi < n_blocks; bi += BM_WAVES) {
						float* ap = accs + L.w_off + bi * 256 + lane * 4;
						*(f4*)ap = staged_product(Zs, As, bi / nbc, bi % nbc, lane, *(f4*)ap);
					}
					phase ^= 1;
				}
				if (l == 0 && !dx.data) break;
				// dA_{l-1} = W_l^T dZ_l
				const half_t* Wl = W + L.lds_off + (4 * q + tr_row) * (L.cols + 8) + tr_col;
				const uint32_t nbc = L.cols / 16;
				f4 da[4];
#pragma unroll
				for (int b = 0; b < 4; ++b) {
					da[b] = f4{0.0f, 0.0f, 0.0f, 0.0f};
					if ((uint32_t)b < nbc) {
#pragma unroll
						for (int s = 0; s < 2; ++s) {
							if (32u * s < L.rows) {
								const half_t* p = Wl + 32 * s * (L.cols + 8) + 16 * b;
								const h8 af = join(lds_read_tr(p), 32u * s + 16 < L.rows ? lds_read_tr(p + 16 * (L.cols + 8)) : zero4());
								da[b] = mfma(af, g[s], da[b]);
							}
						}
					}
				}
				if (l == 0) { // the Identity encoding's backward: the padded columns dropped, float
#pragma unroll
					for (int b = 0; b < 4; ++b) {
#pragma unroll
						for (int r = 0; r < 4; ++r) {
							const uint32_t f = 16 * b + 4 * q + r;
							if (valid && f < d.in_dims) dx.data[(size_t)row * dx.stride_sample + (size_t)f * dx.stride_dim] = (float)(half_t)da[b][r];
						}
					}
					break;
				}
#pragma unroll
				for (int s = 0; s < 2; ++s) {
#pragma unroll
					for (int j = 0; j < 8; ++j) {
						const int b = 2 * s + (j >> 2);
						g[s][j] = (uint32_t)b < nbc ? activation_bwd<half_t>(d.activation, (half_t)da[b][j & 3], av[s][j]) : (half_t)0.0f;
					}
				}
			}
		}
		if (WGRAD) flush_chunk(d, accs, wave, lane, n_chunks == 1 ? nullptr : partials + (size_t)(2 * (seg.begin / BMLP_CHUNK) + ch) * d.n_params, grads + (size_t)k * d.n_params, accumulate != 0);
	}
}

// segments of several chunks: the chunks' fp32 sums added in ascending order, rounded once
__global__ void __launch_bounds__(BM_THREADS) k_bmlp_reduce(const BmlpDesc d, const uint32_t n, const uint32_t* __restrict__ offsets, const float* __restrict__ partials,
                                                            half_t* __restrict__ grads, const uint32_t accumulate) {
	const uint32_t per_net = (d.n_params + BM_THREADS - 1) / BM_THREADS;
	const uint32_t k = blockIdx.x / per_net, i = (blockIdx.x % per_net) * BM_THREADS + threadIdx.x;
	const Segment seg = segment_of(d, offsets, n, k);
	const uint32_t n_chunks = (seg.end - seg.begin + BMLP_CHUNK - 1) / BMLP_CHUNK;
	if (n_chunks < 2 || i >= d.n_params) return;
	const float* p = partials + (size_t)(2 * (seg.begin / BMLP_CHUNK)) * d.n_params + i;
	float sum = p[0];
	for (uint32_t ch = 1; ch < n_chunks; ++ch) sum += p[(size_t)ch * d.n_params];
	store_gradient(grads + (size_t)k * d.n_params + i, sum, accumulate != 0);
}

// ----------------------------------------------------------------------------------------------------------------------- second order
// The gradients of S = <v, dL/dinput> (the recipe of Network::second_order_*, model.h), in two launches.  With z_k = W_k h_{k-1},
// h_k = a_k(z_k), g_K = dL/dy, d_k = g_k a_k', g_{k-1} = W_k^T d_k:
//   up    u_0 = v, z'_k = W_k u_{k-1} (fp32, never stored), u_k = a_k' z'_k, c_k = a_k'' z'_k                 dS/d(dL/dy) = u_K
//   down  r_k = c_k g_k, p_k = r_k + a_k' W_{k+1}^T p_{k+1}, dS/dW_k = d_k^T u_{k-1} + p_k^T h_{k-1}, dS/dinput = W_1^T p_1
// a' and a'' are evaluated in fp32 from z_k rounded to half (act_d1 / act_d2), and every stored matrix is rounded to half once.

// where layer l's rows live in the buffers the up pass leaves: the hidden layers like `hidden`, the last layer behind them
struct Slot { size_t base; uint32_t stride; };
__device__ inline Slot slot_of(const BmlpDesc& d, const uint32_t n, const uint32_t l) {
	return l + 1 == d.n_layers ? Slot{(size_t)(d.n_layers - 1) * n * d.width, d.out_width} : Slot{(size_t)l * n * d.width, d.width};
}
// B fragment s of one row of a direction v: cast to half, zeros in the padding
__device__ inline h8 load_tangent(const BmlpDesc& d, const float* __restrict__ v, const uint32_t stride_sample, const uint32_t stride_dim, const uint32_t row, const bool valid,
                                  const uint32_t s, const uint32_t q) {
	h8 u;
#pragma unroll
	for (int j = 0; j < 8; ++j) {
		const uint32_t f = k_chain(s, q, j);
		u[j] = valid && f < d.in_dims ? (half_t)v[(size_t)row * stride_sample + (size_t)f * stride_dim] : (half_t)0.0f;
	}
	return u;
}

// (half)p with p rounded to fp32 first.  Left alone, the compiler folds "fp32 multiply + convert" into v_fma_mixlo_f16 (one rounding from
// the exact product) in some instantiations and not in others, which is one half step apart once in 10^4 elements (see k_grid.hip).
__device__ inline half_t rounded_half(float p) {
	asm volatile("" : "+v"(p));
	return (half_t)p;
}

// Up pass: the forward chain and NT tangent chains of a 16-row tile per wave, side by side: every weight fragment read from LDS feeds
// 1 + NT MFMAs, and activations and tangents stay in registers between layers as in k_bmlp_fwd.  input_jvp (STORE false) writes jvp and,
// if asked, the output; the second-order call (STORE, NT = 1) writes u_K if asked and leaves u_k, z_k and c_k for the down pass.
template <int NT, bool STORE>
__global__ void __launch_bounds__(BM_THREADS) k_bmlp_tangent(const BmlpDesc d, const uint32_t S, const uint32_t n, const uint32_t* __restrict__ offsets, const MatView x, const MatView v,
                                                             const uint32_t v_next, const half_t* __restrict__ params, half_t* __restrict__ jvp, const uint32_t jvp_ld,
                                                             half_t* __restrict__ out, half_t* __restrict__ U, half_t* __restrict__ Z, half_t* __restrict__ C) {
	extern __shared__ __attribute__((aligned(16))) half_t W[];
	if (blockIdx.x >= d.n_networks * S) {
		const uint32_t z = blockIdx.x - d.n_networks * S;
		if (jvp) for_unowned(d, offsets, n, z, NT * d.out_width, [&](uint32_t row, uint32_t col) { jvp[(size_t)row * jvp_ld + col] = (half_t)0.0f; });
		if (out) for_unowned(d, offsets, n, z, d.out_width, [&](uint32_t row, uint32_t col) { out[(size_t)row * d.out_width + col] = (half_t)0.0f; });
		return;
	}
	const uint32_t k = blockIdx.x / S, s_wg = blockIdx.x % S;
	const Segment seg = segment_of(d, offsets, n, k);
	const uint32_t n_tiles = (seg.end - seg.begin + 15) / 16;
	if (s_wg * BM_WAVES >= n_tiles) return;
	load_weights(d, params + (size_t)k * d.n_params, W);
	__syncthreads();

	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
	for (uint32_t t = s_wg * BM_WAVES + wave; t < n_tiles; t += S * BM_WAVES) {
		const uint32_t row = seg.begin + t * 16 + c;
		const bool valid = row < seg.end;
		h8 hf[2], uf[NT][2];
#pragma unroll
		for (int s = 0; s < 2; ++s) {
			hf[s] = load_input(d, x, row, valid, s, q);
#pragma unroll
			for (int i = 0; i < NT; ++i) uf[i][s] = load_tangent(d, v.data + (size_t)i * v_next, v.stride_sample, v.stride_dim, row, valid, s, q);
		}
		for (uint32_t l = 0; l < d.n_layers; ++l) {
			const BmlpLayer L = d.layers[l];
			const half_t* Wl = W + L.lds_off + c * (L.cols + 8) + 4 * q;
			const uint32_t nb = L.rows / 16;
			const bool last = l + 1 == d.n_layers;
			const uint32_t act = last ? d.output_activation : d.activation;
			const bool curved = bmlp_curved(act);
			const Slot at = slot_of(d, n, l);
			h4 y[4], yu[NT][4];
#pragma unroll
			for (int b = 0; b < 4; ++b) {
				y[b] = zero4();
#pragma unroll
				for (int i = 0; i < NT; ++i) yu[i][b] = zero4();
				if ((uint32_t)b < nb) {
					f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f}, du[NT];
#pragma unroll
					for (int i = 0; i < NT; ++i) du[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
					for (int s = 0; s < 2; ++s) {
						if (32u * s < L.cols) {
							const half_t* p = Wl + b * 16 * (L.cols + 8) + 32 * s;
							const h8 af = join(*(const h4*)p, 32u * s + 16 < L.cols ? *(const h4*)(p + 16) : zero4());
							acc = mfma(af, hf[s], acc);
#pragma unroll
							for (int i = 0; i < NT; ++i) du[i] = mfma(af, uf[i][s], du[i]);
						}
					}
					h4 zb, cb = zero4();
#pragma unroll
					for (int r = 0; r < 4; ++r) {
						zb[r] = (half_t)acc[r];
						y[b][r] = activation_fwd<half_t>(act, zb[r]);
						const float d1 = act_d1(act, (float)zb[r]);
#pragma unroll
						for (int i = 0; i < NT; ++i) yu[i][b][r] = rounded_half(d1 * du[i][r]);
						if (STORE && curved) cb[r] = rounded_half(act_d2(act, (float)zb[r]) * du[0][r]);
					}
					if (valid) {
						const uint32_t col = 16 * b + 4 * q;
						if (last) {
							if (out) *(h4*)(out + (size_t)row * d.out_width + col) = y[b];
							if (jvp) {
#pragma unroll
								for (int i = 0; i < NT; ++i) *(h4*)(jvp + (size_t)row * jvp_ld + i * d.out_width + col) = yu[i][b];
							}
						} else if (STORE) {
							*(h4*)(U + at.base + (size_t)row * at.stride + col) = yu[0][b];
						}
						if (STORE && act != (uint32_t)Activation::None) *(h4*)(Z + at.base + (size_t)row * at.stride + col) = zb;
						if (STORE && curved) *(h4*)(C + at.base + (size_t)row * at.stride + col) = cb;
					}
				}
			}
#pragma unroll
			for (int s = 0; s < 2; ++s) {
				hf[s] = join(y[2 * s], y[2 * s + 1]);
#pragma unroll
				for (int i = 0; i < NT; ++i) uf[i][s] = join(yu[i][2 * s], yu[i][2 * s + 1]);
			}
		}
	}
}

// Down pass: k_bmlp_bwd with two chains.  Per round of 64 rows and layer, from the last to the first, a wave forms d_l and (CURVED, from
// the last layer with curvature down) p_l of its 16 rows, adds d_l^T u_{l-1} and p_l^T h_{l-1} into the same fp32 block of dW_l -- one
// stage buffer each, both read under one barrier, a second barrier before the next layer writes them again -- and propagates W_l^T d_l
// (rounded to half: g_{l-1}) and W_l^T p_l (fp32) from the same transposed weight fragments.  The weight gradients are rounded once, after
// both terms, in the first-order kernel's order: chunks from the segment's start, rounds through the accumulator, k_bmlp_reduce.
template <bool WGRAD, bool CURVED>
__global__ void __launch_bounds__(BM_THREADS) k_bmlp_bwd2(const BmlpDesc d, const uint32_t S, const uint32_t n, const uint32_t* __restrict__ offsets, const MatView x, const MatView v,
                                                          const half_t* __restrict__ hidden, const half_t* __restrict__ dy, const half_t* __restrict__ params,
                                                          const half_t* __restrict__ U, const half_t* __restrict__ Z, const half_t* __restrict__ C, const MatViewMut dx,
                                                          half_t* __restrict__ grads, const uint32_t accumulate, float* __restrict__ partials) {
	extern __shared__ __attribute__((aligned(16))) half_t lds[];
	half_t* W = lds;
	half_t* stage = W + d.lds_halves;
	float* accs = (float*)(stage + 2 * BM_STAGE);
	if (blockIdx.x >= d.n_networks * S) {
		if (dx.data) for_unowned(d, offsets, n, blockIdx.x - d.n_networks * S, d.in_dims, [&](uint32_t row, uint32_t col) { dx.data[(size_t)row * dx.stride_sample + (size_t)col * dx.stride_dim] = 0.0f; });
		return;
	}
	const uint32_t k = blockIdx.x / S, s_wg = blockIdx.x % S;
	const Segment seg = segment_of(d, offsets, n, k);
	const uint32_t n_chunks = (seg.end - seg.begin + BMLP_CHUNK - 1) / BMLP_CHUNK;
	if (n_chunks == 0) { // an empty network: +0 under Overwrite, nothing under Accumulate
		if (WGRAD && s_wg == 0 && !accumulate) {
			for (uint32_t i = threadIdx.x; i < d.n_params; i += BM_THREADS) grads[(size_t)k * d.n_params + i] = (half_t)0.0f;
		}
		return;
	}
	if (s_wg >= n_chunks) return;
	load_weights(d, params + (size_t)k * d.n_params, W);
	__syncthreads();

	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
	const uint32_t tr_row = c >> 2, tr_col = 4 * (c & 3);
	// the last layer with curvature: p_l = 0 above it (the hidden layers share one activation, so it is the last layer or the one below)
	const uint32_t top = bmlp_curved(d.output_activation) ? d.n_layers - 1 : d.n_layers - 2;
	uint32_t phase = 0;
	for (uint32_t ch = s_wg; ch < n_chunks; ch += S) {
		const uint32_t chunk_begin = seg.begin + ch * BMLP_CHUNK, chunk_end = min(chunk_begin + BMLP_CHUNK, seg.end);
		if (WGRAD) clear_accumulators(d, accs, wave, lane);
		for (uint32_t r0 = chunk_begin; r0 < chunk_end; r0 += BM_ROUND) {
			const uint32_t row = r0 + 16 * wave + c;
			const bool valid = row < chunk_end;
			h8 g[2]; // g_l, rounded to half
			f4 back[4]; // W_{l+1}^T p_{l+1}, fp32
#pragma unroll
			for (int s = 0; s < 2; ++s) g[s] = load_rows(dy, d.out_width, d.out_width, row, valid, s, q);
#pragma unroll
			for (int b = 0; b < 4; ++b) back[b] = f4{0.0f, 0.0f, 0.0f, 0.0f};
			for (uint32_t l = d.n_layers - 1;; --l) {
				const BmlpLayer L = d.layers[l];
				const uint32_t act = l + 1 == d.n_layers ? d.output_activation : d.activation;
				const bool curved = CURVED && bmlp_curved(act), with_p = CURVED && l <= top;
				const Slot at = slot_of(d, n, l);
				const uint32_t nb = L.rows / 16;
				h8 dl[2], pl[2];
#pragma unroll
				for (int s = 0; s < 2; ++s) {
					dl[s] = g[s]; // no activation: d_l = g_l, p_l = W_{l+1}^T p_{l+1}
					h8 zl, cl;
					if (act != (uint32_t)Activation::None) zl = load_rows(Z + at.base, at.stride, L.rows, row, valid, s, q);
					if (curved) cl = load_rows(C + at.base, at.stride, L.rows, row, valid, s, q);
#pragma unroll
					for (int j = 0; j < 8; ++j) {
						const int b = 2 * s + (j >> 2);
						const bool in = (uint32_t)b < nb;
						const float d1 = act != (uint32_t)Activation::None ? act_d1(act, (float)zl[j]) : 1.0f;
						if (act != (uint32_t)Activation::None) dl[s][j] = in ? rounded_half((float)g[s][j] * d1) : (half_t)0.0f;
						if (CURVED) {
							const float r = curved ? (float)rounded_half((float)cl[j] * (float)g[s][j]) : 0.0f;
							pl[s][j] = in && with_p ? rounded_half(__builtin_fmaf(d1, back[b][j & 3], r)) : (half_t)0.0f;
						}
					}
				}
				if (WGRAD) {
					h8 uv[2]; // u_{l-1}
#pragma unroll
					for (int s = 0; s < 2; ++s) {
						uv[s] = l == 0 ? load_tangent(d, v.data, v.stride_sample, v.stride_dim, row, valid, s, q)
						               : load_rows(U + (size_t)(l - 1) * n * d.width, d.width, d.width, row, valid, s, q);
					}
					half_t* Ds = stage + (CURVED ? 0 : phase) * BM_STAGE;
					half_t* Us = Ds + BM_ROUND * BM_LD;
					half_t* Ps = stage + BM_STAGE;
					half_t* Hs = Ps + BM_ROUND * BM_LD;
					const uint32_t mine = (16 * wave + c) * BM_LD + 4 * q;
					stage_row(Ds + mine, dl);
					stage_row(Us + mine, uv);
					if (with_p) {
						h8 hv[2]; // h_{l-1}
#pragma unroll
						for (int s = 0; s < 2; ++s) hv[s] = l == 0 ? load_input(d, x, row, valid, s, q) : load_rows(hidden + (size_t)(l - 1) * n * d.width, d.width, d.width, row, valid, s, q);
						stage_row(Ps + mine, pl);
						stage_row(Hs + mine, hv);
					}
					__syncthreads();
					const uint32_t nbc = L.cols / 16, n_blocks = nb * nbc;
					for (uint32_t bi = wave; bi < n_blocks; bi += BM_WAVES) {
						float* ap = accs + L.w_off + bi * 256 + lane * 4;
						f4 acc = staged_product(Ds, Us, bi / nbc, bi % nbc, lane, *(f4*)ap);
						if (with_p) acc = staged_product(Ps, Hs, bi / nbc, bi % nbc, lane, acc);
						*(f4*)ap = acc;
					}
					if (CURVED) __syncthreads(); // both buffers are written again by the next layer
					else phase ^= 1;             // one product per layer: two alternating buffers, one barrier
				}
				if (l == 0 && !(CURVED && dx.data)) break;
				// W_l^T d_l and W_l^T p_l: every transposed weight fragment feeds both
				const half_t* Wl = W + L.lds_off + (4 * q + tr_row) * (L.cols + 8) + tr_col;
				const uint32_t nbc = L.cols / 16;
				f4 da[4];
#pragma unroll
				for (int b = 0; b < 4; ++b) {
					da[b] = f4{0.0f, 0.0f, 0.0f, 0.0f};
					back[b] = f4{0.0f, 0.0f, 0.0f, 0.0f};
					if ((uint32_t)b < nbc) {
#pragma unroll
						for (int s = 0; s < 2; ++s) {
							if (32u * s < L.rows) {
								const half_t* p = Wl + 32 * s * (L.cols + 8) + 16 * b;
								const h8 af = join(lds_read_tr(p), 32u * s + 16 < L.rows ? lds_read_tr(p + 16 * (L.cols + 8)) : zero4());
								if (l > 0) da[b] = mfma(af, dl[s], da[b]);
								if (with_p) back[b] = mfma(af, pl[s], back[b]);
							}
						}
					}
				}
				if (l == 0) { // dS/dinput = W_1^T p_1: the padded columns dropped, float
#pragma unroll
					for (int b = 0; b < 4; ++b) {
#pragma unroll
						for (int r = 0; r < 4; ++r) {
							const uint32_t f = 16 * b + 4 * q + r;
							if (valid && f < d.in_dims) dx.data[(size_t)row * dx.stride_sample + (size_t)f * dx.stride_dim] = (float)(half_t)back[b][r];
						}
					}
					break;
				}
#pragma unroll
				for (int s = 0; s < 2; ++s) {
#pragma unroll
					for (int j = 0; j < 8; ++j) {
						const int b = 2 * s + (j >> 2);
						g[s][j] = (uint32_t)b < nbc ? (half_t)da[b][j & 3] : (half_t)0.0f;
					}
				}
			}
		}
		if (WGRAD) flush_chunk(d, accs, wave, lane, n_chunks == 1 ? nullptr : partials + (size_t)(2 * (seg.begin / BMLP_CHUNK) + ch) * d.n_params, grads + (size_t)k * d.n_params, accumulate != 0);
	}
}

uint32_t cu_count() {
	static const uint32_t count = [] {
		int dev = 0, v = 0;
		HIP_CHECK_THROW(hipGetDevice(&dev));
		HIP_CHECK_THROW(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
		return (uint32_t)std::max(v, 1);
	}();
	return count;
}
// workgroups per network: one per `rows_per_workgroup` of the average segment, and no more than fill the device four times over
uint32_t workgroups_per_network(const BmlpDesc& d, const uint32_t n, const uint32_t rows_per_workgroup) {
	const uint32_t by_rows = div_round_up(div_round_up(n, d.n_networks), rows_per_workgroup);
	return std::max(1u, std::min(by_rows, div_round_up(4 * cu_count(), d.n_networks)));
}
template <typename K>
void allow_lds(K kernel, const size_t bytes) {
	if (bytes > 64 * 1024) HIP_CHECK_THROW(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

} // namespace

void bmlp_forward(hipStream_t stream, const BmlpDesc& d, uint32_t n, const uint32_t* offsets, MatView x, const void* params, void* out, void* hidden) {
	if (n == 0) return;
	const uint32_t S = workgroups_per_network(d, n, BM_WAVES * BM_T * 16);
	const size_t lds = bmlp_forward_lds_bytes(d);
	const dim3 grid(d.n_networks * S + BM_ZERO_BLOCKS);
	auto go = [&](auto kernel) {
		allow_lds(kernel, lds);
		hipLaunchKernelGGL(kernel, grid, dim3(BM_THREADS), lds, stream, d, S, n, offsets, x, (const half_t*)params, (half_t*)out, (half_t*)hidden);
		HIP_CHECK_THROW(hipGetLastError());
	};
	if (hidden) go(k_bmlp_fwd<true>);
	else go(k_bmlp_fwd<false>);
}

void bmlp_backward(hipStream_t stream, const BmlpDesc& d, uint32_t n, const uint32_t* offsets, MatView x, const void* hidden, const void* out, const void* dL_dout,
                   const void* params, const MatViewMut* dL_dinput, void* gradients, GradientMode mode, float* partials) {
	if (n == 0) return;
	const bool wgrad = mode != GradientMode::Ignore;
	if (!wgrad && !dL_dinput) return;
	const uint32_t S = workgroups_per_network(d, n, BMLP_CHUNK), accumulate = mode == GradientMode::Accumulate ? 1u : 0u;
	const size_t lds = wgrad ? bmlp_backward_lds_bytes(d) : bmlp_forward_lds_bytes(d);
	const MatViewMut dx = dL_dinput ? *dL_dinput : MatViewMut{nullptr, 0u, 0u};
	const dim3 grid(d.n_networks * S + BM_ZERO_BLOCKS);
	auto go = [&](auto kernel) {
		allow_lds(kernel, lds);
		hipLaunchKernelGGL(kernel, grid, dim3(BM_THREADS), lds, stream, d, S, n, offsets, x, (const half_t*)hidden, (const half_t*)out, (const half_t*)dL_dout, (const half_t*)params, dx,
		                   (half_t*)gradients, accumulate, partials);
		HIP_CHECK_THROW(hipGetLastError());
	};
	if (wgrad) go(k_bmlp_bwd<true>);
	else go(k_bmlp_bwd<false>);
	if (wgrad && partials) {
		hipLaunchKernelGGL(k_bmlp_reduce, dim3(d.n_networks * div_round_up(d.n_params, BM_THREADS)), dim3(BM_THREADS), 0, stream, d, n, offsets, (const float*)partials, (half_t*)gradients,
		                   accumulate);
		HIP_CHECK_THROW(hipGetLastError());
	}
}

void bmlp_tangent(hipStream_t stream, const BmlpDesc& d, uint32_t n, const uint32_t* offsets, MatView x, MatView v, uint32_t v_next, uint32_t n_tangents, const void* params,
                  void* jvp, uint32_t jvp_ld, void* out, void* u, void* z, void* c) {
	if (n == 0) return;
	const bool store = u != nullptr;
	CHECK_THROW(n_tangents >= 1 && n_tangents <= BMLP_TANGENT_GROUP && (!store || (n_tangents == 1 && z && c)));
	const uint32_t S = workgroups_per_network(d, n, 2 * BM_WAVES * 16); // two trips, so that a workgroup's weight load serves 128 rows
	const size_t lds = bmlp_forward_lds_bytes(d);
	const dim3 grid(d.n_networks * S + BM_ZERO_BLOCKS);
	auto go = [&](auto kernel) {
		allow_lds(kernel, lds);
		hipLaunchKernelGGL(kernel, grid, dim3(BM_THREADS), lds, stream, d, S, n, offsets, x, v, v_next, (const half_t*)params, (half_t*)jvp, jvp_ld, (half_t*)out, (half_t*)u, (half_t*)z,
		                   (half_t*)c);
		HIP_CHECK_THROW(hipGetLastError());
	};
	if (store) go(k_bmlp_tangent<1, true>);
	else if (n_tangents == 1) go(k_bmlp_tangent<1, false>);
	else if (n_tangents == 2) go(k_bmlp_tangent<2, false>);
	else go(k_bmlp_tangent<3, false>);
}

void bmlp_backward_second(hipStream_t stream, const BmlpDesc& d, uint32_t n, const uint32_t* offsets, MatView x, MatView v, const void* hidden, const void* dL_dout, const void* params,
                          const void* u, const void* z, const void* c, const MatViewMut* dL_dinput, void* gradients, GradientMode mode, float* partials) {
	if (n == 0) return;
	const bool wgrad = mode != GradientMode::Ignore, curved = bmlp_any_curvature(d);
	const MatViewMut dx = dL_dinput && curved ? *dL_dinput : MatViewMut{nullptr, 0u, 0u};
	if (!wgrad && !dx.data) return;
	const uint32_t S = workgroups_per_network(d, n, BMLP_CHUNK), accumulate = mode == GradientMode::Accumulate ? 1u : 0u;
	const size_t lds = wgrad ? bmlp_backward_lds_bytes(d) : bmlp_forward_lds_bytes(d);
	const dim3 grid(d.n_networks * S + BM_ZERO_BLOCKS);
	auto go = [&](auto kernel) {
		allow_lds(kernel, lds);
		hipLaunchKernelGGL(kernel, grid, dim3(BM_THREADS), lds, stream, d, S, n, offsets, x, v, (const half_t*)hidden, (const half_t*)dL_dout, (const half_t*)params, (const half_t*)u,
		                   (const half_t*)z, (const half_t*)c, dx, (half_t*)gradients, accumulate, partials);
		HIP_CHECK_THROW(hipGetLastError());
	};
	if (wgrad && curved) go(k_bmlp_bwd2<true, true>);
	else if (wgrad) go(k_bmlp_bwd2<true, false>);
	else go(k_bmlp_bwd2<false, true>);
	if (wgrad && partials) {
		hipLaunchKernelGGL(k_bmlp_reduce, dim3(d.n_networks * div_round_up(d.n_params, BM_THREADS)), dim3(BM_THREADS), 0, stream, d, n, offsets, (const float*)partials, (half_t*)gradients,
		                   accumulate);
		HIP_CHECK_THROW(hipGetLastError());
	}
}

} // namespace tcnn_amd
