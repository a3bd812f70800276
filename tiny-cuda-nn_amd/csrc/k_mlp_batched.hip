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
		if (WGRAD) { // the wave's own blocks (nobody else ever touches them: no barrier)
			for (uint32_t l = 0; l < d.n_layers; ++l) {
				const uint32_t n_blocks = d.layers[l].rows * d.layers[l].cols / 256;
				for (uint32_t bi = wave; bi < n_blocks; bi += BM_WAVES) *(f4*)(accs + d.layers[l].w_off + bi * 256 + lane * 4) = f4{0.0f, 0.0f, 0.0f, 0.0f};
			}
		}
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
						const uint32_t rb = bi / nbc, cb = bi % nbc;
						float* ap = accs + L.w_off + bi * 256 + lane * 4;
						f4 acc = *(f4*)ap;
#pragma unroll
						for (int ks = 0; ks < 2; ++ks) {
							const uint32_t r = 32 * ks + 8 * q + tr_row;
							const h8 af = join(lds_read_tr(Zs + r * BM_LD + 16 * rb + tr_col), lds_read_tr(Zs + (r + 4) * BM_LD + 16 * rb + tr_col));
							const h8 bf = join(lds_read_tr(As + r * BM_LD + 16 * cb + tr_col), lds_read_tr(As + (r + 4) * BM_LD + 16 * cb + tr_col));
							acc = mfma(af, bf, acc);
						}
						*(f4*)ap = acc;
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
		if (WGRAD) {
			// a segment of one chunk: rounded and stored (or added) here; else the chunk's fp32 sum goes to its slot for k_bmlp_reduce
			const bool direct = n_chunks == 1;
			float* slot = direct ? nullptr : partials + (size_t)(2 * (seg.begin / BMLP_CHUNK) + ch) * d.n_params;
			half_t* gk = grads + (size_t)k * d.n_params;
			for (uint32_t l = 0; l < d.n_layers; ++l) {
				const BmlpLayer L = d.layers[l];
				const uint32_t nbc = L.cols / 16, n_blocks = (L.rows / 16) * nbc;
				for (uint32_t bi = wave; bi < n_blocks; bi += BM_WAVES) {
					const f4 acc = *(const f4*)(accs + L.w_off + bi * 256 + lane * 4);
					const uint32_t at = L.w_off + (16 * (bi / nbc) + 4 * q) * L.cols + 16 * (bi % nbc) + c;
#pragma unroll
					for (int r = 0; r < 4; ++r) {
						if (direct) store_gradient(gk + at + r * L.cols, acc[r], accumulate != 0);
						else slot[at + r * L.cols] = acc[r];
					}
				}
			}
		}
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

} // namespace tcnn_amd
