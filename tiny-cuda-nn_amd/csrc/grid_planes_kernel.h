// grid_planes_kernel.h -- the training-step form of the grid encoding forward pass (kernel_grid, grid.h:49-212) for gfx950.
//
// Same arithmetic as k_grid_fwd (fp32 corner weights, fp16 fma chain in corner order -- bit-identical results), different
// SHAPE, chosen for where the time goes on MI355X: the gathers of one level hit a 2^log2_hashmap_size * F * 2 byte table
// (2 MB for T = 2^19, F = 2) that fits in ONE XCD's 4 MB L2 but not next to the other 15 levels.
//   * level-major work list, cut into per-XCD runs on the host (grid_planes_plan): workgroup b runs on XCD b % 8 and walks
//     that XCD's run in order, so an XCD gathers from one or two tables at a time and they stay in its L2;
//   * a thread owns ONE level of SPT samples (8 x 4 gathers in flight), and the output is written as level planes
//     half [L][n][F] (dense 256-B stores per wave) which the fused MLP kernel reads directly;
//   * the sample filter of the owner-computes scatter is produced here.  Round 4 (LISTS): as HIT LISTS (GridHitLists, tcnn_common.h) --
//     a workgroup's item (FP_THREADS x FP_SPT samples of one level) is counting-sorted by chunk in LDS -- a rank per element from one
//     returning LDS add on the chunk's counter, a 64-lane scan for the chunks' offsets -- and leaves as ONE contiguous, chunk-sorted run
//     in the item's own region of the level's pool (coalesced stores) with its 65 offsets beside it.  No global atomics.  The scatter
//     then walks the items' runs of its chunk instead of scanning a bit plane.  Round 5: an element is a cell ROW with its two entries and
//     its two half weights (8 bytes + a 16-bit sample number) -- this kernel has them in registers anyway, and the owner then needs neither coordinates nor hashes.
//     Before: bit planes over samples per (level, chunk), built in LDS with integer ORs (or ballots for levels with few chunks); kept
//     for callers without lists.
// Two translation units instantiate the kernel: k_grid_planes.hip its generic body, k_grid_planes_plain.hip the PLAIN one (built without the
// packed fp32 instructions, build.py).
#pragma once

#include "grid_device.h"
#include "mlp_side_jobs.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace tcnn_amd {
namespace {

constexpr int FP_THREADS = 128; // 2 waves per workgroup
// ... and with hit lists: a work item is FP_LIST_THREADS x FP_SPT samples, and the item's run of a chunk (samples x rows / chunks elements
// of 8 bytes) is what the chunk's owner reads in one piece -- 16 elements = 128 bytes from a 512-sample item, and every piece drags the
// rest of its first and last 128-byte line along (measured in the owners: 19 us per task from such runs, 10 from one contiguous list,
// profiles/r05_scatter_dev.txt)
#ifndef TCNN_FP_LIST_THREADS
#define TCNN_FP_LIST_THREADS 256
#endif
constexpr int FP_LIST_THREADS = TCNN_FP_LIST_THREADS;

constexpr int FP_MAX_CHUNKS = GRID_FILTER_MAX_CHUNKS; // bit planes per level: levels cut into more chunks get no filter (they are binned, k_grid_bin.hip)
constexpr int FP_PER_LANE = FP_MAX_CHUNKS / 64;       // chunks whose words one lane carries out (chunk = lane + 64 j)

// PLAIN: the address `bytes` behind a wave-uniform base where the offsets fit 32 bits (grid_planes_plain) -- an access with a scalar base
// and a 32-bit offset, where `base[(size_t)index * ...]` builds the whole address in vector registers.
template <typename T>
__device__ inline T* near_at(T* base, uint32_t bytes) {
	typedef typename std::conditional<std::is_const<T>::value, const char, char>::type byte_t;
	return (T*)((byte_t*)base + bytes);
}

// FP_SPT = samples per thread = consecutive 64-sample groups per wave; a work item is FP_THREADS * FP_SPT samples of one level.
// Shapes: 4 (16 gathers in flight per thread; 8 is kept for A/B runs), and 2 for the big 3-D grids whose 8 corners x 4 features would
// not fit the registers.
// PLAIN (GridForwardRoute::plain, decided on the host by grid_planes_plain): hit lists, Linear interpolation, a hash that is a product with
// primes, and every table, plane and coordinate within 32-bit byte offsets.  The launch constants are compile-time constants then, a
// level's kind picks one of three phase-1 bodies per item, the two corners of a row share their index terms, and addresses are a scalar
// base + a 32-bit offset.  Same work items, same loads, same bits (DESIGN.md "The forward kernel's instruction stream").  !PLAIN is the
// body as it was and serves everything else.
template <int D, int F, int FP_SPT, bool LISTS, bool PLAIN>
__global__ void __launch_bounds__(LISTS ? FP_LIST_THREADS : FP_THREADS) k_grid_fwd_planes(
	const GridMeta* __restrict__ meta, const uint32_t* __restrict__ work, const uint32_t max_items, const uint32_t blocks_per_xcd, const uint32_t n, const MatView x,
	const half_t* __restrict__ grid, half_t* __restrict__ out, unsigned long long* __restrict__ bits, const MlpPrepJob prep, const GridHitLists lists
) {
	typedef typename VecOf<half_t, F>::type vecF;
	constexpr int THREADS = LISTS ? FP_LIST_THREADS : FP_THREADS;
	if (prep.image) { // side job (mlp_side_jobs.h): the fragment images of the network this batch is encoded for; independent of everything below
		const uint32_t total = (prep.desc.n_frags_fwd + prep.desc.n_frags_bwd + prep.desc.n_frags_r32) * 512;
		for (uint32_t e = blockIdx.x * THREADS + threadIdx.x; e < total; e += gridDim.x * THREADS) mlp_prep_element(prep.desc, (const half_t*)prep.params, (half_t*)prep.image, e);
	}
	constexpr int FP_WAVE_SAMPLES = 64 * FP_SPT;
	constexpr int FP_ITEM_SAMPLES = THREADS * FP_SPT;
	constexpr int STAGE_ELEMS = FP_ITEM_SAMPLES << (D - 1); // one element per (sample, row) of an item
	// bit planes (!LISTS) or the item's counting sort (LISTS): the staged elements, counters, offsets
	constexpr int STAGE_U64 = STAGE_ELEMS * (int)GRID_HIT_WORDS / 2 + STAGE_ELEMS / 4; // the item's elements: 8 bytes each + their 16-bit sample numbers
	static_assert(!LISTS || FP_ITEM_SAMPLES <= 65536, "16-bit sample numbers inside an item");
	__shared__ __attribute__((aligned(16))) unsigned long long lds_raw[LISTS ? STAGE_U64 + 72 : (FP_THREADS / 64) * FP_SPT * FP_MAX_CHUNKS];
	typedef unsigned long long plane_row[FP_SPT][FP_MAX_CHUNKS];
	plane_row* planes = (plane_row*)lds_raw; // [FP_THREADS / 64][FP_SPT][FP_MAX_CHUNKS]
	typedef __attribute__((address_space(3))) uint32_t lds_u32;
	uint32_t* l_stage = (uint32_t*)lds_raw;                 // [STAGE_ELEMS][GRID_HIT_WORDS] the item's elements in chunk order
	uint16_t* l_sidx = (uint16_t*)(lds_raw + STAGE_ELEMS * (int)GRID_HIT_WORDS / 2); // [STAGE_ELEMS] their samples, relative to the item's first
	uint32_t* l_cnt = (uint32_t*)(lds_raw + STAGE_U64);     // [64] elements of this item per chunk (zero between items)
	uint32_t* l_off = l_cnt + 64;                           // [64] first staged position of the chunk
	uint32_t* l_total = l_cnt + 128;
	static_assert(FP_MAX_CHUNKS == 64, "one lane per chunk");
	if constexpr (LISTS) {
		if (threadIdx.x < 64) l_cnt[threadIdx.x] = 0;
		// the counter set of the next forward launch on this stream (nobody reads it any more: the scatter that did has finished)
		if (blockIdx.x == gridDim.x - 1 && lists.zero_counts) {
			for (uint32_t e = threadIdx.x; e < meta->n_levels * GRID_HIT_COUNT_STRIDE; e += THREADS) lists.zero_counts[e] = 0;
		}
		__syncthreads();
	}

	const uint32_t tid = threadIdx.x;
	const uint32_t lane = tid & 63;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
	const uint32_t n_items = work[xcd];
	const uint32_t* __restrict__ items = work + 8 + (size_t)xcd * max_items;

	const uint32_t interpolation = PLAIN ? (uint32_t)InterpolationType::Linear : meta->interpolation;
	const uint32_t hash_type = PLAIN ? (uint32_t)HashType::Prime : meta->hash_type; // (PLAIN: any of the prime hashes -- they differ in meta->primes only)
	uint32_t primes[D];
#pragma unroll
	for (int d = 0; d < D; ++d) primes[d] = meta->primes[d];
	const uint32_t n_words = n / 64;
	constexpr int C = 1 << D;
	constexpr int R_ROWS = C / 2;
	constexpr uint32_t HIT_SHIFT = grid_hit_mask_shift(D);
	constexpr uint32_t CH_SHIFT = 18; // PLAIN: cr carries the chunk as the byte offset of its l_off word
	static_assert(!PLAIN || LISTS, "the PLAIN body writes hit lists");

	for (uint32_t it = slot; it < n_items; it += blocks_per_xcd) {
		const uint32_t w = items[it];
		const uint32_t level = w >> 24;
		// first sample of this wave: a wave's FP_WAVE_SAMPLES positions lie inside one window of the item (GridItemMap), a dense run of samples
		uint32_t base = (w & 0xffffffu) * FP_ITEM_SAMPLES + wave * FP_WAVE_SAMPLES;
		if constexpr (LISTS) base = grid_item_sample(lists.map, w & 0xffffffu, wave * FP_WAVE_SAMPLES);
		if constexpr (!LISTS) { if (base >= n) continue; } // (LISTS: the waves of a workgroup meet at barriers; a wave past the end recomputes the last sample and emits nothing)
		const GridLevel lv = meta->levels[level];
		const half_t* __restrict__ lgrid = grid + (size_t)lv.offset * F;
		half_t* __restrict__ lout = out + (size_t)level * n * F;
		const uint32_t n_chunks = lv.scatter_n_chunks;
		const bool want_bits = !LISTS && bits != nullptr && n_chunks > 1 && n_chunks <= FP_MAX_CHUNKS;
		const bool lds_or = want_bits && n_chunks > 8;
		const bool want_lists = LISTS && n_chunks > 1 && n_chunks <= FP_MAX_CHUNKS; // workgroup-uniform: depends on the level only
		uint32_t cr[FP_SPT][R_ROWS]; // per (sample, row): chunk << 16 (PLAIN: << CH_SHIFT) | rank inside (item, chunk); ~0: no element
		uint32_t ipair[FP_SPT][R_ROWS]; // ... and its word 1: entry of corner A | entry of corner B << 16, relative to the chunk (0xffff: none)
		const bool nearest = !PLAIN && interpolation == (uint32_t)InterpolationType::Nearest;

		if (lds_or) {
#pragma unroll
			for (int k = 0; k < FP_SPT; ++k)
#pragma unroll
				for (int j = 0; j < FP_PER_LANE; ++j) planes[wave][k][lane + 64 * j] = 0ull;
		}

		// ---- phase 1: positions, indices, all gathers in flight.
		// A gather costs ~2 clocks per lane per CU whatever its width (tools/ubench/gather.hip), so the two corners of a cell
		// that differ only in x are fetched as ONE 2-entry load wherever they are neighbours in memory: always for dense-style
		// levels (index(x + 1) = index(x) + 1), and for hashed levels with prime[0] == 1 when x is even (index(x + 1) =
		// index(x) ^ 1).  A lane whose second corner is not in the pair issues an extra load; masked-off lanes cost nothing.
		constexpr int R = C / 2; // rows = corner pairs (x, x + 1)
		typedef typename VecOf<half_t, 2 * F>::type vecP __attribute__((aligned(2 * F)));
		vecP P[FP_SPT][R];
		vecF E[FP_SPT][R];
		uint32_t sel[FP_SPT]; // per row 3 bits: corner 0 is the pair's high entry | corner 1 is the pair's high entry | corner 1 came by its own load
		float pos[FP_SPT][D];
		unsigned long long touched[FP_SPT];
		auto note_chunk = [&](const int k, const uint32_t index) {
			const uint32_t ch = scatter_chunk(lv, index);
			if (lds_or) {
				// bit `lane` of word [k][ch]; integer LDS atomics run at ~4 lane-ops/clk/CU
				__hip_atomic_fetch_or((__attribute__((address_space(3))) uint32_t*)&planes[wave][k][ch] + (lane >> 5), 1u << (lane & 31), __ATOMIC_RELAXED,
				                      __HIP_MEMORY_SCOPE_WAVEFRONT);
			} else {
				touched[k] |= 1ull << ch;
			}
		};
		if constexpr (!PLAIN) {
#pragma unroll
			for (int k = 0; k < FP_SPT; ++k) {
				const uint32_t i = min(base + k * 64 + lane, n - 1); // groups past the end recompute the last sample and store nothing
				float xin[D];
				load_coords<D>(x, i, xin);
				uint32_t cell[D];
				float pd;
#pragma unroll
				for (int d = 0; d < D; ++d) cell[d] = pos_fract(xin[d], lv.scale, interpolation, &pos[k][d], &pd);
				touched[k] = 0;
				sel[k] = 0;
				if constexpr (LISTS) {
#pragma unroll
					for (int r = 0; r < R_ROWS; ++r) { cr[k][r] = 0xffffffffu; ipair[k][r] = 0; }
				}
				const bool lists_here = LISTS && want_lists && base + k * 64 + lane < n;
#pragma unroll
				for (int r = 0; r < R; ++r) {
					if (r > 0 && nearest) { P[k][r] = P[k][0]; E[k][r] = E[k][0]; continue; }
					uint32_t local[D];
					local[0] = cell[0];
#pragma unroll
					for (int d = 1; d < D; ++d) local[d] = cell[d] + ((r >> (d - 1)) & 1);
					const uint32_t idx0 = level_index<D>(lv, primes, hash_type, local);
					local[0] = cell[0] + 1;
					const uint32_t idx1 = nearest ? idx0 : level_index<D>(lv, primes, hash_type, local);
					const uint32_t a0 = lv.hashed ? (idx0 & ~1u) : min(idx0, lv.size - 2u);
					P[k][r] = *(const vecP*)&lgrid[(size_t)a0 * F];
					const uint32_t d1 = idx1 - a0;
					const bool own = d1 > 1u;
					vecF e;
#pragma unroll
					for (int f = 0; f < F; ++f) { if constexpr (F == 1) e = (half_t)0.0f; else e[f] = (half_t)0.0f; }
					if (own) e = *(const vecF*)&lgrid[(size_t)idx1 * F];
					E[k][r] = e;
					sel[k] |= ((idx0 - a0) | ((d1 & 1u) << 1) | (own ? 4u : 0u)) << (3 * r);
					if (want_bits) {
						note_chunk(k, idx0);
						if (!nearest) note_chunk(k, idx1);
					}
					if constexpr (LISTS) {
						// One element per (sample, row), in the list of corner A's chunk; corner B rides along when it lies in the same chunk -- else (a
						// row that straddles two chunks, one in ~8000 on hashed levels) it goes to the level's straggler list.
						if (lists_here) {
							const uint32_t ch_a = scatter_chunk(lv, idx0), first = ch_a * lv.scatter_per_chunk;
							uint32_t rel_b = idx0 - first; // no corner B in this chunk: the element names A's entry twice and gives the second a zero weight
							if (!nearest) {
								const uint32_t ch_b = scatter_chunk(lv, idx1);
								if (ch_b == ch_a) rel_b = idx1 - first;
								else {
									const uint32_t at = atomicAdd(&lists.counts[level * GRID_HIT_COUNT_STRIDE], 1u);
									if (at < lists.straggler_capacity) {
										typedef uint32_t u2 __attribute__((ext_vector_type(2)));
										*(u2*)&lists.stragglers[((size_t)level * lists.straggler_capacity + at) * 2] = u2{i | (2u << (2 * r)) << HIT_SHIFT, ch_b};
									}
								}
							}
							ipair[k][r] = (idx0 - first) | rel_b << 16;
							const uint32_t rank = __hip_atomic_fetch_add((lds_u32*)&l_cnt[ch_a], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
							cr[k][r] = ch_a << 16 | rank;
						}
					}
				}
			}
		} else {
			// One phase-1 body per kind of level, chosen per item.  KIND 1: hashed into a power-of-two table cut into power-of-two chunks -- every
			// hashed level of a HashGrid; 2: dense; 0: whatever else the level says, read per row.
			auto phase1 = [&](auto kind) __attribute__((always_inline)) {
				constexpr int KIND = decltype(kind)::value;
				const bool hashed = KIND == 0 ? lv.hashed != 0 : KIND == 1;
				// KIND 1, 2: index = wrap(t_0 (+) t_1 (+) ...), t_d = cell_d * mult_d, (+) = xor (hashed) or + (dense) -- grid_index() as level_index<D>
				// computes it, with (cell_d + 1) * mult_d taken as t_d + mult_d: the same uint32
				uint32_t mult[D];
#pragma unroll
				for (int d = 0; d < D; ++d) mult[d] = hashed ? primes[d] : lv.stride[d];
				auto wrap = [&](const uint32_t index) -> uint32_t {
					if (KIND == 1 || lv.size_mask) return index & lv.size_mask;
					return index >= lv.size ? index % lv.size : index;
				};
				const bool chunk_shift = KIND == 1 || lv.scatter_shift != 0xffffffffu;
#pragma unroll
				for (int k = 0; k < FP_SPT; ++k) {
					const uint32_t i = min(base + k * 64 + lane, n - 1); // groups past the end recompute the last sample and store nothing
					float xin[D];
					if ((D == 2 || D == 4) && x.stride_dim == 1 && x.stride_sample == D) { // load_coords' wide load
						typedef float vecD __attribute__((ext_vector_type(D)));
						const vecD v = *(const vecD*)near_at(x.data, i * (D * 4));
#pragma unroll
						for (int d = 0; d < D; ++d) xin[d] = v[d];
					} else load_coords<D>(x, i, xin);
					uint32_t cell[D], term[D];
					float pd;
#pragma unroll
					for (int d = 0; d < D; ++d) {
						cell[d] = pos_fract(xin[d], lv.scale, interpolation, &pos[k][d], &pd);
						term[d] = cell[d] * mult[d];
					}
					sel[k] = 0;
					const bool lists_here = want_lists && base + k * 64 + lane < n;
#pragma unroll
					for (int r = 0; r < R; ++r) {
						cr[k][r] = 0xffffffffu;
						ipair[k][r] = 0;
						uint32_t idx0, idx1;
						if constexpr (KIND == 0) {
							uint32_t local[D];
							local[0] = cell[0];
#pragma unroll
							for (int d = 1; d < D; ++d) local[d] = cell[d] + ((r >> (d - 1)) & 1);
							idx0 = level_index<D, false>(lv, primes, hash_type, local);
							local[0] = cell[0] + 1;
							idx1 = level_index<D, false>(lv, primes, hash_type, local);
						} else {
							uint32_t rest = 0; // the row's share: dimensions 1 .. D - 1
#pragma unroll
							for (int d = 1; d < D; ++d) {
								const uint32_t t = term[d] + (((r >> (d - 1)) & 1) ? mult[d] : 0u);
								rest = KIND == 1 ? rest ^ t : rest + t;
							}
							idx0 = wrap(KIND == 1 ? term[0] ^ rest : term[0] + rest);
							idx1 = wrap(KIND == 1 ? (term[0] + mult[0]) ^ rest : term[0] + mult[0] + rest);
						}
						const uint32_t a0 = hashed ? (idx0 & ~1u) : min(idx0, lv.size - 2u);
						P[k][r] = *(const vecP*)near_at(lgrid, a0 * (F * 2));
						const uint32_t d1 = idx1 - a0;
						const bool own = d1 > 1u;
						vecF e;
#pragma unroll
						for (int f = 0; f < F; ++f) { if constexpr (F == 1) e = (half_t)0.0f; else e[f] = (half_t)0.0f; }
						if (own) e = *(const vecF*)near_at(lgrid, idx1 * (F * 2));
						E[k][r] = e;
						sel[k] |= ((idx0 - a0) | ((d1 & 1u) << 1) | (own ? 4u : 0u)) << (3 * r);
						if (lists_here) { // the row's element, as in the generic body
							// A's chunk and its entry inside it (power-of-two chunks: the high and the low bits)
							const uint32_t ch_a = chunk_shift ? idx0 >> lv.scatter_shift : idx0 / lv.scatter_per_chunk;
							const uint32_t rel_a = chunk_shift ? (idx0 & (lv.scatter_per_chunk - 1u)) : idx0 - ch_a * lv.scatter_per_chunk;
							// B lies in A's chunk <=> first <= idx1 < first + per_chunk: one unsigned comparison, and B's chunk only where a straggler needs it
							const uint32_t from_first = idx1 - (idx0 - rel_a);
							uint32_t rel_b = rel_a;
							if (from_first < lv.scatter_per_chunk) rel_b = from_first;
							else {
								const uint32_t at = atomicAdd(&lists.counts[level * GRID_HIT_COUNT_STRIDE], 1u);
								if (at < lists.straggler_capacity) {
									typedef uint32_t u2 __attribute__((ext_vector_type(2)));
									*(u2*)&lists.stragglers[((size_t)level * lists.straggler_capacity + at) * 2] = u2{i | (2u << (2 * r)) << HIT_SHIFT, scatter_chunk(lv, idx1)};
								}
							}
							ipair[k][r] = rel_a | rel_b << 16;
							const uint32_t rank = __hip_atomic_fetch_add((lds_u32*)&l_cnt[ch_a], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
							cr[k][r] = ch_a << CH_SHIFT | rank;
						}
					}
				}
			};
			if (lv.hashed && lv.size_mask && lv.scatter_shift != 0xffffffffu) phase1(std::integral_constant<int, 1>{});
			else if (!lv.hashed) phase1(std::integral_constant<int, 2>{});
			else phase1(std::integral_constant<int, 0>{});
		}
		if constexpr (LISTS) {
			if (want_lists) {
				__syncthreads(); // every element of the item has its rank
				if (wave == 0) {
					const uint32_t cnt = l_cnt[lane];
					l_cnt[lane] = 0;
					uint32_t incl = cnt;
#pragma unroll
					for (int o = 1; o < 64; o <<= 1) {
						const uint32_t up = __shfl_up(incl, o);
						if (lane >= (uint32_t)o) incl += up;
					}
					l_off[lane] = incl - cnt;
					uint32_t* heads = lists.heads + (size_t)level * GRID_HIT_HEADS * lists.n_items + (w & 0xffffffu); // [chunk][item]
#ifdef TCNN_AMD_DEV
					if (!(lists.dev_flags & 4u))
#endif
					heads[(size_t)lane * lists.n_items] = incl - cnt;
					if (lane == 63) { heads[(size_t)64 * lists.n_items] = incl; *l_total = incl; }
				}
				__syncthreads(); // the chunks' offsets are there (the gathers of phase 1 are in flight meanwhile)
			}
		}

		// ---- phase 2: interpolation (grid.h:142-169) and the plane stores
#pragma unroll
		for (int k = 0; k < FP_SPT; ++k) {
			const uint32_t i = base + k * 64 + lane;
			vecF v[C];
#pragma unroll
			for (int r = 0; r < R; ++r) {
				const uint32_t s = sel[k] >> (3 * r);
				vecF lo, hi;
#pragma unroll
				for (int f = 0; f < F; ++f) { lo[f] = P[k][r][f]; hi[f] = P[k][r][F + f]; }
				v[2 * r] = (s & 1u) ? hi : lo;
				v[2 * r + 1] = (s & 4u) ? E[k][r] : ((s & 2u) ? hi : lo);
			}
			half_t acc[F];
			half_t whs[C]; // the corners' weights as halves: what the scatter multiplies dL/dy with (grid.h:254)
#pragma unroll
			for (int idx = 0; idx < C; ++idx) whs[idx] = (half_t)1.0f;
			if (nearest) { // grid.h:121-140
#pragma unroll
				for (int f = 0; f < F; ++f) acc[f] = v[0][f];
			} else {
#pragma unroll
				for (int f = 0; f < F; ++f) acc[f] = (half_t)0.0f;
#pragma unroll
				for (int idx = 0; idx < C; ++idx) {
					float weight = 1;
#pragma unroll
					for (int d = 0; d < D; ++d) weight *= (idx & (1 << d)) == 0 ? 1 - pos[k][d] : pos[k][d];
					asm volatile("" : "+v"(weight)); // round to fp32 first, then to fp16 (see k_grid.hip)
					const half_t wh = (half_t)weight;
					whs[idx] = wh;
#pragma unroll
					for (int f = 0; f < F; ++f) {
						half_t val;
						val = v[idx][f];
						acc[f] = __builtin_fmaf16(wh, val, acc[f]);
					}
				}
			}
			if (base + k * 64 < n) {
				vecF o;
#pragma unroll
				for (int f = 0; f < F; ++f) { if constexpr (F == 1) o = acc[f]; else o[f] = acc[f]; }
				if constexpr (PLAIN) *(vecF*)near_at(lout, i * (F * 2)) = o;
				else *(vecF*)&lout[(size_t)i * F] = o;
			}
			if constexpr (LISTS) { // this sample's elements, staged at their place in chunk order
				if (want_lists) {
#pragma unroll
					for (int r = 0; r < R_ROWS; ++r) {
						const uint32_t v = cr[k][r];
						if (v != 0xffffffffu) {
							const uint32_t at = (PLAIN ? *(const uint32_t*)((const char*)l_off + (v >> 16)) : l_off[v >> 16]) + (v & 0xffffu);
							typedef uint32_t u2 __attribute__((ext_vector_type(2)));
							const uint32_t pr = ipair[k][r];
							const bool no_b = (pr >> 16) == (pr & 0xffffu); // (two corners of a row are never the same entry)
							*(u2*)(l_stage + at * GRID_HIT_WORDS) = u2{pr, (uint32_t)__builtin_bit_cast(uint16_t, whs[2 * r]) | (no_b ? 0u : (uint32_t)__builtin_bit_cast(uint16_t, whs[2 * r + 1]) << 16)};
							l_sidx[at] = (uint16_t)(wave * FP_WAVE_SAMPLES + k * 64 + lane);
						}
					}
				}
			}
		}

		// ---- phase 3 (LISTS): the item's elements, staged in chunk order, leave as one run into the item's region of the level's pool
		if constexpr (LISTS) {
			if (want_lists) {
				__syncthreads();
				typedef uint32_t u4 __attribute__((ext_vector_type(4)));
				// (a region is a whole number of 16-byte quads: the last one of a run may carry a few words of the item before)
				const uint32_t total = *l_total, quads = (total * GRID_HIT_WORDS + 3) / 4, squads = (total + 7) / 8;
				const size_t region = ((size_t)level * lists.n_items + (w & 0xffffffu)) * lists.item_capacity;
				u4* dst = (u4*)(lists.elems + region * GRID_HIT_WORDS);
				u4* sdst = (u4*)(lists.sidx + region);
#ifdef TCNN_AMD_DEV
				if (!(lists.dev_flags & 1u))
#endif
				{ // (plain stores: streamed ones cost the scatter 13 us -- it reads the lists out of the Infinity Cache, which streamed stores pass by)
#ifdef TCNN_AMD_DEV
					if (lists.dev_flags & 8u) { // sc1: written through, not kept in this XCD's L2
						const auto rs_e = __builtin_amdgcn_make_buffer_rsrc((void*)dst, 0, (int)(quads * 16u), 0x00020000);
						const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)sdst, 0, (int)(squads * 16u), 0x00020000);
						for (uint32_t p = tid; p < quads; p += THREADS) __builtin_amdgcn_raw_buffer_store_b128(((const u4*)l_stage)[p], rs_e, p * 16u, 0, 16);
						for (uint32_t p = tid; p < squads; p += THREADS) __builtin_amdgcn_raw_buffer_store_b128(((const u4*)l_sidx)[p], rs_s, p * 16u, 0, 16);
					} else
#endif
					{
					for (uint32_t p = tid; p < quads; p += THREADS) dst[p] = ((const u4*)l_stage)[p];
					for (uint32_t p = tid; p < squads; p += THREADS) sdst[p] = ((const u4*)l_sidx)[p];
					}
				}
			}
		}
		// ---- phase 3: bit planes.  Lane c ends up with the FP_SPT consecutive words of chunk c (and of chunk c + 64): dense runs per lane.
		if (want_bits) {
#pragma unroll
			for (int j = 0; j < FP_PER_LANE; ++j) {
				if (j > 0 && !lds_or) break; // the ballot form serves levels with at most 8 chunks
				unsigned long long mine[FP_SPT];
				const uint32_t ch = lane + 64 * j;
				if (lds_or) {
					__builtin_amdgcn_wave_barrier(); // LDS serves one wave's instructions in order; keep the compiler from moving the reads up
#pragma unroll
					for (int k = 0; k < FP_SPT; ++k) mine[k] = planes[wave][k][ch];
				} else {
#pragma unroll
					for (int k = 0; k < FP_SPT; ++k) {
						mine[k] = 0;
						for (uint32_t c = 0; c < n_chunks; ++c) {
							const unsigned long long b = __ballot((touched[k] >> c) & 1ull);
							if (lane == c) mine[k] = b;
						}
					}
				}
				if (ch < n_chunks) {
					unsigned long long* dst = bits + ((size_t)level * FP_MAX_CHUNKS + ch) * n_words + base / 64;
					if (base + FP_WAVE_SAMPLES <= n) {
						typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
#pragma unroll
						for (int k = 0; k < FP_SPT; k += 2) *(u64x2*)&dst[k] = u64x2{mine[k], mine[k + 1]};
					} else {
#pragma unroll
						for (int k = 0; k < FP_SPT; ++k) if (base + k * 64 < n) dst[k] = mine[k];
					}
				}
			}
		}
	}
}

template <int D, int F, int SPT, bool PLAIN>
void launch_planes(hipStream_t s, const GridMeta* dm, const uint32_t* work, uint32_t max_items, uint32_t blocks_per_xcd, uint32_t n, MatView x, const void* grid, void* out, uint64_t* bits,
                   const MlpPrepJob* prep_job, const GridHitLists* hit_lists) {
	MlpPrepJob prep{};
	if (prep_job) prep = *prep_job;
	static_assert(!PLAIN || (D == 2 && F == 2 && SPT != 8), "the PLAIN body's shapes");
	CHECK_THROW(!PLAIN || hit_lists);
	if (hit_lists) {
		if constexpr (SPT == 8) throw std::runtime_error{"grid_forward_planes: hit lists come from the 2- and 4-samples-per-thread shapes"};
		else
		hipLaunchKernelGGL((k_grid_fwd_planes<D, F, SPT, true, PLAIN>), dim3(8 * blocks_per_xcd), dim3(FP_LIST_THREADS), 0, s, dm, work, max_items, blocks_per_xcd, n, x, (const half_t*)grid, (half_t*)out,
		                   nullptr, prep, *hit_lists);
	} else if constexpr (!PLAIN) {
		hipLaunchKernelGGL((k_grid_fwd_planes<D, F, SPT, false, false>), dim3(8 * blocks_per_xcd), dim3(FP_THREADS), 0, s, dm, work, max_items, blocks_per_xcd, n, x, (const half_t*)grid, (half_t*)out,
		                   (unsigned long long*)bits, prep, GridHitLists{});
	}
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace

// the PLAIN instantiations (k_grid_planes_plain.hip); hit_lists is not null
void grid_forward_planes_plain(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, const uint32_t* dev_work, uint32_t max_items, uint32_t blocks_per_xcd, uint32_t n, MatView x,
                               const void* grid, void* out_planes, const MlpPrepJob* prep_job, const GridHitLists* hit_lists);

} // namespace tcnn_amd
