// k_grid_planes.hip -- the host side of the training-step form of the grid encoding forward pass (the kernel: grid_planes_kernel.h): which shape
// serves a grid, the level-major work list cut into per-XCD runs, the launch of the generic instantiations; and the transpositions between
// level planes and rows.
#include "grid_planes_kernel.h"

namespace tcnn_amd {
namespace {

uint32_t max_scatter_chunks(const GridMeta& meta) {
	uint32_t m = 1;
	for (uint32_t l = 0; l < meta.n_levels; ++l) m = std::max(m, meta.levels[l].scatter_n_chunks);
	return m;
}

} // namespace

uint32_t grid_hit_item_samples(const GridMeta& meta) { return FP_LIST_THREADS * grid_planes_spt(meta); }

// samples per thread of the kernel shape used for this grid (see k_grid_fwd_planes)
uint32_t grid_planes_spt(const GridMeta& meta) {
	// 4 samples per thread (16 gathers in flight, half the registers, twice the waves per CU) measured against 8 on C3a, four runs
	// each: 56.1-56.9 us against 58.7-59.2.  TCNN_AMD_FWD_SPT=8 keeps the old shape (A/B runs).
	const char* spt_env = lab_env("TCNN_AMD_FWD_SPT"); // laboratory knob
	const uint32_t forced = spt_env ? (uint32_t)atoi(spt_env) : 0u;
	if (max_scatter_chunks(meta) > (uint32_t)FP_MAX_CHUNKS) return 2u;
	if (forced == 8 || forced == 4 || forced == 2) return forced;
	// 3-D grids that write hit lists: four cell rows per sample make an item of 1024 samples 4096 list elements -- 40 KB of LDS staging, three
	// workgroups per CU.  Items of 512 samples (round 5, L = 16, F = 2, T = 2^19 at 2^18 samples): forward 151-161 -> 117-123 us, the gradient
	// kernels 86-89 -> 92-94 (twice the items per chunk), step 0.340 -> 0.307 ms.  In 2-D the same halving loses (C3a: gradient 55 -> 63 us).
	if (meta.n_pos_dims == 3 && grid_scatter_prefers_lists(meta)) return 2u;
	return 4u;
}

bool grid_planes_supported(const GridMeta& meta, uint32_t n) {
	const uint32_t F = meta.n_features_per_level;
	return (F == 2 || F == 4 || F == 8) && (meta.n_pos_dims == 2 || meta.n_pos_dims == 3) && meta.n_levels < 256 && n % 64 == 0 && n > 0 &&
	       div_round_up(n, FP_THREADS * grid_planes_spt(meta)) < (1u << 24);
}

// Work list: [0..7] = number of items of XCD x, then 8 runs of max_items entries (level << 24 | item index inside the level).
// Levels are laid end to end in order and the sequence is cut into 8 runs of equal estimated cost, so every XCD gathers
// from at most a few consecutive levels (usually two) and each table is pulled into at most two L2s.
void grid_planes_plan(const GridMeta& meta, uint32_t n, bool hit_lists, std::vector<uint32_t>& work, uint32_t& max_items, uint32_t& blocks_per_xcd) {
	const uint32_t threads = hit_lists ? FP_LIST_THREADS : FP_THREADS;
	const uint32_t items_per_level = div_round_up(n, threads * grid_planes_spt(meta));
	// relative cost of one item: tables beyond a few hundred KB miss the per-CU cache on nearly every corner pair
	float coarse_cost = 0.6f;
	if (const char* e = lab_env("TCNN_AMD_FWD_COARSE_COST")) coarse_cost = (float)atof(e); // laboratory knob
	std::vector<float> cost(meta.n_levels);
	double total = 0;
	for (uint32_t l = 0; l < meta.n_levels; ++l) {
		const size_t bytes = (size_t)meta.levels[l].size * meta.n_features_per_level * 2;
		cost[l] = bytes > (256u << 10) ? 1.0f : coarse_cost;
		total += (double)cost[l] * items_per_level;
	}
	// profiling aid: TCNN_AMD_FWD_LEVELS="lo,hi" restricts the work list to levels lo..hi (results are then incomplete!)
	uint32_t dbg_lo = 0, dbg_hi = meta.n_levels;
	if (const char* e = lab_env("TCNN_AMD_FWD_LEVELS")) sscanf(e, "%u,%u", &dbg_lo, &dbg_hi);
	(void)total;
	// A level whose table does not fit an XCD's L2 anyway (> 4 MB: config 5's 32 MB tables) is NOT given to one XCD: with per-XCD level runs
	// eight such tables are in flight at once -- 256 MB, the whole Infinity Cache, beside the plane stores -- nothing stays resident and
	// every 16-byte pair costs a DRAM burst (3.07 GB read for 537 MB of gathers, measured).  Its items are dealt out to all XCDs in turn
	// instead, behind the levels that do fit: all XCDs then work on the same one or two big tables at a time, which stay in the Infinity Cache.
	size_t wide_bytes = (size_t)4 << 20;
	if (const char* e = lab_env("TCNN_AMD_FWD_WIDE_MB")) wide_bytes = (size_t)std::max(atoi(e), 0) << 20; // 0: never (A/B runs)
	auto is_wide = [&](uint32_t l) { return wide_bytes > 0 && (size_t)meta.levels[l].size * meta.n_features_per_level * 2 > wide_bytes; };
	double narrow_total = 0;
	for (uint32_t l = 0; l < meta.n_levels; ++l) if (l >= dbg_lo && l <= dbg_hi && !is_wide(l)) narrow_total += (double)cost[l] * items_per_level;
	std::vector<std::vector<uint32_t>> runs(8);
	double acc = 0;
	for (uint32_t l = 0; l < meta.n_levels; ++l) {
		if (l < dbg_lo || l > dbg_hi || is_wide(l)) continue;
		for (uint32_t i = 0; i < items_per_level; ++i) {
			const uint32_t bin = std::min<uint32_t>((uint32_t)((acc + 0.5 * cost[l]) * 8.0 / narrow_total), 7u);
			runs[bin].push_back(l << 24 | i);
			acc += cost[l];
		}
	}
	{ // even the runs out before the wide levels follow (they start together)
		size_t longest = 0;
		for (auto& r : runs) longest = std::max(longest, r.size());
		uint32_t next = 0;
		for (uint32_t l = 0; l < meta.n_levels; ++l) {
			if (l < dbg_lo || l > dbg_hi || !is_wide(l)) continue;
			for (uint32_t i = 0; i < items_per_level; ++i) {
				// fill the shortest run first until all are level, then round robin
				size_t best = next % 8;
				for (size_t b = 0; b < 8; ++b) if (runs[b].size() < runs[best].size()) best = b;
				runs[best].push_back(l << 24 | i);
				++next;
			}
		}
		(void)longest;
	}
	max_items = 0;
	for (auto& r : runs) max_items = std::max<uint32_t>(max_items, (uint32_t)r.size());
	work.assign(8 + (size_t)8 * max_items, 0xffffffffu);
	for (uint32_t b = 0; b < 8; ++b) {
		work[b] = (uint32_t)runs[b].size();
		std::copy(runs[b].begin(), runs[b].end(), work.begin() + 8 + (size_t)b * max_items);
	}
	// 16 waves per CU on each XCD's 32 CUs (8 workgroups of 128 threads), fewer when there is less work
	blocks_per_xcd = std::max(1u, std::min(256u * FP_THREADS / threads, max_items));
	if (const char* e = lab_env("TCNN_AMD_FWD_BLOCKS_PER_XCD")) blocks_per_xcd = std::max(1, atoi(e)); // laboratory knob
}

void grid_forward_planes(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, const uint32_t* dev_work, uint32_t max_items, uint32_t blocks_per_xcd, uint32_t n,
                         MatView x, const void* grid, void* out_planes, uint64_t* chunk_bits, const MlpPrepJob* prep_job, const GridHitLists* hit_lists, bool plain) {
	CHECK_THROW(grid_planes_supported(meta, n));
	CHECK_THROW(!plain || grid_planes_plain(meta, n)); // (the route's decision; what the PLAIN body relies on is checked here once more)
	CHECK_THROW(!hit_lists || (hit_lists->elems && hit_lists->heads && hit_lists->stragglers && hit_lists->counts && n <= grid_hit_max_samples(meta) &&
	                           hit_lists->item_samples == grid_hit_item_samples(meta) && hit_lists->n_items == div_round_up(n, hit_lists->item_samples) &&
	                           hit_lists->sidx && hit_lists->item_capacity >= (hit_lists->item_samples << (meta.n_pos_dims - 1)) && hit_lists->item_capacity % 8 == 0));
	if (hit_lists) { // the item map: whole items only unless the items are runs of consecutive samples; a wave's positions inside one window
		const GridItemMap& m = hit_lists->map;
		CHECK_THROW(m.window > 0 && m.window == (1u << m.window_shift) && m.window * m.n_windows == hit_lists->item_samples && m.window % (64 * grid_planes_spt(meta)) == 0);
		CHECK_THROW(m.n_windows == 1 || (n % hit_lists->item_samples == 0 && m.stride == hit_lists->n_items * m.window));
	}
	if (lab_env("TCNN_AMD_FWD_GENERIC")) plain = false; // laboratory knob: the generic body for every grid (A/B runs)
	const uint32_t F = meta.n_features_per_level;
#define TCNN_PLANES_F(D, SPT) \
	switch (F) { \
		case 2: return launch_planes<D, 2, SPT, false>(stream, dev_meta, dev_work, max_items, blocks_per_xcd, n, x, grid, out_planes, chunk_bits, prep_job, hit_lists); \
		case 4: return launch_planes<D, 4, SPT, false>(stream, dev_meta, dev_work, max_items, blocks_per_xcd, n, x, grid, out_planes, chunk_bits, prep_job, hit_lists); \
		default: return launch_planes<D, 8, SPT, false>(stream, dev_meta, dev_work, max_items, blocks_per_xcd, n, x, grid, out_planes, chunk_bits, prep_job, hit_lists); \
	}
#define TCNN_PLANES(D) \
	if (grid_planes_spt(meta) == 8) { TCNN_PLANES_F(D, 8) } else if (grid_planes_spt(meta) == 4) { TCNN_PLANES_F(D, 4) } else { TCNN_PLANES_F(D, 2) }
	if (plain && hit_lists && grid_planes_spt(meta) != 8) return grid_forward_planes_plain(stream, meta, dev_meta, dev_work, max_items, blocks_per_xcd, n, x, grid, out_planes, prep_job, hit_lists);
	if (meta.n_pos_dims == 2) { TCNN_PLANES(2) } else { TCNN_PLANES(3) }
#undef TCNN_PLANES
#undef TCNN_PLANES_F
}

// Level planes [level][n][F] (what k_grid_fwd_planes writes) -> rows [n][row_words] of the same halves, as 32-bit words: 64 samples per
// workgroup through LDS, both sides coalesced (a level's 64 x F / 2 words are contiguous in the planes, a tile's 64 rows in the output).
namespace {
constexpr uint32_t PR_THREADS = 256, PR_SAMPLES = 64, PR_MAX_WORDS = 128;
__global__ void __launch_bounds__(PR_THREADS) k_planes_to_rows(const uint32_t* __restrict__ planes, uint32_t* __restrict__ rows, const uint32_t n, const uint32_t words_per_level,
                                                                const uint32_t words, const uint32_t row_words) {
	__shared__ uint32_t tile[PR_SAMPLES * (PR_MAX_WORDS + 1)];
	const uint32_t i0 = blockIdx.x * PR_SAMPLES, pitch = words + 1;
	const uint32_t per_level = PR_SAMPLES * words_per_level;
	for (uint32_t idx = threadIdx.x; idx < PR_SAMPLES * words; idx += PR_THREADS) {
		const uint32_t l = idx / per_level, r = idx - l * per_level;
		const uint32_t i = r / words_per_level, k = r - i * words_per_level;
		tile[i * pitch + l * words_per_level + k] = planes[((size_t)l * n + i0) * words_per_level + r];
	}
	__syncthreads();
	for (uint32_t idx = threadIdx.x; idx < PR_SAMPLES * words; idx += PR_THREADS) {
		const uint32_t i = idx / words, w = idx - i * words;
		rows[(size_t)(i0 + i) * row_words + w] = tile[i * pitch + w];
	}
}
// the other way round: rows [n][row_words] -> level planes (dL/dy of a caller's own network for the list-fed gradient kernel, whose streamed
// tasks read a level's gradients sample after sample)
__global__ void __launch_bounds__(PR_THREADS) k_rows_to_planes(const uint32_t* __restrict__ rows, uint32_t* __restrict__ planes, const uint32_t n, const uint32_t words_per_level,
                                                                const uint32_t words, const uint32_t row_words) {
	__shared__ uint32_t tile[PR_SAMPLES * (PR_MAX_WORDS + 1)];
	const uint32_t i0 = blockIdx.x * PR_SAMPLES, pitch = words + 1;
	const uint32_t per_level = PR_SAMPLES * words_per_level;
	for (uint32_t idx = threadIdx.x; idx < PR_SAMPLES * words; idx += PR_THREADS) {
		const uint32_t i = idx / words, w = idx - i * words;
		tile[i * pitch + w] = rows[(size_t)(i0 + i) * row_words + w];
	}
	__syncthreads();
	for (uint32_t idx = threadIdx.x; idx < PR_SAMPLES * words; idx += PR_THREADS) {
		const uint32_t l = idx / per_level, r = idx - l * per_level;
		const uint32_t i = r / words_per_level, k = r - i * words_per_level;
		planes[((size_t)l * n + i0) * words_per_level + r] = tile[i * pitch + l * words_per_level + k];
	}
}
} // namespace

bool grid_planes_to_rows_supported(const GridMeta& meta, uint32_t n, uint32_t width) {
	const uint32_t F = meta.n_features_per_level;
	return n > 0 && n % PR_SAMPLES == 0 && F % 2 == 0 && width > 0 && width % F == 0 && width / 2 <= PR_MAX_WORDS;
}

void grid_planes_to_rows(hipStream_t stream, const GridMeta& meta, uint32_t n, uint32_t width, const void* planes, void* rows, uint32_t row_stride) {
	CHECK_THROW(grid_planes_to_rows_supported(meta, n, width) && row_stride % 2 == 0 && row_stride >= width);
	hipLaunchKernelGGL(k_planes_to_rows, dim3(n / PR_SAMPLES), dim3(PR_THREADS), 0, stream, (const uint32_t*)planes, (uint32_t*)rows, n, meta.n_features_per_level / 2, width / 2, row_stride / 2);
}

void grid_rows_to_planes(hipStream_t stream, const GridMeta& meta, uint32_t n, uint32_t width, const void* rows, uint32_t row_stride, void* planes) {
	CHECK_THROW(grid_planes_to_rows_supported(meta, n, width) && row_stride % 2 == 0 && row_stride >= width);
	hipLaunchKernelGGL(k_rows_to_planes, dim3(n / PR_SAMPLES), dim3(PR_THREADS), 0, stream, (const uint32_t*)rows, (uint32_t*)planes, n, meta.n_features_per_level / 2, width / 2, row_stride / 2);
}

} // namespace tcnn_amd
