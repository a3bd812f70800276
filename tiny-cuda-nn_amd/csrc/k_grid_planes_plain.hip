// k_grid_planes_plain.hip -- the PLAIN instantiations of k_grid_fwd_planes (grid_planes_kernel.h; chosen by GridForwardRoute::plain), in a
// translation unit of their own: it is built without the packed fp32 instructions (build.py EXTRA_FLAGS), which the generic instantiations
// next door cannot be without losing registers.
#include "grid_planes_kernel.h"

namespace tcnn_amd {

void grid_forward_planes_plain(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, const uint32_t* dev_work, uint32_t max_items, uint32_t blocks_per_xcd, uint32_t n, MatView x,
                               const void* grid, void* out_planes, const MlpPrepJob* prep_job, const GridHitLists* hit_lists) {
	CHECK_THROW(grid_planes_plain(meta, n) && hit_lists);
	const uint32_t spt = grid_planes_spt(meta);
	if (spt == 4) return launch_planes<2, 2, 4, true>(stream, dev_meta, dev_work, max_items, blocks_per_xcd, n, x, grid, out_planes, nullptr, prep_job, hit_lists);
	if (spt == 2) return launch_planes<2, 2, 2, true>(stream, dev_meta, dev_work, max_items, blocks_per_xcd, n, x, grid, out_planes, nullptr, prep_job, hit_lists);
	throw std::runtime_error{"grid_forward_planes_plain: 2 or 4 samples per thread"};
}

} // namespace tcnn_amd
