// mlp_train_kernels.h -- what the files of fused training kernels offer the dispatcher (mlp_train_plan / mlp_train_launch, at the end of
// k_train.hip), and nobody else.  Per family:
//   X_plan(d, r, sw, p): does the file have a kernel for request r?  If so it fills p's kernel, name, grid and the fields its launch reads.
//                        Each answers for itself; the order of preference is the dispatcher's.
//   X_launch(...)      : runs p.grid workgroups of that kernel.  Decides nothing.
#pragma once

#include "tcnn_common.h"

namespace tcnn_amd {

// the one way these kernels are launched: raise the kernel's dynamic-LDS limit, launch, check
template <typename K, typename... A> void launch_with_lds(K kernel, hipStream_t stream, uint32_t grid, uint32_t block, uint32_t lds_bytes, const A&... args) {
	HIP_CHECK_THROW(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes, stream, args...);
	HIP_CHECK_THROW(hipGetLastError());
}

inline bool loss_l2_or_relative(const MlpTrainRequest& r) { return !r.external_dL_dy && (r.loss == LossType::L2 || r.loss == LossType::RelativeL2); }

// k_train_r32ob.hip: BASELINE config 2, OneBlob(64 bins, 2 dims) -> 64 -> 64 -> 16 with the encoding evaluated in the kernel
bool r32ob_plan(const MlpDesc& d, const MlpTrainRequest& r, const Switches& sw, MlpTrainPlan& p);
void r32ob_launch(hipStream_t stream, const MlpDesc& d, const MlpTrainPlan& p, const MlpTrainArgs& a);
// k_train_r32w.hip: BASELINE config 5's MLP part, 64 -> 128 -> 128 -> 16 fed by level planes of 4 features.  The one kernel without a grid
// formula of its own: the dispatcher gives it the workgroups k_train.hip's table would launch for this network and batch
bool r32w_plan(const MlpDesc& d, const MlpTrainRequest& r, const Switches& sw, MlpTrainPlan& p);
void r32w_launch(hipStream_t stream, const MlpDesc& d, const MlpTrainPlan& p, const MlpTrainArgs& a);
// k_train_regs.hip: (16 | 32) -> 64 -> [64 ->] 16 with everything in registers.  regs_shape: the network and the batch size alone (the queries);
// regs_grid: its workgroups for a batch
bool regs_shape(const MlpDesc& d, uint32_t n, const Switches& sw);
uint32_t regs_grid(uint32_t n);
bool regs_plan(const MlpDesc& d, const MlpTrainRequest& r, const Switches& sw, MlpTrainPlan& p);
void regs_launch(hipStream_t stream, const MlpDesc& d, const MlpTrainPlan& p, const MlpTrainArgs& a);
// k_train_r32.hip (and k_train_r32a.hip through it): BASELINE configs 3, 32 -> 64 -> 64 -> 16 fed by a 2-D grid with 2 features per level
bool r32_plan(const MlpDesc& d, const MlpTrainRequest& r, const Switches& sw, MlpTrainPlan& p);
void r32_launch(hipStream_t stream, const MlpDesc& d, const MlpTrainPlan& p, const MlpTrainArgs& a);

} // namespace tcnn_amd
