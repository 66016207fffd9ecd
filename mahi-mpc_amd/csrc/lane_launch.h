// lane_launch.h -- the lane-per-instance Riccati kernels (sqp_lane.h) are compiled in their own translation unit,
// lane_kernels.hip, with the basic instead of the greedy SGPR register allocator (-mllvm -sgpr-regalloc=basic):
// five exo lane-kernel builds at the 512-register limit computed wrong steps with the greedy allocator of ROCm 7.2's
// LLVM and right ones with either basic allocator, from the same IR ("wrong-result builds").
// mmpc.hip launches them only through this entry point, so no lane kernel is instantiated in its translation unit.
// The entry takes the solve's key (kernel_variant.h); lane_kernels.hip's predicate names the keys it instantiates.
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_variant.h"
#include "sqp_wave.h"

namespace mmpc {
struct LaneWork;
// 0; -1 when model_id is not compiled into this library; -2 when the model has no lane kernel for the key (Mehrotra's
// rule, an exact Hessian without second derivatives) -- nothing is launched then
int launch_lane_kernels(int model_id, const KernelVariant& v, dim3 grid, dim3 block, hipStream_t stream,
                        const SolveParams& p, const LaneWork& lw);
// the phase-timing table of the lane kernels (diagnostic build; mmpc_debug_phase_cycles adds it to its own)
hipError_t lane_phase_cycles(unsigned long long* out16, int n, bool reset);
}  // namespace mmpc
