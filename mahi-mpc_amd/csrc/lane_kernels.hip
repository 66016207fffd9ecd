// lane_kernels.hip -- translation unit of the lane-per-instance Riccati kernels (sqp_lane.h), built with
// -mllvm -sgpr-regalloc=basic (Makefile LANEFLAGS; why: lane_launch.h).  A library generated for SX-defined dynamics
// (ModelGenerator::compile_model) compiles this file with the same -DMMPC_USER_MODEL_HEADER as mmpc.hip.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/mmpc.h"
#include "lane_launch.h"
#include "models.h"
#include "sqp_lane.h"
#ifdef MMPC_USER_MODEL_HEADER
#include MMPC_USER_MODEL_HEADER
#define MMPC_LANE_BUILTIN_MODELS 0
#else
#define MMPC_LANE_BUILTIN_MODELS 1
#endif

namespace mmpc {
namespace {
// the lane kernels of a model: the monotone barrier rule only, the exact Hessian for models with second derivatives
// (fp64 factor: a canonical key is never fp32 and exact); per-instance bounds (IB) on the bounded instantiations only
template <class Model>
constexpr bool has_lane_kernel(const KernelVariant& v) {
    return canonical(v) && !v.mehr && (!v.exact || HasHess<Model>::value);
}
template <class Model>
int launch_model(const KernelVariant& v, dim3 grid, dim3 block, hipStream_t stream, const SolveParams& p,
                 const LaneWork& lw) {
    return with_variant(v, [&](auto sv) {
        constexpr KernelVariant V = decltype(sv)::value;
        if constexpr (has_lane_kernel<Model>(V)) {
            using FT = std::conditional_t<V.fp32, float, double>;
            sqp_lane_kernel<Model, FT, V.ub, V.xb, V.exact, V.instb><<<grid, block, 0, stream>>>(p, lw);
            return 0;
        } else {
            return -2;
        }
    });
}
}  // namespace

int launch_lane_kernels(int model_id, const KernelVariant& v, dim3 grid, dim3 block, hipStream_t stream,
                        const SolveParams& p, const LaneWork& lw) {
#if MMPC_LANE_BUILTIN_MODELS
    if (model_id == MMPC_MODEL_TWO_LINK_ARM) return launch_model<TwoLinkArm>(v, grid, block, stream, p, lw);
    if (model_id == MMPC_MODEL_EXO_ARM) return launch_model<ExoArm>(v, grid, block, stream, p, lw);
#else
    if (model_id == MMPC_MODEL_USER) return launch_model<UserModel>(v, grid, block, stream, p, lw);
#endif
    return -1;
}

// this translation unit's copy of the phase-timing table (device variables are per code object without -fgpu-rdc)
hipError_t lane_phase_cycles(unsigned long long* out16, int n, bool reset) { return phase_table_read(out16, n, reset); }
}  // namespace mmpc
