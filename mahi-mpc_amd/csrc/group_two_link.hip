// group_two_link.hip -- the built-in 2-link arm's 16-lane group kernels (sqp_group.h; the cfg#2 headline path) in
// translation units of their own.  This file is compiled twice (Makefile); each unit has one launch entry that takes the
// solve's key (kernel_variant.h) and a constexpr predicate naming the keys it instantiates:
//   * build/group_two_link.o: the UNBOUNDED kernels sqp_group_kernel<TwoLinkArm, false, false, EXACT> (Gauss-Newton and
//     exact Hessian, the cfg#2 path) with LLVM's default (greedy) register allocators -- they allocate without VGPR
//     spills or scratch (tests/test_build_flags.py checks the built code object's metadata), and run ~1 % faster than
//     with the basic SGPR allocator;
//   * build/group_two_link_bounded.o (-DMMPC_GROUP_BOUNDED_UNIT): the control-bounded and state-bounded kernels -- four
//     sqp_group_kernel<TwoLinkArm, BOUNDED, XB, EXACT>, two sqp_group_mehrotra_kernel (the other barrier rule), six
//     sqp_group_instb_kernel (per-instance control bounds) -- with -mllvm -sgpr-regalloc=basic like every other unit:
//     they reach the 512-register limit with VGPR spills to scratch, the profile of the greedy-allocator miscompiles
//     of DESIGN.md 4b.
#include <hip/hip_runtime.h>

#include "../../include/mmpc.h"
#include "group_launch.h"
#include "models.h"

namespace mmpc {
namespace {
#ifdef MMPC_GROUP_BOUNDED_UNIT
constexpr bool in_unit(const KernelVariant& v) { return canonical(v) && !v.fp32 && (v.ub || v.xb); }
#else
constexpr bool in_unit(const KernelVariant& v) { return canonical(v) && !v.fp32 && !v.ub && !v.xb; }
#endif
hipError_t launch_unit(const KernelVariant& v, dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                       const SolveParams& p, const GroupWork& gwk) {
    return with_variant(v, [&](auto sv) {
        if constexpr (in_unit(decltype(sv)::value))
            return launch_group_kernel<TwoLinkArm>(sv, grid, block, lds, stream, p, gwk);
        else
            return hipErrorInvalidValue;
    });
}
}  // namespace

// this translation unit's copy of the phase-timing table (as lane_kernels.hip)
#ifndef MMPC_GROUP_BOUNDED_UNIT
hipError_t launch_group_two_link(const KernelVariant& v, dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                                 const SolveParams& p, const GroupWork& gwk) {
    return launch_unit(v, grid, block, lds, stream, p, gwk);
}
hipError_t group_two_link_phase_cycles(unsigned long long* out16, int n, bool reset) {
    return phase_table_read(out16, n, reset);
}
#else
hipError_t launch_group_two_link_bounded(const KernelVariant& v, dim3 grid, dim3 block, size_t lds,
                                         hipStream_t stream, const SolveParams& p, const GroupWork& gwk) {
    return launch_unit(v, grid, block, lds, stream, p, gwk);
}
hipError_t group_two_link_bounded_phase_cycles(unsigned long long* out16, int n, bool reset) {
    return phase_table_read(out16, n, reset);
}
#endif
}  // namespace mmpc
