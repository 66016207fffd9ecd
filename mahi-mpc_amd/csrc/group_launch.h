// group_launch.h -- launching the 16-lane group kernels (sqp_group.h) by key (kernel_variant.h).
// launch_group_kernel is the one mapping from a key to the three __global__ names and the one place that raises a
// kernel's dynamic-LDS limit; mmpc.hip (exo / generated models) and group_two_link.hip instantiate it.
// The built-in 2-link arm's group kernels live in group_two_link.hip, compiled as two units: the unbounded kernels
// (cfg#2) with the greedy register allocators, the bounded ones with the basic SGPR allocator (why: that file's
// header); mmpc.hip launches them through the two entries below, one per unit, each taking the key.
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_variant.h"
#include "sqp_group.h"

namespace mmpc {
// sqp_group_instb_kernel with a row of bounds per instance, else sqp_group_mehrotra_kernel under Mehrotra's rule, else
// sqp_group_kernel
template <class M, class SV>
auto group_kernel() {
    constexpr KernelVariant v = SV::value;
    static_assert(canonical(v) && !v.fp32, "the 16-lane kernels' variants");
    if constexpr (v.instb) return &sqp_group_instb_kernel<M, v.ub, v.xb, v.exact, v.mehr>;
    else if constexpr (v.mehr) return &sqp_group_mehrotra_kernel<M, v.exact>;
    else return &sqp_group_kernel<M, v.ub, v.xb, v.exact>;
}
template <class M, class SV>
hipError_t launch_group_kernel(SV, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const SolveParams& p,
                               const GroupWork& gwk) {
    auto* const k = group_kernel<M, SV>();
    if (lds > 64 * 1024) {   // gfx950: up to 160 KB per workgroup once the attribute is raised
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    k<<<grid, block, lds, stream>>>(p, gwk);
    return hipGetLastError();
}

// the 2-link arm's units; a key outside the unit's kernels: hipErrorInvalidValue, nothing launched
// unbounded solves, both Hessians (build/group_two_link.o)
hipError_t launch_group_two_link(const KernelVariant& v, dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                                 const SolveParams& p, const GroupWork& gwk);
// control-bounded and state-bounded solves: shared or per-instance control bounds, both barrier rules
// (build/group_two_link_bounded.o)
hipError_t launch_group_two_link_bounded(const KernelVariant& v, dim3 grid, dim3 block, size_t lds,
                                         hipStream_t stream, const SolveParams& p, const GroupWork& gwk);
// the phase-timing tables of those units (diagnostic build; mmpc_debug_phase_cycles adds them to its own)
// (the first n <= kPhaseTableSlots slots of the unit's table)
hipError_t group_two_link_phase_cycles(unsigned long long* out16, int n, bool reset);
hipError_t group_two_link_bounded_phase_cycles(unsigned long long* out16, int n, bool reset);
}  // namespace mmpc
