// kernel_variant.h -- which instantiation of a Riccati kernel runs a solve.  Host code only.
//
// KernelVariant is the one key of that choice.  launch_kernel (mmpc.hip) builds it once per solve, in canonical form;
// everything after it -- LDS and workspace sizes, the workspace layout, the launch entries of group_launch.h and
// lane_launch.h -- takes the key, never loose booleans.  with_variant turns a key into template arguments; each call
// site pairs it with a constexpr predicate naming the combinations that unit instantiates, so a combination outside
// the predicate instantiates nothing.
#pragma once
#include <type_traits>

namespace mmpc {
struct KernelVariant {
    bool ub = false;      // control bounds alone: the projected SQP (the kernels' BOUNDED)
    bool xb = false;      // state bounds: the interior point, which takes the control bounds too (XB)
    bool exact = false;   // exact Hessian of the Lagrangian (EXACT); Gauss-Newton otherwise
    bool instb = false;   // a row of control bounds per instance (IB, SolveParams::b_stride != 0)
    bool mehr = false;    // Mehrotra's predictor-corrector barrier rule (MEHR)
    bool fp32 = false;    // fp32 Riccati factor (lane kernels)
};
// the form launch_kernel builds: xb absorbs ub, instb only with a bound, mehr only with xb, fp32 never exact
constexpr bool canonical(const KernelVariant& v) {
    return !(v.ub && v.xb) && (!v.instb || v.ub || v.xb) && (!v.mehr || v.xb) && !(v.fp32 && v.exact);
}
// named keys of the host's sizing ("the largest variant" is a maximum over some of these)
constexpr KernelVariant kVariantUb{true, false, false, false, false, false};
constexpr KernelVariant kVariantXb{false, true, false, false, false, false};
constexpr KernelVariant kVariantXbMehrotra{false, true, false, false, true, false};

// a key as a type: decltype(v)::value is usable in `if constexpr` and as template arguments
template <bool UB, bool XB, bool EXACT, bool INSTB, bool MEHR, bool FP32>
struct StaticVariant {
    static constexpr KernelVariant value{UB, XB, EXACT, INSTB, MEHR, FP32};
};
template <class F>
auto lift_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}
// f(StaticVariant<...>{}) for the run-time key v
template <class F>
auto with_variant(const KernelVariant& v, F&& f) {
    return lift_bool(v.ub, [&](auto ub) {
        return lift_bool(v.xb, [&](auto xb) {
            return lift_bool(v.exact, [&](auto exact) {
                return lift_bool(v.instb, [&](auto instb) {
                    return lift_bool(v.mehr, [&](auto mehr) {
                        return lift_bool(v.fp32, [&](auto fp32) {
                            return f(StaticVariant<decltype(ub)::value, decltype(xb)::value, decltype(exact)::value,
                                                   decltype(instb)::value, decltype(mehr)::value,
                                                   decltype(fp32)::value>{});
                        });
                    });
                });
            });
        });
    });
}
}  // namespace mmpc
