// dispatch.hpp -- run-time values to template arguments, for the translation units that launch the panel kernels (spmm, sddmm, attention and
// its backward): each run-time choice is written once here.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace spmv {

// f(std::integral_constant<int, CW>()) for the lane-group width cw of 1, 2, 4, 8 (anything else: 8)
template <typename F>
__host__ __device__ __forceinline__ void with_width(int cw, F f)
{
    switch (cw) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    default: f(std::integral_constant<int, 8>()); break;
    }
}

// log2 of, and the narrowest lane group that covers kc columns of a panel at 16 bytes (16 / sizeof(T) columns) per lane, 8 lanes at the
// most.  spmm's rule for a panel and sddmm's for k: for sddmm it fixes the summation order, for spmm it changes no bit.
template <typename T> inline int panel_group_lg(int kc)
{
    constexpr int V = 16 / (int) sizeof(T);
    return kc <= V ? 0 : (kc <= 2 * V ? 1 : (kc <= 4 * V ? 2 : 3));
}
template <typename T> inline int panel_group_width(int kc) { return 1 << panel_group_lg<T>(kc); }

// f(T(), std::bool_constant<VEC>()) for the value type (double if f64, else float) and the 16-byte-access flag
template <typename F> inline void with_type_vec(bool f64, bool vec, F f)
{
    if (f64) { if (vec) f(double(), std::true_type()); else f(double(), std::false_type()); }
    else { if (vec) f(float(), std::true_type()); else f(float(), std::false_type()); }
}

} // namespace spmv
