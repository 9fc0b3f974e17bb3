// spmv_bicgstab.hip -- translation unit of the BiCGStab vector kernels (kernels/bicgstab.hpp).  Launches only: the workspace, staging, the two
// multiplies of an iteration, the host's looks at the state and the error channel stay in spmv_shim.hip (shim/bicgstab.hpp), which calls
// bicg_start_launch once per solve and, per iteration, bicg_first_launch behind v = A ph and bicg_second_launch behind t = A sh.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/bicgstab.hpp"

namespace spmv {

template <typename T, bool WIDE, bool DINV>
static void bicg_start_t(const BicgArgs &a, bool use_x0, hipStream_t stream)
{
    const T *b = (const T *) a.b, *v = (const T *) a.v, *dinv = (const T *) a.dinv;
    if (use_x0) bicg_init_kernel<T, WIDE, DINV, true><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, b, (T *) a.x, v, dinv, (T *) a.r, (T *) a.rhat, (T *) a.p, (T *) a.y, a.part);
    else bicg_init_kernel<T, WIDE, DINV, false><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, b, (T *) a.x, v, dinv, (T *) a.r, (T *) a.rhat, (T *) a.p, (T *) a.y, a.part);
    if (a.hist) bicg_begin_kernel<true><<<1, kBlock, 0, stream>>>(a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
    else bicg_begin_kernel<false><<<1, kBlock, 0, stream>>>(a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void bicg_first_t(const BicgArgs &a, int k, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    bicg_rv_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, (const T *) a.rhat, (const T *) a.v, a.part, a.state);
    bicg_half_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, (const T *) a.p, (const T *) a.v, (T *) a.x, (T *) a.r, (const T *) a.dinv, (T *) a.y, a.part, a.state, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void bicg_second_t(const BicgArgs &a, int k, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    bicg_ts_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, (const T *) a.t, (const T *) a.r, a.part, a.state);
    bicg_update_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, (const T *) a.t, (T *) a.r, (const T *) a.y, (T *) a.x, (const T *) a.rhat, a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
    bicg_direction_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, (const T *) a.r, (T *) a.p, (const T *) a.v, (const T *) a.dinv, (T *) a.y, a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
}

// the instantiation of F that a.f64 / a.wide / a.dinv select
#define BICG_DISPATCH(F, ...)                                                                                                \
    do {                                                                                                                     \
        const bool dinv__ = a.dinv != nullptr;                                                                               \
        if (a.f64) {                                                                                                         \
            if (a.wide) { if (dinv__) F<double, true, true>(__VA_ARGS__); else F<double, true, false>(__VA_ARGS__); }        \
            else { if (dinv__) F<double, false, true>(__VA_ARGS__); else F<double, false, false>(__VA_ARGS__); }             \
        } else {                                                                                                             \
            if (a.wide) { if (dinv__) F<float, true, true>(__VA_ARGS__); else F<float, true, false>(__VA_ARGS__); }          \
            else { if (dinv__) F<float, false, true>(__VA_ARGS__); else F<float, false, false>(__VA_ARGS__); }               \
        }                                                                                                                    \
    } while (0)

static bool bicg_args_ok(const BicgArgs &a) { return a.m > 0 && a.parts >= 1 && a.parts <= kCgMaxParts && a.span * a.parts >= a.m; }

hipError_t bicg_start_launch(const BicgArgs &a, bool use_x0, hipStream_t stream)
{
    if (!bicg_args_ok(a)) return hipErrorInvalidValue;
    BICG_DISPATCH(bicg_start_t, a, use_x0, stream);
    return hipGetLastError();
}

hipError_t bicg_first_launch(const BicgArgs &a, int k, hipStream_t stream)
{
    if (!bicg_args_ok(a) || k < 1) return hipErrorInvalidValue;
    BICG_DISPATCH(bicg_first_t, a, k, stream);
    return hipGetLastError();
}

hipError_t bicg_second_launch(const BicgArgs &a, int k, hipStream_t stream)
{
    if (!bicg_args_ok(a) || k < 1) return hipErrorInvalidValue;
    BICG_DISPATCH(bicg_second_t, a, k, stream);
    return hipGetLastError();
}

} // namespace spmv
