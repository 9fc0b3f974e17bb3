// spmv_cg.hip -- translation unit of the conjugate-gradient vector kernels (kernels/cg.hpp).  Launches only: the workspace, staging, the
// multiply q = A p, the host's looks at the state and the error channel stay in spmv_shim.hip (shim/cg.hpp), which calls cg_start_launch once
// per solve and cg_iteration_launch once per iteration, behind the multiply.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/cg.hpp"

namespace spmv {

template <typename T, bool WIDE, bool DINV>
static void cg_start_t(const CgArgs &a, bool use_x0, hipStream_t stream)
{
    const T *b = (const T *) a.b, *q = (const T *) a.q, *dinv = (const T *) a.dinv;
    if (use_x0) cg_init_kernel<T, WIDE, DINV, true><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, b, (T *) a.x, q, dinv, (T *) a.r, (T *) a.p, a.part);
    else cg_init_kernel<T, WIDE, DINV, false><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, b, (T *) a.x, q, dinv, (T *) a.r, (T *) a.p, a.part);
    if (a.hist) cg_begin_kernel<true><<<1, kBlock, 0, stream>>>(a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
    else cg_begin_kernel<false><<<1, kBlock, 0, stream>>>(a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void cg_iteration_t(const CgArgs &a, int k, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    const T *dinv = (const T *) a.dinv;
    cg_dot_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, (const T *) a.p, (const T *) a.q, a.part, a.state);
    cg_update_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, (const T *) a.p, (const T *) a.q, (T *) a.x, (T *) a.r, dinv, a.part, a.state, a.nostop);
    cg_direction_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, (const T *) a.r, dinv, (T *) a.p, a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
}

// the instantiation of F that a.f64 / a.wide / a.dinv select
#define CG_DISPATCH(F, ...)                                                                                                  \
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

hipError_t cg_start_launch(const CgArgs &a, bool use_x0, hipStream_t stream)
{
    if (a.m <= 0 || a.parts < 1 || a.parts > kCgMaxParts) return hipErrorInvalidValue;
    CG_DISPATCH(cg_start_t, a, use_x0, stream);
    return hipGetLastError();
}

hipError_t cg_iteration_launch(const CgArgs &a, int k, hipStream_t stream)
{
    if (a.m <= 0 || a.parts < 1 || a.parts > kCgMaxParts || k < 1) return hipErrorInvalidValue;
    CG_DISPATCH(cg_iteration_t, a, k, stream);
    return hipGetLastError();
}

} // namespace spmv
