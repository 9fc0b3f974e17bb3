// spmv_attention.hip -- translation unit of the fused sparse attention (kernels/attention.hpp).  Launches only: the tables, the long rows'
// parking space, staging and the error channel stay in spmv_shim.hip (shim/attention.hpp), which calls attention_launch once per call.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/attention.hpp"

namespace spmv {

template <typename T, int CW, bool VEC>
static void attention_launch_cw(const AttentionArgs &a, hipStream_t stream)
{
    constexpr int waves = kBlock / kWave, V = SpmmShape<T>::V;
    // the narrowest lane group that covers a panel's columns of one head (spmm's rule; it changes no bit)
    const int lgv = a.dv <= V ? 0 : (a.dv <= 2 * V ? 1 : (a.dv <= 4 * V ? 2 : 3));
    const T scale = (T) a.scale;
    const T *q = (const T *) a.q, *kk = (const T *) a.kk, *v = (const T *) a.v;
    T *o = (T *) a.o;
    if (a.nb > 0)
        attention_rows_kernel<T, CW, VEC><<<(a.nb + waves - 1) / waves, kBlock, 0, stream>>>(a.nb, a.split, a.rowptr, a.colidx, a.heads, a.k, a.dv, lgv, scale, q, a.ldq, kk, a.ldk, v,
                                                                                           a.ldv, o, a.ldo);
    if (a.nlong > 0)
        attention_long_kernel<T, CW, VEC><<<a.nlong < a.cus * 8 ? a.nlong : a.cus * 8, kBlock, 0, stream>>>(a.nlong, a.longs, a.long_off, a.rowptr, a.colidx, a.heads, a.k, a.dv, lgv,
                                                                                                          scale, q, a.ldq, kk, a.ldk, v, a.ldv, o, a.ldo, (T *) a.park);
}

template <typename T, bool VEC>
static void attention_launch_t(const AttentionArgs &a, hipStream_t stream)
{
    switch (sddmm_group_width(a.k, SddmmShape<T>::W)) { // a function of k and the value type alone: it fixes the scores' summation order
    case 1: attention_launch_cw<T, 1, VEC>(a, stream); break;
    case 2: attention_launch_cw<T, 2, VEC>(a, stream); break;
    case 4: attention_launch_cw<T, 4, VEC>(a, stream); break;
    default: attention_launch_cw<T, 8, VEC>(a, stream); break;
    }
}

hipError_t attention_launch(const AttentionArgs &a, bool f64, hipStream_t stream)
{
    if (a.m <= 0) return hipSuccess;
    if (f64) { if (a.vec) attention_launch_t<double, true>(a, stream); else attention_launch_t<double, false>(a, stream); }
    else { if (a.vec) attention_launch_t<float, true>(a, stream); else attention_launch_t<float, false>(a, stream); }
    return hipGetLastError();
}

} // namespace spmv
