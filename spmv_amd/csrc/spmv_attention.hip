// spmv_attention.hip -- translation unit of the fused sparse attention (kernels/attention.hpp) and of the merge of two partial results
// (kernels/attention_merge.hpp).  Launches only: the tables, the long rows'
// parking space, staging and the error channel stay in spmv_shim.hip (shim/attention.hpp), which calls attention_launch once per call.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/attention.hpp"
#include "kernels/attention_merge.hpp"

namespace spmv {

template <typename T, int CW, bool VEC, bool BIAS, bool GROUPED, bool LSE = false>
static void attention_launch_cw(const AttentionArgs &a, hipStream_t stream)
{
    constexpr int waves = kBlock / kWave;
    const int lgv = panel_group_lg<T>(a.dv); // the narrowest lane group that covers a panel's columns of one head (spmm's rule; it changes no bit)
    const T scale = (T) a.scale;
    const int gs = a.gs < 1 ? 1 : a.gs;
    const T *q = (const T *) a.q, *kk = (const T *) a.kk, *v = (const T *) a.v;
    T *o = (T *) a.o;
    const T *bias = (const T *) a.bias;
    T *lse = LSE ? (T *) a.lse : nullptr;
    if (a.nb > 0)
        attention_rows_kernel<T, CW, VEC, BIAS, GROUPED, LSE><<<(a.nb + waves - 1) / waves, kBlock, 0, stream>>>(a.nb, a.split, a.rowptr, a.colidx, a.heads, a.k, a.dv, lgv, scale, q, a.ldq, kk, a.ldk,
                                                                                                 v, a.ldv, o, a.ldo, bias, a.ldb, gs, lse, a.ldl);
    if (a.nlong > 0)
        attention_long_kernel<T, CW, VEC, BIAS, GROUPED, LSE><<<a.nlong < a.cus * 8 ? a.nlong : a.cus * 8, kBlock, 0, stream>>>(a.nlong, a.longs, a.long_off, a.rowptr, a.colidx, a.heads, a.k, a.dv,
                                                                                                                lgv, scale, q, a.ldq, kk, a.ldk, v, a.ldv, o, a.ldo, (T *) a.park, bias,
                                                                                                                a.ldb, gs, lse, a.ldl);
}

hipError_t attention_launch(const AttentionArgs &a, bool f64, hipStream_t stream)
{
    if (a.m <= 0) return hipSuccess;
    with_type_vec(f64, a.vec, [&](auto t, auto vec) {
        using T = decltype(t);
        // sddmm's lane group for k: a function of k and the value type alone, it fixes the scores' summation order
        // a bias has instantiations of its own: without one, the kernels are the code without the bias's loads and addition
        with_width(panel_group_width<T>(a.k), [&](auto CW) {
            // so have grouped heads (gs > 1): without them, the kernels do not know the groups' counter either
            constexpr int cw = decltype(CW)::value;
            constexpr bool vc = decltype(vec)::value;
            // and so has the log-sum-exp output: the BIAS code, a bias or not, with the stores of L
            if (a.lse) {
                if (a.gs > 1) attention_launch_cw<T, cw, vc, true, true, true>(a, stream);
                else attention_launch_cw<T, cw, vc, true, false, true>(a, stream);
            } else if (a.gs > 1) {
                if (a.bias) attention_launch_cw<T, cw, vc, true, true>(a, stream);
                else attention_launch_cw<T, cw, vc, false, true>(a, stream);
            } else {
                if (a.bias) attention_launch_cw<T, cw, vc, true, false>(a, stream);
                else attention_launch_cw<T, cw, vc, false, false>(a, stream);
            }
        });
    });
    return hipGetLastError();
}

// ---- the merge of two partial results: one grid-stride launch, a lane group per (row, head)
hipError_t attention_merge_launch(const AttentionMergeArgs &a, bool f64, hipStream_t stream)
{
    if (a.m <= 0) return hipSuccess;
    with_type_vec(f64, a.vec, [&](auto t, auto vec) {
        using T = decltype(t);
        // the narrowest lane group that covers a head's dv columns at 16 bytes per lane: it changes no bit
        with_width(panel_group_width<T>(a.dv), [&](auto CW) {
            constexpr int cw = decltype(CW)::value, G = kBlock / cw;
            const long long ngroups = (long long) a.m * a.heads;
            const long long blocks = (ngroups + G - 1) / G, cap = (long long) a.cus * 8;
            attention_merge_kernel<T, cw, decltype(vec)::value><<<(unsigned) (blocks < cap ? blocks : cap), kBlock, 0, stream>>>(
                ngroups, a.heads, a.dv, (const T *) a.o1, a.ldo1, (const T *) a.l1, a.ldl1, (const T *) a.o2, a.ldo2, (const T *) a.l2, a.ldl2, (T *) a.o, a.ldo, (T *) a.l,
                a.ldl);
        });
    });
    return hipGetLastError();
}

} // namespace spmv
