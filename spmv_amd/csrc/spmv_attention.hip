// spmv_attention.hip -- translation unit of the fused sparse attention (kernels/attention.hpp) and of the merge of two partial results
// (kernels/attention_merge.hpp).  Launches only: the tables, the long rows' parking space, staging and the error channel stay in spmv_shim.hip
// (shim/attention.hpp), which calls attention_launch once per call.
//
// Compiled once per SPMV_ATT_IO, the element type of Q, K and V in memory (the values of SPMV_HIP_T_*), so that the parts build side by side:
//   0  the handle's type (float and double), for O as well; this part also holds attention_launch, which routes on io_type, and the merge
//   1  fp16, 2  bf16: float arithmetic, O float or that type; always the BIAS + LSE family (a null bias and a null L are wave-uniform tests in
//      the kernels), so the set per type is O's type x CW x VEC x GROUPED
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/attention.hpp"
#include "kernels/attention_merge.hpp"

#ifndef SPMV_ATT_IO
#error "SPMV_ATT_IO must be 0 (the handle's types), 1 (fp16) or 2 (bf16)"
#endif

namespace spmv {

// this part's storage type of Q, K and V beside the arithmetic type T
template <typename T> using Stored = std::conditional_t<SPMV_ATT_IO == 0, T, std::conditional_t<SPMV_ATT_IO == 1, f16_t, bf16_t>>;

// T: the arithmetic type; SI: Q's, K's and V's type in memory; SO: O's
template <typename T, typename SI, typename SO, int CW, bool VEC, bool BIAS, bool GROUPED, bool LSE>
static void attention_launch_cw(const AttentionArgs &a, hipStream_t stream)
{
    constexpr int waves = kBlock / kWave;
    // the narrowest lane group that covers a panel's columns of one head (spmm's rule; it changes no bit).  T's, as CW is: with 16-bit operands the
    // lane mapping is the float kernels' (kernels/attention.hpp)
    const int lgv = panel_group_lg<T>(a.dv);
    const T scale = (T) a.scale;
    const int gs = a.gs < 1 ? 1 : a.gs;
    const SI *q = (const SI *) a.q, *kk = (const SI *) a.kk, *v = (const SI *) a.v;
    SO *o = (SO *) a.o;
    const T *bias = (const T *) a.bias;
    T *lse = (T *) a.lse; // nullptr wherever LSE is false (attention_launch_t)
    if (a.nb > 0)
        attention_rows_kernel<T, CW, VEC, BIAS, GROUPED, LSE, SI, SO><<<(a.nb + waves - 1) / waves, kBlock, 0, stream>>>(
            a.nb, a.split, a.rowptr, a.colidx, a.heads, a.k, a.dv, lgv, scale, q, a.ldq, kk, a.ldk, v, a.ldv, o, a.ldo, bias, a.ldb, gs, lse, a.ldl);
    if (a.nlong > 0)
        attention_long_kernel<T, CW, VEC, BIAS, GROUPED, LSE, SI, SO><<<a.nlong < a.cus * 8 ? a.nlong : a.cus * 8, kBlock, 0, stream>>>(
            a.nlong, a.longs, a.long_off, a.rowptr, a.colidx, a.heads, a.k, a.dv, lgv, scale, q, a.ldq, kk, a.ldk, v, a.ldv, o, a.ldo, (T *) a.park, bias, a.ldb, gs, lse, a.ldl);
}

// The kernels of one call.  Three families: the log-sum-exp output has instantiations of its own -- the BIAS code, a bias or not, with the
// stores of L --, and so has a bias: without one, the kernels are the code without the bias's loads and addition.  16-bit operands are always the
// first family.  Grouped heads (gs > 1) have theirs in each: without them, the kernels do not know the groups' counter either.
template <typename T, typename SI, bool VEC>
static void attention_launch_t(const AttentionArgs &a, hipStream_t stream)
{
    constexpr bool sixteen = !std::is_same_v<SI, T>;
    const bool lse_family = sixteen || a.lse, bias_family = lse_family || a.bias;
    // sddmm's lane group for k: a function of k and the arithmetic type alone, it fixes the scores' summation order
    with_width(panel_group_width<T>(a.k), [&](auto CW) {
        constexpr int cw = decltype(CW)::value;
        auto family = [&](auto so, auto grouped) {
            using SO = decltype(so);
            constexpr bool gr = decltype(grouped)::value;
            if (lse_family) attention_launch_cw<T, SI, SO, cw, VEC, true, gr, true>(a, stream);
            else if constexpr (!sixteen) {
                if (bias_family) attention_launch_cw<T, SI, SO, cw, VEC, true, gr, false>(a, stream);
                else attention_launch_cw<T, SI, SO, cw, VEC, false, gr, false>(a, stream);
            }
        };
        auto groups = [&](auto so) { if (a.gs > 1) family(so, std::true_type()); else family(so, std::false_type()); };
        if (!sixteen || a.o_type == 0) groups(T()); else groups(SI()); // O: the handle's type, or with 16-bit operands float or theirs
    });
}

template <> hipError_t attention_launch_part<SPMV_ATT_IO>(const AttentionArgs &a, bool f64, hipStream_t stream)
{
    with_type_vec(f64, a.vec, [&](auto t, auto vec) {
        using T = decltype(t);
        // 16-bit operands: float arithmetic only (the shim asks for a float handle)
        if constexpr (SPMV_ATT_IO == 0 || std::is_same_v<T, float>) attention_launch_t<T, Stored<T>, decltype(vec)::value>(a, stream);
    });
    return hipGetLastError();
}

#if SPMV_ATT_IO == 0
hipError_t attention_launch(const AttentionArgs &a, bool f64, hipStream_t stream)
{
    if (a.m <= 0) return hipSuccess;
    switch (a.io_type) { // SPMV_HIP_T_*: to the part that holds the instantiations
    case 0: return attention_launch_part<0>(a, f64, stream);
    case 1: return attention_launch_part<1>(a, f64, stream);
    default: return attention_launch_part<2>(a, f64, stream);
    }
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
#endif

} // namespace spmv
