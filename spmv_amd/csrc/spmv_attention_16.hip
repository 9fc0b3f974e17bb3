// spmv_attention_16.hip -- translation unit of the fused sparse attention on 16-bit Q, K and V (spmv_hip_attention_gqa_lse_16): the kernels of
// kernels/attention.hpp with fp16 or bf16 as the storage type of Q / K / V and float or that type as O's.  Launches only, like
// spmv_attention.hip: shim/attention.hpp calls attention_16_launch once per call.
//
// Always the BIAS + LSE family (a null bias and a null L are wave-uniform tests in the kernels), so the set is storage type x O's type x CW x VEC x
// GROUPED.  Compiled once per storage type (SPMV_ATT16_TYPE = 1: fp16, 2: bf16; the values of SPMV_HIP_T_F16 / _BF16) so that the two halves
// build side by side.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/attention.hpp"

#ifndef SPMV_ATT16_TYPE
#error "SPMV_ATT16_TYPE must be 1 (fp16) or 2 (bf16)"
#endif

namespace spmv {

template <typename SI, typename SO, int CW, bool VEC, bool GROUPED>
static void attention_16_launch_cw(const AttentionArgs &a, hipStream_t stream)
{
    using T = float;
    constexpr int waves = kBlock / kWave;
    const int lgv = panel_group_lg<T>(a.dv); // float's lane group, as CW is: the lane mapping is the float kernels' (kernels/attention.hpp)
    const T scale = (T) a.scale;
    const int gs = a.gs < 1 ? 1 : a.gs;
    const SI *q = (const SI *) a.q, *kk = (const SI *) a.kk, *v = (const SI *) a.v;
    SO *o = (SO *) a.o;
    const T *bias = (const T *) a.bias;
    T *lse = (T *) a.lse;
    if (a.nb > 0)
        attention_rows_kernel<T, CW, VEC, true, GROUPED, true, SI, SO><<<(a.nb + waves - 1) / waves, kBlock, 0, stream>>>(a.nb, a.split, a.rowptr, a.colidx, a.heads, a.k, a.dv, lgv, scale, q,
                                                                                                                      a.ldq, kk, a.ldk, v, a.ldv, o, a.ldo, bias, a.ldb, gs, lse, a.ldl);
    if (a.nlong > 0)
        attention_long_kernel<T, CW, VEC, true, GROUPED, true, SI, SO><<<a.nlong < a.cus * 8 ? a.nlong : a.cus * 8, kBlock, 0, stream>>>(a.nlong, a.longs, a.long_off, a.rowptr, a.colidx, a.heads,
                                                                                                                                     a.k, a.dv, lgv, scale, q, a.ldq, kk, a.ldk, v, a.ldv, o,
                                                                                                                                     a.ldo, (T *) a.park, bias, a.ldb, gs, lse, a.ldl);
}

template <typename SI>
static void attention_16_launch_type(const AttentionArgs &a, hipStream_t stream)
{
    with_width(panel_group_width<float>(a.k), [&](auto CW) {
        constexpr int cw = decltype(CW)::value;
        auto go = [&](auto so, auto vec, auto grouped) {
            attention_16_launch_cw<SI, decltype(so), cw, decltype(vec)::value, decltype(grouped)::value>(a, stream);
        };
        auto with_flags = [&](auto so) {
            if (a.vec) { if (a.gs > 1) go(so, std::true_type(), std::true_type()); else go(so, std::true_type(), std::false_type()); }
            else { if (a.gs > 1) go(so, std::false_type(), std::true_type()); else go(so, std::false_type(), std::false_type()); }
        };
        if (a.o_type == 0) with_flags(float()); else with_flags(SI());
    });
}

#if SPMV_ATT16_TYPE == 1
hipError_t attention_16_launch_f16(const AttentionArgs &a, hipStream_t stream)
{
    if (a.m <= 0) return hipSuccess;
    attention_16_launch_type<f16_t>(a, stream);
    return hipGetLastError();
}
#else
hipError_t attention_16_launch_bf16(const AttentionArgs &a, hipStream_t stream)
{
    if (a.m <= 0) return hipSuccess;
    attention_16_launch_type<bf16_t>(a, stream);
    return hipGetLastError();
}

hipError_t attention_16_launch_f16(const AttentionArgs &a, hipStream_t stream);

hipError_t attention_16_launch(const AttentionArgs &a, hipStream_t stream) { return a.io_type == 1 ? attention_16_launch_f16(a, stream) : attention_16_launch_bf16(a, stream); }
#endif

} // namespace spmv
