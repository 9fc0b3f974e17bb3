// spmv_attention_backward_16.hip -- translation unit of the fused attention backward on 16-bit Q, K, V and G (spmv_hip_attention_gqa_backward_16):
// the kernels of kernels/attention_backward.hpp with fp16 or bf16 as the storage type of Q / K / V / G, float or that type as dQ's (the row
// kernels) and as dK's and dV's (the column kernels).  Launches only, like spmv_attention_backward.hip: shim/attention_backward.hpp calls
// attention_backward_16_launch once per call; the rounds and the pointer offsets are those of attention_bwd_launch_t there.
//
// Always the BIAS family of the row kernels (a null bias and a null dB are wave-uniform tests), so the set per storage type is
//   row kernels     dQ's type (2) x STATS (2) x CW (4) x VEC (2) x GROUPED (2) = 64 of each of the two
//   column kernels  CW (4) x VEC (2) x {one K / V head per head: float or 16-bit output; GROUPED: float output only} (3) = 24 of each of the two
// and the two narrowing kernels.  No GROUPED column kernel has a 16-bit output: with gs > 1 the sums of a group are made in the handle's float
// arrays and rounded once at the end (attention_bwd_narrow_kernel).  Compiled once per storage type (SPMV_ATTB16_TYPE = 1: fp16, 2: bf16; the
// values of SPMV_HIP_T_F16 / _BF16) so that the two halves build side by side.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/attention_backward.hpp"

#ifndef SPMV_ATTB16_TYPE
#error "SPMV_ATTB16_TYPE must be 1 (fp16) or 2 (bf16)"
#endif

namespace spmv {

using T16 = float; // the arithmetic type: the lane mapping (CW, cwd, lgk, the panels) is float's, as in the forward (kernels/attention.hpp)

// the row pass over A: P and dS into the handle's arrays, dQ in SQ; the bias read and dB written where they are given
template <typename SI, typename SQ, int CW, bool VEC, bool GROUPED, bool STATS>
static void attention_bwd16_rows_cw(const AttentionBwdArgs &a, hipStream_t stream)
{
    using T = T16;
    constexpr int waves = kBlock / kWave;
    const int lgk = panel_group_lg<T>(a.k);
    const int cwd = panel_group_width<T>(a.dv);
    const T scale = (T) a.scale;
    const SI *q = (const SI *) a.q, *kk = (const SI *) a.kk, *v = (const SI *) a.v, *g = (const SI *) a.g;
    SQ *dq = (SQ *) a.dq;
    T *p = (T *) a.p, *ds = (T *) a.ds;
    const T *bias = (const T *) a.bias;
    T *db = (T *) a.db;
    const T *o = STATS ? (const T *) a.o : nullptr, *lse = STATS ? (const T *) a.lse : nullptr;
    if (a.nb > 0)
        attention_bwd_rows_kernel<T, CW, VEC, true, GROUPED, STATS, SI, SQ><<<(a.nb + waves - 1) / waves, kBlock, 0, stream>>>(
            a.nb, a.split, a.rowptr, a.colidx, a.heads, a.plane, a.k, a.dv, cwd, lgk, scale, q, a.ldq, kk, a.ldk, v, a.ldv, g, a.ldg, dq, a.lddq, a.dvo ? p : nullptr,
            a.dk ? ds : nullptr, bias, a.ldb, db, a.lddb, a.gs, a.gpos, o, a.ldo, lse, a.ldl);
    if (a.nlong > 0)
        attention_bwd_long_kernel<T, CW, VEC, true, GROUPED, STATS, SI, SQ><<<a.nlong < a.cus * 8 ? a.nlong : a.cus * 8, kBlock, 0, stream>>>(
            a.nlong, a.longs, a.rowptr, a.colidx, a.heads, a.plane, a.k, a.dv, cwd, lgk, scale, q, a.ldq, kk, a.ldk, v, a.ldv, g, a.ldg, dq, a.lddq, p, ds, bias, a.ldb, db,
            a.lddb, a.gs, a.gpos, o, a.ldo, lse, a.ldl);
}

// panel `c` of the column pass over A^T: kcv columns of dV, kck columns of dK, in SO
template <typename SI, typename SO, int CW, bool VEC, bool GROUPED>
static void attention_bwd16_cols_cw(const AttentionBwdArgs &a, int c, int kcv, int kck, hipStream_t stream)
{
    using T = T16;
    constexpr int waves = kBlock / kWave;
    const T *pv = (const T *) a.p, *dsv = (const T *) a.ds;
    const SI *g = (const SI *) a.g + c, *q = (const SI *) a.q + c;
    SO *dvo = a.dvo ? (SO *) a.dvo + c : nullptr, *dk = a.dk ? (SO *) a.dk + c : nullptr;
    if (a.t_nb > 0)
        attention_bwd_cols_kernel<T, CW, VEC, GROUPED, SI, SO><<<(a.t_nb + waves - 1) / waves, kBlock, 0, stream>>>(
            a.t_nb, a.t_split, a.t_rowptr, a.t_colidx, a.perm, a.heads, a.plane, a.k, a.dv, pv, dsv, kcv, g, a.ldg, dvo, a.lddv, kck, q, a.ldq, dk, a.lddk, a.gs, a.gpos);
    if (a.t_nlong > 0)
        attention_bwd_cols_long_kernel<T, CW, VEC, GROUPED, SI, SO><<<a.t_nlong < a.cus * 8 ? a.t_nlong : a.cus * 8, kBlock, 0, stream>>>(
            a.t_nlong, a.t_longs, a.t_rowptr, a.t_colidx, a.perm, a.heads, a.plane, a.k, a.dv, pv, dsv, kcv, g, a.ldg, dvo, a.lddv, kck, q, a.ldq, dk, a.lddk, a.gs, a.gpos);
}

// one round: a.heads heads from the pointers' first columns, planes 0 .. a.heads - 1 (attention_bwd_round of spmv_attention_backward.hip)
template <typename SI, bool VEC, bool GROUPED>
static void attention_bwd16_round(const AttentionBwdArgs &a, hipStream_t stream)
{
    using T = T16;
    constexpr int KP = SpmmShape<T>::KP;
    if (a.m > 0)
        with_width(panel_group_width<T>(a.k), [&](auto CW) {
            constexpr int cw = decltype(CW)::value;
            auto go = [&](auto sq) {
                if (a.o && a.lse) attention_bwd16_rows_cw<SI, decltype(sq), cw, VEC, GROUPED, true>(a, stream);
                else attention_bwd16_rows_cw<SI, decltype(sq), cw, VEC, GROUPED, false>(a, stream);
            };
            if (a.dq_type == 0) go(T()); else go(SI());
        });
    if (!a.dk && !a.dvo) return;
    const int wk = a.dk ? a.k : 0, wv = a.dvo ? a.dv : 0;
    for (int c = 0; c < wk || c < wv; c += KP) {
        const int kcv = wv - c < KP ? wv - c : KP, kck = wk - c < KP ? wk - c : KP;
        const int kc = kcv > kck ? kcv : kck;
        with_width(panel_group_width<T>(kc), [&](auto CW) {
            constexpr int cw = decltype(CW)::value;
            if constexpr (GROUPED) attention_bwd16_cols_cw<SI, T, cw, VEC, true>(a, c, kcv, kck, stream); // float sums: the caller's 16-bit arrays are written by the narrowing
            else if (a.dkv_type == 0) attention_bwd16_cols_cw<SI, T, cw, VEC, false>(a, c, kcv, kck, stream);
            else attention_bwd16_cols_cw<SI, SI, cw, VEC, false>(a, c, kcv, kck, stream);
        });
    }
}

template <typename S>
static void attention_bwd16_narrow(const float *src, void *dst, long long ldd, long long rows, int w, int cus, hipStream_t stream)
{
    if (!dst || rows <= 0 || w <= 0) return;
    const long long total = rows * ((w + 3) / 4), blocks = (total + kBlock - 1) / kBlock, cap = (long long) cus * 16;
    const int grid = (int) (blocks < cap ? blocks : cap);
    const bool vec = w % 4 == 0 && ((uintptr_t) dst & 7) == 0 && (ldd * 2) % 8 == 0 && ((uintptr_t) src & 15) == 0;
    if (vec) attention_bwd_narrow_kernel<S, true><<<grid, kBlock, 0, stream>>>(rows, w, src, (S *) dst, ldd);
    else attention_bwd_narrow_kernel<S, false><<<grid, kBlock, 0, stream>>>(rows, w, src, (S *) dst, ldd);
}

template <typename SI, bool VEC>
static void attention_bwd16_launch_t(const AttentionBwdArgs &a, hipStream_t stream)
{
    const int hg = a.hg < 1 ? 1 : a.hg, gs = a.gs < 1 ? 1 : a.gs;
    const size_t sq = a.dq_type ? 2 : 4, so = a.dkv_type ? 2 : 4; // element sizes of dq and of dk / dvo
    for (int h0 = 0; h0 < a.heads; h0 += hg) { // a round's column pass has read the planes before the next round's row pass writes them: one stream
        AttentionBwdArgs r = a;
        r.heads = a.heads - h0 < hg ? a.heads - h0 : hg;
        r.gs = gs;
        r.gpos = h0 % gs; // > 0: the round starts inside a group, whose float dK / dV so far the round before has stored
        const long long ck = (long long) h0 * a.k, cv = (long long) h0 * a.dv;               // the round's first columns
        const long long gk = (long long) (h0 / gs) * a.k, gv = (long long) (h0 / gs) * a.dv; // and those of its first head's K / V block
        r.q = (const SI *) a.q + ck;
        r.kk = (const SI *) a.kk + gk;
        r.v = (const SI *) a.v + gv;
        r.g = (const SI *) a.g + cv;
        if (a.dq) r.dq = (char *) a.dq + sq * (size_t) ck;
        if (a.dk) r.dk = (char *) a.dk + so * (size_t) gk;
        if (a.dvo) r.dvo = (char *) a.dvo + so * (size_t) gv;
        if (a.bias) r.bias = (const float *) a.bias + (long long) h0 * a.ldb;
        if (a.db) r.db = (float *) a.db + (long long) h0 * a.lddb;
        if (a.o) r.o = (const float *) a.o + cv;
        if (a.lse) r.lse = (const float *) a.lse + (long long) h0 * a.ldl;
        if (gs > 1) attention_bwd16_round<SI, VEC, true>(r, stream);
        else attention_bwd16_round<SI, VEC, false>(r, stream);
    }
    // the grouped sums, complete in float after the last round: every element of a 16-bit dK / dV rounded once
    if (a.nar_dk) attention_bwd16_narrow<SI>((const float *) a.dk, a.nar_dk, a.nar_lddk, a.n, a.kv_heads * a.k, a.cus, stream);
    if (a.nar_dv) attention_bwd16_narrow<SI>((const float *) a.dvo, a.nar_dv, a.nar_lddv, a.n, a.kv_heads * a.dv, a.cus, stream);
}

#if SPMV_ATTB16_TYPE == 1
hipError_t attention_backward_16_launch_f16(const AttentionBwdArgs &a, hipStream_t stream)
{
    if (a.vec) attention_bwd16_launch_t<f16_t, true>(a, stream); else attention_bwd16_launch_t<f16_t, false>(a, stream);
    return hipGetLastError();
}
#else
hipError_t attention_backward_16_launch_bf16(const AttentionBwdArgs &a, hipStream_t stream)
{
    if (a.vec) attention_bwd16_launch_t<bf16_t, true>(a, stream); else attention_bwd16_launch_t<bf16_t, false>(a, stream);
    return hipGetLastError();
}

hipError_t attention_backward_16_launch_f16(const AttentionBwdArgs &a, hipStream_t stream);

hipError_t attention_backward_16_launch(const AttentionBwdArgs &a, hipStream_t stream)
{
    return a.io_type == 1 ? attention_backward_16_launch_f16(a, stream) : attention_backward_16_launch_bf16(a, stream);
}
#endif

} // namespace spmv
