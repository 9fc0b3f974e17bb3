// spmv_attention_backward.hip -- translation unit of the fused attention backward (kernels/attention_backward.hpp).  Launches only: the
// tables, the transpose, the two nnz-sized arrays, staging and the error channel stay in spmv_shim.hip (shim/attention_backward.hpp), which
// calls attention_backward_launch once per call.  A call is ceil(heads / hg) rounds -- a row pass and a column pass over up to hg heads each,
// the head loop inside the kernels --, the pointers offset here to the round's first head.
//
// Compiled once per SPMV_ATT_IO, the element type of Q, K, V and G in memory (the values of SPMV_HIP_T_*), so that the parts build side by side:
//   0  the handle's type (float and double), for dQ, dK and dV as well; this part also holds attention_backward_launch, which routes on io_type
//   1  fp16, 2  bf16: float arithmetic, dQ (the row kernels) and dK / dV (the column kernels) float or that type.  Always the BIAS family of
//      the row kernels (a null bias and a null dB are wave-uniform tests), so the set per type is
//        row kernels     dQ's type (2) x STATS (2) x CW (4) x VEC (2) x GROUPED (2) = 64 of each of the two
//        column kernels  CW (4) x VEC (2) x {one K / V head per head: float or 16-bit output; GROUPED: float output only} (3) = 24 of each
//      and the two narrowing kernels.  No GROUPED column kernel has a 16-bit output: with gs > 1 the sums of a group are made in the handle's
//      float arrays and rounded once at the end (attention_bwd_narrow_kernel)
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/attention_backward.hpp"

#ifndef SPMV_ATT_IO
#error "SPMV_ATT_IO must be 0 (the handle's types), 1 (fp16) or 2 (bf16)"
#endif

namespace spmv {

// this part's storage type of Q, K, V and G beside the arithmetic type T
template <typename T> using Stored = std::conditional_t<SPMV_ATT_IO == 0, T, std::conditional_t<SPMV_ATT_IO == 1, f16_t, bf16_t>>;

// the row pass over A: P and dS into the handle's arrays, dQ in SQ; BIAS: the bias read and dB written where they are given.  The lane mapping
// (CW, cwd, lgk, the panels) is T's: with 16-bit operands float's, as in the forward (kernels/attention.hpp)
template <typename T, typename SI, typename SQ, int CW, bool VEC, bool BIAS, bool GROUPED, bool STATS>
static void attention_bwd_rows_cw(const AttentionBwdArgs &a, hipStream_t stream)
{
    constexpr int waves = kBlock / kWave;
    const int lgk = panel_group_lg<T>(a.k);    // the narrowest lane group that covers a panel's columns (spmm's rule; it changes no bit)
    const int cwd = panel_group_width<T>(a.dv); // a function of dv and the arithmetic type alone: it fixes dP's summation order
    const T scale = (T) a.scale;
    const SI *q = (const SI *) a.q, *kk = (const SI *) a.kk, *v = (const SI *) a.v, *g = (const SI *) a.g;
    SQ *dq = (SQ *) a.dq;
    T *p = (T *) a.p, *ds = (T *) a.ds;
    const T *bias = (const T *) a.bias;
    T *db = (T *) a.db;
    const T *o = STATS ? (const T *) a.o : nullptr, *lse = STATS ? (const T *) a.lse : nullptr;
    if (a.nb > 0)
        attention_bwd_rows_kernel<T, CW, VEC, BIAS, GROUPED, STATS, SI, SQ><<<(a.nb + waves - 1) / waves, kBlock, 0, stream>>>(
            a.nb, a.split, a.rowptr, a.colidx, a.heads, a.plane, a.k, a.dv, cwd, lgk, scale, q, a.ldq, kk, a.ldk, v, a.ldv, g, a.ldg, dq, a.lddq, a.dvo ? p : nullptr,
            a.dk ? ds : nullptr, bias, a.ldb, db, a.lddb, a.gs, a.gpos, o, a.ldo, lse, a.ldl);
    if (a.nlong > 0)
        attention_bwd_long_kernel<T, CW, VEC, BIAS, GROUPED, STATS, SI, SQ><<<a.nlong < a.cus * 8 ? a.nlong : a.cus * 8, kBlock, 0, stream>>>(
            a.nlong, a.longs, a.rowptr, a.colidx, a.heads, a.plane, a.k, a.dv, cwd, lgk, scale, q, a.ldq, kk, a.ldk, v, a.ldv, g, a.ldg, dq, a.lddq, p, ds, bias, a.ldb, db,
            a.lddb, a.gs, a.gpos, o, a.ldo, lse, a.ldl);
}

// panel `c` of the column pass over A^T: kcv columns of dV, kck columns of dK, in SO
template <typename T, typename SI, typename SO, int CW, bool VEC, bool GROUPED>
static void attention_bwd_cols_cw(const AttentionBwdArgs &a, int c, int kcv, int kck, hipStream_t stream)
{
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

// one round: a.heads heads from the pointers' first columns, planes 0 .. a.heads - 1.  GROUPED (a.gs > 1): the instantiations that know the
// groups -- the K / V block of a head in the row pass, the sums over a group's heads in the column pass; without it, all four kernels are the
// code from before the groups existed
template <typename T, typename SI, bool VEC, bool GROUPED>
static void attention_bwd_round(const AttentionBwdArgs &a, hipStream_t stream)
{
    constexpr bool sixteen = !std::is_same_v<SI, T>;
    constexpr int KP = SpmmShape<T>::KP;
    // the row kernels' three families.  The final O and L given: the STATS instantiations (BIAS ones, a bias and a wanted dB or not).  A bias or a
    // wanted dB has instantiations of its own: without them, the row kernels are the code without the bias's loads, addition and store; 16-bit
    // operands have only the BIAS ones
    const bool stats = a.o && a.lse, bias_family = sixteen || stats || a.bias || a.db;
    // sddmm's lane group for k: a function of k and the arithmetic type alone, it fixes the scores' summation order
    if (a.m > 0)
        with_width(panel_group_width<T>(a.k), [&](auto CW) {
            constexpr int cw = decltype(CW)::value;
            auto family = [&](auto sq) {
                using SQ = decltype(sq);
                if (stats) attention_bwd_rows_cw<T, SI, SQ, cw, VEC, true, GROUPED, true>(a, stream);
                else if (bias_family) attention_bwd_rows_cw<T, SI, SQ, cw, VEC, true, GROUPED, false>(a, stream);
                else if constexpr (!sixteen) attention_bwd_rows_cw<T, SI, SQ, cw, VEC, false, GROUPED, false>(a, stream);
            };
            if (!sixteen || a.dq_type == 0) family(T()); else family(SI()); // dQ: the handle's type, or with 16-bit operands float or theirs
        });
    if (!a.dk && !a.dvo) return;
    const int wk = a.dk ? a.k : 0, wv = a.dvo ? a.dv : 0;
    for (int c = 0; c < wk || c < wv; c += KP) { // panel c / KP of both outputs, of every head of the round, in one pass over A^T
        const int kcv = wv - c < KP ? wv - c : KP, kck = wk - c < KP ? wk - c : KP; // <= 0: that output has no such panel
        const int kc = kcv > kck ? kcv : kck;
        // the narrowest lane group that covers the wider panel's columns
        with_width(panel_group_width<T>(kc), [&](auto CW) {
            constexpr int cw = decltype(CW)::value;
            // dK and dV: the handle's type, or with 16-bit operands float or theirs -- over groups float only: the caller's 16-bit arrays are
            // written by the narrowing
            if (!sixteen || GROUPED || a.dkv_type == 0) attention_bwd_cols_cw<T, SI, T, cw, VEC, GROUPED>(a, c, kcv, kck, stream);
            else if constexpr (sixteen && !GROUPED) attention_bwd_cols_cw<T, SI, SI, cw, VEC, false>(a, c, kcv, kck, stream);
        });
    }
}

template <typename S>
static void attention_bwd_narrow(const float *src, void *dst, long long ldd, long long rows, int w, int cus, hipStream_t stream)
{
    if (!dst || rows <= 0 || w <= 0) return;
    const long long total = rows * ((w + 3) / 4), blocks = (total + kBlock - 1) / kBlock, cap = (long long) cus * 16;
    const int grid = (int) (blocks < cap ? blocks : cap);
    const bool vec = w % 4 == 0 && ((uintptr_t) dst & 7) == 0 && (ldd * 2) % 8 == 0 && ((uintptr_t) src & 15) == 0;
    if (vec) attention_bwd_narrow_kernel<S, true><<<grid, kBlock, 0, stream>>>(rows, w, src, (S *) dst, ldd);
    else attention_bwd_narrow_kernel<S, false><<<grid, kBlock, 0, stream>>>(rows, w, src, (S *) dst, ldd);
}

// p + i elements of es bytes each; nullptr (not given, not wanted) stays nullptr
template <typename P> static P *at(P *p, size_t es, long long i) { return p ? (P *) ((const char *) p + (long long) es * i) : nullptr; }

template <typename T, typename SI, bool VEC>
static void attention_bwd_launch_t(const AttentionBwdArgs &a, hipStream_t stream)
{
    const int hg = a.hg < 1 ? 1 : a.hg, gs = a.gs < 1 ? 1 : a.gs;
    // element sizes: Q / K / V / G, dQ, dK / dV (a type other than 0 is io_type's: 16-bit operands only); the rest is T
    const size_t si = sizeof(SI), sq = a.dq_type ? sizeof(SI) : sizeof(T), so = a.dkv_type ? sizeof(SI) : sizeof(T), st = sizeof(T);
    for (int h0 = 0; h0 < a.heads; h0 += hg) { // a round's column pass has read the planes before the next round's row pass writes them: one stream
        AttentionBwdArgs r = a;
        r.heads = a.heads - h0 < hg ? a.heads - h0 : hg;
        r.gs = gs;
        r.gpos = h0 % gs; // > 0: the round starts inside a group, whose dK / dV so far the round before has stored
        const long long ck = (long long) h0 * a.k, cv = (long long) h0 * a.dv; // the round's first columns
        const long long gk = (long long) (h0 / gs) * a.k, gv = (long long) (h0 / gs) * a.dv; // and those of its first head's K / V block
        r.q = at(a.q, si, ck);
        r.kk = at(a.kk, si, gk);
        r.v = at(a.v, si, gv);
        r.g = at(a.g, si, cv);
        r.dq = at(a.dq, sq, ck);
        r.dk = at(a.dk, so, gk);
        r.dvo = at(a.dvo, so, gv);
        r.bias = at(a.bias, st, (long long) h0 * a.ldb); // the round's first planes: dB goes straight to the caller's, at head h0 + g
        r.db = at(a.db, st, (long long) h0 * a.lddb);
        r.o = at(a.o, st, cv);
        r.lse = at(a.lse, st, (long long) h0 * a.ldl);
        if (gs > 1) attention_bwd_round<T, SI, VEC, true>(r, stream);
        else attention_bwd_round<T, SI, VEC, false>(r, stream);
    }
    // 16-bit dK / dV over groups: the sums, complete in float after the last round, every element rounded once
    if constexpr (!std::is_same_v<SI, T>) {
        if (a.nar_dk) attention_bwd_narrow<SI>((const float *) a.dk, a.nar_dk, a.nar_lddk, a.n, a.kv_heads * a.k, a.cus, stream);
        if (a.nar_dv) attention_bwd_narrow<SI>((const float *) a.dvo, a.nar_dv, a.nar_lddv, a.n, a.kv_heads * a.dv, a.cus, stream);
    }
}

template <> hipError_t attention_backward_launch_part<SPMV_ATT_IO>(const AttentionBwdArgs &a, bool f64, hipStream_t stream)
{
    with_type_vec(f64, a.vec, [&](auto t, auto vec) {
        using T = decltype(t);
        // 16-bit operands: float arithmetic only (the shim asks for a float handle)
        if constexpr (SPMV_ATT_IO == 0 || std::is_same_v<T, float>) attention_bwd_launch_t<T, Stored<T>, decltype(vec)::value>(a, stream);
    });
    return hipGetLastError();
}

#if SPMV_ATT_IO == 0
hipError_t attention_backward_launch(const AttentionBwdArgs &a, bool f64, hipStream_t stream)
{
    switch (a.io_type) { // SPMV_HIP_T_*: to the part that holds the instantiations
    case 0: return attention_backward_launch_part<0>(a, f64, stream);
    case 1: return attention_backward_launch_part<1>(a, f64, stream);
    default: return attention_backward_launch_part<2>(a, f64, stream);
    }
}
#endif

} // namespace spmv
