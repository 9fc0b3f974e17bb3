// spmv_attention_backward.hip -- translation unit of the fused attention backward (kernels/attention_backward.hpp).  Launches only: the
// tables, the transpose, the two nnz-sized arrays, staging and the error channel stay in spmv_shim.hip (shim/attention_backward.hpp), which
// calls attention_backward_launch once per call.  A call is ceil(heads / hg) rounds -- a row pass and a column pass over up to hg heads each,
// the head loop inside the kernels --, the pointers offset here to the round's first head.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/attention_backward.hpp"

namespace spmv {

// the row pass over A: P and dS into the handle's arrays, dQ; BIAS: the bias read and dB written as well
template <typename T, int CW, bool VEC, bool BIAS, bool GROUPED, bool STATS = false>
static void attention_bwd_rows_cw(const AttentionBwdArgs &a, hipStream_t stream)
{
    constexpr int waves = kBlock / kWave;
    const int lgk = panel_group_lg<T>(a.k);    // the narrowest lane group that covers a panel's columns (spmm's rule; it changes no bit)
    const int cwd = panel_group_width<T>(a.dv); // a function of dv and the value type alone: it fixes dP's summation order
    const T scale = (T) a.scale;
    const T *q = (const T *) a.q, *kk = (const T *) a.kk, *v = (const T *) a.v, *g = (const T *) a.g;
    T *dq = (T *) a.dq, *p = (T *) a.p, *ds = (T *) a.ds;
    const T *bias = (const T *) a.bias;
    T *db = (T *) a.db;
    const T *o = STATS ? (const T *) a.o : nullptr, *lse = STATS ? (const T *) a.lse : nullptr;
    if (a.nb > 0)
        attention_bwd_rows_kernel<T, CW, VEC, BIAS, GROUPED, STATS><<<(a.nb + waves - 1) / waves, kBlock, 0, stream>>>(a.nb, a.split, a.rowptr, a.colidx, a.heads, a.plane, a.k, a.dv, cwd, lgk, scale,
                                                                                               q, a.ldq, kk, a.ldk, v, a.ldv, g, a.ldg, dq, a.lddq, a.dvo ? p : nullptr,
                                                                                               a.dk ? ds : nullptr, bias, a.ldb, db, a.lddb, a.gs, a.gpos, o, a.ldo, lse, a.ldl);
    if (a.nlong > 0)
        attention_bwd_long_kernel<T, CW, VEC, BIAS, GROUPED, STATS><<<a.nlong < a.cus * 8 ? a.nlong : a.cus * 8, kBlock, 0, stream>>>(a.nlong, a.longs, a.rowptr, a.colidx, a.heads, a.plane, a.k, a.dv, cwd, lgk,
                                                                                                              scale, q, a.ldq, kk, a.ldk, v, a.ldv, g, a.ldg, dq, a.lddq, p, ds, bias, a.ldb, db, a.lddb, a.gs, a.gpos, o, a.ldo, lse, a.ldl);
}

// panel `c` of the column pass over A^T: kcv columns of dV, kck columns of dK
template <typename T, int CW, bool VEC, bool GROUPED>
static void attention_bwd_cols_cw(const AttentionBwdArgs &a, int c, int kcv, int kck, hipStream_t stream)
{
    constexpr int waves = kBlock / kWave;
    const T *pv = (const T *) a.p, *dsv = (const T *) a.ds;
    const T *g = (const T *) a.g + c, *q = (const T *) a.q + c;
    T *dvo = a.dvo ? (T *) a.dvo + c : nullptr, *dk = a.dk ? (T *) a.dk + c : nullptr;
    if (a.t_nb > 0)
        attention_bwd_cols_kernel<T, CW, VEC, GROUPED><<<(a.t_nb + waves - 1) / waves, kBlock, 0, stream>>>(a.t_nb, a.t_split, a.t_rowptr, a.t_colidx, a.perm, a.heads, a.plane, a.k,
                                                                                                          a.dv, pv, dsv, kcv, g, a.ldg, dvo, a.lddv, kck, q, a.ldq, dk, a.lddk, a.gs,
                                                                                                          a.gpos);
    if (a.t_nlong > 0)
        attention_bwd_cols_long_kernel<T, CW, VEC, GROUPED><<<a.t_nlong < a.cus * 8 ? a.t_nlong : a.cus * 8, kBlock, 0, stream>>>(a.t_nlong, a.t_longs, a.t_rowptr, a.t_colidx,
                                                                                                                                a.perm, a.heads, a.plane, a.k, a.dv, pv, dsv, kcv, g,
                                                                                                                                a.ldg, dvo, a.lddv, kck, q, a.ldq, dk, a.lddk, a.gs,
                                                                                                                                a.gpos);
}

// one round: a.heads heads from the pointers' first columns, planes 0 .. a.heads - 1.  GROUPED (a.gs > 1): the instantiations that know the
// groups -- the K / V block of a head in the row pass, the sums over a group's heads in the column pass; without it, all four kernels are the
// code from before the groups existed
template <typename T, bool VEC, bool GROUPED>
static void attention_bwd_round(const AttentionBwdArgs &a, hipStream_t stream)
{
    constexpr int KP = SpmmShape<T>::KP;
    // sddmm's lane group for k: a function of k and the value type alone, it fixes the scores' summation order
    // a bias or a wanted dB has instantiations of its own: without them, the row kernels are the code without the bias's loads, addition and store
    if (a.m > 0)
        with_width(panel_group_width<T>(a.k), [&](auto CW) {
            // the final O and L given: the STATS instantiations (BIAS ones, a bias and a wanted dB or not)
            if (a.o && a.lse) attention_bwd_rows_cw<T, decltype(CW)::value, VEC, true, GROUPED, true>(a, stream);
            else if (a.bias || a.db) attention_bwd_rows_cw<T, decltype(CW)::value, VEC, true, GROUPED>(a, stream);
            else attention_bwd_rows_cw<T, decltype(CW)::value, VEC, false, GROUPED>(a, stream);
        });
    if (!a.dk && !a.dvo) return;
    const int wk = a.dk ? a.k : 0, wv = a.dvo ? a.dv : 0;
    for (int c = 0; c < wk || c < wv; c += KP) { // panel c / KP of both outputs, of every head of the round, in one pass over A^T
        const int kcv = wv - c < KP ? wv - c : KP, kck = wk - c < KP ? wk - c : KP; // <= 0: that output has no such panel
        const int kc = kcv > kck ? kcv : kck;
        // the narrowest lane group that covers the wider panel's columns
        with_width(panel_group_width<T>(kc), [&](auto CW) { attention_bwd_cols_cw<T, decltype(CW)::value, VEC, GROUPED>(a, c, kcv, kck, stream); });
    }
}

template <typename T, bool VEC>
static void attention_bwd_launch_t(const AttentionBwdArgs &a, hipStream_t stream)
{
    const int hg = a.hg < 1 ? 1 : a.hg, gs = a.gs < 1 ? 1 : a.gs;
    for (int h0 = 0; h0 < a.heads; h0 += hg) { // a round's column pass has read the planes before the next round's row pass writes them: one stream
        AttentionBwdArgs r = a;
        r.heads = a.heads - h0 < hg ? a.heads - h0 : hg;
        r.gs = gs;
        r.gpos = h0 % gs; // > 0: the round starts inside a group, whose dK / dV so far the round before has stored
        const long long ck = (long long) h0 * a.k, cv = (long long) h0 * a.dv; // the round's first columns
        const long long gk = (long long) (h0 / gs) * a.k, gv = (long long) (h0 / gs) * a.dv; // and those of its first head's K / V block
        r.q = (const T *) a.q + ck;
        r.kk = (const T *) a.kk + gk;
        r.v = (const T *) a.v + gv;
        r.g = (const T *) a.g + cv;
        if (a.dq) r.dq = (T *) a.dq + ck;
        if (a.dk) r.dk = (T *) a.dk + gk;
        if (a.dvo) r.dvo = (T *) a.dvo + gv;
        if (a.bias) r.bias = (const T *) a.bias + (long long) h0 * a.ldb; // the round's first planes: dB goes straight to the caller's, at head h0 + g
        if (a.db) r.db = (T *) a.db + (long long) h0 * a.lddb;
        if (a.o) r.o = (const T *) a.o + cv;
        if (a.lse) r.lse = (const T *) a.lse + (long long) h0 * a.ldl;
        if (gs > 1) attention_bwd_round<T, VEC, true>(r, stream);
        else attention_bwd_round<T, VEC, false>(r, stream);
    }
}

hipError_t attention_backward_launch(const AttentionBwdArgs &a, bool f64, hipStream_t stream)
{
    with_type_vec(f64, a.vec, [&](auto t, auto vec) { attention_bwd_launch_t<decltype(t), decltype(vec)::value>(a, stream); });
    return hipGetLastError();
}

} // namespace spmv
