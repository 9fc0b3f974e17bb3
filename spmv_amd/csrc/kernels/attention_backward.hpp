// attention_backward.hpp -- the gradients of O = softmax_rows(scale * Q K^T on A's pattern) V (spmv_hip_attention_backward): with G = dL/dO,
//   dP_p = <G[i, :dv], V[j_p, :dv]>,  D_i = sum over row i of P_q dP_q,  dS_p = P_p (dP_p - D_i) scale,
//   dQ = A_dS K,  dK = A_dS^T Q,  dV = A_P^T G          (A_X: A's pattern holding X as values)
// in two passes over the pattern: one over A's rows, one over the rows of the device-built A^T.  A's values are neither read nor written.
//
// Row pass (attention_bwd_rows_kernel): attention_rows_kernel's structure -- spmm's batch table, a wave per batch, chunks of whole rows
// (chunk_take) -- with a second value array per wave in LDS.  Per chunk:
//   A. dots     tiles of 64 entries: the scaled scores t_p (att_tile_scores, sddmm's lane groups for k) into the first array and dP_p
//               (the same machinery over G and V rows, sddmm's lane groups for dv) into the second; ColIdx is read once for both.
//   B. softmax  the row softmax's passes (row_pass_width) over the two arrays: Z_i and exp(t - M_i) from the first, row_softmax_regs
//               written out (see there); P and D_i by row_dot_regs from those registers and dP; P and dS = P (dP - D) scale written
//               back, every element by the lane that read it.
//   C. stores   P and dS coalesced, in CSR order, into the handle-owned arrays attb_p / attb_ds -- P only when dV is wanted, dS only
//               when dK is: they are what the column pass gathers.
//   D. dQ       rows_times_panels over K with values dS, still in LDS.
// Rows longer than kSpmmLongThr (attention_bwd_long_kernel, a workgroup each): the row's own ranges of attb_p / attb_ds are its
// parking space -- t becomes P in place (long_row_softmax), dP becomes dS in place (long_row_dot), every element written by the thread
// that read it --, then long_row_panel per panel of k.
//
// Column pass (attention_bwd_cols_kernel, attention_bwd_cols_long_kernel): spmm's executors (staged_walk, long_row_panel) on A^T's tables
// (its rowptr, its colidx = rows of A, its own batch table and long list).  There is no value array: a chunk loads perm[q] (the CSR index in
// A of A^T's entry q) coalesced and gathers attb_p[perm[q]] and / or attb_ds[perm[q]] into the wave's two LDS arrays.  Two chains run off
// the one index stream, one after the other: dV's panel against G rows with values P, dK's panel against Q rows with values dS.  One launch
// does panel r of both.
//
// Heads (spmv_hip_attention_heads_backward): Q, K, dQ, dK are `heads` blocks of k columns side by side, V, G, dV `heads` blocks of dv columns,
// and attb_p / attb_ds are planes of `plane` (= nnz) elements, plane hd holding head hd's P / dS in CSR order.  The head loop is inside all
// four kernels: the row pass fetches a chunk's pattern once and keeps it in LDS for every head (s_p / s_d and, in long rows, each plane's own
// range of the row are reused or used head after head); the column pass stages a row group's A^T columns once when the group is one chunk --
// s_col then serves every head -- and reads perm again per head (L2 has just served it).  Each head's arithmetic is the single-head code on
// offset pointers, so head hd has the bits of the single-head call on its slices.  spmv_hip_attention_backward is heads = 1.  The launch
// side offsets the pointers to a round's first head (kernels see heads = the round's count and planes from 0).
//
// Bias and its gradient (spmv_hip_attention_bias_backward; the BIAS instantiations of the two row kernels): t_p = (s_p * scale) + B_p exactly
// as in the forward pass (kernels/attention.hpp), and dB_p = P_p (dP_p - D_i) -- the value dS_p is made from by one more multiplication --
// stored from its register by the lane / thread that owns the entry, straight into the caller's plane of the head (db + hd * lddb, CSR
// order).  Either of bias and db may be nullptr in a BIAS instantiation (wave-uniform tests); the column pass knows neither.  The
// instantiations without BIAS are the code from before the bias existed.
//
// Grouped heads (spmv_hip_attention_gqa_backward): K, V, dK and dV hold heads / gs blocks and query head hd belongs to block hd / gs.  The
// row pass only addresses K and V differently (a counter beside hd, outside the per-entry code); P, dS and dB stay per QUERY head.  All four
// kernels have GROUPED instantiations for it, launched when gs > 1; the others do not look at gs and gpos and are the code from before.  The
// column pass computes each head's dK / dV term as before and adds the terms of a group in ascending head: the first is taken as it is,
// every other one is one plain addition, nothing is contracted -- (((t0 + t1) + t2) + ..), the chain a caller can restate.  No head-wide
// dK or dV exists in memory: the running sums are registers (short columns) or the output element itself, read and written by one thread
// (long columns; and wherever a round ends inside a group, the next round continuing from what it finds).
//
// Driven by the final log-sum-exp (spmv_hip_attention_gqa_backward_lse; the STATS instantiations of the two row kernels, which are BIAS ones):
// the caller hands in O (m x heads * dv) and L (`heads` planes of m), the FINAL output and row log-sum-exp of the attention these entries are
// a part of.  Phase B is then a map: P_p = exp(t_p - L_i) -- one subtraction, one exp; no maximum, no sum, no division -- and
// D_i = <G[i, hd * dv ..], O[i, hd * dv ..]>, sddmm's dot for dv columns made by the block that makes dP (attb_tile_dots with "entry" = chunk
// row, q = G, kk = O; one dot per long row), left in LDS with the rows' L beside it.  dB, dS, the stores for the column pass and dQ are as
// before; the column kernels are not touched.  The instantiations without STATS do not look at o and lse and are the code from before.
//
// 16-bit operands (spmv_hip_attention_gqa_backward_16; the instantiations with a storage type other than T, launched from
// spmv_attention_backward.hip's 16-bit parts): Q, K, V and G are fp16 or bf16 in memory (SI), dQ is float or that type (SQ, the row kernels) and dK / dV are
// float or that type (SO, the column kernels) -- kernels/storage16.hpp.  The blocks widen what they load and round what they store; attb_p /
// attb_ds, s_p / s_d, the bias, dB, O, L, scale and every arithmetic step stay float, and the lane mapping stays float's (4 columns per lane, an
// 8-byte segment of a 16-bit operand), so a float output has the bits of the float kernels on the widened operands and a 16-bit one is that value
// rounded ONCE.  The STATS dot <G row, O row> meets a 16-bit row and a float one (att_tile_scores' second storage type).  A 16-bit dK / dV is
// never read back as a partial sum: the GROUPED column kernels exist with float outputs only (static_assert) -- with gs > 1 the launch side
// hands them two handle-owned float arrays (n x kv_heads * k, n x kv_heads * dv), in which the rounds and the long columns add as before, and
// attention_bwd_narrow_kernel rounds every element once into the caller's arrays at the end.  With the defaults (SI = SQ = SO = T) the kernels
// are the code from before.
//
// Arithmetic and order: the composition's, because its blocks are the composition's (kernels/row_blocks.hpp) -- t and P are
// spmv_hip_attention's; dP is sddmm's dot for dv; D is row_softmax_backward's by row length; dS is one subtraction and two plain
// multiplications; dQ, dK and dV are spmm's chains.  Contraction is pinned off: the fmas written out are the only fused operations.
// No atomics, no waiting between workgroups, no scratch memory.
#pragma once
#include "attention.hpp"
#include "dispatch.hpp"
#include "row_blocks.hpp"

namespace spmv {

// what one call's launches need (device pointers); an output that is not wanted is nullptr
struct AttentionBwdArgs {
    int m = 0, k = 0, dv = 0, cus = 256; // k, dv: per head
    int heads = 1, hg = 1;               // heads of the call; heads per round (the planes of p / ds)
    int gs = 1, gpos = 0;                // query heads per K / V head (kk, v, dk, dvo are heads / gs blocks wide); a round: its first head's place in its group
    long long plane = 0;                 // elements per plane of p / ds: nnz
    int nb = 0, nlong = 0; // A: spmm's tables
    const int *split = nullptr, *longs = nullptr, *rowptr = nullptr, *colidx = nullptr;
    int t_rows = 0, t_nb = 0, t_nlong = 0; // A^T (read only when dk or dvo is wanted)
    const int *t_split = nullptr, *t_longs = nullptr, *t_rowptr = nullptr, *t_colidx = nullptr, *perm = nullptr;
    void *p = nullptr, *ds = nullptr; // attb_p, attb_ds: hg planes of nnz elements each, CSR order
    const void *q = nullptr, *kk = nullptr, *v = nullptr, *g = nullptr;
    void *dq = nullptr, *dk = nullptr, *dvo = nullptr;
    long long ldq = 0, ldk = 0, ldv = 0, ldg = 0, lddq = 0, lddk = 0, lddv = 0;
    double scale = 1.0;
    bool vec = false; // every operand, leading dimension and head's first column allows 16-byte accesses
    const void *bias = nullptr; // nullptr: no bias; else head hd's plane at bias + hd * ldb (ldb = 0: one plane shared), CSR order
    void *db = nullptr;         // nullptr: not wanted; else head hd's plane of dL/dB at db + hd * lddb
    long long ldb = 0, lddb = 0;
    const void *o = nullptr, *lse = nullptr; // both set: the STATS row pass from the final O (m x heads * dv) and L (head hd's row i at lse + hd * ldl + i)
    long long ldo = 0, ldl = 0;
    // 16-bit operands only (else all 0 and nullptr).  io_type (SPMV_HIP_T_F16 / _BF16): the element type of q, kk, v, g; dq_type / dkv_type: 0 -- dq / dk and
    // dvo are float --, or io_type.  gs > 1 with 16-bit dK / dV: dk and dvo are the handle's float arrays (dkv_type 0, lddk = kv_heads * k,
    // lddv = kv_heads * dv) and nar_dk / nar_dv the caller's 16-bit ones, rounded into after the last round (nullptr: not wanted)
    int io_type = 0, dq_type = 0, dkv_type = 0;
    void *nar_dk = nullptr, *nar_dv = nullptr;
    long long nar_lddk = 0, nar_lddv = 0;
    int n = 0, kv_heads = 1; // the rows and K / V heads of dk / dvo (the narrowing)
};

// spmv_attention_backward.hip: the launches of one call on `stream`, ceil(heads / hg) rounds of a row pass and a column pass, and with 16-bit
// operands the narrowing of grouped 16-bit dK / dV.  It routes on io_type to the part of that file that holds the instantiations
hipError_t attention_backward_launch(const AttentionBwdArgs &a, bool f64, hipStream_t stream);
template <int IO> hipError_t attention_backward_launch_part(const AttentionBwdArgs &a, bool f64, hipStream_t stream);
template <> hipError_t attention_backward_launch_part<0>(const AttentionBwdArgs &a, bool f64, hipStream_t stream);
template <> hipError_t attention_backward_launch_part<1>(const AttentionBwdArgs &a, bool f64, hipStream_t stream);
template <> hipError_t attention_backward_launch_part<2>(const AttentionBwdArgs &a, bool f64, hipStream_t stream);

// att_tile_scores without the scaling, for a lane group width known at run time (wave-uniform): dP's dots, sddmm's order for dv columns.
// The multiplication by one changes no bit.  S, S2: the storage types of g and of v (att_tile_scores).
template <typename T, bool VEC, typename S = T, typename S2 = S>
__device__ __forceinline__ void attb_tile_dots(int cw, int i, int j, int lane, int dv, const S *__restrict__ g, long long ldg, const S2 *__restrict__ v, long long ldv, T *slot)
{
    with_width(cw, [&](auto CW) { att_tile_scores<T, decltype(CW)::value, VEC>(i, j, lane, dv, g, ldg, v, ldv, T(1), slot); });
}

// One wave per batch [split[b], split[b + 1]) of whole rows; rows longer than kSpmmLongThr are left to attention_bwd_long_kernel.
// CW: sddmm's lane group for k; cwd: the same for dv; 1 << lgk: spmm's lane group for min(k, KP) columns.
// p_out / ds_out / dq: nullptr when dV / dK / dQ is not wanted.  heads: the chunk's columns stay in s_col while the four phases run once per
// head over s_p / s_d, head hd on the columns from hd * k (Q, K, dQ) and hd * dv (V, G) and on plane hd of p_out / ds_out.
// BIAS: bias (added to the scaled scores) and db (P (dP - D), before the scaling) as in the header; either may be nullptr.
// STATS (with BIAS): P and D from the final o and lse (see the header) instead of the row's own reductions.
// SI, SQ: the storage types of Q / K / V / G and of dQ; other than T: 16-bit operands (see the header).
template <typename T, int CW, bool VEC, bool BIAS, bool GROUPED, bool STATS = false, typename SI = T, typename SQ = T>
__global__ __launch_bounds__(kBlock) void attention_bwd_rows_kernel(int nb, const int *__restrict__ split, const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                                    int heads, long long plane, int k, int dv, int cwd, int lgk, T scale,
                                                                    const SI *__restrict__ q, long long ldq, const SI *__restrict__ kk, long long ldk,
                                                                    const SI *__restrict__ v, long long ldv, const SI *__restrict__ g, long long ldg, SQ *__restrict__ dq,
                                                                    long long lddq, T *__restrict__ p_out, T *__restrict__ ds_out, const T *__restrict__ bias,
                                                                    long long ldb, T *__restrict__ db, long long lddb, int gs, int gpos,
                                                                    const T *__restrict__ o = nullptr, long long ldo = 0, const T *__restrict__ lse = nullptr,
                                                                    long long ldl = 0)
{
#pragma clang fp contract(off)
    static_assert(!STATS || BIAS, "the STATS instantiations are BIAS ones");
    constexpr int V = SpmmShape<T>::V, CH = kSpmmChunk;
    __shared__ int s_col[kBlock / kWave][CH];
    __shared__ T s_p[kBlock / kWave][CH];
    __shared__ T s_d[kBlock / kWave][CH];
    [[maybe_unused]] __shared__ T s_D[kBlock / kWave][STATS ? kWave : 1], s_L[kBlock / kWave][STATS ? kWave : 1]; // STATS: D and L of the chunk's rows
    const int w = (int) (threadIdx.x / kWave);
    const int b = blockIdx.x * (kBlock / kWave) + w;
    if (b >= nb) return; // whole waves only; no workgroup barrier follows
    const int lane0 = threadIdx.x & (kWave - 1);
    const int cwk = 1 << lgk, R = kWave >> lgk;
    const int r0 = split[b], r1 = split[b + 1];
    const T ninf = -__builtin_huge_val(), nzero = T(-0.0);
    for (int g0 = r0; g0 < r1;) {
        const ChunkRows ch = chunk_take(rowptr, g0, r1, lane0);
        if (ch.nr == 0) { ++g0; continue; } // a long row: nothing of it here
        const int sl = ch.sl, ll = ch.ll, base = ch.base, nr = ch.nr, nq = ch.nq;

        [[maybe_unused]] int kvh = 0, gc = gpos; // GROUPED: the head's K / V block, kept by counting -- wave-uniform, in scalar registers
        for (int hd = 0; hd < heads; ++hd) {
            const int lane = att_per_head(lane0), subk = lane >> lgk, ck0 = (lane & (cwk - 1)) * V;
            const int hkv = GROUPED ? kvh : hd;
            const SI *qh = q + (long long) hd * k, *kh = kk + (long long) hkv * k, *vh = v + (long long) hkv * dv, *gh = g + (long long) hd * dv; // the head's first columns; K and V: its group's
            if constexpr (GROUPED) {
                if (++gc == gs) { gc = 0; ++kvh; }
            }
            // A. columns (the first head reads them from memory, the others from LDS), scaled scores and dP into LDS
            for (int t0 = 0; t0 < nq; t0 += kWave) {
                const int e = t0 + lane;
                const int pos = chunk_row_of(ch.el, e);
                int i = -1, j = 0;
                if (e < nq) {
                    i = g0 + pos;
                    if (hd == 0) {
                        j = ld_stream(colidx + base + e);
                        s_col[w][e] = j;
                    } else j = s_col[w][e]; // written by this lane
                }
                [[maybe_unused]] T be = T(0);
                if constexpr (BIAS) {
                    if (bias && e < nq) be = ld_stream(bias + (long long) hd * ldb + base + e); // in flight during the dots
                }
                att_tile_scores<T, CW, VEC>(i, j, lane, k, qh, ldq, kh, ldk, scale, s_p[w] + t0);
                if constexpr (BIAS) {
                    if (bias) { // wave-uniform
                        wave_lds_sync();
                        if (e < nq) s_p[w][e] = att_add_bias(s_p[w][e], be); // the product comes back from LDS: never an fma (kernels/attention.hpp)
                    }
                }
                attb_tile_dots<T, VEC>(cwd, i, j, lane, dv, gh, ldg, vh, ldv, s_d[w] + t0);
            }
            if constexpr (STATS) { // D of chunk row l = <G row, O row> of the head, by lane l's "entry" (row g0 + l of G, row g0 + l of O); its L beside it
                const int ir = lane < nr ? g0 + lane : -1;
                attb_tile_dots<T, VEC>(cwd, ir, g0 + lane, lane, dv, gh, ldg, o + (long long) hd * dv, ldo, s_D[w]);
                if (lane < nr) s_L[w][lane] = lse[(long long) hd * ldl + g0 + lane];
            }
            wave_lds_sync();

            // B (STATS). a map over the chunk's entries, lane l on the entries l, l + 64, ..: an element is read and written by the same lane
            if constexpr (STATS) {
                T *dbc = db ? db + (long long) hd * lddb + base : nullptr; // the chunk's range of the head's plane
                for (int t0 = 0; t0 < nq; t0 += kWave) {
                    const int e = t0 + lane;
                    const int pos = chunk_row_of(ch.el, e); // every lane shuffles
                    if (e < nq) {
                        const T pe = row_exp(s_p[w][e] - s_L[w][pos]);
                        const T d0 = pe * (s_d[w][e] - s_D[w][pos]);
                        if (dbc) dbc[e] = d0;
                        s_p[w][e] = pe;
                        s_d[w][e] = att_scale(d0, scale);
                    }
                }
            }
            // B. the row softmax and its backward in place in LDS, in row_reduce_rows_kernel's passes.  An element is read and written by the same lane.
            for (int h0 = 0; !STATS && h0 < nr;) {
                const int hl = h0 + lane; // lane l looks at chunk row h0 + l
                const int sh = __shfl(sl, hl & (kWave - 1), kWave) - base, lh0 = __shfl(ll, hl & (kWave - 1), kWave);
                const int lh = hl < nr ? lh0 : 0;
                int cw, lg;
                row_pass_width(row_width(lh), cw, lg);
                const int sub = lane >> lg, t = lane & (cw - 1);
                const int s = __shfl(sh, sub, kWave), len = __shfl(lh, sub, kWave);
                const bool wide = cw == kWave; // the only passes in which a lane holds more than one term
                T *row = s_p[w] + s, *drow = s_d[w] + s;
                T x[kRowChain], y[kRowChain];
                x[0] = t < len ? row[t] : ninf;
                y[0] = t < len ? drow[t] : nzero;
                if (wide) {
#pragma unroll
                    for (int u = 1; u < kRowChain; ++u) {
                        const bool have = t + u * kWave < len;
                        x[u] = have ? row[t + u * kWave] : ninf;
                        y[u] = have ? drow[t + u * kWave] : nzero;
                    }
                }
                // row_softmax_regs, written out: as a call it costs attention_bwd_rows_kernel<float, 4, false> two registers and with them, at
                // 129, a wave per SIMD.  The one copy of that block: keep the two alike.
                T mx = x[0];
                if (wide) {
#pragma unroll
                    for (int u = 1; u < kRowChain; ++u) mx = row_max(mx, x[u]);
                }
                const T M = row_group_reduce<true>(mx, cw);
                const T e0 = row_exp(x[0] - M);
                x[0] = t < len ? e0 : nzero;
                T acc = x[0];
                if (wide) {
#pragma unroll
                    for (int u = 1; u < kRowChain; ++u) {
                        const bool have = t + u * kWave < len;
                        if (__ballot(have) == 0) break;
                        x[u] = row_exp(x[u] - M);
                        acc = have ? acc + x[u] : acc;
                    }
                }
                const T Z = row_group_reduce<false>(acc, cw);
                const T D = row_dot_regs<T, true>(x, y, t, len, cw, wide, Z); // x becomes P
                if constexpr (BIAS) {
                    T *dbr = db ? db + (long long) hd * lddb + base + s : nullptr; // the row's range of the head's plane
                    if (t < len) {
                        const T d0 = x[0] * (y[0] - D);
                        if (dbr) dbr[t] = d0;
                        row[t] = x[0];
                        drow[t] = att_scale(d0, scale);
                    }
                    if (wide) {
#pragma unroll
                        for (int u = 1; u < kRowChain; ++u)
                            if (t + u * kWave < len) {
                                const T du = x[u] * (y[u] - D);
                                if (dbr) dbr[t + u * kWave] = du;
                                row[t + u * kWave] = x[u];
                                drow[t + u * kWave] = att_scale(du, scale);
                            }
                    }
                } else {
                    if (t < len) {
                        row[t] = x[0];
                        drow[t] = att_scale(x[0] * (y[0] - D), scale);
                    }
                    if (wide) {
#pragma unroll
                        for (int u = 1; u < kRowChain; ++u)
                            if (t + u * kWave < len) {
                                row[t + u * kWave] = x[u];
                                drow[t + u * kWave] = att_scale(x[u] * (y[u] - D), scale);
                            }
                    }
                }
                h0 += kWave >> lg;
            }
            wave_lds_sync();

            // C. what the column pass gathers: P and dS in CSR order, coalesced
            if (p_out)
                for (int e = lane; e < nq; e += kWave) p_out[hd * plane + base + e] = s_p[w][e];
            if (ds_out)
                for (int e = lane; e < nq; e += kWave) ds_out[hd * plane + base + e] = s_d[w][e];

            // D. dQ = A_dS K; the panels reuse dS
            if (dq) rows_times_panels<T, VEC>(ch, g0, R, subk, ck0, s_col[w], s_d[w], kh, ldk, k, dq + (long long) hd * k, lddq);
            wave_lds_sync(); // the next head overwrites s_p / s_d, the next chunk s_col as well
        }
        g0 += nr;
    }
}

// one workgroup per long row (len > kSpmmLongThr >= 256: every thread has a first term); the row's ranges of every plane of pa (attb_p) and
// da (attb_ds) are its own: no other workgroup of this launch touches them.  Head hd parks in plane hd's range.  BIAS, STATS: as in the rows kernel.
template <typename T, int CW, bool VEC, bool BIAS, bool GROUPED, bool STATS = false, typename SI = T, typename SQ = T>
__global__ __launch_bounds__(kBlock) void attention_bwd_long_kernel(int nlong, const int *__restrict__ longs, const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                                    int heads, long long plane, int k, int dv, int cwd, int lgk, T scale,
                                                                    const SI *__restrict__ q, long long ldq, const SI *__restrict__ kk, long long ldk,
                                                                    const SI *__restrict__ v, long long ldv, const SI *__restrict__ g, long long ldg, SQ *__restrict__ dq,
                                                                    long long lddq, T *pa, T *da, const T *__restrict__ bias, long long ldb, T *__restrict__ db,
                                                                    long long lddb, int gs, int gpos, const T *__restrict__ o = nullptr, long long ldo = 0,
                                                                    const T *__restrict__ lse = nullptr, long long ldl = 0)
{
#pragma clang fp contract(off)
    static_assert(!STATS || BIAS, "the STATS instantiations are BIAS ones");
    constexpr int V = SpmmShape<T>::V, KP = SpmmShape<T>::KP;
    __shared__ T part[kSpmmSegs][KP];
    __shared__ T s_slot[kBlock / kWave][kWave], s_slot2[kBlock / kWave][kWave];
    __shared__ T s_max[kBlock / kWave], s_sum[kBlock / kWave];
    const int cwk = 1 << lgk, G = kBlock >> lgk;
    for (int i = blockIdx.x; i < nlong; i += gridDim.x) {
        const int r = longs[i], s = rowptr[r], len = rowptr[r + 1] - s;
        const int *col = colidx + s;
        [[maybe_unused]] int kvh = 0, gc = gpos; // GROUPED: the head's K / V block, kept by counting
        for (int hd = 0; hd < heads; ++hd) {
            const int hkv = GROUPED ? kvh : hd;
            const SI *qh = q + (long long) hd * k, *kh = kk + (long long) hkv * k, *vh = v + (long long) hkv * dv, *gh = g + (long long) hd * dv; // the head's first columns; K and V: its group's
            if constexpr (GROUPED) {
                if (++gc == gs) { gc = 0; ++kvh; }
            }
            const int tid = att_per_head((int) threadIdx.x), w = tid / kWave, lane = tid & (kWave - 1);
            const int subk = tid >> lgk, ck0 = (tid & (cwk - 1)) * V;
            T *t = pa + hd * plane + s, *d = da + hd * plane + s;
            // 1. the scaled scores and dP, parked: tiles of 64 entries, wave w takes the tiles w, w + 4, .. (entry p is thread p % 256's in every phase)
            for (int t0 = w * kWave; t0 < len; t0 += kBlock) {
                const int p = t0 + lane;
                const bool valid = p < len;
                const int j = valid ? col[p] : 0;
                att_tile_scores<T, CW, VEC>(valid ? r : -1, j, lane, k, qh, ldq, kh, ldk, scale, s_slot[w]);
                attb_tile_dots<T, VEC>(cwd, valid ? r : -1, j, lane, dv, gh, ldg, vh, ldv, s_slot2[w]);
                wave_lds_sync();
                if (valid) {
                    if constexpr (BIAS) t[p] = bias ? att_add_bias(s_slot[w][lane], bias[(long long) hd * ldb + s + p]) : s_slot[w][lane];
                    else t[p] = s_slot[w][lane];
                    d[p] = s_slot2[w][lane];
                }
                wave_lds_sync();
            }
            __syncthreads();
            if constexpr (STATS) {
                // 2 + 3 (STATS). one dot <G row, O row> by the first wave (lane 0's "entry"), then the map over the parked range: P and dS in
                // place, every element by the thread that parked it
                if (w == 0) attb_tile_dots<T, VEC>(cwd, lane == 0 ? r : -1, r, lane, dv, gh, ldg, o + (long long) hd * dv, ldo, s_slot[0]);
                __syncthreads();
                const T D = s_slot[0][0], lr = lse[(long long) hd * ldl + r];
                T *dbr = db ? db + (long long) hd * lddb + s : nullptr; // the row's range of the head's plane
                for (int p = tid; p < len; p += kBlock) {
                    const T pe = row_exp(t[p] - lr);
                    const T dp = pe * (d[p] - D);
                    if (dbr) dbr[p] = dp;
                    t[p] = pe;
                    d[p] = att_scale(dp, scale);
                }
            } else {
            // 2. maximum, sum, map over the parked scores, P written in place
            long_row_softmax(t, t, 0, len, tid, s_max, s_sum);
            // 3. D over P and the parked dP, dS written in place
            const T D = long_row_dot(t, d, 0, len, tid, s_sum);
            if constexpr (BIAS) {
                T *dbr = db ? db + (long long) hd * lddb + s : nullptr; // the row's range of the head's plane
                for (int p = tid; p < len; p += kBlock) {
                    const T dp = t[p] * (d[p] - D);
                    if (dbr) dbr[p] = dp;
                    d[p] = att_scale(dp, scale);
                }
            } else {
                for (int p = tid; p < len; p += kBlock) d[p] = att_scale(t[p] * (d[p] - D), scale);
            }
            }
            __syncthreads();
            // 4. dQ = A_dS K, panel by panel; a panel's last barrier also lets the next panel / head / row write part, s_max, s_sum again
            if (dq)
                for (int c = 0; c < k; c += KP)
                    long_row_panel<T>(len, min(KP, k - c), G, subk, ck0, tid, part, dq + (long long) r * lddq + (long long) hd * k + c,
                                      [&](int lo, int hi, int nc, T (&acc)[V]) { spmm_chain<T, VEC, false>(lo, hi, col, d, kh + c, ldk, ck0, nc, acc); });
        }
    }
}

// spmm_rows_kernel on A^T's tables, two outputs off one index stream.  One wave per batch of A^T's rows (A's columns); CW lanes per row for
// the wider of the two panels.  kcv / kck: the columns of this panel of dV / dK (<= 0: not wanted, or no such panel); g, dvo, q, dk are
// offset to the panel's first column of the first head.  pv / dsv: attb_p / attb_ds, plane hd gathered through perm.
// The head loop is around a row group's walk (a row's accumulators live across its chunks, so they cannot be kept for every head).  A group of
// at most kSpmmChunk entries is ONE chunk: its columns are staged by the first head and stay in s_col for the others; a larger group (or one
// with a long row in it) stages them again.  perm is read again by every head: L2 has just served it.
// GROUPED (spmv_hip_attention_gqa_backward with gs > 1): dvo and dk are heads / gs blocks wide, offset to the block of the round's first head,
// whose place in its group is gpos.  A lane's accv / acck of the heads of a group are added, in ascending head, into a running pair in
// registers -- the group's first head is taken as it is, every other one is one plain addition -- and stored once per K / V block; a round
// that starts inside a group (gpos > 0) first reads back what the lane itself stored in the round before, one that ends inside one stores
// what it has.  Without GROUPED gs and gpos are not looked at and the kernel is the code from before the groups existed.
// SI, SO: the storage types of G / Q and of dV / dK.  A 16-bit output is stored once per element and never read: no GROUPED instantiation has one.
template <typename T, int CW, bool VEC, bool GROUPED, typename SI = T, typename SO = T>
__global__ __launch_bounds__(kBlock) void attention_bwd_cols_kernel(int nb, const int *__restrict__ split, const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                                    const int *__restrict__ perm, int heads, long long plane, int k, int dv, const T *__restrict__ pv,
                                                                    const T *__restrict__ dsv, int kcv, const SI *__restrict__ g, long long ldg, SO *__restrict__ dvo,
                                                                    long long lddv, int kck, const SI *__restrict__ q, long long ldq, SO *__restrict__ dk, long long lddk,
                                                                    int gs, int gpos)
{
#pragma clang fp contract(off)
    static_assert(!GROUPED || std::is_same_v<SO, T>, "a 16-bit dK / dV is never read back: the grouped sums are made in float");
    constexpr int V = SpmmShape<T>::V, R = kWave / CW, CH = kSpmmChunk;
    __shared__ int s_col[kBlock / kWave][CH];
    __shared__ T s_p[kBlock / kWave][CH];
    __shared__ T s_d[kBlock / kWave][CH];
    const int w = (int) (threadIdx.x / kWave);
    const int b = blockIdx.x * (kBlock / kWave) + w;
    if (b >= nb) return; // whole waves only; no workgroup barrier follows
    const int lane = threadIdx.x & (kWave - 1), sub = lane / CW, c0 = (lane % CW) * V;
    const int ncv = min(V, kcv - c0), nck = min(V, kck - c0); // <= 0: a lane beyond the panel's columns (it still helps staging)
    const int r0 = split[b], r1 = split[b + 1];
    for (int g0 = r0; g0 < r1; g0 += R) {
        const int g1 = min(g0 + R, r1), r = g0 + sub;
        const bool have = r < g1;
        const int s = have ? rowptr[r] : 0, e = have ? rowptr[r + 1] : 0;
        const bool longrow = e - s > kSpmmLongThr;
        const bool one = rowptr[g1] - rowptr[g0] <= CH; // the whole group is one chunk (and holds no long row): wave-uniform
        [[maybe_unused]] T runv[V], runk[V]; // GROUPED: the sums over the group's heads so far
        [[maybe_unused]] int kvh = 0, gc = gpos;
        for (int hd = 0; hd < heads; ++hd) {
            const T *ph = pv + hd * plane, *dh = dsv + hd * plane;
            const SI *gh = g + (long long) hd * dv, *qh = q + (long long) hd * k; // the head's panel
            T accv[V], acck[V];
#pragma unroll
            for (int t = 0; t < V; ++t) accv[t] = acck[t] = T(0);
            staged_walk(
                rowptr, g0, g1, s, e, longrow, lane,
                [&](int i, int p) {
                    if (hd == 0 || !one) s_col[w][i] = ld_stream(colidx + p);
                    const int pp = ld_stream(perm + p);
                    if (kcv > 0) s_p[w][i] = ph[pp];
                    if (kck > 0) s_d[w][i] = dh[pp];
                },
                [&](int lo, int hi) {
                    if (!longrow && ncv > 0) spmm_chain<T, VEC, false>(lo, hi, s_col[w], s_p[w], gh, ldg, c0, ncv, accv);
                    if (!longrow && nck > 0) spmm_chain<T, VEC, false>(lo, hi, s_col[w], s_d[w], qh, ldq, c0, nck, acck);
                });
            if constexpr (!GROUPED) {
                if (have && !longrow && ncv > 0) spmm_store_y<T, VEC>(dvo + (long long) r * lddv + (long long) hd * dv + c0, ncv, accv);
                if (have && !longrow && nck > 0) spmm_store_y<T, VEC>(dk + (long long) r * lddk + (long long) hd * k + c0, nck, acck);
            } else {
                const bool first = gc == 0, back = hd == 0 && gc > 0, last = gc + 1 == gs || hd + 1 == heads; // wave-uniform
                if (have && !longrow && ncv > 0) {
                    SO *y = dvo + (long long) r * lddv + (long long) kvh * dv + c0;
                    if (back) spmm_load_x<T, VEC>(y, ncv, runv); // this lane's own store of the round before
#pragma unroll
                    for (int t = 0; t < V; ++t) runv[t] = first ? accv[t] : runv[t] + accv[t];
                    if (last) spmm_store_y<T, VEC>(y, ncv, runv);
                }
                if (have && !longrow && nck > 0) {
                    SO *y = dk + (long long) r * lddk + (long long) kvh * k + c0;
                    if (back) spmm_load_x<T, VEC>(y, nck, runk);
#pragma unroll
                    for (int t = 0; t < V; ++t) runk[t] = first ? acck[t] : runk[t] + acck[t];
                    if (last) spmm_store_y<T, VEC>(y, nck, runk);
                }
                if (++gc == gs) { gc = 0; ++kvh; }
            }
        }
    }
}

// spmm_long_kernel on A^T's long rows (columns of A with more than kSpmmLongThr entries), a workgroup each: per head, first dV's panel, then dK's
// GROUPED: head hd's panel goes to its K / V block of dvo / dk, stored by the group's first head and added to what the same thread stored there
// by every other one (long_row_panel's add) -- also across rounds (gpos: the round's first head's place in its group).  Else every head stores.
template <typename T, int CW, bool VEC, bool GROUPED, typename SI = T, typename SO = T>
__global__ __launch_bounds__(kBlock) void attention_bwd_cols_long_kernel(int nlong, const int *__restrict__ longs, const int *__restrict__ rowptr,
                                                                         const int *__restrict__ colidx, const int *__restrict__ perm, int heads, long long plane, int k, int dv,
                                                                         const T *__restrict__ pv, const T *__restrict__ dsv, int kcv, const SI *__restrict__ g, long long ldg,
                                                                         SO *__restrict__ dvo, long long lddv, int kck, const SI *__restrict__ q, long long ldq, SO *__restrict__ dk,
                                                                         long long lddk, int gs, int gpos)
{
#pragma clang fp contract(off)
    static_assert(!GROUPED || std::is_same_v<SO, T>, "a 16-bit dK / dV is never added to: the grouped sums are made in float");
    constexpr int V = SpmmShape<T>::V, KP = SpmmShape<T>::KP, G = kBlock / CW;
    __shared__ T part[kSpmmSegs][KP];
    const int tid = (int) threadIdx.x, sub = tid / CW, c0 = (tid % CW) * V;
    for (int i = blockIdx.x; i < nlong; i += gridDim.x) {
        const int r = longs[i], s = rowptr[r], e = rowptr[r + 1];
        [[maybe_unused]] int kvh = 0, gc = gpos;
        for (int hd = 0; hd < heads; ++hd) {
            const int hkv = GROUPED ? kvh : hd;
            for (int o = 0; o < 2; ++o) { // 0: dV (values P, X = G); 1: dK (values dS, X = Q)
                const int kc = o ? kck : kcv;
                if (kc <= 0) continue; // uniform over the workgroup
                const T *val = (o ? dsv : pv) + hd * plane;
                const SI *x = o ? q + (long long) hd * k : g + (long long) hd * dv;
                const long long ldx = o ? ldq : ldg;
                SO *y = o ? dk + (long long) r * lddk + (long long) hkv * k : dvo + (long long) r * lddv + (long long) hkv * dv;
                long_row_panel<T>(
                    e - s, kc, G, sub, c0, tid, part, y,
                    [&](int lo, int hi, int nc, T (&acc)[V]) {
                        // the global streams of A^T, the values gathered through perm
                        spmm_chain_with<T, VEC>(
                            s + lo, s + hi, [=](int j) { return ld_stream(colidx + j); }, [=](int j) { return val[ld_stream(perm + j)]; }, x, ldx, c0, nc, acc);
                    },
                    GROUPED && gc > 0);
            }
            if constexpr (GROUPED) {
                if (++gc == gs) { gc = 0; ++kvh; }
            }
        }
    }
}

// dst[r, c] = src[r, c] rounded once to the 16-bit type S, r < rows, c < w: src float with leading dimension w (the handle's arrays of the grouped
// column pass), dst with leading dimension ldd.  A thread takes one segment of 4 columns (spmm_load_x / spmm_store_y: VEC -- w a multiple of 4 and
// dst's rows 8-byte aligned -- one 16-byte load and one 8-byte store).  Every element of dst's rows x w block is written, by one thread.
template <typename S, bool VEC>
__global__ __launch_bounds__(kBlock) void attention_bwd_narrow_kernel(long long rows, int w, const float *__restrict__ src, S *__restrict__ dst, long long ldd)
{
    const int segs = (w + 3) / 4;
    const long long total = rows * segs, stride = (long long) gridDim.x * kBlock;
    for (long long i = (long long) blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const long long r = i / segs;
        const int c0 = (int) (i - r * segs) * 4, nc = min(4, w - c0);
        float x[4];
        spmm_load_x<float, VEC>(src + r * w + c0, nc, x);
        spmm_store_y<float, VEC>(dst + r * ldd + c0, nc, x);
    }
}

} // namespace spmv
