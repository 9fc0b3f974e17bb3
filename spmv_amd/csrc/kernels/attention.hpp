// attention.hpp -- O[i, c] = sum over the stored entries p = (i, j_p) of row i of softmax_i(scale * <Q[i, :k], K[j_p, :k]>)[p] * V[j_p, c], c < dv
// (spmv_hip_attention): sddmm, the row softmax and spmm over the resident pattern in one pass.  Q is m x k, K is n x k, V is n x dv, O is
// m x dv, all row-major with leading dimensions.  A's values are neither read nor written; the scores and P never reach HBM for rows of up to
// kSpmmLongThr entries.
//
// Heads (spmv_hip_attention_heads): Q and K are `heads` blocks of k columns side by side, V and O `heads` blocks of dv columns; head hd is the
// single-head product on the columns from hd * k (Q, K) and hd * dv (V, O).  The head loop is inside both kernels, around the three phases:
// the pattern of a chunk is fetched once and kept in LDS for every head, the scores' LDS and the long rows' parking space are reused head after
// head, and each head's arithmetic is the single-head code on offset pointers -- so head hd has the bits of the single-head call on its slices.
// spmv_hip_attention is heads = 1.
//
// Work split: spmm's tables (shim/spmm.hpp) -- equal-nnz batches of whole rows, one wave per batch, and the list of rows longer than
// kSpmmLongThr, a workgroup each.
//
// Short rows (attention_rows_kernel).  A wave walks its batch in chunks of whole rows (chunk_take) -- so every row of a chunk is WHOLE in
// the wave's LDS, which the softmax needs and spmm's chunks do not give.
//   1. scores   tiles of 64 entries: lane l loads ColIdx of entry l (coalesced) and finds its row (chunk_row_of); sddmm's lane groups
//               (att_tile_scores: sddmm_chain, group_sum_dpp) multiply, scale and leave t_p in LDS beside the column.
//   2. softmax  the row softmax's passes (row_pass_width, row_softmax_regs), reading and writing LDS instead of HBM.
//   3. P V      rows_times_panels over V, with P still in LDS.
// Long rows (attention_long_kernel): the scaled scores are parked in a handle-owned array of (sum of the long rows' lengths) elements --
// written once, then long_row_softmax in place --, then long_row_panel per panel of dv.  The parked row is a few KiB per workgroup: L2
// traffic.
//
// Bias (spmv_hip_attention_bias; the BIAS instantiations): t_p = (s_p * scale) + B[hd * ldb + p], a plain multiplication and then a plain addition,
// B in planes of CSR order -- ldb = 0: one plane for every head.  The product always goes through LDS before the addition (att_add_bias reads it
// back): the build's -ffp-contract=fast lets the backend fuse a multiplication and an addition that meet in registers whatever the pragma
// says, and the contract is the two roundings.  Short rows: lane l loads the bias of entry l beside its column (coalesced, streaming) before
// the dots and, after the tile's scores are in LDS, adds it to its own entry's; long rows: added where the score is parked.  Everything after
// t_p is unchanged.  The instantiations without BIAS are the code from before the bias existed.
//
// Grouped heads (spmv_hip_attention_gqa; the GROUPED instantiations, launched when gs > 1): K and V hold heads / gs blocks only and head hd
// reads block hd / gs of them -- a wave-uniform integer kept by a counter beside hd, outside the per-entry code; nothing else differs, so
// head hd has the bits of the single-head call on Q's block hd and K's and V's block hd / gs.  Consecutive heads of a group gather the same
// K and V rows: that reuse is left to the caches.  The instantiations without GROUPED do not look at gs and are the code
// from before the groups existed (as a runtime argument alone gs moved the register allocation of every instantiation: DESIGN.md 3.21).
//
// Log-sum-exp (spmv_hip_attention_gqa_lse; the LSE instantiations, launched when L is wanted): L[hd * ldl + i] = M_i + log(Z_i), M_i and Z_i the
// very registers the row softmax divides by (row_softmax_regs_m, long_row_softmax_mz), log the device library's, one plain addition -- stored
// by lane 0 of the row's group (short rows; a row without entries gets -inf there) or thread 0 of the workgroup (long rows).  O's arithmetic is
// untouched.  LSE implies BIAS, with bias == nullptr allowed there (a wave-uniform test); the instantiations without LSE do not look at lse and
// ldl and are the code from before.
//
// 16-bit operands (spmv_hip_attention_gqa_lse_16; the instantiations with SI or SO other than T, launched from spmv_attention.hip's 16-bit parts): Q, K and V
// are fp16 or bf16 in memory (SI) and O is float or that type (SO) -- kernels/storage16.hpp.  The blocks widen what they load and round what they
// store; the parked scores, s_p, the bias, L, scale and every arithmetic step stay float, and the lane mapping stays float's -- W = V = 4 columns
// per lane, CW = panel_group_width<float>(k), lgv = panel_group_lg<float>(dv) --, because it fixes the summation order: O (before the one
// rounding of a 16-bit O) and L have the bits of the float kernels on the widened operands.  A lane's segment is 8 bytes: VEC is one 8-byte
// access there.  These instantiations are always the BIAS + LSE family and also test lse for nullptr (wave-uniform); with SI = SO = T (the
// defaults) that test is true at compile time and the kernels are the code from before.
//
// Arithmetic and order: the composition's, because its blocks are the composition's (kernels/row_blocks.hpp) -- s_p is sddmm's dot for this
// k (kernels/sddmm.hpp), t_p = s_p * scale one plain multiplication, M_i / Z_i / P_p = exp(t_p - M_i) / Z_i the row softmax's by row length,
// O[i, c] spmm's chain.  The result is a function of the matrix, k, dv and the value type alone.  Contraction is pinned off: the fmas written
// out are the only fused operations.  No atomics, no waiting between workgroups, no scratch memory.
#pragma once
#include "common.hpp"
#include "row_blocks.hpp"
#include "row_softmax.hpp"
#include "sddmm.hpp"
#include "spmm.hpp"

namespace spmv {

// what one call's launches need (device pointers)
struct AttentionArgs {
    int m = 0, heads = 1, k = 0, dv = 0, nb = 0, nlong = 0, cus = 256; // k, dv: per head
    int gs = 1; // query heads per K / V head: kk and v are heads / gs blocks wide, head hd reads block hd / gs
    const int *split = nullptr, *longs = nullptr, *rowptr = nullptr, *colidx = nullptr;
    const int *long_off = nullptr; // first parked element of long row i of the list
    void *park = nullptr;          // the long rows' scores, then P
    const void *q = nullptr, *kk = nullptr, *v = nullptr;
    void *o = nullptr;
    long long ldq = 0, ldk = 0, ldv = 0, ldo = 0;
    double scale = 1.0;
    bool vec = false; // q, kk, v, o, their leading dimensions and every head's first column allow 16-byte accesses (16-bit operands: 8-byte)
    int io_type = 0, o_type = 0; // SPMV_HIP_T_*: the element type of q, kk, v and of o; 0 = the handle's, else F16 or BF16 (float arithmetic; o_type 0 or io_type)
    const void *bias = nullptr; // nullptr: no bias; else planes of nnz elements in CSR order, head hd's at bias + hd * ldb (ldb = 0: one plane shared)
    long long ldb = 0;
    void *lse = nullptr; // nullptr: not wanted; else `heads` planes of m elements, head hd's row i at lse + hd * ldl + i
    long long ldl = 0;
};

// spmv_attention.hip: the launches of one call on `stream`.  It routes on io_type to the part of that file -- one per element type of Q, K and V,
// compiled side by side -- that holds the instantiations
hipError_t attention_launch(const AttentionArgs &a, bool f64, hipStream_t stream);
template <int IO> hipError_t attention_launch_part(const AttentionArgs &a, bool f64, hipStream_t stream);
template <> hipError_t attention_launch_part<0>(const AttentionArgs &a, bool f64, hipStream_t stream);
template <> hipError_t attention_launch_part<1>(const AttentionArgs &a, bool f64, hipStream_t stream);
template <> hipError_t attention_launch_part<2>(const AttentionArgs &a, bool f64, hipStream_t stream);

// lengths of the listed long rows (the shim turns them into long_off)
static __global__ __launch_bounds__(kBlock) void attention_long_len_kernel(int nlong, const int *__restrict__ longs, const int *__restrict__ rowptr, int *__restrict__ len)
{
    const long long stride = (long long) gridDim.x * kBlock;
    for (long long i = (long long) blockIdx.x * kBlock + threadIdx.x; i < nlong; i += stride) len[i] = rowptr[longs[i] + 1] - rowptr[longs[i]];
}

// x, as a value the compiler computes with again in every head: what a thread derives from its index (addresses, lane-group coordinates) is
// cheap to redo and would otherwise be hoisted out of the head loop and kept in registers across all three phases
__device__ __forceinline__ int att_per_head(int x)
{
    asm volatile("" : "+v"(x));
    return x;
}

template <typename T>
__device__ __forceinline__ T att_scale(T s, T scale)
{
#pragma clang fp contract(off)
    return s * scale;
}

// t_p with a bias, from the scaled score READ BACK FROM LDS (see the header): the composition's second rounding, never an fma
template <typename T>
__device__ __forceinline__ T att_add_bias(T t, T b)
{
#pragma clang fp contract(off)
    return t + b;
}

// The scaled scores of one tile of 64 entries.  Lane l passes its entry's row i (-1: no entry) and column j; the tile's entries are multiplied
// in CW rounds of 64 / CW, CW adjacent lanes per entry (sddmm_kernel's rounds, the same chain and the same tree), and t of entry e lands in
// slot[e] (the wave's own LDS; the caller synchronizes).  Every lane of the wave must call.  S, S2: the storage types of q and of kk (sddmm_chain).
template <typename T, int CW, bool VEC, typename S = T, typename S2 = S>
__device__ __forceinline__ void att_tile_scores(int i, int j, int lane, int k, const S *__restrict__ q, long long ldq, const S2 *__restrict__ kk, long long ldk, T scale,
                                                T *slot)
{
    constexpr int W = SddmmShape<T>::W, G = kWave / CW;
    const int sub = lane / CW, c0 = (lane % CW) * W;
#pragma unroll 2
    for (int round = 0; round < CW; ++round) {
        const int e = round * G + sub;
        const int ie = __shfl(i, e, kWave), je = __shfl(j, e, kWave);
        T acc = T(-0.0); // x + (-0) = x for every x, signed zeros included
        if (ie >= 0 && c0 < k) acc = sddmm_chain<T, VEC>(q + (long long) ie * ldq, kk + (long long) je * ldk, c0, CW * W, k);
        acc = group_sum_dpp<CW>(acc);
        if (ie >= 0 && lane % CW == 0) slot[e] = att_scale(acc, scale);
    }
}

// One wave per batch [split[b], split[b + 1]) of whole rows; rows longer than kSpmmLongThr are left to attention_long_kernel.
// CW: sddmm's lane group for k; 1 << lgv: spmm's lane group for min(dv, KP) columns.  heads: the chunk's columns stay in s_col while the
// three phases run once per head over s_p, head hd on the columns from hd * k of Q and K and from hd * dv of V and O.  BIAS: head hd adds
// bias[hd * ldb + p] to the scaled score of entry p (bias is not nullptr, except with LSE).  GROUPED: gs > 1 heads per K / V block.
// LSE (with BIAS): lse is not nullptr and gets every row's M + log(Z) of every head; bias may be nullptr.  SI, SO: the storage types of
// Q / K / V and of O; other than T (16-bit operands): an LSE instantiation in which lse may be nullptr as well.
template <typename T, int CW, bool VEC, bool BIAS, bool GROUPED, bool LSE = false, typename SI = T, typename SO = T>
__global__ __launch_bounds__(kBlock) void attention_rows_kernel(int nb, const int *__restrict__ split, const int *__restrict__ rowptr, const int *__restrict__ colidx, int heads,
                                                                int k, int dv, int lgv, T scale, const SI *__restrict__ q, long long ldq, const SI *__restrict__ kk, long long ldk,
                                                                const SI *__restrict__ v, long long ldv, SO *__restrict__ o, long long ldo, const T *__restrict__ bias,
                                                                long long ldb, int gs, T *__restrict__ lse = nullptr, long long ldl = 0)
{
#pragma clang fp contract(off)
    static_assert(!LSE || BIAS, "the LSE instantiations are BIAS ones");
    constexpr bool LOPT = !std::is_same_v<SI, T> || !std::is_same_v<SO, T>; // lse may be nullptr
    static_assert(!LOPT || LSE, "the 16-bit instantiations are LSE ones");
    constexpr int V = SpmmShape<T>::V, CH = kSpmmChunk;
    __shared__ int s_col[kBlock / kWave][CH];
    __shared__ T s_p[kBlock / kWave][CH];
    const int w = (int) (threadIdx.x / kWave);
    const int b = blockIdx.x * (kBlock / kWave) + w;
    if (b >= nb) return; // whole waves only; no workgroup barrier follows
    const int lane0 = threadIdx.x & (kWave - 1);
    const int cwv = 1 << lgv, R = kWave >> lgv;
    const int r0 = split[b], r1 = split[b + 1];
    const T ninf = -__builtin_huge_val();
    for (int g0 = r0; g0 < r1;) {
        const ChunkRows ch = chunk_take(rowptr, g0, r1, lane0);
        if (ch.nr == 0) { ++g0; continue; } // a long row: nothing of it here
        const int sl = ch.sl, ll = ch.ll, base = ch.base, nr = ch.nr, nq = ch.nq;

        [[maybe_unused]] int kvh = 0, gc = 0; // GROUPED: kvh = hd / gs, kept by counting -- wave-uniform, in scalar registers
        for (int hd = 0; hd < heads; ++hd) {
            const int lane = att_per_head(lane0), subv = lane >> lgv, cv0 = (lane & (cwv - 1)) * V;
            const int hkv = GROUPED ? kvh : hd;
            const SI *qh = q + (long long) hd * k, *kh = kk + (long long) hkv * k, *vh = v + (long long) hkv * dv; // the head's first columns; K and V: its group's
            if constexpr (GROUPED) {
                if (++gc == gs) { gc = 0; ++kvh; }
            }
            SO *oh = o + (long long) hd * dv;
            // 1. columns (the first head reads them from memory, the others from LDS) and scaled scores into LDS
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
                if constexpr (BIAS) {
                    const bool hb = !LSE || bias != nullptr; // wave-uniform; without LSE: true at compile time
                    const T be = hb && e < nq ? ld_stream(bias + (long long) hd * ldb + base + e) : T(0); // in flight during the dots
                    att_tile_scores<T, CW, VEC>(i, j, lane, k, qh, ldq, kh, ldk, scale, s_p[w] + t0);
                    if (hb) {
                        wave_lds_sync();
                        if (e < nq) s_p[w][e] = att_add_bias(s_p[w][e], be); // lane l: its own entry, written by another lane
                    }
                } else att_tile_scores<T, CW, VEC>(i, j, lane, k, qh, ldq, kh, ldk, scale, s_p[w] + t0);
            }
            wave_lds_sync();

            // 2. the row softmax in place in LDS, in row_reduce_rows_kernel's passes.  An element is read and written by the same lane.
            for (int h0 = 0; h0 < nr;) {
                const int hl = h0 + lane; // lane l looks at chunk row h0 + l
                const int sh = __shfl(sl, hl & (kWave - 1), kWave) - base, lh0 = __shfl(ll, hl & (kWave - 1), kWave);
                const int lh = hl < nr ? lh0 : 0;
                int cw, lg;
                row_pass_width(row_width(lh), cw, lg);
                const int sub = lane >> lg, t = lane & (cw - 1);
                const int s = __shfl(sh, sub, kWave), len = __shfl(lh, sub, kWave);
                const bool wide = cw == kWave; // the only passes in which a lane holds more than one term
                T *row = s_p[w] + s;
                T x[kRowChain];
                x[0] = t < len ? row[t] : ninf;
                if (wide) {
#pragma unroll
                    for (int u = 1; u < kRowChain; ++u) x[u] = t + u * kWave < len ? row[t + u * kWave] : ninf;
                }
                T Z;
                if constexpr (LSE) {
                    T M;
                    Z = row_softmax_regs_m(x, t, len, cw, wide, M);
                    // one lane per served row; a row without entries: -inf
                    if ((!LOPT || lse != nullptr) && t == 0 && h0 + sub < nr) lse[(long long) hd * ldl + g0 + h0 + sub] = len > 0 ? row_lse(M, Z) : ninf;
                } else Z = row_softmax_regs(x, t, len, cw, wide);
                if (t < len) row[t] = x[0] / Z;
                if (wide) {
#pragma unroll
                    for (int u = 1; u < kRowChain; ++u)
                        if (t + u * kWave < len) row[t + u * kWave] = x[u] / Z;
                }
                h0 += kWave >> lg;
            }
            wave_lds_sync();

            // 3. O = P V; the panels reuse P
            rows_times_panels<T, VEC>(ch, g0, R, subv, cv0, s_col[w], s_p[w], vh, ldv, dv, oh, ldo);
            wave_lds_sync(); // the next head overwrites s_p, the next chunk s_col as well
        }
        g0 += nr;
    }
}

// one workgroup per long row (len > kSpmmLongThr >= 256: every thread has a first term); park + long_off[i]: len elements of its own, used by
// one head after the other (the barrier that ends a head's last panel is also the one before the next head parks its scores).  BIAS: the
// bias is added where the score is parked.  LSE: as in the rows kernel, thread 0 stores.
template <typename T, int CW, bool VEC, bool BIAS, bool GROUPED, bool LSE = false, typename SI = T, typename SO = T>
__global__ __launch_bounds__(kBlock) void attention_long_kernel(int nlong, const int *__restrict__ longs, const int *__restrict__ long_off, const int *__restrict__ rowptr,
                                                                const int *__restrict__ colidx, int heads, int k, int dv, int lgv, T scale, const SI *__restrict__ q, long long ldq,
                                                                const SI *__restrict__ kk, long long ldk, const SI *__restrict__ v, long long ldv, SO *__restrict__ o, long long ldo,
                                                                T *park, const T *__restrict__ bias, long long ldb, int gs, T *__restrict__ lse = nullptr,
                                                                long long ldl = 0)
{
#pragma clang fp contract(off)
    static_assert(!LSE || BIAS, "the LSE instantiations are BIAS ones");
    constexpr bool LOPT = !std::is_same_v<SI, T> || !std::is_same_v<SO, T>; // lse may be nullptr
    static_assert(!LOPT || LSE, "the 16-bit instantiations are LSE ones");
    constexpr int V = SpmmShape<T>::V, KP = SpmmShape<T>::KP;
    __shared__ T part[kSpmmSegs][KP];
    __shared__ T s_slot[kBlock / kWave][kWave];
    __shared__ T s_max[kBlock / kWave], s_sum[kBlock / kWave];
    const int cwv = 1 << lgv, G = kBlock >> lgv;
    for (int i = blockIdx.x; i < nlong; i += gridDim.x) {
        const int r = longs[i], s = rowptr[r], len = rowptr[r + 1] - s;
        const int *col = colidx + s;
        T *t = park + long_off[i];
        [[maybe_unused]] int kvh = 0, gc = 0; // GROUPED: kvh = hd / gs, kept by counting
        for (int hd = 0; hd < heads; ++hd) {
            const int hkv = GROUPED ? kvh : hd;
            const SI *qh = q + (long long) hd * k, *kh = kk + (long long) hkv * k, *vh = v + (long long) hkv * dv; // the head's first columns; K and V: its group's
            SO *oh = o + (long long) hd * dv;
            if constexpr (GROUPED) {
                if (++gc == gs) { gc = 0; ++kvh; }
            }
            const int tid = att_per_head((int) threadIdx.x), w = tid / kWave, lane = tid & (kWave - 1);
            const int subv = tid >> lgv, cv0 = (tid & (cwv - 1)) * V;
            // 1. the scaled scores, parked: tiles of 64 entries, wave w takes the tiles w, w + 4, .. (entry p is thread p % 256's in every phase)
            for (int t0 = w * kWave; t0 < len; t0 += kBlock) {
                const int p = t0 + lane;
                const bool valid = p < len;
                const int j = valid ? col[p] : 0;
                att_tile_scores<T, CW, VEC>(valid ? r : -1, j, lane, k, qh, ldq, kh, ldk, scale, s_slot[w]);
                wave_lds_sync();
                if constexpr (BIAS) {
                    if constexpr (LSE) {
                        if (valid) t[p] = bias ? att_add_bias(s_slot[w][lane], bias[(long long) hd * ldb + s + p]) : s_slot[w][lane];
                    } else {
                        if (valid) t[p] = att_add_bias(s_slot[w][lane], bias[(long long) hd * ldb + s + p]);
                    }
                } else {
                    if (valid) t[p] = s_slot[w][lane];
                }
                wave_lds_sync();
            }
            __syncthreads();
            // 2. maximum, sum, map over the parked scores, P written in place
            if constexpr (LSE) {
                T M, Z;
                long_row_softmax_mz(t, t, 0, len, tid, s_max, s_sum, M, Z);
                if ((!LOPT || lse != nullptr) && tid == 0) lse[(long long) hd * ldl + r] = row_lse(M, Z);
            } else long_row_softmax(t, t, 0, len, tid, s_max, s_sum);
            // 3. O = P V, panel by panel; a panel's last barrier also lets the next panel / head / row write part and the parked scores again
            for (int c = 0; c < dv; c += KP)
                long_row_panel<T>(len, min(KP, dv - c), G, subv, cv0, tid, part, oh + (long long) r * ldo + c,
                                  [&](int lo, int hi, int nc, T (&acc)[V]) { spmm_chain<T, VEC, false>(lo, hi, col, t, vh + c, ldv, cv0, nc, acc); });
        }
    }
}

} // namespace spmv
