// row_blocks.hpp -- the device blocks that spmm, the row softmax, the fused attention and its backward are built from.  Each block exists
// once, and its comment is the one statement of its summation order: a kernel that promises "the bits of the composition" keeps the promise by
// calling the block the composed kernels call.  Blocks declare no LDS (the kernels do, and pass it in) and every block that does
// floating-point arithmetic pins contraction off itself (the pragma is lexical): the fmas written out are the only fused operations.
//
//   shapes           SpmmShape, kSpmmLongThr / kSpmmSegs / kSpmmChunk, kRowChain
//   X rows, chains   spmm_load_x, spmm_store_y, spmm_chain_with / spmm_chain
//   a row in regs    row_width, row_group_reduce, row_pass_width, row_softmax_regs_m / row_softmax_regs, row_lse, row_dot_regs
//   a long row       long_row_softmax_mz / long_row_softmax, long_row_dot, long_row_panel
//   chunks of rows   chunk_take, chunk_row_of, rows_times_panels, staged_walk
#pragma once
#include "common.hpp"
#include "storage16.hpp"

namespace spmv {

constexpr int kSpmmLongThr = 512; // longer rows: a workgroup each
constexpr int kSpmmSegs = 64;     // ... cut into this many equal segments, combined in a fixed order
constexpr int kSpmmLanes = 8;     // lanes per X row segment at full panel width
constexpr int kSpmmChunk = 512;   // entries of a row group staged through a wave's LDS at a time

constexpr int kRowChain = kSpmmLongThr / kWave; // terms per lane of the longest short row: 8

template <typename T> struct SpmmShape {
    static constexpr int V = 16 / (int) sizeof(T);  // columns per lane
    static constexpr int KP = kSpmmLanes * V;       // panel width
};

// ---- X row segments and the chain over a row's entries --------------------------------------------------------------------------------

// X row segment of one lane: nc (<= V) columns from p; a 16-byte load when allowed and the segment is whole.  S: what X is in memory
// (kernels/storage16.hpp) -- T itself, or a 16-bit type widened here: the same V columns per lane, an 8-byte segment, one 8-byte load when allowed
template <typename T, bool VEC, typename S = T>
__device__ __forceinline__ void spmm_load_x(const S *p, int nc, T (&o)[SpmmShape<T>::V])
{
    constexpr int V = SpmmShape<T>::V;
    if constexpr (!std::is_same_v<S, T>) {
        static_assert(std::is_same_v<T, float> && is_storage16<S>, "16-bit storage is for float arithmetic");
        if (VEC && nc == V) st16_load4(p, o);
        else {
#pragma unroll
            for (int t = 0; t < V; ++t) o[t] = t < nc ? st16_widen(p[t]) : T(0);
        }
    } else if (VEC && nc == V) {
        if constexpr (sizeof(T) == 8) {
            const f64x2 v = *reinterpret_cast<const f64x2 *>(p);
            o[0] = v.x; o[1] = v.y;
        } else {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
    } else {
#pragma unroll
        for (int t = 0; t < V; ++t) o[t] = t < nc ? p[t] : T(0);
    }
}

// Y row segment of one lane.  S: what Y is in memory -- T itself, or a 16-bit type: every element rounded once (st16_narrow), an 8-byte store
// when allowed and the segment is whole
template <typename T, bool VEC, typename S = T>
__device__ __forceinline__ void spmm_store_y(S *p, int nc, const T (&a)[SpmmShape<T>::V])
{
    constexpr int V = SpmmShape<T>::V;
    if constexpr (!std::is_same_v<S, T>) {
        static_assert(std::is_same_v<T, float> && is_storage16<S>, "16-bit storage is for float arithmetic");
        if (VEC && nc == V) st16_store4(p, a);
        else {
#pragma unroll
            for (int t = 0; t < V; ++t)
                if (t < nc) p[t] = st16_narrow<S>(a[t]);
        }
    } else if (VEC && nc == V) {
        if constexpr (sizeof(T) == 8) *reinterpret_cast<f64x2 *>(p) = f64x2{a[0], a[1]};
        else *reinterpret_cast<f32x4 *>(p) = f32x4{a[0], a[1], a[2], a[3]};
    } else {
#pragma unroll
        for (int t = 0; t < V; ++t)
            if (t < nc) p[t] = a[t];
    }
}

// acc[t] = fma(val_of(j), X[col_of(j)][c0 + t], acc[t]) for j = s .. e - 1, strictly in that order: ONE lane's sequential chain per (row,
// column).  Where the column and the value of entry j come from (a global stream, the wave's LDS copy of a chunk, a gather through a
// permutation) is the caller's: the same values in the same order give identical bits.  S: X's storage type (spmm_load_x), told by x.
template <typename T, bool VEC, typename ColOf, typename ValOf, typename S = T>
__device__ __forceinline__ void spmm_chain_with(int s, int e, ColOf col_of, ValOf val_of, const S *__restrict__ x, long long ldx, int c0, int nc, T (&acc)[SpmmShape<T>::V])
{
    constexpr int V = SpmmShape<T>::V, U = 4;
    int j = s;
    for (; j + U <= e; j += U) {
        int c[U];
        T v[U], xv[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            c[u] = col_of(j + u);
            v[u] = val_of(j + u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) spmm_load_x<T, VEC>(x + (long long) c[u] * ldx + c0, nc, xv[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < V; ++t) acc[t] = fmadd(v[u], xv[u][t], acc[t]);
    }
    for (; j < e; ++j) {
        const int c = col_of(j);
        const T v = val_of(j);
        T xv[V];
        spmm_load_x<T, VEC>(x + (long long) c * ldx + c0, nc, xv);
#pragma unroll
        for (int t = 0; t < V; ++t) acc[t] = fmadd(v, xv[t], acc[t]);
    }
}

// the chain over colidx[j], val[j].  NT: the two are global streams read once; else the wave's LDS copy of a chunk, or a parked row
template <typename T, bool VEC, bool NT, typename S = T>
__device__ __forceinline__ void spmm_chain(int s, int e, const int *__restrict__ colidx, const T *__restrict__ val, const S *__restrict__ x, long long ldx,
                                           int c0, int nc, T (&acc)[SpmmShape<T>::V])
{
    spmm_chain_with<T, VEC>(
        s, e, [=](int j) { return NT ? ld_stream(colidx + j) : colidx[j]; }, [=](int j) { return NT ? ld_stream(val + j) : val[j]; }, x, ldx, c0, nc, acc);
}

// ---- one row in the registers of a lane group ---------------------------------------------------------------------------------------------

__device__ __forceinline__ float row_exp(float x) { return expf(x); }
__device__ __forceinline__ double row_exp(double x) { return exp(x); }
__device__ __forceinline__ float row_max(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double row_max(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float row_log(float x) { return logf(x); }
__device__ __forceinline__ double row_log(double x) { return log(x); }

// the row's log-sum-exp from the softmax's own M and Z: the device library's log and one plain addition
template <typename T>
__device__ __forceinline__ T row_lse(T M, T Z)
{
#pragma clang fp contract(off)
    return M + row_log(Z);
}

// lanes a row of len entries needs: W = 1 for len <= 1, else the smallest power of two >= len, 64 at the most
__device__ __forceinline__ int row_width(int len) { return len <= 1 ? 1 : (len >= kWave ? kWave : 1 << (32 - __builtin_clz(len - 1))); }

// max (MAX) or sum over groups of cw consecutive lanes, cw a wave-uniform power of two; every lane of the group gets the result.
// The sum is a balanced tree over neighbours: ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)), .. up to cw = 64.
template <bool MAX, typename T>
__device__ __forceinline__ T row_group_reduce(T v, int cw)
{
#pragma clang fp contract(off)
    auto op = [](T a, T b) { if constexpr (MAX) return row_max(a, b); else return a + b; };
    if (cw >= 2) v = op(v, dpp_mov<0xB1>(v));   // quad_perm [1,0,3,2]
    if (cw >= 4) v = op(v, dpp_mov<0x4E>(v));   // quad_perm [2,3,0,1]
    if (cw >= 8) v = op(v, dpp_mov<0x141>(v));  // row_half_mirror: the other quad of each 8
    if (cw >= 16) v = op(v, dpp_mov<0x140>(v)); // row_mirror: the other half of each 16
    if (cw >= 32) v = op(v, (T) __shfl_xor(v, 16, kWave));
    if (cw >= 64) v = op(v, (T) __shfl_xor(v, 32, kWave));
    return v;
}

// The lane-group width of a pass over short rows.  Lane l holds wl = row_width of the l-th of the next rows (1 for a row that is not served);
// cw adjacent lanes serve one row and the first 64 / cw rows go side by side: cw = 1 << lg is the smallest power of two for which none of
// those rows needs more lanes (six ballots).  Wave-uniform.
__device__ __forceinline__ void row_pass_width(int wl, int &cw, int &lg)
{
    for (cw = 1, lg = 0; cw < kWave; cw <<= 1, ++lg)
        if ((__ballot(wl > cw) & (~0ull >> (kWave - kWave / cw))) == 0) break;
}

// Softmax of a row held by a group of cw lanes; returns Z.  Lane t of the group holds the scores t, t + 64, .. < len in x[0], x[1], ..
// (x[1..] only in wide = (cw == 64) passes), -inf where it has no term.  On return x[j] = exp(x[j] - M) where the lane has a term, x[0] = -0
// where it has none (a further x[j] without a term holds no meaning); the caller divides by Z.
// Order -- a function of the row's length and the value type alone: with W = row_width(len), virtual lane t < W chains the terms t, t + W, ..
// in that order, the first as it is and every further one a plain addition onto the chain; a lane without a term holds -0, the identity of
// IEEE addition; the W chains are added by row_group_reduce's tree.  A group wider than W only adds further -0 lanes: x + (-0) = x for every
// x, the bits are those of width W.  The maximum is exact in any order (fmax drops a NaN; the sum then restores it: exp(NaN - M) is NaN).
// row_softmax_regs_m also hands out M (for the row's log-sum-exp, row_lse); row_softmax_regs is the same code without it.
template <typename T>
__device__ __forceinline__ T row_softmax_regs_m(T (&x)[kRowChain], const int t, const int len, const int cw, const bool wide, T &M)
{
#pragma clang fp contract(off)
    T mx = x[0];
    if (wide) {
#pragma unroll
        for (int j = 1; j < kRowChain; ++j) mx = row_max(mx, x[j]);
    }
    M = row_group_reduce<true>(mx, cw);
    const T e0 = row_exp(x[0] - M), nzero = T(-0.0);
    x[0] = t < len ? e0 : nzero;
    T acc = x[0];
    if (wide) {
#pragma unroll
        for (int j = 1; j < kRowChain; ++j) {
            const bool have = t + j * kWave < len;
            if (__ballot(have) == 0) break;
            x[j] = row_exp(x[j] - M);
            acc = have ? acc + x[j] : acc;
        }
    }
    return row_group_reduce<false>(acc, cw);
}

template <typename T>
__device__ __forceinline__ T row_softmax_regs(T (&x)[kRowChain], const int t, const int len, const int cw, const bool wide)
{
    T M;
    return row_softmax_regs_m(x, t, len, cw, wide, M);
}

// D = sum over the row of x * y, the row held like row_softmax_regs' (what a lane holds where it has no term is not read).  Order: virtual
// lane t chains its terms in the same order, the first a plain product, every further one fma(x, y, chain); a lane without a term holds -0;
// then the same tree.  DIV: x is divided by Z first, each term just before it is used (the backward of attention: exp(t - M) becomes P).
template <typename T, bool DIV = false>
__device__ __forceinline__ T row_dot_regs(T (&x)[kRowChain], const T (&y)[kRowChain], int t, int len, int cw, bool wide, T Z = T(1))
{
#pragma clang fp contract(off)
    if (DIV) x[0] = x[0] / Z;
    T acc = t < len ? x[0] * y[0] : T(-0.0);
    if (wide) {
#pragma unroll
        for (int j = 1; j < kRowChain; ++j) {
            const bool have = t + j * kWave < len;
            if (__ballot(have) == 0) break;
            if (DIV) x[j] = x[j] / Z;
            acc = have ? fmadd(x[j], y[j], acc) : acc;
        }
    }
    return row_group_reduce<false>(acc, cw);
}

// ---- one long row (len > kSpmmLongThr >= 256: every thread has a first term), a workgroup of 256 --------------------------------------------

// out[p] = exp(in[p] - M) / Z for the row's elements p in [s, e); out may be in.  Thread tid chains the terms s + tid, s + tid + 256, ..
// (the first as it is, every further one a plain addition), the 64 chains of a wave are added by row_group_reduce's tree, and the four
// waves' results as (w0 + w1) + (w2 + w3) through s_max / s_sum.  The row is read again for each phase (max, sum, map); every element is
// read and written by the same thread in every phase.  Ends with the barrier after which out is every thread's to read and s_max / s_sum
// may be written again.  long_row_softmax_mz also hands out M and Z (every thread holds them); long_row_softmax is the same code without them.
template <typename T>
__device__ __forceinline__ void long_row_softmax_mz(const T *in, T *out, int s, int e, int tid, T *s_max, T *s_sum, T &M, T &Z)
{
#pragma clang fp contract(off)
    const int w = tid / kWave, lane = tid & (kWave - 1);
    T mx = in[s + tid];
    for (int p = s + tid + kBlock; p < e; p += kBlock) mx = row_max(mx, in[p]);
    mx = row_group_reduce<true>(mx, kWave);
    if (lane == 0) s_max[w] = mx;
    __syncthreads();
    M = row_max(row_max(s_max[0], s_max[1]), row_max(s_max[2], s_max[3]));
    T acc = row_exp(in[s + tid] - M);
    for (int p = s + tid + kBlock; p < e; p += kBlock) acc = acc + row_exp(in[p] - M);
    acc = row_group_reduce<false>(acc, kWave);
    if (lane == 0) s_sum[w] = acc;
    __syncthreads();
    Z = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    for (int p = s + tid; p < e; p += kBlock) out[p] = row_exp(in[p] - M) / Z;
    __syncthreads();
}

template <typename T>
__device__ __forceinline__ void long_row_softmax(const T *in, T *out, int s, int e, int tid, T *s_max, T *s_sum)
{
    T M, Z;
    long_row_softmax_mz(in, out, s, e, tid, s_max, s_sum, M, Z);
}

// D = sum over p in [s, e) of x[p] * y[p], in long_row_softmax's order with the first term a plain product and every further one
// fma(x, y, chain).  The caller maps with D and then places the barrier after which s_sum may be written again.
template <typename T>
__device__ __forceinline__ T long_row_dot(const T *x, const T *y, int s, int e, int tid, T *s_sum)
{
#pragma clang fp contract(off)
    const int w = tid / kWave, lane = tid & (kWave - 1);
    T acc = x[s + tid] * y[s + tid];
    for (int p = s + tid + kBlock; p < e; p += kBlock) acc = fmadd(x[p], y[p], acc);
    acc = row_group_reduce<false>(acc, kWave);
    if (lane == 0) s_sum[w] = acc;
    __syncthreads();
    return (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

// One panel of kc columns of a long row's product: y[c] = sum over the row's len entries of val * X[col][c], c < kc.  The row is cut into
// kSpmmSegs equal segments; lane group sub (of G groups, its lanes' columns from c0) takes the segments sub, sub + G, .., each one chain from
// +0 -- chain(lo, hi, nc, acc) runs it over the entries [lo, hi) of the row --, and the partial sums are added left to right through part.
// Ends with the barrier after which part may be written again.  add: y[c] = y[c] + sum instead -- one plain addition to what the same thread
// of an earlier panel call (or launch of the stream) stored there (the grouped column pass: kernels/attention_backward.hpp).  S: y's storage
// type, told by y -- T itself, or a 16-bit type: the sum rounded once where it is stored (no add there).
template <typename T, typename Chain, typename S = T>
__device__ __forceinline__ void long_row_panel(int len, int kc, int G, int sub, int c0, int tid, T (*part)[SpmmShape<T>::KP], S *y, Chain chain, bool add = false)
{
#pragma clang fp contract(off)
    constexpr int V = SpmmShape<T>::V;
    const int seg = (len + kSpmmSegs - 1) / kSpmmSegs, nc = min(V, kc - c0);
    if (nc > 0)
        for (int g = sub; g < kSpmmSegs; g += G) {
            T acc[V];
#pragma unroll
            for (int t = 0; t < V; ++t) acc[t] = T(0);
            const int lo = min(len, g * seg), hi = min(len, lo + seg);
            chain(lo, hi, nc, acc);
#pragma unroll
            for (int t = 0; t < V; ++t) part[g][c0 + t] = acc[t];
        }
    __syncthreads();
    if (tid < kc) {
        T sum = part[0][tid];
        for (int g = 1; g < kSpmmSegs; ++g) sum += part[g][tid];
        if constexpr (std::is_same_v<S, T>) y[tid] = add ? y[tid] + sum : sum;
        else y[tid] = st16_narrow<S>(sum);
    }
    __syncthreads();
}

// ---- chunks of whole short rows in a wave's LDS ---------------------------------------------------------------------------------------------

// The next rows of [g0, r1), 64 at the most, none longer than kSpmmLongThr, that hold at most kSpmmChunk entries together.  Lane l describes
// row g0 + l: it starts at sl (an entry of the matrix) and has ll entries; the chunk is the rows g0 .. g0 + nr - 1 and the entries
// [base, base + nq) of the matrix; el is where the lane's row ends in the chunk, non-decreasing over the lanes (INT_MAX past the chunk).
// nr == 0: row g0 is a long row (nq and el are not set).
struct ChunkRows {
    int sl, ll, base, nr, nq, el;
};

__device__ __forceinline__ ChunkRows chunk_take(const int *__restrict__ rowptr, int g0, int r1, int lane)
{
    ChunkRows c = {0, -1, 0, 0, 0, 0x7fffffff};
    if (g0 + lane < r1) {
        c.sl = rowptr[g0 + lane];
        c.ll = rowptr[g0 + lane + 1] - c.sl;
    }
    c.base = __builtin_amdgcn_readfirstlane(c.sl); // rowptr[g0]
    const bool fits = c.ll >= 0 && c.ll <= kSpmmLongThr && c.sl + c.ll - c.base <= kSpmmChunk;
    const unsigned long long bad = ~__ballot(fits);
    c.nr = bad ? __ffsll((long long) bad) - 1 : kWave;
    if (c.nr == 0) return c;
    c.nq = __shfl(c.sl + c.ll, c.nr - 1, kWave) - c.base;
    if (lane < c.nr) c.el = c.sl + c.ll - c.base;
    return c;
}

// rows of the chunk that end at or before entry e of the chunk: the row of entry e (six shuffles over el)
__device__ __forceinline__ int chunk_row_of(int el, int e)
{
    int pos = 0;
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1)
        if (__shfl(el, pos + s - 1, kWave) <= e) pos += s;
    return pos;
}

// Y[g0 + h, :k] = sum over the entries of chunk row h of val * X[col, :], h < nr, with col / val the wave's LDS copy of the chunk: R rows
// side by side (lane group sub, its lanes' columns from c0 within a panel), every (row, column) one lane's spmm_chain from +0 over the row's
// entries in CSR order; the panels of KP columns are looped here, with the chunk still in LDS.  SX, SY: the storage types of X and Y, told by x
// and y (spmm_load_x, spmm_store_y).
template <typename T, bool VEC, typename SX = T, typename SY = T>
__device__ __forceinline__ void rows_times_panels(const ChunkRows ch, int g0, int R, int sub, int c0, const int *col, const T *val, const SX *__restrict__ x, long long ldx,
                                                  int k, SY *__restrict__ y, long long ldy)
{
    constexpr int V = SpmmShape<T>::V, KP = SpmmShape<T>::KP;
    for (int h0 = 0; h0 < ch.nr; h0 += R) {
        const int h = h0 + sub;
        const int s = __shfl(ch.sl, h & (kWave - 1), kWave) - ch.base, len = __shfl(ch.ll, h & (kWave - 1), kWave);
        if (h < ch.nr)
            for (int c = 0; c < k; c += KP) {
                const int nc = min(V, min(KP, k - c) - c0); // <= 0: a lane beyond the panel's columns
                if (nc <= 0) continue;
                T acc[V];
#pragma unroll
                for (int u = 0; u < V; ++u) acc[u] = T(0);
                spmm_chain<T, VEC, false>(s, s + len, col, val, x + c, ldx, c0, nc, acc);
                spmm_store_y<T, VEC>(y + (long long) (g0 + h) * ldy + c + c0, nc, acc);
            }
    }
}

// The entries [rowptr[g0], rowptr[g1]) of a row group, staged through the wave's LDS in chunks of up to kSpmmChunk.  The lane's row is
// [s, e) (empty for a lane without one; longrow: longer than kSpmmLongThr, another kernel's).  The chunks jump over the long rows' entries:
// rows are in lane order, so the first long row at or after p is the lowest lane of a ballot.  stage(i, p) copies entry p of the matrix into
// slot i; run(lo, hi) runs the lane's chains over the slots [lo, hi), its row's part of the chunk (every lane calls it: run itself skips
// long rows and lanes without columns).
template <typename Stage, typename Run>
__device__ __forceinline__ void staged_walk(const int *__restrict__ rowptr, int g0, int g1, int s, int e, bool longrow, int lane, Stage stage, Run run)
{
    const int hi = rowptr[g1];
    for (int p = rowptr[g0]; p < hi;) {
        const unsigned long long inside = __ballot(longrow && s <= p && e > p);
        if (inside) { p = __builtin_amdgcn_readlane(e, __ffsll((long long) inside) - 1); continue; } // p is in a long row: past it
        const unsigned long long next = __ballot(longrow && s > p);
        const int lim = next ? __builtin_amdgcn_readlane(s, __ffsll((long long) next) - 1) : hi;
        const int q = min(kSpmmChunk, lim - p);
        for (int i = lane; i < q; i += kWave) stage(i, p + i);
        wave_lds_sync();
        run(max(s, p) - p, min(e, p + q) - p);
        wave_lds_sync();
        p += q;
    }
}

} // namespace spmv
