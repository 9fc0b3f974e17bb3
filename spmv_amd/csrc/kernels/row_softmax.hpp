// row_softmax.hpp -- "reduce a row, then map its entries" over nnz-sized arrays in CSR order (spmv_hip_row_softmax, _backward):
//   forward   Out[p] = exp(S[p] - M_i) / Z_i      M_i = max over row i of S,  Z_i = sum over row i of exp(S[q] - M_i)
//   backward  Out[p] = P[p] * (G[p] - D_i)        D_i = sum over row i of P[q] * G[q]
// Only RowPtr is read of the matrix; ColIdx and A's values are never touched.  One kernel family, instantiated for both directions.
//
// Work split: spmm's tables (shim/spmm.hpp) -- equal-nnz batches of whole rows (kSpmmBatchNnz entries, the upper-bound splitter of
// rowblock.hpp), one wave per batch, and the list of rows longer than kSpmmLongThr, a workgroup each.
//
// Short rows (row_reduce_rows_kernel).  A wave walks its batch in passes.  In a pass CW adjacent lanes serve one row and 64 / CW consecutive
// rows go side by side; CW is the smallest power of two for which none of the next 64 / CW rows needs more lanes than that (six ballots).
// A row's entries are loaded straight into registers (the lanes of a pass read one contiguous piece of the array: HBM is read once and
// written once, nothing is staged in LDS), at most kRowChain per lane, reduced with DPP butterflies, mapped and stored from the same
// registers -- which is what makes Out == S (forward) and Out == G (backward) safe.
//
// Summation order of a row (Z_i, D_i) -- a function of the row's length and the value type alone:
//   W = 1 for len <= 1, else the smallest power of two >= len, 64 at the most;
//   virtual lane t < W chains the terms t, t + W, t + 2 W, .. < len in that order: the first term as it is (forward: exp(S - M); backward:
//   the plain product P * G), every further one added onto the chain (forward: a plain addition; backward: fma(P, G, chain)); a lane
//   without a term holds -0, the identity of IEEE addition;
//   the W chains are added as a balanced tree over neighbours: ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)), .. up to W = 64.
//   A pass whose lane groups are wider than W only adds further -0 lanes: x + (-0) = x for every x, the bits are those of width W.
// Long rows (len > kSpmmLongThr, row_reduce_long_kernel): thread t of 256 chains the terms t, t + 256, .. the same way, the 64 chains of a
// wave are added by the same tree, and the four waves' sums as (w0 + w1) + (w2 + w3) through LDS.  The row is read again through L2 for
// each phase (max, sum, map); every element is read and written by the same thread in every phase, which keeps in-place calls safe.
// The maximum is exact in any order (fmax drops a NaN; the sum then restores it: exp(NaN - M) is NaN).  The map is one subtraction, one
// exp / expf of the device math library and one division (forward), one subtraction and one multiplication (backward).
// Contraction is pinned off: the fmas written out are the only fused operations.  No atomics, no waiting between workgroups, no scratch.
#pragma once
#include "common.hpp"
#include "spmm.hpp"

namespace spmv {

constexpr int kRowChain = kSpmmLongThr / kWave; // terms per lane of the longest short row: 8

// what one call's launch needs (device pointers)
struct RowReduceArgs {
    int m = 0, nb = 0, nlong = 0, cus = 256;
    const int *split = nullptr, *longs = nullptr, *rowptr = nullptr;
    const void *a = nullptr; // S (forward) or P (backward)
    const void *g = nullptr; // G (backward only)
    void *out = nullptr;
    bool backward = false;
};

// spmv_softmax.hip: the launches of one call on `stream`
hipError_t row_reduce_launch(const RowReduceArgs &a, bool f64, hipStream_t stream);

__device__ __forceinline__ float row_exp(float x) { return expf(x); }
__device__ __forceinline__ double row_exp(double x) { return exp(x); }
__device__ __forceinline__ float row_max(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double row_max(double a, double b) { return __builtin_fmax(a, b); }

// lanes a row of len entries needs: the W of the summation order
__device__ __forceinline__ int row_width(int len) { return len <= 1 ? 1 : (len >= kWave ? kWave : 1 << (32 - __builtin_clz(len - 1))); }

// max (MAX) or sum over groups of cw consecutive lanes, cw a wave-uniform power of two; every lane of the group gets the result
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

// One wave per batch [split[b], split[b + 1]) of whole rows; rows longer than kSpmmLongThr are left to row_reduce_long_kernel.
template <typename T, bool BWD>
__global__ __launch_bounds__(kBlock) void row_reduce_rows_kernel(int nb, const int *__restrict__ split, const int *__restrict__ rowptr, const T *a, const T *g, T *out)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x * (kBlock / kWave) + (int) (threadIdx.x / kWave);
    if (b >= nb) return; // whole waves only; no workgroup barrier follows
    const int lane = threadIdx.x & (kWave - 1);
    const int r0 = split[b], r1 = split[b + 1];
    const T ninf = -__builtin_huge_val(), nzero = T(-0.0);
    for (int g0 = r0; g0 < r1;) {
        // lane l looks at row g0 + l: the pass takes the first 64 / cw of them
        int sl = 0, ll = 0;
        if (g0 + lane < r1) {
            sl = rowptr[g0 + lane];
            ll = rowptr[g0 + lane + 1] - sl;
            if (ll > kSpmmLongThr) ll = 0; // a long row: nothing of it here
        }
        const int wl = row_width(ll);
        int cw = 1, lg = 0;
        for (; cw < kWave; cw <<= 1, ++lg)
            if ((__ballot(wl > cw) & (~0ull >> (kWave - kWave / cw))) == 0) break;
        const int sub = lane >> lg, t = lane & (cw - 1);
        const int s = __shfl(sl, sub, kWave), len = __shfl(ll, sub, kWave);
        const bool wide = cw == kWave; // the only passes in which a lane holds more than one term
        T x[kRowChain], y[kRowChain];
        x[0] = t < len ? ld_stream(a + s + t) : (BWD ? nzero : ninf);
        if (BWD) y[0] = t < len ? ld_stream(g + s + t) : nzero;
        if (wide) {
#pragma unroll
            for (int j = 1; j < kRowChain; ++j) {
                const int i = t + j * kWave;
                x[j] = i < len ? ld_stream(a + s + i) : (BWD ? nzero : ninf);
                if (BWD) y[j] = i < len ? ld_stream(g + s + i) : nzero;
            }
        }
        if constexpr (!BWD) {
            T mx = x[0];
            if (wide) {
#pragma unroll
                for (int j = 1; j < kRowChain; ++j) mx = row_max(mx, x[j]);
            }
            const T M = row_group_reduce<true>(mx, cw);
            const T e0 = row_exp(x[0] - M);
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
            const T Z = row_group_reduce<false>(acc, cw);
            if (t < len) out[s + t] = x[0] / Z;
            if (wide) {
#pragma unroll
                for (int j = 1; j < kRowChain; ++j)
                    if (t + j * kWave < len) out[s + t + j * kWave] = x[j] / Z;
            }
        } else {
            T acc = t < len ? x[0] * y[0] : nzero;
            if (wide) {
#pragma unroll
                for (int j = 1; j < kRowChain; ++j) acc = t + j * kWave < len ? fmadd(x[j], y[j], acc) : acc;
            }
            const T D = row_group_reduce<false>(acc, cw);
            if (t < len) out[s + t] = x[0] * (y[0] - D);
            if (wide) {
#pragma unroll
                for (int j = 1; j < kRowChain; ++j)
                    if (t + j * kWave < len) out[s + t + j * kWave] = x[j] * (y[j] - D);
            }
        }
        g0 += kWave >> lg;
    }
}

// one workgroup per long row (len > kSpmmLongThr >= 256: every thread has a first term)
template <typename T, bool BWD>
__global__ __launch_bounds__(kBlock) void row_reduce_long_kernel(int nlong, const int *__restrict__ longs, const int *__restrict__ rowptr, const T *a, const T *g, T *out)
{
#pragma clang fp contract(off)
    __shared__ T s_max[kBlock / kWave], s_sum[kBlock / kWave];
    const int tid = (int) threadIdx.x, w = tid / kWave, lane = tid & (kWave - 1);
    for (int i = blockIdx.x; i < nlong; i += gridDim.x) {
        const int r = longs[i], s = rowptr[r], e = rowptr[r + 1];
        T M = T(0);
        if constexpr (!BWD) {
            T mx = a[s + tid];
            for (int p = s + tid + kBlock; p < e; p += kBlock) mx = row_max(mx, a[p]);
            mx = row_group_reduce<true>(mx, kWave);
            if (lane == 0) s_max[w] = mx;
            __syncthreads();
            M = row_max(row_max(s_max[0], s_max[1]), row_max(s_max[2], s_max[3]));
        }
        T acc;
        if constexpr (BWD) {
            acc = a[s + tid] * g[s + tid];
            for (int p = s + tid + kBlock; p < e; p += kBlock) acc = fmadd(a[p], g[p], acc);
        } else {
            acc = row_exp(a[s + tid] - M);
            for (int p = s + tid + kBlock; p < e; p += kBlock) acc = acc + row_exp(a[p] - M);
        }
        acc = row_group_reduce<false>(acc, kWave);
        if (lane == 0) s_sum[w] = acc;
        __syncthreads();
        const T Z = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        for (int p = s + tid; p < e; p += kBlock) {
            if constexpr (BWD) out[p] = a[p] * (g[p] - Z);
            else out[p] = row_exp(a[p] - M) / Z;
        }
        __syncthreads(); // the next row writes s_max / s_sum again
    }
}

} // namespace spmv
