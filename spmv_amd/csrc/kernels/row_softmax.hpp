// row_softmax.hpp -- "reduce a row, then map its entries" over nnz-sized arrays in CSR order (spmv_hip_row_softmax, _backward):
//   forward   Out[p] = exp(S[p] - M_i) / Z_i      M_i = max over row i of S,  Z_i = sum over row i of exp(S[q] - M_i)
//   backward  Out[p] = P[p] * (G[p] - D_i)        D_i = sum over row i of P[q] * G[q]
// Only RowPtr is read of the matrix; ColIdx and A's values are never touched.  One kernel family, instantiated for both directions.
//
// Work split: spmm's tables (shim/spmm.hpp) -- equal-nnz batches of whole rows (kSpmmBatchNnz entries, the upper-bound splitter of
// rowblock.hpp), one wave per batch, and the list of rows longer than kSpmmLongThr, a workgroup each.
//
// Short rows (row_reduce_rows_kernel).  A wave walks its batch in passes (row_pass_width: CW adjacent lanes serve one row, 64 / CW
// consecutive rows go side by side).  A row's entries are loaded straight into registers (the lanes of a pass read one contiguous piece of
// the array: HBM is read once and written once, nothing is staged in LDS), at most kRowChain per lane, reduced by row_softmax_regs /
// row_dot_regs, mapped and stored from the same registers -- which is what makes Out == S (forward) and Out == G (backward) safe.
// Long rows (len > kSpmmLongThr, row_reduce_long_kernel): long_row_softmax / long_row_dot over the row in place; the row is read again
// through L2 for each phase, every element by the same thread, which keeps in-place calls safe.
//
// Summation order of a row (Z_i, D_i) -- a function of the row's length and the value type alone: the blocks' (kernels/row_blocks.hpp).
// The map is one subtraction, one exp / expf of the device math library and one division (forward), one subtraction and one
// multiplication (backward).  Contraction is pinned off: the fmas written out are the only fused operations.  No atomics, no waiting
// between workgroups, no scratch.
#pragma once
#include "common.hpp"
#include "row_blocks.hpp"
#include "spmm.hpp"

namespace spmv {

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
        int cw, lg;
        row_pass_width(row_width(ll), cw, lg);
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
            const T Z = row_softmax_regs(x, t, len, cw, wide);
            if (t < len) out[s + t] = x[0] / Z;
            if (wide) {
#pragma unroll
                for (int j = 1; j < kRowChain; ++j)
                    if (t + j * kWave < len) out[s + t + j * kWave] = x[j] / Z;
            }
        } else {
            const T D = row_dot_regs(x, y, t, len, cw, wide);
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
    const int tid = (int) threadIdx.x;
    for (int i = blockIdx.x; i < nlong; i += gridDim.x) {
        const int r = longs[i], s = rowptr[r], e = rowptr[r + 1];
        if constexpr (BWD) {
            const T D = long_row_dot(a, g, s, e, tid, s_sum);
            for (int p = s + tid; p < e; p += kBlock) out[p] = a[p] * (g[p] - D);
            __syncthreads(); // the next row writes s_sum again
        } else long_row_softmax(a, out, s, e, tid, s_max, s_sum);
    }
}

} // namespace spmv
