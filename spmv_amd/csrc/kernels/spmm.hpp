// spmm.hpp -- Y = A X for k right-hand sides (spmv_hip_spmm): X is n x k, Y is m x k, both row-major with leading dimensions.
//
// One pass over the resident CSR (rowptr, colidx, val) per panel of up to KP columns (KP = 16 fp64 / 32 fp32: eight lanes of
// 16 bytes).  The KC columns of one X row are read by CW adjacent lanes as one contiguous segment, V = 16 / sizeof(T) columns per
// lane -- a 16-byte load where the address allows, element loads otherwise.  Column indices and values are staged through LDS with
// coalesced loads and read there by the CW lanes of their row as one broadcast, so A is fetched from HBM once per panel.
//
// Summation order (the blocks' of kernels/row_blocks.hpp): every (row, column) result is ONE lane's sequential fma chain over the row's
// entries in CSR order (spmm_chain; rows up to kSpmmLongThr entries), or, for longer rows, kSpmmSegs fixed segments of that chain added
// left to right in LDS (long_row_panel).  Neither depends on k, the panel, the lane layout, the load width, ldx / ldy or the pointers' kind:
// results are bit-identical whatever those are.
//
// Work split: equal-nnz row batches of kSpmmBatchNnz entries (the upper-bound splitter of rowblock.hpp), one wave per batch, R = 64 / CW
// rows side by side, their column indices and values staged through LDS with coalesced loads; rows longer than kSpmmLongThr are skipped
// there and multiplied by a workgroup each (spmm_long_kernel).  No atomics.
#pragma once
#include "common.hpp"
#include "row_blocks.hpp"

namespace spmv {

constexpr int kSpmmBatchNnz = 2048; // entries per wave batch (rows are whole: a batch holds up to this + one row's worth)

// what one panel's launch needs (device pointers; x, y already offset to the panel's first column)
struct SpmmArgs {
    int m = 0, nb = 0, nlong = 0, kc = 0, cus = 256;
    const int *split = nullptr, *longs = nullptr, *rowptr = nullptr, *colidx = nullptr;
    const void *val = nullptr, *x = nullptr;
    void *y = nullptr;
    long long ldx = 0, ldy = 0;
    bool vec = false; // x, y, ldx and ldy allow 16-byte accesses
};

// spmv_spmm.hip: launches both kernels of one panel on `stream`
hipError_t spmm_launch(const SpmmArgs &a, bool f64, hipStream_t stream);

// rows longer than thr, in row order of discovery (the list's order does not affect any result)
static __global__ __launch_bounds__(kBlock) void spmm_long_list_kernel(int m, int thr, const int *__restrict__ rowptr, int *__restrict__ list, int *__restrict__ count)
{
    const long long stride = (long long) gridDim.x * kBlock;
    for (long long r = (long long) blockIdx.x * kBlock + threadIdx.x; r < m; r += stride)
        if (rowptr[r + 1] - rowptr[r] > thr) list[atomicAdd(count, 1)] = (int) r;
}

// One wave per batch [split[b], split[b + 1]); CW lanes per row, R = 64 / CW consecutive rows at a time (a row group).  The group's
// entries are staged through the wave's LDS (staged_walk, which also jumps over the rows that belong to spmm_long_kernel), and every lane
// group reads its row's entries from there (the CW lanes of a row read the same slot: one broadcast).
template <typename T, int CW, bool VEC>
__global__ __launch_bounds__(kBlock) void spmm_rows_kernel(int nb, const int *__restrict__ split, const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                           const T *__restrict__ val, int kc, const T *__restrict__ x, long long ldx, T *__restrict__ y, long long ldy)
{
    constexpr int V = SpmmShape<T>::V, R = kWave / CW, CH = kSpmmChunk;
    __shared__ int s_col[kBlock / kWave][CH];
    __shared__ T s_val[kBlock / kWave][CH];
    const int w = (int) (threadIdx.x / kWave);
    const int b = blockIdx.x * (kBlock / kWave) + w;
    if (b >= nb) return; // whole waves only; no workgroup barrier follows
    const int lane = threadIdx.x & (kWave - 1), sub = lane / CW, c0 = (lane % CW) * V;
    const int nc = min(V, kc - c0); // <= 0: a lane beyond the panel's columns (it still helps staging)
    const int r0 = split[b], r1 = split[b + 1];
    for (int g0 = r0; g0 < r1; g0 += R) {
        const int g1 = min(g0 + R, r1), r = g0 + sub;
        const bool have = r < g1;
        const int s = have ? rowptr[r] : 0, e = have ? rowptr[r + 1] : 0;
        const bool longrow = e - s > kSpmmLongThr;
        T acc[V];
#pragma unroll
        for (int t = 0; t < V; ++t) acc[t] = T(0);
        staged_walk(
            rowptr, g0, g1, s, e, longrow, lane,
            [&](int i, int p) {
                s_col[w][i] = ld_stream(colidx + p);
                s_val[w][i] = ld_stream(val + p);
            },
            [&](int lo, int hi) {
                if (!longrow && nc > 0) spmm_chain<T, VEC, false>(lo, hi, s_col[w], s_val[w], x, ldx, c0, nc, acc);
            });
        if (have && !longrow && nc > 0) spmm_store_y<T, VEC>(y + (long long) r * ldy + c0, nc, acc);
    }
}

// one workgroup per long row: kSpmmSegs equal segments (lane group g takes g, g + 256 / CW, ...), partial sums added left to right in LDS
template <typename T, int CW, bool VEC>
__global__ __launch_bounds__(kBlock) void spmm_long_kernel(int nlong, const int *__restrict__ longs, const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                           const T *__restrict__ val, int kc, const T *__restrict__ x, long long ldx, T *__restrict__ y, long long ldy)
{
    constexpr int V = SpmmShape<T>::V, KP = SpmmShape<T>::KP, G = kBlock / CW;
    __shared__ T part[kSpmmSegs][KP];
    const int tid = (int) threadIdx.x, sub = tid / CW, c0 = (tid % CW) * V;
    for (int i = blockIdx.x; i < nlong; i += gridDim.x) {
        const int r = longs[i], s = rowptr[r], e = rowptr[r + 1];
        long_row_panel<T>(e - s, kc, G, sub, c0, tid, part, y + (long long) r * ldy,
                          [&](int lo, int hi, int nc, T (&acc)[V]) { spmm_chain<T, VEC, true>(s + lo, s + hi, colidx, val, x, ldx, c0, nc, acc); });
    }
}

} // namespace spmv
