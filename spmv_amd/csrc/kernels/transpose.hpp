// transpose.hpp -- A^T of the resident CSR, built on the device (spmv_hip_spmv_transpose).
//
// perm[p] = the CSR index in A of the entry at position p of A^T's CSR: the entry indices 0 .. nnz-1 sorted STABLY by column, so that
// row j of A^T lists its entries in ascending row of A (CSR order is row order).  The transpose is therefore a function of the matrix alone.
//
// Sort: least-significant-digit radix sort of (column, entry index) pairs, kTrBits bits per pass, ceil(log2 n / kTrBits) passes.  Each pass:
//   tr_hist_kernel     per tile of kTrTile consecutive pairs, the count of every digit (LDS atomics: counts do not depend on order),
//                      stored digit-major: cnt[digit * tiles + tile];
//   (scan)             the exclusive prefix of cnt in that order (the three-pass int32 scan of csr5.hpp / split.hpp) = where every
//                      (digit, tile) run starts in the output;
//   tr_scatter_kernel  stable placement: wave w of a tile holds kTrItems x 64 consecutive pairs, steps through them in order and ranks each
//                      pair among the earlier pairs of its digit with ballots over the digit's bits; the waves' per-digit counts are
//                      combined in wave order.  No global atomics: every position is a function of the input.
// rowptr_T[c] = lower_bound(sorted columns, c); colidx_T[p] = row of A of entry perm[p] (row_of: one wave per row writes its number);
// val_T[p] = val[perm[p]] (tr_gather_kernel, also the values refresh).
#pragma once
#include "common.hpp"

namespace spmv {

constexpr int kTrBits = 8;
constexpr int kTrDigits = 1 << kTrBits;
constexpr int kTrItems = 16;                 // pairs per lane and tile
constexpr int kTrTile = kBlock * kTrItems;   // 4096 pairs per workgroup
static_assert(kTrDigits == kBlock, "one thread per digit in the per-tile tables");

// row_of[q] = r for every entry q of row r; one wave per row
static __global__ __launch_bounds__(kBlock) void tr_rows_kernel(int m, const int *__restrict__ rowptr, int *__restrict__ row_of)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long wave = ((long long) blockIdx.x * kBlock + threadIdx.x) / kWave, waves = (long long) gridDim.x * (kBlock / kWave);
    for (long long r = wave; r < m; r += waves)
        for (int q = rowptr[r] + lane; q < rowptr[r + 1]; q += kWave) row_of[q] = (int) r;
}

// digit counts of one tile of keys, digit-major
static __global__ __launch_bounds__(kBlock) void tr_hist_kernel(long long nnz, int tiles, int shift, const int *__restrict__ keys, int *__restrict__ cnt)
{
    __shared__ int h[kTrDigits];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long) blockIdx.x * kTrTile;
#pragma unroll 4
    for (int j = 0; j < kTrItems; ++j) {
        const long long i = base + (long long) j * kBlock + threadIdx.x;
        if (i < nnz) atomicAdd(&h[(ld_stream(keys + i) >> shift) & (kTrDigits - 1)], 1);
    }
    __syncthreads();
    cnt[(long long) threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter of one tile.  off: the exclusive digit-major prefix of tr_hist_kernel's counts.  vals == NULL: the pair's value is its
// position (the first pass: entry indices).
static __global__ __launch_bounds__(kBlock) void tr_scatter_kernel(long long nnz, int tiles, int shift, const int *__restrict__ keys, const int *__restrict__ vals,
                                                                  const int *__restrict__ off, int *__restrict__ keys_out, int *__restrict__ vals_out)
{
    __shared__ int wcnt[kBlock / kWave][kTrDigits]; // per wave: pairs of each digit seen so far, then the wave's first output position per digit
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    for (int i = threadIdx.x; i < (kBlock / kWave) * kTrDigits; i += kBlock) (&wcnt[0][0])[i] = 0;
    __syncthreads();
    const long long base = (long long) blockIdx.x * kTrTile + (long long) w * (kTrItems * kWave);
    const unsigned long long below = (1ull << lane) - 1ull;
    int key[kTrItems], val[kTrItems], rank[kTrItems];
#pragma unroll
    for (int j = 0; j < kTrItems; ++j) {
        const long long i = base + (long long) j * kWave + lane;
        const bool valid = i < nnz;
        key[j] = valid ? ld_stream(keys + i) : 0;
        val[j] = valid ? (vals ? ld_stream(vals + i) : (int) i) : 0;
        const int d = (key[j] >> shift) & (kTrDigits - 1);
        unsigned long long peers = __ballot(valid); // the valid lanes whose digit equals this lane's
#pragma unroll
        for (int b = 0; b < kTrBits; ++b) {
            const unsigned long long set = __ballot((d >> b) & 1);
            peers &= ((d >> b) & 1) ? set : ~set;
        }
        const int before = wcnt[w][d]; // read by every lane of the step before the digit's last lane adds the step's count
        rank[j] = before + __popcll(peers & below);
        if (valid && lane == 63 - __clzll(peers)) wcnt[w][d] = before + __popcll(peers);
    }
    __syncthreads();
    { // thread t = digit t: the waves' runs of that digit follow each other in wave order from the tile's offset
        int run = off[(long long) threadIdx.x * tiles + blockIdx.x];
#pragma unroll
        for (int v = 0; v < kBlock / kWave; ++v) { const int c = wcnt[v][threadIdx.x]; wcnt[v][threadIdx.x] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTrItems; ++j) {
        const long long i = base + (long long) j * kWave + lane;
        if (i < nnz) {
            const int pos = wcnt[w][(key[j] >> shift) & (kTrDigits - 1)] + rank[j];
            keys_out[pos] = key[j];
            vals_out[pos] = val[j];
        }
    }
}

// rowptr_T[c] = first position of column c in the sorted columns (lower bound), c = 0 .. n
static __global__ __launch_bounds__(kBlock) void tr_rowptr_kernel(int n, long long nnz, const int *__restrict__ sorted, int *__restrict__ rowptr_t)
{
    const long long stride = (long long) gridDim.x * kBlock;
    for (long long c = (long long) blockIdx.x * kBlock + threadIdx.x; c <= n; c += stride) {
        long long lo = 0, hi = nnz;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (sorted[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        rowptr_t[c] = (int) lo;
    }
}

// colidx_T[p] = row of A holding entry perm[p]
static __global__ __launch_bounds__(kBlock) void tr_columns_kernel(long long nnz, const int *__restrict__ perm, const int *__restrict__ row_of, int *__restrict__ colidx_t)
{
    const long long stride = (long long) gridDim.x * kBlock;
    for (long long p = (long long) blockIdx.x * kBlock + threadIdx.x; p < nnz; p += stride) colidx_t[p] = row_of[ld_stream(perm + p)];
}

// val_T[p] = val[perm[p]]
template <typename T>
__global__ __launch_bounds__(kBlock) void tr_gather_kernel(long long nnz, const int *__restrict__ perm, const T *__restrict__ val, T *__restrict__ val_t)
{
    const long long stride = (long long) gridDim.x * kBlock;
    for (long long p = (long long) blockIdx.x * kBlock + threadIdx.x; p < nnz; p += stride) val_t[p] = val[ld_stream(perm + p)];
}

// launches (spmv_transpose.hip); each returns hipGetLastError() of its launches
hipError_t tr_rows_launch(int m, const int *rowptr, int *row_of, int cus, hipStream_t stream);
hipError_t tr_hist_launch(long long nnz, int tiles, int shift, const int *keys, int *cnt, hipStream_t stream);
hipError_t tr_scatter_launch(long long nnz, int tiles, int shift, const int *keys, const int *vals, const int *off, int *keys_out, int *vals_out, hipStream_t stream);
hipError_t tr_rowptr_launch(int n, long long nnz, const int *sorted, int *rowptr_t, int cus, hipStream_t stream);
hipError_t tr_columns_launch(long long nnz, const int *perm, const int *row_of, int *colidx_t, int cus, hipStream_t stream);
hipError_t tr_gather_launch(long long nnz, const int *perm, const void *val, void *val_t, bool f64, int cus, hipStream_t stream);

} // namespace spmv
