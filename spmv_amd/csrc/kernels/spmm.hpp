// spmm.hpp -- Y = A X for k right-hand sides (spmv_hip_spmm): X is n x k, Y is m x k, both row-major with leading dimensions.
//
// One pass over the resident CSR (rowptr, colidx, val) per panel of up to KP columns (KP = 16 fp64 / 32 fp32: eight lanes of
// 16 bytes).  The KC columns of one X row are read by CW adjacent lanes as one contiguous segment, V = 16 / sizeof(T) columns per
// lane -- a 16-byte load where the address allows, element loads otherwise.  Column indices and values are staged through LDS with
// coalesced loads and read there by the CW lanes of their row as one broadcast, so A is fetched from HBM once per panel.
//
// Summation order: every (row, column) result is ONE lane's sequential fma chain over the row's entries in CSR order (rows up to
// kSpmmLongThr entries), or, for longer rows, kSpmmSegs fixed segments of that chain added left to right in LDS.  Neither depends on
// k, the panel, the lane layout, the load width, ldx / ldy or the pointers' kind: results are bit-identical whatever those are.
//
// Work split: equal-nnz row batches of kSpmmBatchNnz entries (the upper-bound splitter of rowblock.hpp), one wave per batch, R = 64 / CW
// rows side by side, their column indices and values staged through LDS with coalesced loads; rows longer than kSpmmLongThr are skipped
// there and multiplied by a workgroup each (spmm_long_kernel).  No atomics.
#pragma once
#include "common.hpp"

namespace spmv {

constexpr int kSpmmBatchNnz = 2048; // entries per wave batch (rows are whole: a batch holds up to this + one row's worth)
constexpr int kSpmmLongThr = 512;   // longer rows: a workgroup each
constexpr int kSpmmSegs = 64;       // ... cut into this many equal segments, combined in a fixed order
constexpr int kSpmmLanes = 8;       // lanes per X row segment at full panel width
constexpr int kSpmmChunk = 512;     // entries of a row group staged through a wave's LDS at a time

template <typename T> struct SpmmShape {
    static constexpr int V = 16 / (int) sizeof(T);  // columns per lane
    static constexpr int KP = kSpmmLanes * V;       // panel width
};

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

// X row segment of one lane: nc (<= V) columns from p; a 16-byte load when allowed and the segment is whole
template <typename T, bool VEC>
__device__ __forceinline__ void spmm_load_x(const T *p, int nc, T (&o)[SpmmShape<T>::V])
{
    constexpr int V = SpmmShape<T>::V;
    if (VEC && nc == V) {
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

template <typename T, bool VEC>
__device__ __forceinline__ void spmm_store_y(T *p, int nc, const T (&a)[SpmmShape<T>::V])
{
    constexpr int V = SpmmShape<T>::V;
    if (VEC && nc == V) {
        if constexpr (sizeof(T) == 8) *reinterpret_cast<f64x2 *>(p) = f64x2{a[0], a[1]};
        else *reinterpret_cast<f32x4 *>(p) = f32x4{a[0], a[1], a[2], a[3]};
    } else {
#pragma unroll
        for (int t = 0; t < V; ++t)
            if (t < nc) p[t] = a[t];
    }
}

// acc[t] += sum over entries [s, e) of val * X[col][c0 + t], strictly in entry order.  NT: colidx / val are the global streams; else the
// wave's LDS copy of a chunk (same values, same order: the two sources give identical bits)
template <typename T, bool VEC, bool NT>
__device__ __forceinline__ void spmm_chain(int s, int e, const int *__restrict__ colidx, const T *__restrict__ val, const T *__restrict__ x, long long ldx,
                                           int c0, int nc, T (&acc)[SpmmShape<T>::V])
{
    constexpr int V = SpmmShape<T>::V, U = 4;
    int j = s;
    for (; j + U <= e; j += U) {
        int c[U];
        T v[U], xv[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            c[u] = NT ? ld_stream(colidx + j + u) : colidx[j + u];
            v[u] = NT ? ld_stream(val + j + u) : val[j + u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) spmm_load_x<T, VEC>(x + (long long) c[u] * ldx + c0, nc, xv[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < V; ++t) acc[t] = fmadd(v[u], xv[u][t], acc[t]);
    }
    for (; j < e; ++j) {
        const int c = NT ? ld_stream(colidx + j) : colidx[j];
        const T v = NT ? ld_stream(val + j) : val[j];
        T xv[V];
        spmm_load_x<T, VEC>(x + (long long) c * ldx + c0, nc, xv);
#pragma unroll
        for (int t = 0; t < V; ++t) acc[t] = fmadd(v, xv[t], acc[t]);
    }
}

// One wave per batch [split[b], split[b + 1]); CW lanes per row, R = 64 / CW consecutive rows at a time (a row group).  The group's
// entries are staged through the wave's LDS in chunks of up to kSpmmChunk with coalesced loads, and every lane group reads its row's
// entries from there (the CW lanes of a row read the same slot: one broadcast).  Rows longer than kSpmmLongThr belong to spmm_long_kernel:
// the chunks jump over their entries (rows are in lane order, so the first long row at or after p is the lowest lane of a ballot).
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
        const int hi = rowptr[g1];
        for (int p = rowptr[g0]; p < hi;) {
            const unsigned long long inside = __ballot(longrow && s <= p && e > p);
            if (inside) { p = __builtin_amdgcn_readlane(e, __ffsll((long long) inside) - 1); continue; } // p is in a long row: past it
            const unsigned long long next = __ballot(longrow && s > p);
            const int lim = next ? __builtin_amdgcn_readlane(s, __ffsll((long long) next) - 1) : hi;
            const int q = min(CH, lim - p);
            for (int i = lane; i < q; i += kWave) {
                s_col[w][i] = ld_stream(colidx + p + i);
                s_val[w][i] = ld_stream(val + p + i);
            }
            wave_lds_sync();
            if (!longrow && nc > 0) spmm_chain<T, VEC, false>(max(s, p) - p, min(e, p + q) - p, s_col[w], s_val[w], x, ldx, c0, nc, acc);
            wave_lds_sync();
            p += q;
        }
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
    const int sub = (int) threadIdx.x / CW, c0 = ((int) threadIdx.x % CW) * V;
    const int nc = min(V, kc - c0);
    for (int i = blockIdx.x; i < nlong; i += gridDim.x) {
        const int r = longs[i], s = rowptr[r], e = rowptr[r + 1];
        const int seg = (e - s + kSpmmSegs - 1) / kSpmmSegs;
        if (nc > 0)
            for (int g = sub; g < kSpmmSegs; g += G) {
                T acc[V];
#pragma unroll
                for (int t = 0; t < V; ++t) acc[t] = T(0);
                const int a = min(e, s + g * seg), z = min(e, a + seg);
                spmm_chain<T, VEC, true>(a, z, colidx, val, x, ldx, c0, nc, acc);
#pragma unroll
                for (int t = 0; t < V; ++t) part[g][c0 + t] = acc[t];
            }
        __syncthreads();
        if ((int) threadIdx.x < kc) {
            T sum = part[0][threadIdx.x];
            for (int g = 1; g < kSpmmSegs; ++g) sum += part[g][threadIdx.x];
            y[(long long) r * ldy + threadIdx.x] = sum;
        }
        __syncthreads();
    }
}

} // namespace spmv
