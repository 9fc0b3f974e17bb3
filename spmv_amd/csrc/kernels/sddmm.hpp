// sddmm.hpp -- Out[p] = sum over c < k of U[i, c] * V[j, c] for every stored entry p = (i, j) of the resident CSR (spmv_hip_sddmm):
// the dense product U V^T sampled on A's pattern.  U is m x k, V is n x k, both row-major with leading dimensions; A's values are not read.
//
// Work split: equal ENTRY counts, kSddmmWaveNnz consecutive entries per wave, whatever the rows look like.  A wave takes its entries in
// tiles of 64: lane l owns entry p = tile + l for the pattern (one coalesced colidx load), for the row lookup and for the store of Out[p]
// (one coalesced store).  Rows are recovered from rowptr: one upper-bound search per wave for its first entry, then every lane walks
// forward from the row of the tile's first entry (doubling steps, then bisection between the last two probes: one probe while the entry is
// still in that row, two or three for rows of a few dozen entries, log2 of the distance past runs of empty rows).  The pattern is read once
// per call whatever k is.
//
// Products: the tile's 64 entries are multiplied in CW rounds of G = 64 / CW entries.  In a round the CW adjacent lanes of group g read the
// k-segments of U's row i and V's row j of entry round * G + g as contiguous runs, W = 16 / sizeof(T) columns per lane -- one 16-byte load
// where the address allows (VEC), element loads otherwise -- looping over chunks of CW * W columns when k is larger.  Consecutive entries
// share i: the groups of a round read the same U line in the same instruction, and the next round finds it in L1.
//
// Summation order of one entry -- a function of k and the value type alone:
//   CW = the smallest of 1, 2, 4, 8 with CW * W >= k (8 beyond that);
//   lane l of the group chains the columns c = l * W + t + q * CW * W < k, q = 0, 1, ... outermost, t = 0 .. W - 1 innermost: the first
//   product is a plain multiplication, every further one an fma onto the chain; a lane without any column holds -0, the identity of IEEE addition;
//   the lanes' chains are added as ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7)) (CW = 8; the left half of it for CW = 4, l0 + l1 for 2).
// k = 1 is therefore the single correctly rounded product U[i] * V[j].  Lanes past k neither read nor write.  No atomics, no waiting
// between workgroups, no scratch.
#pragma once
#include "common.hpp"
#include "storage16.hpp"

namespace spmv {

constexpr int kSddmmWaveNnz = 2048; // entries per wave: 32 tiles of 64
constexpr int kSddmmLanes = 8;      // widest lane group

template <typename T> struct SddmmShape {
    static constexpr int W = 16 / (int) sizeof(T); // columns per lane and chunk
    static constexpr int KC = kSddmmLanes * W;     // columns per chunk at full group width: 16 fp64 / 32 fp32
};

// what one call's launch needs (device pointers)
struct SddmmArgs {
    int m = 0, k = 0;
    long long nnz = 0;
    const int *rowptr = nullptr, *colidx = nullptr;
    const void *u = nullptr, *v = nullptr;
    void *out = nullptr;
    long long ldu = 0, ldv = 0;
    bool vec = false; // u, v, ldu and ldv allow 16-byte loads
};

// spmv_sddmm.hip: the one launch of a call on `stream`
hipError_t sddmm_launch(const SddmmArgs &a, bool f64, hipStream_t stream);

// nc (1 .. W) columns from p; a 16-byte load when allowed and the segment is whole.  S: what the operand is in memory (kernels/storage16.hpp) --
// T itself, or a 16-bit type widened here: the same W columns per lane, so the segment is 8 bytes and the wide form one 8-byte load
template <typename T, bool VEC, typename S = T>
__device__ __forceinline__ void sddmm_load(const S *p, int nc, T (&o)[SddmmShape<T>::W])
{
    constexpr int W = SddmmShape<T>::W;
    if constexpr (!std::is_same_v<S, T>) {
        static_assert(std::is_same_v<T, float> && is_storage16<S>, "16-bit storage is for float arithmetic");
        if (VEC && nc == W) st16_load4(p, o);
        else {
#pragma unroll
            for (int t = 0; t < W; ++t) o[t] = t < nc ? st16_widen(p[t]) : T(0);
        }
    } else if (VEC && nc == W) {
        if constexpr (sizeof(T) == 8) {
            const f64x2 v = *reinterpret_cast<const f64x2 *>(p);
            o[0] = v.x; o[1] = v.y;
        } else {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
    } else {
#pragma unroll
        for (int t = 0; t < W; ++t) o[t] = t < nc ? p[t] : T(0);
    }
}

// one lane's chain over its columns c0, c0 + 1, .., then c0 + step, .. (c0 < k); S, S2: the storage types of u and of v (sddmm_load), told by the
// pointers -- they differ where a 16-bit row meets a float one (the backward's <G row, O row>)
template <typename T, bool VEC, typename S = T, typename S2 = S>
__device__ __forceinline__ T sddmm_chain(const S *__restrict__ u, const S2 *__restrict__ v, int c0, int step, int k)
{
#pragma clang fp contract(off) // the explicit fmas below are the only fused operations
    constexpr int W = SddmmShape<T>::W;
    T a[W], b[W];
    int nc = min(W, k - c0);
    sddmm_load<T, VEC>(u + c0, nc, a);
    sddmm_load<T, VEC>(v + c0, nc, b);
    T acc = a[0] * b[0];
#pragma unroll
    for (int t = 1; t < W; ++t) acc = t < nc ? fmadd(a[t], b[t], acc) : acc;
    for (int c = c0 + step; c < k; c += step) {
        nc = min(W, k - c);
        sddmm_load<T, VEC>(u + c, nc, a);
        sddmm_load<T, VEC>(v + c, nc, b);
#pragma unroll
        for (int t = 0; t < W; ++t) acc = t < nc ? fmadd(a[t], b[t], acc) : acc;
    }
    return acc;
}

template <typename T, int CW, bool VEC>
__global__ __launch_bounds__(kBlock) void sddmm_kernel(int m, long long nnz, const int *__restrict__ rowptr, const int *__restrict__ colidx, int k,
                                                       const T *__restrict__ u, long long ldu, const T *__restrict__ v, long long ldv, T *__restrict__ out)
{
    constexpr int W = SddmmShape<T>::W, G = kWave / CW;
    __shared__ T s_out[kBlock / kWave][kWave];
    const int w = (int) (threadIdx.x / kWave), lane = threadIdx.x & (kWave - 1);
    const long long p0 = ((long long) blockIdx.x * (kBlock / kWave) + w) * kSddmmWaveNnz;
    if (p0 >= nnz) return; // whole waves only; no workgroup barrier follows
    const long long p1 = min(p0 + kSddmmWaveNnz, nnz);
    const int sub = lane / CW, c0 = (lane % CW) * W;
    int rf = upper_bound_dev(rowptr, m + 1, p0) - 1; // the row of entry p0 (p0 < nnz = rowptr[m]: 0 <= rf < m)
    for (long long base = p0; base < p1; base += kWave) {
        const long long p = base + lane;
        const bool valid = p < p1;
        int i = -1, j = 0;
        if (valid) {
            j = ld_stream(colidx + p);
            i = rf;
            if ((long long) rowptr[i + 1] <= p) { // further on: rowptr[lo + 1] <= p < rowptr[hi + 1], hi <= m - 1
                int lo = i, hi, step = 1;
                for (;;) {
                    hi = (int) min((long long) lo + step, (long long) m - 1);
                    if ((long long) rowptr[hi + 1] > p) break;
                    lo = hi;
                    step <<= 1;
                }
                while (hi - lo > 1) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if ((long long) rowptr[mid + 1] > p) hi = mid; else lo = mid;
                }
                i = hi;
            }
        }
#pragma unroll 2
        for (int round = 0; round < CW; ++round) {
            const int e = round * G + sub;
            const int ie = __shfl(i, e, kWave), je = __shfl(j, e, kWave);
            T acc = T(-0.0); // x + (-0) = x for every x, signed zeros included
            if (ie >= 0 && c0 < k) acc = sddmm_chain<T, VEC>(u + (long long) ie * ldu, v + (long long) je * ldv, c0, CW * W, k);
            acc = group_sum_dpp<CW>(acc);
            if (ie >= 0 && lane % CW == 0) s_out[w][e] = acc;
        }
        wave_lds_sync();
        if (valid) out[p] = s_out[w][lane];
        wave_lds_sync();
        rf = __shfl(i, kWave - 1, kWave); // the last entry's row: where the next tile starts looking (not used after a partial tile)
    }
}

} // namespace spmv
