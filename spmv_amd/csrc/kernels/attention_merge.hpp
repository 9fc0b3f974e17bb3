// attention_merge.hpp -- two partial attention results over disjoint parts of one key / value set, combined by their row log-sum-exps
// (spmv_hip_attention_merge).  O1, O2 and O are m x heads * dv, row-major with leading dimensions; L1, L2 and L are `heads` planes of m
// elements.  Per row i and head h, in the handle's precision:
//   Lm  = max(L1, L2)                                  (fmax: drops a NaN; the exp restores it)
//   w1  = exp(L1 - Lm),  w2 = exp(L2 - Lm),  W = w1 + w2
//   O_c = fma(w2, O2_c, w1 * O1_c) / W,  c < dv
//   L   = Lm + log(W)
// and Lm == -inf (both parts empty on the row): O = +0, L = -inf.  Contraction is pinned off: the fma written out is the only fused operation;
// exp and log are the device library's.  The matrix is not read.
//
// Work split: one grid-stride launch; a group of CW adjacent lanes per (row, head) -- the head the fastest index, so the groups of a workgroup walk
// O's rows contiguously --, its lanes across the dv columns, 16 / sizeof(T) columns per lane and step.  The group's first lane reads L1 and L2
// once and hands them to the others; it also stores L.  16-byte accesses when every operand allows them; the width changes no bit (every
// element is one lane's own expression).  O may be O1 and L may be L1 (a running accumulator): every element is read and then written by the
// same thread, so no pointer is __restrict__.  No LDS, no atomics.
#pragma once
#include "common.hpp"
#include "row_blocks.hpp"

namespace spmv {

// what one call's launch needs (device pointers)
struct AttentionMergeArgs {
    int m = 0, heads = 1, dv = 0, cus = 256;
    const void *o1 = nullptr, *l1 = nullptr, *o2 = nullptr, *l2 = nullptr;
    void *o = nullptr, *l = nullptr; // l: nullptr = the merged log-sum-exp is not wanted
    long long ldo1 = 0, ldl1 = 0, ldo2 = 0, ldl2 = 0, ldo = 0, ldl = 0;
    bool vec = false; // o1, o2, o, their leading dimensions and every head's first column allow 16-byte accesses
};

// spmv_attention.hip: the launch of one call on `stream`
hipError_t attention_merge_launch(const AttentionMergeArgs &a, bool f64, hipStream_t stream);

template <typename T, int CW, bool VEC>
__global__ __launch_bounds__(kBlock) void attention_merge_kernel(long long ngroups, int heads, int dv, const T *o1, long long ldo1, const T *l1, long long ldl1, const T *o2,
                                                                 long long ldo2, const T *l2, long long ldl2, T *o, long long ldo, T *l, long long ldl)
{
#pragma clang fp contract(off)
    constexpr int V = SpmmShape<T>::V, G = kBlock / CW;
    const int lane = threadIdx.x & (kWave - 1), sub = (int) threadIdx.x / CW, t = (int) threadIdx.x % CW;
    const T ninf = -__builtin_huge_val();
    const long long stride = (long long) gridDim.x * G;
    for (long long g0 = (long long) blockIdx.x * G; g0 < ngroups; g0 += stride) { // uniform over the workgroup: every lane reaches the shuffles
        const long long gi = g0 + sub;
        const bool have = gi < ngroups;
        const long long i = have ? gi / heads : 0;
        const int h = have ? (int) (gi % heads) : 0;
        T a = ninf, b = ninf;
        if (have && t == 0) {
            a = l1[h * ldl1 + i];
            b = l2[h * ldl2 + i];
        }
        if (CW > 1) {
            a = (T) __shfl(a, lane & ~(CW - 1), kWave);
            b = (T) __shfl(b, lane & ~(CW - 1), kWave);
        }
        if (!have) continue;
        const T lm = row_max(a, b);
        const bool empty = lm == ninf;
        const T w1 = row_exp(a - lm), w2 = row_exp(b - lm), W = w1 + w2;
        const T *x1 = o1 + i * ldo1 + (long long) h * dv, *x2 = o2 + i * ldo2 + (long long) h * dv;
        T *y = o + i * ldo + (long long) h * dv;
        for (int c = t * V; c < dv; c += CW * V) {
            const int nc = min(V, dv - c);
            T u[V], v[V], r[V];
            spmm_load_x<T, VEC>(x1 + c, nc, u);
            spmm_load_x<T, VEC>(x2 + c, nc, v);
#pragma unroll
            for (int q = 0; q < V; ++q) r[q] = empty ? T(0) : fmadd(w2, v[q], w1 * u[q]) / W;
            spmm_store_y<T, VEC>(y + c, nc, r);
        }
        if (l && t == 0) l[h * ldl + i] = empty ? ninf : row_lse(lm, W);
    }
}

} // namespace spmv
