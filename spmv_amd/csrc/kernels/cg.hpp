// cg.hpp -- the vector kernels of spmv_hip_cg (preconditioned conjugate gradients that stay on the device): cg_init, cg_begin, cg_dot,
// cg_update and cg_direction.  One iteration is the handle's own multiply q = A p followed by
//
//   cg_dot        reads p, q                  leaves the partials of <p,q>
//   cg_update     reads p, q, x, r, (Dinv)    x += alpha p, r -= alpha q; leaves the partials of <r,z> and <r,r>, z = Dinv .* r
//   cg_direction  reads r, (Dinv), p          p = z + beta p (z recomputed, never stored); block 0 writes the state
//
// Hand-off between workgroups is the kernel boundary and nothing else: a kernel writes ONE fp64 partial per workgroup (at most kCgMaxParts),
// and every workgroup of the next kernel adds those partials again itself, in the fixed order below, and derives alpha / beta / the stop test
// from the sums -- redundantly, with the same bits everywhere.  No atomics, no in-launch flags or counters, no fences, no spinning, no
// cooperative launch; alpha and beta never visit the host, and finishing a dot costs no launch.
//
// The state (CgState) is written by block 0 of cg_begin / cg_update / cg_direction and read by the kernels that FOLLOW: no kernel reads a
// word that its own launch writes, so every wave of every workgroup of a launch sees the same state and takes the same early return.  That
// is why the end of the loop is two words.  `end_direction` is written by cg_begin and cg_direction and read by cg_dot and cg_update;
// `end_update` is written by cg_update and read by cg_direction.  A kernel that finds the word it reads set passes the end on in the word it
// writes (block 0) and returns, so from the launch that ends the loop on every later kernel of the batch returns at once.  status,
// iterations and rr are only written by the kernels; bb is written by cg_begin alone and read by cg_direction.
//
// Order of a dot over m elements (include/spmv_hip.h "the arithmetic contract"; tests/cg_cases.py restates it in numpy):
//   P = min(1024, ceil(m / 1024)) workgroups, L = 1024 ceil(m / (1024 P)); workgroup j owns [j L, min(m, (j + 1) L)).  The element at offset
//   o of its workgroup goes to thread (o / 4) % 256, slot o % 4, step o / 1024; each (thread, slot) accumulator starts at +0.0 and adds its
//   fp64 products by ascending step (an absent element adds +0.0: an accumulator is never -0.0, so leaving it out is the same bits).  Thread:
//   (a0 + a1) + (a2 + a3).  Wave: the adjacent-pair binary tree over 64 lanes (group_sum_dpp: an xor butterfly, the same sums since addition
//   commutes).  Workgroup: (w0 + w1) + (w2 + w3).  Final sum: the P partials padded with +0.0 to 1024, thread t takes 4t .. 4t + 3 as
//   (a + b) + (c + d), then the same wave and workgroup trees.
// Every product and every sum is a separate operation: contraction is off in every function of this file, AND spmv_cg.hip is compiled with
// -ffp-contract=off (build.py, HIP_SOURCE_FLAGS): under the library's -ffp-contract=fast the back end fuses a multiply and an add whatever the
// pragma says.  The only fused operations left in the ISA are the five of each kernel's one fp64 division.
#pragma once
#include "common.hpp"

namespace spmv {

constexpr int kCgChunk = 4 * kBlock; // elements a workgroup takes per step: 4 per thread
constexpr int kCgMaxParts = 1024;    // most workgroups of a vector kernel = most partials of a dot

// device copy of what spmv_hip_cg reports (status: the SPMV_HIP_CG_* values)
struct CgState {
    int end_update;    // written by cg_update, read by cg_direction
    int end_direction; // written by cg_begin and cg_direction, read by cg_dot and cg_update; the host reads both
    int status, iterations;
    double rr, bb;
};

// the partial arrays, kCgMaxParts doubles each; entries behind the P in use stay +0.0 from the allocation on.  <r,z> has two: iteration k
// reads the old sum from (k - 1) & 1 while it writes the new one to k & 1
enum { kCgPartPQ, kCgPartRZ0, kCgPartRZ1, kCgPartRR, kCgPartBB, kCgPartArrays };

// what one solve's launches need (device pointers)
struct CgArgs {
    int m = 0, parts = 0;
    long long span = 0;            // L
    void *r = nullptr, *p = nullptr, *q = nullptr, *x = nullptr;
    const void *b = nullptr, *dinv = nullptr;
    double *part = nullptr;        // kCgPartArrays arrays
    CgState *state = nullptr;
    double *hist = nullptr;        // NULL: not wanted
    double rtol2 = 0, atol2 = 0;   // rtol^2, atol^2
    int nostop = 0;                // the timer: no test ever ends the loop
    bool wide = false;             // b, x and dinv allow 16-byte accesses (r, p, q always do)
    bool f64 = true;
};

// spmv_cg.hip
hipError_t cg_start_launch(const CgArgs &a, bool use_x0, hipStream_t stream);    // cg_init + cg_begin; q holds A x0 when use_x0
hipError_t cg_iteration_launch(const CgArgs &a, int k, hipStream_t stream);      // cg_dot + cg_update + cg_direction of iteration k >= 1; q holds A p

__device__ __forceinline__ bool cg_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); } // false for NaN too

// 4 consecutive elements from `o` (a multiple of 4 inside the workgroup's range), absent ones (>= end) as 0
template <typename T, bool WIDE>
__device__ __forceinline__ void cg_load4(const T *__restrict__ a, long long o, long long end, T (&v)[4])
{
    if (WIDE && o + 4 <= end) {
        if constexpr (sizeof(T) == 4) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(a + o);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            const f64x2 t = *reinterpret_cast<const f64x2 *>(a + o), u = *reinterpret_cast<const f64x2 *>(a + o + 2);
            v[0] = t.x; v[1] = t.y; v[2] = u.x; v[3] = u.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = o + k < end ? a[o + k] : T(0);
    }
}

template <typename T, bool WIDE>
__device__ __forceinline__ void cg_store4(T *__restrict__ a, long long o, long long end, const T (&v)[4])
{
    if (WIDE && o + 4 <= end) {
        if constexpr (sizeof(T) == 4) {
            f32x4 t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
            *reinterpret_cast<f32x4 *>(a + o) = t;
        } else {
            f64x2 t, u; t.x = v[0]; t.y = v[1]; u.x = v[2]; u.y = v[3];
            *reinterpret_cast<f64x2 *>(a + o) = t;
            *reinterpret_cast<f64x2 *>(a + o + 2) = u;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (o + k < end) a[o + k] = v[k];
    }
}

// N sums at once over the workgroup: the wave tree, then (w0 + w1) + (w2 + w3); every thread returns with the totals.  `s` is LDS of this
// call's own (N x 4 doubles): two calls of one kernel use two arrays, so no barrier is needed between them.
template <int N>
__device__ __forceinline__ void cg_block_tree(double (&v)[N], double (*s)[kBlock / kWave])
{
#pragma clang fp contract(off)
    static_assert(kBlock / kWave == 4, "the workgroup tree is written for four waves");
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        v[n] = group_sum_dpp<kWave>(v[n]);
        if (lane == 0) s[n][wave] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = (s[n][0] + s[n][1]) + (s[n][2] + s[n][3]);
}

// the final sums of N partial arrays (ids[n] of `part`), in every thread of every workgroup
template <int N>
__device__ __forceinline__ void cg_final_sums(const double *__restrict__ part, const int (&ids)[N], double (&v)[N], double (*s)[kBlock / kWave])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const f64x2 *src = reinterpret_cast<const f64x2 *>(part + (size_t) ids[n] * kCgMaxParts + 4 * threadIdx.x);
        const f64x2 ab = src[0], cd = src[1]; // entries behind P are +0.0
        v[n] = (ab.x + ab.y) + (cd.x + cd.y);
    }
    cg_block_tree<N>(v, s);
}

// a thread's four accumulators -> its sum
__device__ __forceinline__ double cg_thread_sum(const double (&a)[4])
{
#pragma clang fp contract(off)
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// r = b (x = 0 is written) or r = b - q with q = A x0; p = z = Dinv .* r; the partials of <r,z>, <r,r> and <b,b>
template <typename T, bool WIDE, bool DINV, bool X0>
__global__ __launch_bounds__(kBlock) void cg_init_kernel(int m, long long span, const T *__restrict__ b, T *x, const T *__restrict__ q,
                                                         const T *__restrict__ dinv, T *__restrict__ r, T *__restrict__ p, double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double s_own[3][kBlock / kWave];
    const long long begin = (long long) blockIdx.x * span, end = begin + span < m ? begin + span : (long long) m;
    double rz[4] = {0, 0, 0, 0}, rr[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vb[4], vr[4], vz[4];
        cg_load4<T, WIDE>(b, o, end, vb);
        if (X0) {
            T vq[4];
            cg_load4<T, true>(q, o, end, vq);
#pragma unroll
            for (int k = 0; k < 4; ++k) vr[k] = vb[k] - vq[k];
        } else {
            const T zero[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
            for (int k = 0; k < 4; ++k) vr[k] = vb[k];
            cg_store4<T, WIDE>(x, o, end, zero);
        }
        if (DINV) {
            T vd[4];
            cg_load4<T, WIDE>(dinv, o, end, vd);
#pragma unroll
            for (int k = 0; k < 4; ++k) vz[k] = vd[k] * vr[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) vz[k] = vr[k];
        }
        cg_store4<T, true>(r, o, end, vr);
        cg_store4<T, true>(p, o, end, vz);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rz[k] += (double) vr[k] * (double) vz[k];
            rr[k] += (double) vr[k] * (double) vr[k];
            bb[k] += (double) vb[k] * (double) vb[k];
        }
    }
    double own[3] = {cg_thread_sum(rz), cg_thread_sum(rr), cg_thread_sum(bb)};
    cg_block_tree<3>(own, s_own);
    if (threadIdx.x == 0) {
        part[(size_t) kCgPartRZ0 * kCgMaxParts + blockIdx.x] = own[0];
        part[(size_t) kCgPartRR * kCgMaxParts + blockIdx.x] = own[1];
        part[(size_t) kCgPartBB * kCgMaxParts + blockIdx.x] = own[2];
    }
}

// one workgroup: the state of iteration 0 (the host has zeroed it)
template <bool HIST>
__global__ __launch_bounds__(kBlock) void cg_begin_kernel(const double *__restrict__ part, CgState *st, double *__restrict__ hist, double rtol2, double atol2, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[3][kBlock / kWave];
    const int ids[3] = {kCgPartRZ0, kCgPartRR, kCgPartBB};
    double v[3];
    cg_final_sums<3>(part, ids, v, s_fin);
    if (threadIdx.x != 0) return;
    double rr = v[1];
    const double rz = v[0], bb = v[2];
    int status = -1;
    if (!nostop) {
        if (!cg_finite(bb) || !cg_finite(rr) || !cg_finite(rz)) status = 3;
        else if (bb == 0) { status = 0; rr = 0; } // the solution is x = 0: the host zeroes X
        else if (rr <= __builtin_fmax(rtol2 * bb, atol2)) status = 0;
        else if (rz <= 0) status = 2;
    }
    st->iterations = 0;
    st->rr = rr;
    st->bb = bb;
    if (HIST) hist[0] = rr;
    if (status >= 0) { st->status = status; st->end_direction = 1; }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void cg_dot_kernel(int m, long long span, const T *__restrict__ p, const T *__restrict__ q, double *__restrict__ part, const CgState *st)
{
#pragma clang fp contract(off)
    __shared__ double s_own[1][kBlock / kWave];
    if (st->end_direction) return; // cg_direction of the iteration before passed on an end that cg_update found
    const long long begin = (long long) blockIdx.x * span, end = begin + span < m ? begin + span : (long long) m;
    double pq[4] = {0, 0, 0, 0};
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vp[4], vq[4];
        cg_load4<T, true>(p, o, end, vp);
        cg_load4<T, true>(q, o, end, vq);
#pragma unroll
        for (int k = 0; k < 4; ++k) pq[k] += (double) vp[k] * (double) vq[k];
    }
    double own[1] = {cg_thread_sum(pq)};
    cg_block_tree<1>(own, s_own);
    if (threadIdx.x == 0) part[(size_t) kCgPartPQ * kCgMaxParts + blockIdx.x] = own[0];
}

// iteration k: alpha = <r,z>_old / <p,q> rounded to T once; x = x + alpha p, r = r - alpha q in T (a multiply, then an add); the partials of the
// new <r,z> and <r,r>.  <p,q> <= 0 (breakdown) or a non-finite scalar: block 0 records it and NO workgroup applies the update.
template <typename T, bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void cg_update_kernel(int m, long long span, int k, const T *__restrict__ p, const T *__restrict__ q, T *__restrict__ x, T *__restrict__ r,
                                                           const T *__restrict__ dinv, double *__restrict__ part, CgState *st, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[2][kBlock / kWave], s_own[2][kBlock / kWave];
    if (st->end_direction) { // an earlier launch's word: the same in every wave
        if (blockIdx.x == 0 && threadIdx.x == 0) st->end_update = 1;
        return;
    }
    const int rz_old = (k - 1) & 1 ? kCgPartRZ1 : kCgPartRZ0, rz_new = k & 1 ? kCgPartRZ1 : kCgPartRZ0;
    const int ids[2] = {rz_old, kCgPartPQ};
    double v[2];
    cg_final_sums<2>(part, ids, v, s_fin);
    const double alpha64 = v[0] / v[1];
    const T alpha = (T) alpha64;
    if (!nostop) {
        int status = -1;
        if (!cg_finite(v[1]) || !cg_finite(v[0])) status = 3;
        else if (v[1] <= 0) status = 2;
        else if (!cg_finite((double) alpha)) status = 3;
        if (status >= 0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { st->status = status; st->end_update = 1; }
            return;
        }
    }
    const long long begin = (long long) blockIdx.x * span, end = begin + span < m ? begin + span : (long long) m;
    double rz[4] = {0, 0, 0, 0}, rr[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vp[4], vq[4], vx[4], vr[4], vz[4];
        cg_load4<T, true>(p, o, end, vp);
        cg_load4<T, true>(q, o, end, vq);
        cg_load4<T, WIDE>(x, o, end, vx);
        cg_load4<T, true>(r, o, end, vr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T ap = alpha * vp[i], aq = alpha * vq[i];
            vx[i] = vx[i] + ap;
            vr[i] = vr[i] - aq;
        }
        if (DINV) {
            T vd[4];
            cg_load4<T, WIDE>(dinv, o, end, vd);
#pragma unroll
            for (int i = 0; i < 4; ++i) vz[i] = vd[i] * vr[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) vz[i] = vr[i];
        }
        cg_store4<T, WIDE>(x, o, end, vx);
        cg_store4<T, true>(r, o, end, vr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rz[i] += (double) vr[i] * (double) vz[i];
            rr[i] += (double) vr[i] * (double) vr[i];
        }
    }
    double own[2] = {cg_thread_sum(rz), cg_thread_sum(rr)};
    cg_block_tree<2>(own, s_own);
    if (threadIdx.x == 0) {
        part[(size_t) rz_new * kCgMaxParts + blockIdx.x] = own[0];
        part[(size_t) kCgPartRR * kCgMaxParts + blockIdx.x] = own[1];
    }
}

// iteration k: the stop test on the sums cg_update left, then beta = <r,z>_new / <r,z>_old rounded to T once and p = z + beta p in T.  Block 0
// writes the state (and the history); when the loop ends here no workgroup touches p.
template <typename T, bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void cg_direction_kernel(int m, long long span, int k, const T *__restrict__ r, const T *__restrict__ dinv, T *__restrict__ p,
                                                              const double *__restrict__ part, CgState *st, double *__restrict__ hist, double rtol2, double atol2, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[3][kBlock / kWave];
    if (st->end_update) { // written by cg_update, this iteration's or an earlier one's: the same in every wave
        if (blockIdx.x == 0 && threadIdx.x == 0) st->end_direction = 1;
        return;
    }
    const int ids[3] = {k & 1 ? kCgPartRZ1 : kCgPartRZ0, (k - 1) & 1 ? kCgPartRZ1 : kCgPartRZ0, kCgPartRR};
    double v[3];
    cg_final_sums<3>(part, ids, v, s_fin);
    const double rz = v[0], rr = v[2];
    const T beta = (T) (rz / v[1]);
    int status = -1;
    if (!nostop) {
        if (!cg_finite(rr) || !cg_finite(rz)) status = 3;
        else if (rr <= __builtin_fmax(rtol2 * st->bb, atol2)) status = 0;
        else if (rz <= 0) status = 2;
        else if (!cg_finite((double) beta)) status = 3;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->iterations = k;
        st->rr = rr;
        if (hist) hist[k] = rr;
        if (status >= 0) { st->status = status; st->end_direction = 1; }
    }
    if (status >= 0) return;
    const long long begin = (long long) blockIdx.x * span, end = begin + span < m ? begin + span : (long long) m;
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vr[4], vp[4], vz[4];
        cg_load4<T, true>(r, o, end, vr);
        cg_load4<T, true>(p, o, end, vp);
        if (DINV) {
            T vd[4];
            cg_load4<T, WIDE>(dinv, o, end, vd);
#pragma unroll
            for (int i = 0; i < 4; ++i) vz[i] = vd[i] * vr[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) vz[i] = vr[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T bp = beta * vp[i];
            vp[i] = vz[i] + bp;
        }
        cg_store4<T, true>(p, o, end, vp);
    }
}

} // namespace spmv
