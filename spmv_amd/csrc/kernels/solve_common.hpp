// solve_common.hpp -- what the vector kernels of the six device-resident solvers share (cg.hpp, bicgstab.hpp, cg_columns.hpp, gmres.hpp, cg_mixed.hpp, lsqr.hpp): the
// state and the arguments of a solve, the 4-element accesses, the sums of a dot, and the two kernels that more than one solver launches -- the
// dot that leaves one array of partials (cg_dot_kernel) and the state of iteration 0 (cg_begin_kernel).
//
// Order of a dot over m elements (include/spmv_hip.h "the arithmetic contract"; tests/cg_cases.py restates it in numpy):
//   P = min(1024, ceil(m / 1024)) workgroups, L = 1024 ceil(m / (1024 P)); workgroup j owns [j L, min(m, (j + 1) L)).  The element at offset
//   o of its workgroup goes to thread (o / 4) % 256, slot o % 4, step o / 1024; each (thread, slot) accumulator starts at +0.0 and adds its
//   fp64 products by ascending step (an absent element adds +0.0: an accumulator is never -0.0, so leaving it out is the same bits).  Thread:
//   (a0 + a1) + (a2 + a3).  Wave: the adjacent-pair binary tree over 64 lanes (group_sum_dpp: an xor butterfly, the same sums since addition
//   commutes).  Workgroup: (w0 + w1) + (w2 + w3).  Final sum: the P partials padded with +0.0 to 1024, thread t takes 4t .. 4t + 3 as
//   (a + b) + (c + d), then the same wave and workgroup trees.
// Every product and every sum is a separate operation: contraction is off in every function of this file and of the solvers' files, AND
// spmv_solve.hip is compiled with -ffp-contract=off (build.py, HIP_SOURCE_FLAGS): under the library's -ffp-contract=fast the back end fuses a
// multiply and an add whatever the pragma says.  The only fused operations left in the ISA are the five of each kernel's one fp64 division.
#pragma once
#include "common.hpp"

namespace spmv {

constexpr int kCgChunk = 4 * kBlock; // elements a workgroup takes per step: 4 per thread
constexpr int kCgMaxParts = 1024;    // most workgroups of a vector kernel = most partials of a dot

// device copy of what a solve reports (status: the SPMV_HIP_CG_* values).  The three end words: cg.hpp and bicgstab.hpp say which kernel
// writes and which reads each; spmv_hip_cg never writes end_half, which stays 0 from the host's memset.  The host reads all three
struct SolveState {
    int end_half, end_update, end_direction;
    int status, iterations;
    double rr, bb;
};

struct ColsState; // cg_columns.hpp: the per-column state of spmv_hip_cg_columns

// what one solve's launches need (device pointers)
struct SolveArgs {
    int m = 0, parts = 0;
    int n = 0, parts_n = 0;        // spmv_hip_lsqr, whose x, v and w have n elements: that length and its P,
    long long span_n = 0;          // and its L
    double ls_tol = 0, damp = 0;   // spmv_hip_lsqr
    int k = 1;                     // right-hand sides: 1 but for spmv_hip_cg_columns, whose workspace vectors are m x k with ld = k
    long long ldb = 1, ldx = 1;    // leading dimensions of b and x
    long long span = 0;            // L
    void *vec[6] = {};             // the workspace vectors: the solver's own enum names the slots (kCgVec*, kBicgVec*)
    char *base = nullptr;          // spmv_hip_gmres, which has more than six: workspace vector i is base + i * stride
    size_t stride = 0;
    int restart = 0;               // spmv_hip_gmres: steps per cycle
    double drop2 = 0;              // spmv_hip_cg_mixed: update_drop^2,
    int every = 0, budget = 0;     // update_every and max_iterations
    void *x = nullptr;
    const void *b = nullptr, *dinv = nullptr;
    double *part = nullptr;        // the solver's partial arrays, kCgMaxParts doubles each
    SolveState *state = nullptr;
    ColsState *cols = nullptr;     // spmv_hip_cg_columns: in the place of `state`
    double *hist = nullptr;        // NULL: not wanted
    double rtol2 = 0, atol2 = 0;   // rtol^2, atol^2
    int nostop = 0;                // the timer: no test ever ends the loop
    bool wide = false;             // b, x and dinv allow 16-byte accesses (the workspace vectors always do); k columns: b and x are compact and aligned
    bool f64 = true;
};

__device__ __forceinline__ bool cg_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); } // false for NaN too

// the range [begin, end) of the m elements that this workgroup owns
struct CgRange { long long begin, end; };
__device__ __forceinline__ CgRange cg_range(int m, long long span)
{
    const long long begin = (long long) blockIdx.x * span, end = begin + span < m ? begin + span : (long long) m;
    return {begin, end};
}

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

// vz = Dinv .* vr for the 4 elements from `o`, or vz = vr without Dinv.  Dinv is loaded into vz itself: with an array of its own here the fp32
// kernels allocate more registers.  spmv_hip_cg's kernels use it; spmv_hip_bicgstab's y = Dinv .* s stays written out: through this helper
// four of its fp32 kernels take 4 to 6 more VGPRs
template <typename T, bool WIDE, bool DINV>
__device__ __forceinline__ void cg_precondition4(const T *dinv, long long o, long long end, const T (&vr)[4], T (&vz)[4])
{
#pragma clang fp contract(off)
    if (DINV) {
        cg_load4<T, WIDE>(dinv, o, end, vz);
#pragma unroll
        for (int k = 0; k < 4; ++k) vz[k] = vz[k] * vr[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) vz[k] = vr[k];
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

// one workgroup: the state of iteration 0 (the host has zeroed it) from the partials of <r,z> (BiCGStab: rho = <rhat,r>), <r,r> and <b,b> that the
// solver's init kernel left in the arrays id_rz, id_rr and id_bb.  SPD: <r,z> <= 0 is a breakdown (CG alone).  Writes end_direction
template <bool HIST, bool SPD>
__global__ __launch_bounds__(kBlock) void cg_begin_kernel(const double *__restrict__ part, int id_rz, int id_rr, int id_bb, SolveState *st, double *__restrict__ hist,
                                                          double rtol2, double atol2, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[3][kBlock / kWave];
    const int ids[3] = {id_rz, id_rr, id_bb};
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
        else if (SPD && rz <= 0) status = 2;
    }
    st->iterations = 0;
    st->rr = rr;
    st->bb = bb;
    if (HIST) hist[0] = rr;
    if (status >= 0) { st->status = status; st->end_direction = 1; }
}

// the partials of <p,q> into the array `part` (one row of the solver's partial arrays); returns at once when the word at `ended` is set: the
// end word that the kernel before it in the loop writes (spmv_hip_cg's <p,q>, spmv_hip_bicgstab's <rhat,v>: end_direction)
template <typename T>
__global__ __launch_bounds__(kBlock) void cg_dot_kernel(int m, long long span, const T *__restrict__ p, const T *__restrict__ q, double *__restrict__ part, const int *ended)
{
#pragma clang fp contract(off)
    __shared__ double s_own[1][kBlock / kWave];
    if (*ended) return; // cg_direction of the iteration before passed on an end that cg_update found
    const auto [begin, end] = cg_range(m, span);
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
    if (threadIdx.x == 0) part[blockIdx.x] = own[0];
}

} // namespace spmv
