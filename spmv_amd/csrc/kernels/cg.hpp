// cg.hpp -- the vector kernels of spmv_hip_cg (preconditioned conjugate gradients that stay on the device): cg_init, cg_begin, cg_dot,
// cg_update and cg_direction.  One iteration is the handle's own multiply q = A p followed by
//
//   cg_dot        reads p, q                  leaves the partials of <p,q>
//   cg_update     reads p, q, x, r, (Dinv)    x += alpha p, r -= alpha q; leaves the partials of <r,z> and <r,r>, z = Dinv .* r
//   cg_direction  reads r, (Dinv), p          p = z + beta p (z recomputed, never stored); block 0 writes the state
//
// Hand-off between workgroups is the kernel boundary and nothing else: a kernel writes ONE fp64 partial per workgroup (at most kCgMaxParts),
// and every workgroup of the next kernel adds those partials again itself, in the fixed order of solve_common.hpp, and derives alpha / beta / the stop test
// from the sums -- redundantly, with the same bits everywhere.  No atomics, no in-launch flags or counters, no fences, no spinning, no
// cooperative launch; alpha and beta never visit the host, and finishing a dot costs no launch.
//
// The state (SolveState) is written by block 0 of cg_begin / cg_update / cg_direction and read by the kernels that FOLLOW: no kernel reads a
// word that its own launch writes, so every wave of every workgroup of a launch sees the same state and takes the same early return.  That
// is why the end of the loop is two words.  `end_direction` is written by cg_begin and cg_direction and read by cg_dot and cg_update;
// `end_update` is written by cg_update and read by cg_direction.  A kernel that finds the word it reads set passes the end on in the word it
// writes (block 0) and returns, so from the launch that ends the loop on every later kernel of the batch returns at once.  status,
// iterations and rr are only written by the kernels; bb is written by cg_begin alone and read by cg_direction.
//
// The order of a dot and why contraction is off in every function: solve_common.hpp, which also holds cg_begin and cg_dot -- spmv_hip_bicgstab
// starts its loop and forms <rhat,v> with the same two kernels.
#pragma once
#include "solve_common.hpp"

namespace spmv {

// the workspace vectors: SolveArgs::vec
enum { kCgVecR, kCgVecP, kCgVecQ, kCgVectors };

// the partial arrays, kCgMaxParts doubles each; entries behind the P in use stay +0.0 from the allocation on.  <r,z> has two: iteration k
// reads the old sum from (k - 1) & 1 while it writes the new one to k & 1
enum { kCgPartPQ, kCgPartRZ0, kCgPartRZ1, kCgPartRR, kCgPartBB, kCgPartArrays };

// spmv_solve.hip
hipError_t cg_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream);    // cg_init + cg_begin; q holds A x0 when use_x0
hipError_t cg_iteration_launch(const SolveArgs &a, int k, hipStream_t stream);      // cg_dot + cg_update + cg_direction of iteration k >= 1; q holds A p

// r = b (x = 0 is written) or r = b - q with q = A x0; p = z = Dinv .* r; the partials of <r,z>, <r,r> and <b,b>
template <typename T, bool WIDE, bool DINV, bool X0>
__global__ __launch_bounds__(kBlock) void cg_init_kernel(int m, long long span, const T *__restrict__ b, T *x, const T *__restrict__ q,
                                                         const T *__restrict__ dinv, T *__restrict__ r, T *__restrict__ p, double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double s_own[3][kBlock / kWave];
    const auto [begin, end] = cg_range(m, span);
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
        cg_precondition4<T, WIDE, DINV>(dinv, o, end, vr, vz);
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

// iteration k: alpha = <r,z>_old / <p,q> rounded to T once; x = x + alpha p, r = r - alpha q in T (a multiply, then an add); the partials of the
// new <r,z> and <r,r>.  <p,q> <= 0 (breakdown) or a non-finite scalar: block 0 records it and NO workgroup applies the update.
template <typename T, bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void cg_update_kernel(int m, long long span, int k, const T *__restrict__ p, const T *__restrict__ q, T *__restrict__ x, T *__restrict__ r,
                                                           const T *__restrict__ dinv, double *__restrict__ part, SolveState *st, int nostop)
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
    const auto [begin, end] = cg_range(m, span);
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
        cg_precondition4<T, WIDE, DINV>(dinv, o, end, vr, vz);
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
                                                              const double *__restrict__ part, SolveState *st, double *__restrict__ hist, double rtol2, double atol2, int nostop)
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
    const auto [begin, end] = cg_range(m, span);
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vr[4], vp[4], vz[4];
        cg_load4<T, true>(r, o, end, vr);
        cg_load4<T, true>(p, o, end, vp);
        cg_precondition4<T, WIDE, DINV>(dinv, o, end, vr, vz);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T bp = beta * vp[i];
            vp[i] = vz[i] + bp;
        }
        cg_store4<T, true>(p, o, end, vp);
    }
}

} // namespace spmv
