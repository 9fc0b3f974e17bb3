// bicgstab.hpp -- the vector kernels of spmv_hip_bicgstab (right-preconditioned BiCGStab that stays on the device): bicg_init, bicg_begin and,
// per iteration, behind the handle's own multiplies v = A ph and t = A sh (ph = Dinv .* p, sh = Dinv .* s; p and s themselves without Dinv),
//
//   bicg_rv         reads rhat, v                    leaves the partials of <rhat,v>
//   bicg_half       reads ph, v, x, r, (Dinv)        alpha; x += alpha ph; r <- s = r - alpha v in place; y <- Dinv .* s; the partials of <s,s>
//   bicg_ts         reads t, s                       leaves the partials of <t,s> and <t,t>
//   bicg_update     reads t, s, sh, x, rhat          the half-step stop test; omega; x += omega sh; r <- s - omega t in place; the partials of
//                                                    <rhat,r> and <r,r>
//   bicg_direction  reads r, p, v, (Dinv)            the stop test; beta; p = r + beta (p - omega v); y <- Dinv .* p; block 0 writes the state
//
// s lives in r.  y exists only with Dinv: it holds ph from bicg_direction (bicg_init) to bicg_half, which overwrites it element by element
// with sh.  Everything that crosses workgroups is solve_common.hpp's: ONE fp64 partial per workgroup and dot, every workgroup of a later kernel adds the
// partials again itself in the fixed order (cg_final_sums) and derives alpha / omega / beta and the stop tests from the sums, with the same
// bits everywhere.  The partial arrays of an iteration stay in place until the next one overwrites them, so bicg_direction forms alpha
// and omega again from <rhat,v>, <t,s> and <t,t>; rho has two arrays, iteration k reads (k - 1) & 1 and writes k & 1.  Hand-off between
// workgroups is the kernel boundary and nothing else: no atomics, no in-launch flags, no fences, no spinning, no cooperative launch.
//
// The state (SolveState): no kernel reads a word that its own launch writes, so every wave of a launch sees the same state and takes the same
// early return.  Three kernels of an iteration can end the loop, hence three words:
//   end_half       written by bicg_half                      read by bicg_ts and bicg_update
//   end_update     written by bicg_update                    read by bicg_direction
//   end_direction  written by bicg_begin and bicg_direction  read by bicg_rv and bicg_half
// A kernel that finds the word it reads set passes the end on in the word it writes (block 0) and returns, so from the launch that ends the
// loop on every later kernel of the batch returns at once.  bb is written by bicg_begin alone.
//
// The order of a dot is solve_common.hpp's (include/spmv_hip.h, "the arithmetic contract"); every product and every sum is a separate operation:
// contraction is off in every function of this file AND spmv_solve.hip is compiled with -ffp-contract=off (build.py, HIP_SOURCE_FLAGS).
// bicg_begin and bicg_rv are solve_common.hpp's cg_begin_kernel (without CG's <r,z> <= 0 test) and cg_dot_kernel.
#pragma once
#include "solve_common.hpp"

namespace spmv {

// the workspace vectors: SolveArgs::vec
enum { kBicgVecR, kBicgVecRhat, kBicgVecP, kBicgVecV, kBicgVecT, kBicgVecY, kBicgVectors };

// the partial arrays, kCgMaxParts doubles each; entries behind the P in use stay +0.0 from the allocation on
enum { kBicgPartRV, kBicgPartSS, kBicgPartTS, kBicgPartTT, kBicgPartRho0, kBicgPartRho1, kBicgPartRR, kBicgPartBB, kBicgPartArrays };

// spmv_solve.hip
hipError_t bicg_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream); // bicg_init + bicg_begin; v holds A x0 when use_x0
hipError_t bicg_first_launch(const SolveArgs &a, int k, hipStream_t stream);       // bicg_rv + bicg_half of iteration k >= 1; v holds A ph
hipError_t bicg_second_launch(const SolveArgs &a, int k, hipStream_t stream);      // bicg_ts + bicg_update + bicg_direction; t holds A sh

// r = b (x = 0 is written) or r = b - v with v = A x0; rhat = p = r; y = Dinv .* p; the partials of <rhat,r>, <r,r> and <b,b>
template <typename T, bool WIDE, bool DINV, bool X0>
__global__ __launch_bounds__(kBlock) void bicg_init_kernel(int m, long long span, const T *__restrict__ b, T *x, const T *__restrict__ v, const T *__restrict__ dinv,
                                                           T *__restrict__ r, T *__restrict__ rhat, T *__restrict__ p, T *__restrict__ y, double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double s_own[3][kBlock / kWave];
    const auto [begin, end] = cg_range(m, span);
    double rho[4] = {0, 0, 0, 0}, rr[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vb[4], vr[4];
        cg_load4<T, WIDE>(b, o, end, vb);
        if (X0) {
            T vv[4];
            cg_load4<T, true>(v, o, end, vv);
#pragma unroll
            for (int i = 0; i < 4; ++i) vr[i] = vb[i] - vv[i];
        } else {
            const T zero[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
            for (int i = 0; i < 4; ++i) vr[i] = vb[i];
            cg_store4<T, WIDE>(x, o, end, zero);
        }
        cg_store4<T, true>(r, o, end, vr);
        cg_store4<T, true>(rhat, o, end, vr);
        cg_store4<T, true>(p, o, end, vr);
        if (DINV) {
            T vd[4], vy[4];
            cg_load4<T, WIDE>(dinv, o, end, vd);
#pragma unroll
            for (int i = 0; i < 4; ++i) vy[i] = vd[i] * vr[i];
            cg_store4<T, true>(y, o, end, vy);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rho[i] += (double) vr[i] * (double) vr[i]; // rhat = r
            rr[i] += (double) vr[i] * (double) vr[i];
            bb[i] += (double) vb[i] * (double) vb[i];
        }
    }
    double own[3] = {cg_thread_sum(rho), cg_thread_sum(rr), cg_thread_sum(bb)};
    cg_block_tree<3>(own, s_own);
    if (threadIdx.x == 0) {
        part[(size_t) kBicgPartRho0 * kCgMaxParts + blockIdx.x] = own[0];
        part[(size_t) kBicgPartRR * kCgMaxParts + blockIdx.x] = own[1];
        part[(size_t) kBicgPartBB * kCgMaxParts + blockIdx.x] = own[2];
    }
}

// iteration k: alpha = rho / <rhat,v> rounded to T once; x = x + alpha ph, s = r - alpha v (into r) in T, a multiply and then an add; y = Dinv .* s;
// the partials of <s,s>.  ph is y with Dinv (read before this element's sh is written over it) and p without.  <rhat,v> = 0 or rho = 0
// (breakdown) or a non-finite scalar: block 0 records it and NO workgroup applies the half step.
template <typename T, bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void bicg_half_kernel(int m, long long span, int k, const T *__restrict__ p, const T *__restrict__ v, T *__restrict__ x, T *__restrict__ r,
                                                           const T *__restrict__ dinv, T *__restrict__ y, double *__restrict__ part, SolveState *st, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[2][kBlock / kWave], s_own[1][kBlock / kWave];
    if (st->end_direction) { // an earlier launch's word: the same in every wave
        if (blockIdx.x == 0 && threadIdx.x == 0) st->end_half = 1;
        return;
    }
    const int ids[2] = {(k - 1) & 1 ? kBicgPartRho1 : kBicgPartRho0, kBicgPartRV};
    double f[2];
    cg_final_sums<2>(part, ids, f, s_fin);
    const T alpha = (T) (f[0] / f[1]);
    if (!nostop) {
        int status = -1;
        if (!cg_finite(f[1]) || !cg_finite(f[0])) status = 3;
        else if (f[1] == 0 || f[0] == 0) status = 2;
        else if (!cg_finite((double) alpha)) status = 3;
        if (status >= 0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { st->status = status; st->end_half = 1; }
            return;
        }
    }
    const auto [begin, end] = cg_range(m, span);
    double ss[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vp[4], vv[4], vx[4], vr[4];
        cg_load4<T, true>(DINV ? (const T *) y : p, o, end, vp);
        cg_load4<T, true>(v, o, end, vv);
        cg_load4<T, WIDE>(x, o, end, vx);
        cg_load4<T, true>(r, o, end, vr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T ap = alpha * vp[i], av = alpha * vv[i];
            vx[i] = vx[i] + ap;
            vr[i] = vr[i] - av;
        }
        cg_store4<T, WIDE>(x, o, end, vx);
        cg_store4<T, true>(r, o, end, vr);
        if (DINV) {
            T vd[4], vy[4];
            cg_load4<T, WIDE>(dinv, o, end, vd);
#pragma unroll
            for (int i = 0; i < 4; ++i) vy[i] = vd[i] * vr[i];
            cg_store4<T, true>(y, o, end, vy);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) ss[i] += (double) vr[i] * (double) vr[i];
    }
    double own[1] = {cg_thread_sum(ss)};
    cg_block_tree<1>(own, s_own);
    if (threadIdx.x == 0) part[(size_t) kBicgPartSS * kCgMaxParts + blockIdx.x] = own[0];
}

template <typename T>
__global__ __launch_bounds__(kBlock) void bicg_ts_kernel(int m, long long span, const T *__restrict__ t, const T *__restrict__ s, double *__restrict__ part, const SolveState *st)
{
#pragma clang fp contract(off)
    __shared__ double s_own[2][kBlock / kWave];
    if (st->end_half) return;
    const auto [begin, end] = cg_range(m, span);
    double ts[4] = {0, 0, 0, 0}, tt[4] = {0, 0, 0, 0};
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vt[4], vs[4];
        cg_load4<T, true>(t, o, end, vt);
        cg_load4<T, true>(s, o, end, vs);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ts[i] += (double) vt[i] * (double) vs[i];
            tt[i] += (double) vt[i] * (double) vt[i];
        }
    }
    double own[2] = {cg_thread_sum(ts), cg_thread_sum(tt)};
    cg_block_tree<2>(own, s_own);
    if (threadIdx.x == 0) {
        part[(size_t) kBicgPartTS * kCgMaxParts + blockIdx.x] = own[0];
        part[(size_t) kBicgPartTT * kCgMaxParts + blockIdx.x] = own[1];
    }
}

// iteration k: the stop test of the half step on <s,s>, then omega = <t,s> / <t,t> rounded to T once; x = x + omega sh, r = s - omega t (s is in
// r) in T; the partials of the new rho = <rhat,r> and of <r,r>.  sh is y with Dinv and s without.  When the loop ends here -- the half step
// met the stop test, <t,t> = 0, <t,s> = 0, omega = 0 (breakdown) or a non-finite scalar -- block 0 records iteration k with rr = <s,s> and NO
// workgroup applies the second half: x keeps the half step.
template <typename T, bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void bicg_update_kernel(int m, long long span, int k, const T *__restrict__ t, T *__restrict__ r, const T *__restrict__ y, T *__restrict__ x,
                                                             const T *__restrict__ rhat, double *__restrict__ part, SolveState *st, double *__restrict__ hist, double rtol2,
                                                             double atol2, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[3][kBlock / kWave], s_own[2][kBlock / kWave];
    if (st->end_half) { // written by bicg_half, this iteration's or an earlier one's: the same in every wave
        if (blockIdx.x == 0 && threadIdx.x == 0) st->end_update = 1;
        return;
    }
    const int ids[3] = {kBicgPartSS, kBicgPartTS, kBicgPartTT};
    double f[3];
    cg_final_sums<3>(part, ids, f, s_fin);
    const double ss = f[0], ts = f[1], tt = f[2];
    const T omega = (T) (ts / tt);
    if (!nostop) {
        int status = -1;
        if (!cg_finite(ss)) status = 3;
        else if (ss <= __builtin_fmax(rtol2 * st->bb, atol2)) status = 0;
        else if (!cg_finite(ts) || !cg_finite(tt)) status = 3;
        else if (tt == 0 || ts == 0) status = 2;
        else if (!cg_finite((double) omega)) status = 3;
        else if (omega == T(0)) status = 2;
        if (status >= 0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                st->iterations = k;
                st->rr = ss;
                if (hist) hist[k] = ss;
                st->status = status;
                st->end_update = 1;
            }
            return;
        }
    }
    const int rho_new = k & 1 ? kBicgPartRho1 : kBicgPartRho0;
    const auto [begin, end] = cg_range(m, span);
    double rho[4] = {0, 0, 0, 0}, rr[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vt[4], vs[4], vh[4], vx[4], va[4];
        cg_load4<T, true>(t, o, end, vt);
        cg_load4<T, true>(r, o, end, vs);
        if (DINV) cg_load4<T, true>(y, o, end, vh);
        cg_load4<T, WIDE>(x, o, end, vx);
        cg_load4<T, true>(rhat, o, end, va);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T oh = omega * (DINV ? vh[i] : vs[i]), ot = omega * vt[i];
            vx[i] = vx[i] + oh;
            vs[i] = vs[i] - ot;
        }
        cg_store4<T, WIDE>(x, o, end, vx);
        cg_store4<T, true>(r, o, end, vs);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rho[i] += (double) va[i] * (double) vs[i];
            rr[i] += (double) vs[i] * (double) vs[i];
        }
    }
    double own[2] = {cg_thread_sum(rho), cg_thread_sum(rr)};
    cg_block_tree<2>(own, s_own);
    if (threadIdx.x == 0) {
        part[(size_t) rho_new * kCgMaxParts + blockIdx.x] = own[0];
        part[(size_t) kBicgPartRR * kCgMaxParts + blockIdx.x] = own[1];
    }
}

// iteration k: the stop test on the sums bicg_update left, then beta = (rho_new / rho_old) * (alpha / omega) in fp64 -- alpha and omega formed
// again from the partials that are still in place, rounded to T as they were applied -- rounded to T once, and p = r + beta (p - omega v) in T:
// omega v, p minus that, beta times that, r plus that; y = Dinv .* p.  Block 0 writes the state (and the history); when the loop ends here no
// workgroup touches p.
template <typename T, bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void bicg_direction_kernel(int m, long long span, int k, const T *__restrict__ r, T *__restrict__ p, const T *__restrict__ v,
                                                                const T *__restrict__ dinv, T *__restrict__ y, const double *__restrict__ part, SolveState *st,
                                                                double *__restrict__ hist, double rtol2, double atol2, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[6][kBlock / kWave];
    if (st->end_update) { // written by bicg_update, this iteration's or an earlier one's: the same in every wave
        if (blockIdx.x == 0 && threadIdx.x == 0) st->end_direction = 1;
        return;
    }
    const int ids[6] = {k & 1 ? kBicgPartRho1 : kBicgPartRho0, (k - 1) & 1 ? kBicgPartRho1 : kBicgPartRho0, kBicgPartRR, kBicgPartRV, kBicgPartTS, kBicgPartTT};
    double f[6];
    cg_final_sums<6>(part, ids, f, s_fin);
    const double rho_new = f[0], rho_old = f[1], rr = f[2];
    const T alpha = (T) (rho_old / f[3]), omega = (T) (f[4] / f[5]);
    const double ratio = rho_new / rho_old, ao = (double) alpha / (double) omega;
    const T beta = (T) (ratio * ao);
    int status = -1;
    if (!nostop) {
        if (!cg_finite(rr) || !cg_finite(rho_new)) status = 3;
        else if (rr <= __builtin_fmax(rtol2 * st->bb, atol2)) status = 0;
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
        T vr[4], vp[4], vv[4];
        cg_load4<T, true>(r, o, end, vr);
        cg_load4<T, true>(p, o, end, vp);
        cg_load4<T, true>(v, o, end, vv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T ov = omega * vv[i];
            const T d = vp[i] - ov;
            const T bd = beta * d;
            vp[i] = vr[i] + bd;
        }
        cg_store4<T, true>(p, o, end, vp);
        if (DINV) {
            T vd[4], vy[4];
            cg_load4<T, WIDE>(dinv, o, end, vd);
#pragma unroll
            for (int i = 0; i < 4; ++i) vy[i] = vd[i] * vp[i];
            cg_store4<T, true>(y, o, end, vy);
        }
    }
}

} // namespace spmv
