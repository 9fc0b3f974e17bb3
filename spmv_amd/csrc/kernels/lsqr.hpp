// lsqr.hpp -- the vector kernels of spmv_hip_lsqr (LSQR, Paige and Saunders 1982: min |A x - b|^2 + damp^2 |x|^2 for any m x n matrix, on the
// device).  There are vectors of TWO lengths: u and q of m elements, v, w, qt and x of n.  One iteration is
//
//   (q = A v)                 the handle's own multiply
//   lsqr_u       grid P(m)    reads q, u          u = q - T(alpha) u; leaves the partials of <u,u>
//   lsqr_unit_u  grid P(m)    reads u             beta = sqrt(<u,u>); u = u / T(beta)
//   (qt = A^T u)              the attached transpose's own multiply
//   lsqr_v       grid P(n)    reads qt, v         v = qt - T(beta) v; leaves the partials of <v,v>
//   lsqr_step    grid P(n)    reads v, w, x       alpha = sqrt(<v,v>), the whole scalar chain; v = v / T(alpha); x = x + T(phi / rho) w;
//                                                 w = v - T(theta / rho) w; block 0 writes the state, the chain and the history
//
// and the start is lsqr_init (u = B or B - q; the partials of <B,B> and <u,u>), lsqr_unit_u in its START form (the tests of iteration 0),
// v = A^T u, lsqr_vv (x = 0 without an initial guess; the partials of <v,v>) and lsqr_step in its START form (v = v / T(alpha), w = v).
//
// Hand-off between workgroups is the kernel boundary and nothing else (cg.hpp): a kernel leaves ONE fp64 partial per workgroup, every workgroup
// of a later kernel adds the partials again itself, in the fixed order of solve_common.hpp, and derives beta, alpha and the chain from the sums
// -- redundantly, with the same bits everywhere.  <u,u> is re-added by lsqr_unit_u, lsqr_v and lsqr_step; <v,v> by lsqr_step.  No atomics, no
// in-launch flags, no fences, no spinning, no cooperative launch.
//
// The scalar chain (alpha, rhobar, phibar, psi2, a2) lives in the state, double-buffered by iteration parity as <r,z> is in cg.hpp: iteration k
// reads chain[(k - 1) & 1] and block 0 of lsqr_step writes chain[k & 1]; lsqr_u of iteration k + 1 reads alpha from there.
//
// No kernel reads a word that its own launch writes, hence three end words.  `end_half` is written by the START lsqr_unit_u alone (the tests of
// iteration 0) and read by lsqr_vv and the START lsqr_step; `end_direction` is written by lsqr_step (both forms) and read by lsqr_u,
// lsqr_unit_u and lsqr_v; `end_update` is written by lsqr_v, which passes end_direction on, and read by lsqr_step.  From the launch that ends
// the loop on every later vector kernel of the batch returns at once; the two multiplies still run, into q and qt: what a batch enqueues never
// depends on data.  status, iterations, rr, ar and anorm are only written by the kernels; bb is written by the START lsqr_unit_u alone.
//
// A non-finite <u,u> is found by lsqr_unit_u and lsqr_v, which then change nothing, and recorded by lsqr_step, which applies nothing.
#pragma once
#include "solve_common.hpp"

namespace spmv {

// the workspace vectors (SolveArgs::vec): two of m elements, then three of n
enum { kLsqrVecU, kLsqrVecQ, kLsqrVectorsM, kLsqrVecV = kLsqrVectorsM, kLsqrVecW, kLsqrVecQt, kLsqrVectors, kLsqrVectorsN = kLsqrVectors - kLsqrVectorsM };

// the partial arrays, kCgMaxParts doubles each; entries behind the P in use stay +0.0 from the allocation on.  <u,u> has P(m) entries in use, <v,v> P(n)
enum { kLsqrPartUU, kLsqrPartVV, kLsqrPartBB, kLsqrPartArrays };

constexpr int kLsqrLeastSquares = 5; // SPMV_HIP_LSQR_LEAST_SQUARES

struct LsqrChain { double alpha, rhobar, phibar, psi2, a2; };

struct LsqrState {
    SolveState s;       // what the host's look reads; s.rr: the residual estimate phibar^2 + psi2 of the last iteration applied
    double ar, anorm;   // alpha |tau| and sqrt(a2) of the last iteration applied
    LsqrChain chain[2];
};

// spmv_solve.hip
hipError_t lsqr_init_launch(const SolveArgs &a, bool use_x0, hipStream_t stream);   // lsqr_init + the START lsqr_unit_u; q holds A x0 when use_x0
hipError_t lsqr_first_launch(const SolveArgs &a, bool use_x0, hipStream_t stream);  // lsqr_vv + the START lsqr_step; v holds A^T u
hipError_t lsqr_u_launch(const SolveArgs &a, int k, hipStream_t stream);            // lsqr_u + lsqr_unit_u of iteration k >= 1; q holds A v
hipError_t lsqr_v_launch(const SolveArgs &a, int k, hipStream_t stream);            // lsqr_v + lsqr_step of iteration k; qt holds A^T u

// u = b, or u = b - q with q = A x0; the partials of <u,u> and <b,b>
template <typename T, bool WIDE, bool X0>
__global__ __launch_bounds__(kBlock) void lsqr_init_kernel(int m, long long span, const T *__restrict__ b, const T *__restrict__ q, T *__restrict__ u, double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double s_own[2][kBlock / kWave];
    const auto [begin, end] = cg_range(m, span);
    double uu[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vb[4], vu[4];
        cg_load4<T, WIDE>(b, o, end, vb);
        if (X0) {
            T vq[4];
            cg_load4<T, true>(q, o, end, vq);
#pragma unroll
            for (int i = 0; i < 4; ++i) vu[i] = vb[i] - vq[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) vu[i] = vb[i];
        }
        cg_store4<T, true>(u, o, end, vu);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uu[i] += (double) vu[i] * (double) vu[i];
            bb[i] += (double) vb[i] * (double) vb[i];
        }
    }
    double own[2] = {cg_thread_sum(uu), cg_thread_sum(bb)};
    cg_block_tree<2>(own, s_own);
    if (threadIdx.x == 0) {
        part[(size_t) kLsqrPartUU * kCgMaxParts + blockIdx.x] = own[0];
        part[(size_t) kLsqrPartBB * kCgMaxParts + blockIdx.x] = own[1];
    }
}

// beta = sqrt(<u,u>); u = u / T(beta) when beta > 0.  START: behind lsqr_init, the state zeroed by the host; block 0 writes bb, rr = <u,u>,
// history[0] and what the tests of iteration 0 say (end_half); no workgroup divides when they end the loop
template <typename T, bool START>
__global__ __launch_bounds__(kBlock) void lsqr_unit_u_kernel(int m, long long span, T *__restrict__ u, const double *__restrict__ part, LsqrState *st, double *__restrict__ hist,
                                                             double rtol2, double atol2, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[2][kBlock / kWave];
    if (!START && st->s.end_direction) return; // an earlier launch's word: the same in every wave
    const int ids[2] = {kLsqrPartUU, kLsqrPartBB};
    double v[2];
    cg_final_sums<2>(part, ids, v, s_fin);
    const double uu = v[0], bb = v[1];
    if (START) {
        double rr = uu;
        int status = -1;
        if (!nostop) {
            if (!cg_finite(bb) || !cg_finite(uu)) status = 3;
            else if (bb == 0) { status = 0; rr = 0; } // the solution is x = 0: the host zeroes X
            else if (rr <= __builtin_fmax(rtol2 * bb, atol2)) status = 0;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->s.iterations = 0;
            st->s.rr = rr;
            st->s.bb = bb;
            if (hist) hist[0] = rr;
            if (status >= 0) { st->s.status = status; st->s.end_half = 1; }
        }
        if (status >= 0) return;
    } else if (!nostop && !cg_finite(uu)) return; // lsqr_step records it
    const double beta64 = __builtin_sqrt(uu);
    if (!(beta64 > 0)) return;
    const T beta = (T) beta64;
    const auto [begin, end] = cg_range(m, span);
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vu[4];
        cg_load4<T, true>(u, o, end, vu);
#pragma unroll
        for (int i = 0; i < 4; ++i) vu[i] = vu[i] / beta;
        cg_store4<T, true>(u, o, end, vu);
    }
}

// the start, over n: x = 0 without an initial guess -- always, whatever the tests of iteration 0 said --, then the partials of <v,v> of v = A^T u
template <typename T, bool WIDE, bool X0>
__global__ __launch_bounds__(kBlock) void lsqr_vv_kernel(int n, long long span, const T *__restrict__ v, T *__restrict__ x, double *__restrict__ part, const LsqrState *st)
{
#pragma clang fp contract(off)
    __shared__ double s_own[1][kBlock / kWave];
    const auto [begin, end] = cg_range(n, span);
    const bool ended = st->s.end_half != 0; // the START lsqr_unit_u's word
    if (X0 && ended) return;
    double vv[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        if (!X0) {
            const T zero[4] = {T(0), T(0), T(0), T(0)};
            cg_store4<T, WIDE>(x, o, end, zero);
        }
        if (ended) continue;
        T e[4];
        cg_load4<T, true>(v, o, end, e);
#pragma unroll
        for (int i = 0; i < 4; ++i) vv[i] += (double) e[i] * (double) e[i];
    }
    if (ended) return;
    double own[1] = {cg_thread_sum(vv)};
    cg_block_tree<1>(own, s_own);
    if (threadIdx.x == 0) part[(size_t) kLsqrPartVV * kCgMaxParts + blockIdx.x] = own[0];
}

// iteration k, over m: u = q - T(alpha) u in T (a multiply, then a subtraction), alpha from the chain of iteration k - 1; the partials of <u,u>
template <typename T>
__global__ __launch_bounds__(kBlock) void lsqr_u_kernel(int m, long long span, int k, const T *__restrict__ q, T *__restrict__ u, double *__restrict__ part, const LsqrState *st)
{
#pragma clang fp contract(off)
    __shared__ double s_own[1][kBlock / kWave];
    if (st->s.end_direction) return;
    const T alpha = (T) st->chain[(k - 1) & 1].alpha;
    const auto [begin, end] = cg_range(m, span);
    double uu[4] = {0, 0, 0, 0};
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vq[4], vu[4];
        cg_load4<T, true>(q, o, end, vq);
        cg_load4<T, true>(u, o, end, vu);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T au = alpha * vu[i];
            vu[i] = vq[i] - au;
            uu[i] += (double) vu[i] * (double) vu[i];
        }
        cg_store4<T, true>(u, o, end, vu);
    }
    double own[1] = {cg_thread_sum(uu)};
    cg_block_tree<1>(own, s_own);
    if (threadIdx.x == 0) part[(size_t) kLsqrPartUU * kCgMaxParts + blockIdx.x] = own[0];
}

// iteration k, over n: v = qt - T(beta) v in T, beta = sqrt(<u,u>) from lsqr_u's partials; the partials of <v,v>.  Passes the loop's end on
template <typename T>
__global__ __launch_bounds__(kBlock) void lsqr_v_kernel(int n, long long span, const T *__restrict__ qt, T *__restrict__ v, double *__restrict__ part, LsqrState *st, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[1][kBlock / kWave], s_own[1][kBlock / kWave];
    if (st->s.end_direction) { // lsqr_step of an earlier iteration, or of the start
        if (blockIdx.x == 0 && threadIdx.x == 0) st->s.end_update = 1;
        return;
    }
    const int ids[1] = {kLsqrPartUU};
    double f[1];
    cg_final_sums<1>(part, ids, f, s_fin);
    if (!nostop && !cg_finite(f[0])) return; // lsqr_step records it
    const T beta = (T) __builtin_sqrt(f[0]);
    const auto [begin, end] = cg_range(n, span);
    double vv[4] = {0, 0, 0, 0};
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vq[4], e[4];
        cg_load4<T, true>(qt, o, end, vq);
        cg_load4<T, true>(v, o, end, e);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T bv = beta * e[i];
            e[i] = vq[i] - bv;
            vv[i] += (double) e[i] * (double) e[i];
        }
        cg_store4<T, true>(v, o, end, e);
    }
    double own[1] = {cg_thread_sum(vv)};
    cg_block_tree<1>(own, s_own);
    if (threadIdx.x == 0) part[(size_t) kLsqrPartVV * kCgMaxParts + blockIdx.x] = own[0];
}

// over n.  START: alpha = sqrt(<v,v>); v = v / T(alpha); w = v; the chain of iteration 0.  Iteration k >= 1: alpha, the chain of include/spmv_hip.h
// steps 7 to 15 from the chain of iteration k - 1, then v = v / T(alpha), x = x + T(phi / rho) w and, unless the loop ends here,
// w = v - T(theta / rho) w.  A non-finite sum or factor: nothing is applied.  Block 0 writes the state, the chain and the history
template <typename T, bool WIDE, bool START>
__global__ __launch_bounds__(kBlock) void lsqr_step_kernel(int n, long long span, int k, T *__restrict__ v, T *__restrict__ w, T *__restrict__ x, const double *__restrict__ part,
                                                           LsqrState *st, double *__restrict__ hist, double rtol2, double atol2, double ls_tol, double damp, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[2][kBlock / kWave];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (START ? st->s.end_half : st->s.end_update) { // an earlier launch's word: the same in every wave
        if (first) st->s.end_direction = 1;
        return;
    }
    const int ids[2] = {kLsqrPartUU, kLsqrPartVV};
    double f[2];
    cg_final_sums<2>(part, ids, f, s_fin);
    const double uu = f[0], vv = f[1];
    const auto [begin, end] = cg_range(n, span);
    int status = -1;
    if (START) {
        if (!nostop && !cg_finite(vv)) status = 3;
        const double beta = __builtin_sqrt(uu), alpha = __builtin_sqrt(vv), a2 = alpha * alpha;
        if (!nostop && status < 0 && alpha == 0) status = kLsqrLeastSquares;
        if (first) {
            st->chain[0] = LsqrChain{alpha, alpha, beta, 0.0, a2};
            st->ar = status >= 0 ? 0.0 : alpha * beta;
            st->anorm = status == 3 ? 0.0 : __builtin_sqrt(a2);
            if (status >= 0) { st->s.status = status; st->s.end_direction = 1; }
        }
        if (status >= 0 || !(alpha > 0)) return;
        const T ta = (T) alpha;
#pragma unroll 2
        for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
            T e[4];
            cg_load4<T, true>(v, o, end, e);
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = e[i] / ta;
            cg_store4<T, true>(v, o, end, e);
            cg_store4<T, true>(w, o, end, e);
        }
        return;
    }
    const LsqrChain old = st->chain[(k - 1) & 1];
    const double beta = __builtin_sqrt(uu), alpha = __builtin_sqrt(vv);
    const double bsq = beta * beta, asq = alpha * alpha, dsq = damp * damp;
    const double a2 = ((old.a2 + bsq) + asq) + dsq;
    const double rb2 = old.rhobar * old.rhobar, rhobar1 = __builtin_sqrt(rb2 + dsq);
    const double c1 = old.rhobar / rhobar1, s1 = damp / rhobar1;
    const double psi = s1 * old.phibar, phibar1 = c1 * old.phibar, psq = psi * psi, psi2 = old.psi2 + psq;
    const double r12 = rhobar1 * rhobar1, rho = __builtin_sqrt(r12 + bsq);
    const double c = rhobar1 / rho, s = beta / rho;
    const double theta = s * alpha, ca = c * alpha, rhobar = -ca, phi = c * phibar1, phibar = s * phibar1, tau = s * phi;
    const T tx = (T) (phi / rho), tw = (T) (theta / rho);
    const double pb2 = phibar * phibar, rr = pb2 + psi2, ar = alpha * __builtin_fabs(tau);
    bool applied = true;
    if (!nostop) {
        if (!cg_finite(uu) || !cg_finite(vv) || !cg_finite((double) tx) || !cg_finite((double) tw)) { status = 3; applied = false; }
        else if (!cg_finite(rr) || !cg_finite(ar) || !cg_finite(a2)) status = 3;
        else if (rr <= __builtin_fmax(rtol2 * st->s.bb, atol2)) status = 0;
        else {
            const double sa = __builtin_sqrt(a2), sr = __builtin_sqrt(rr), bound = sa * sr;
            if (ar <= ls_tol * bound) status = kLsqrLeastSquares;
        }
    }
    if (first) {
        if (applied) {
            st->chain[k & 1] = LsqrChain{alpha, rhobar, phibar, psi2, a2};
            st->s.iterations = k;
            st->s.rr = rr;
            st->ar = ar;
            st->anorm = __builtin_sqrt(a2);
            if (hist) hist[k] = rr;
        }
        if (status >= 0) { st->s.status = status; st->s.end_direction = 1; }
    }
    if (!applied) return;
    const T ta = (T) alpha;
    const bool unit = alpha > 0, direction = status < 0;
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T e[4], vw[4], vx[4];
        cg_load4<T, true>(v, o, end, e);
        cg_load4<T, true>(w, o, end, vw);
        cg_load4<T, WIDE>(x, o, end, vx);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T xw = tx * vw[i];
            vx[i] = vx[i] + xw;
            if (unit) e[i] = e[i] / ta;
            const T ww = tw * vw[i];
            vw[i] = e[i] - ww;
        }
        cg_store4<T, WIDE>(x, o, end, vx);
        if (unit) cg_store4<T, true>(v, o, end, e);
        if (direction) cg_store4<T, true>(w, o, end, vw);
    }
}

} // namespace spmv
