// cg_mixed.hpp -- the vector kernels of spmv_hip_cg_mixed (conjugate gradients with reliable updates: fp32 iterations on a float copy of the
// matrix, the solution and the TRUE residual kept in fp64): mix_try, mix_residual, mix_resume and mix_direction.  The inner iteration is
// spmv_hip_cg's in float on the partial solution y in the place of x -- cg_dot<float> and cg_update<float> unchanged (cg.hpp) -- and
//
//   mix_direction  reads r, (Dinv), p          cg_direction's tests, p = z + beta p, then the tests that END A SEGMENT; block 0 writes the state
//
// A segment's end sets `end_direction` and names its reason in `segment_end`; from there on every later kernel of the batch returns at once,
// as at a solve's end.  The host finds `segment_end` at its ordinary look and enqueues the UPDATE:
//
//   mix_try        reads x, y                  xn = x + widen(y); block 0 copies the words mix_resume needs (rr, segment_end)
//   (high's multiply q64 = A xn)
//   mix_residual   reads b, q64, (Dinv)        r64 = b - q64 in registers only; leaves the partials of <r64,r64>; r = narrow(r64), z = Dinv .* r;
//                                              leaves the partials of <r,z> and <r,r>
//   mix_resume     reads xn, (r, Dinv)         every workgroup adds the partials and takes the update's decision: commit x = xn, y = 0 (and
//                                              p = z when the direction starts afresh); block 0 re-arms the loop -- clears the end words,
//                                              writes the segment's words -- or writes the final status and leaves the end words set
//
// The start of a solve is the same mix_residual + mix_resume on x0 (or on x = 0, which mix_residual writes).
//
// Hand-off is cg.hpp's: the kernel boundary and nothing else, and no kernel reads a word that its own launch writes.  mix_resume writes
// s.rr, segment_end, seg, seg_first, thr, updates and the end words and reads u_rr and u_reason, the copies mix_try made; mix_direction
// writes s.iterations, s.status, segment_end and end_direction and reads end_update (cg_update's), seg, seg_first and thr (mix_resume's); the
// iteration's number k, the update's number and the budget are kernel arguments.  <r,z> keeps cg.hpp's two arrays: the update behind
// iteration k leaves the segment's first <r,z> where iteration k + 1 looks for the old one, in k & 1.
#pragma once
#include "cg.hpp"

namespace spmv {

// the workspace vectors: two of m doubles, then four of m floats
enum { kMixVecXn, kMixVecQ64, kMixVectors64 };
enum { kMixVecR, kMixVecP, kMixVecQ, kMixVecY, kMixVectors32 };

// the partial arrays: spmv_hip_cg's five and the true residual's
enum { kMixPartTrue = kCgPartArrays, kMixPartArrays };

// why a segment ended (MixState::segment_end; 0: it has not)
enum { kMixEndExact = 1, kMixEndEstimate, kMixEndDrop, kMixEndEvery, kMixEndBudget };

// s: what cg_update<float> reads and writes (the end words, status on a breakdown); s.rr is the TRUE <r64,r64> of the committed x
struct MixState {
    SolveState s;
    int segment_end;   // mix_direction: the reason; mix_resume: 0
    int seg_first;     // the iterations applied before this segment
    int updates;       // committed updates
    int u_reason;      // mix_try's copy of segment_end
    double seg, thr;   // <r,r> at the segment's start; max(rtol^2 bb, atol^2)
    double u_rr;       // mix_try's copy of s.rr
};
static_assert(offsetof(MixState, s) == 0, "cg_update_kernel is handed the MixState as its SolveState");

// spmv_solve.hip; the six vectors are SolveArgs::vec[0 .. 5]: the two of doubles, then the four of floats (slot kMixVectors64 + kMixVecR ...)
hipError_t mix_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream);         // mix_residual + mix_resume of the start; q64 holds A x0 when use_x0
hipError_t mix_iteration_launch(const SolveArgs &a, int k, hipStream_t stream);          // cg_dot + cg_update + mix_direction of iteration k >= 1; q holds A p
hipError_t mix_try_launch(const SolveArgs &a, hipStream_t stream);                        // xn = x + y
hipError_t mix_update_launch(const SolveArgs &a, int k, int update, hipStream_t stream); // mix_residual + mix_resume behind iteration k; q64 holds A xn

// xn = x + widen(y), an fp64 add
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void mix_try_kernel(int m, long long span, const double *x, const float *__restrict__ y, double *__restrict__ xn, MixState *st)
{
#pragma clang fp contract(off)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->u_rr = st->s.rr;
        st->u_reason = st->segment_end;
    }
    const auto [begin, end] = cg_range(m, span);
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        double vx[4];
        float vy[4];
        cg_load4<double, WIDE>(x, o, end, vx);
        cg_load4<float, true>(y, o, end, vy);
#pragma unroll
        for (int i = 0; i < 4; ++i) vx[i] = vx[i] + (double) vy[i];
        cg_store4<double, true>(xn, o, end, vx);
    }
}

// MODE 0: r64 = b, x = 0 is written; 1: r64 = b - q64 with q64 = A x0; 2: the same with q64 = A xn, <b,b> not formed again.  r = narrow(r64),
// z = Dinv .* r; the partials of <r64,r64>, of <r,z> (into the array iteration k + 1 reads the old sum from), of <r,r> and, at the start, of <b,b>
template <bool WIDE, bool DINV, int MODE>
__global__ __launch_bounds__(kBlock) void mix_residual_kernel(int m, long long span, int k, const double *__restrict__ b, double *x, const double *__restrict__ q64,
                                                              const float *__restrict__ dinv, float *__restrict__ r, double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double s_own[4][kBlock / kWave];
    const auto [begin, end] = cg_range(m, span);
    double tt[4] = {0, 0, 0, 0}, rz[4] = {0, 0, 0, 0}, rr[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        double vb[4], v64[4];
        float vr[4], vz[4];
        cg_load4<double, WIDE>(b, o, end, vb);
        if (MODE != 0) {
            double vq[4];
            cg_load4<double, true>(q64, o, end, vq);
#pragma unroll
            for (int i = 0; i < 4; ++i) v64[i] = vb[i] - vq[i];
        } else {
            const double zero[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) v64[i] = vb[i];
            cg_store4<double, WIDE>(x, o, end, zero);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) vr[i] = (float) v64[i];
        cg_precondition4<float, WIDE, DINV>(dinv, o, end, vr, vz);
        cg_store4<float, true>(r, o, end, vr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tt[i] += v64[i] * v64[i];
            rz[i] += (double) vr[i] * (double) vz[i];
            rr[i] += (double) vr[i] * (double) vr[i];
            if (MODE != 2) bb[i] += vb[i] * vb[i];
        }
    }
    double own[4] = {cg_thread_sum(tt), cg_thread_sum(rz), cg_thread_sum(rr), cg_thread_sum(bb)};
    cg_block_tree<4>(own, s_own);
    if (threadIdx.x == 0) {
        part[(size_t) kMixPartTrue * kCgMaxParts + blockIdx.x] = own[0];
        part[(size_t) (k & 1 ? kCgPartRZ1 : kCgPartRZ0) * kCgMaxParts + blockIdx.x] = own[1];
        part[(size_t) kCgPartRR * kCgMaxParts + blockIdx.x] = own[2];
        if (MODE != 2) part[(size_t) kCgPartBB * kCgMaxParts + blockIdx.x] = own[3];
    }
}

// The decision behind mix_residual, taken by every workgroup from the same sums.  START: the tests of a solve's start on x0.  Otherwise the
// update behind iteration k: a non-finite <r64,r64>, or one that did not fall although the segment ended "exact", "estimate" or "drop", ends
// the solve with x, rr and updates as they were; else x = xn is committed as update number `update`.  Behind a commit (or the start):
// converged, the budget, the tests of the next segment's start, in this order; when none ends the solve the loop is re-armed, y = 0, and
// p = z at the start and behind a segment that ended "exact".
template <bool WIDE, bool DINV, bool START>
__global__ __launch_bounds__(kBlock) void mix_resume_kernel(int m, long long span, int k, int update, int budget, const double *__restrict__ xn, double *x, const float *__restrict__ r,
                                                            const float *__restrict__ dinv, float *__restrict__ p, float *__restrict__ y, const double *__restrict__ part, MixState *st,
                                                            double *__restrict__ hist, double rtol2, double atol2, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[4][kBlock / kWave];
    const int ids[4] = {kMixPartTrue, k & 1 ? kCgPartRZ1 : kCgPartRZ0, kCgPartRR, kCgPartBB};
    double v[4];
    cg_final_sums<4>(part, ids, v, s_fin);
    const double rz = v[1], rs = v[2], bb = v[3], thr = __builtin_fmax(rtol2 * bb, atol2);
    double rr = v[0];
    int status = -1;
    bool commit = true, fresh = START;
    if (!nostop) {
        if (START) {
            if (!cg_finite(bb) || !cg_finite(rr)) status = 3;
            else if (bb == 0) { status = 0; rr = 0; } // the solution is x = 0: the host zeroes X
        } else {
            const int reason = st->u_reason; // mix_try's copies: the same in every wave
            if (!cg_finite(rr)) { status = 3; commit = false; }
            else if (reason <= kMixEndDrop && rr >= st->u_rr) { status = 4; commit = false; }
            fresh = reason == kMixEndExact;
        }
        if (status < 0) {
            if (rr <= thr) status = 0;
            else if (k == budget) status = 1;
            else if (!cg_finite(rs) || !cg_finite(rz)) status = 3;
            else if (rs == 0) status = 4;
            else if (rz <= 0) status = 2;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (START) st->s.bb = bb;
        if (commit) {
            st->s.rr = rr;
            if (hist) hist[k] = rr;
            if (!START) st->updates = update;
        }
        st->segment_end = 0;
        if (status >= 0) {
            st->s.status = status;
            st->s.end_update = st->s.end_direction = 1;
        } else {
            st->s.end_update = st->s.end_direction = 0;
            st->seg = rs;
            st->seg_first = k;
            st->thr = thr;
        }
    }
    if (!commit || (START && status >= 0)) return;
    fresh = fresh && status < 0;
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    const auto [begin, end] = cg_range(m, span);
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        if (!START) {
            double vx[4];
            cg_load4<double, true>(xn, o, end, vx);
            cg_store4<double, WIDE>(x, o, end, vx);
        }
        cg_store4<float, true>(y, o, end, zero);
        if (fresh) {
            float vr[4], vz[4];
            cg_load4<float, true>(r, o, end, vr);
            cg_precondition4<float, WIDE, DINV>(dinv, o, end, vr, vz);
            cg_store4<float, true>(p, o, end, vz);
        }
    }
}

// iteration k: cg_direction's tests on the sums cg_update left, with <r,r> = 0 ending the segment "exact" (p untouched); then beta rounded to float
// once and p = z + beta p; then the tests that end the segment with the new p in place: "estimate", "drop", "every", "budget".  Block 0 writes
// the state (and the history: the recurrence's <r,r>)
template <bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void mix_direction_kernel(int m, long long span, int k, const float *__restrict__ r, const float *__restrict__ dinv, float *__restrict__ p,
                                                               const double *__restrict__ part, MixState *st, double *__restrict__ hist, double drop2, int every, int budget, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[3][kBlock / kWave];
    if (st->s.end_update) { // written by cg_update, this iteration's or an earlier one's: the same in every wave
        if (blockIdx.x == 0 && threadIdx.x == 0) st->s.end_direction = 1;
        return;
    }
    const int ids[3] = {k & 1 ? kCgPartRZ1 : kCgPartRZ0, (k - 1) & 1 ? kCgPartRZ1 : kCgPartRZ0, kCgPartRR};
    double v[3];
    cg_final_sums<3>(part, ids, v, s_fin);
    const double rz = v[0], rs = v[2];
    const float beta = (float) (rz / v[1]);
    int status = -1, reason = 0;
    if (!nostop) {
        if (!cg_finite(rs) || !cg_finite(rz)) status = 3;
        else if (rs == 0) reason = kMixEndExact;
        else if (rz <= 0) status = 2;
        else if (!cg_finite((double) beta)) status = 3;
        else if (rs <= st->thr) reason = kMixEndEstimate;
        else if (rs <= drop2 * st->seg) reason = kMixEndDrop;
        else if (every > 0 && k - st->seg_first == every) reason = kMixEndEvery;
        else if (k == budget) reason = kMixEndBudget;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->s.iterations = k;
        if (hist) hist[k] = rs;
        if (status >= 0) st->s.status = status;
        else if (reason) st->segment_end = reason;
        if (status >= 0 || reason) st->s.end_direction = 1;
    }
    if (status >= 0 || reason == kMixEndExact) return;
    const auto [begin, end] = cg_range(m, span);
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        float vr[4], vp[4], vz[4];
        cg_load4<float, true>(r, o, end, vr);
        cg_load4<float, true>(p, o, end, vp);
        cg_precondition4<float, WIDE, DINV>(dinv, o, end, vr, vz);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float bp = beta * vp[i];
            vp[i] = vz[i] + bp;
        }
        cg_store4<float, true>(p, o, end, vp);
    }
}

} // namespace spmv
