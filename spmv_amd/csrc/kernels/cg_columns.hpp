// cg_columns.hpp -- the vector kernels of spmv_hip_cg_columns: conjugate gradients for k INDEPENDENT right-hand sides (1 <= k <= kCcgMaxK) that
// share one pass over A per iteration.  B and X are m x k, row-major with leading dimensions; the workspace vectors r, p and q are COMPACT
// (ld = k).  One iteration is q = A p for all k columns (spmv_hip_spmm's executor) followed by
//
//   ccg_dot        grid P   reads p, q                  leaves the partials of <p,q>, one per workgroup and column
//   ccg_alpha      grid k   reads those partials         column c's alpha, its tests, end_update[c]
//   ccg_update     grid P   reads p, q, x, r, (Dinv)    x += alpha p, r -= alpha q per live column; the partials of <r,z> and <r,r>
//   ccg_beta       grid k   reads those partials         column c's beta, stop test, iterations, rr, history, end_direction[c]
//   ccg_direction  grid P   reads r, (Dinv), p          p = z + beta p per live column
//
// Column c of a call is spmv_hip_cg's recurrence word for word (kernels/cg.hpp): the same updates in the same order, the same tests in the same
// order, alpha and beta fp64 quotients rounded to T once.  Hand-off between workgroups is the kernel boundary and nothing else, as there: no
// atomics, no flags, no fences, no spinning, no cooperative launch.  What differs from cg.hpp is WHO finishes a dot: with k columns "every
// workgroup re-adds the partials" would read up to 3 k arrays of 8 KiB per workgroup out of L2, so one workgroup per column finishes that
// column's sums in a small launch of its own (ccg_begin / ccg_alpha / ccg_beta) and leaves alpha / beta in the state for the next launch --
// also a kernel-boundary hand-off, with the bits of cg_final_sums.
//
// The state (ColsState): per-column arrays.  No kernel reads a word that its own launch writes: end_direction[] is written by ccg_begin and
// ccg_beta and read by ccg_dot and ccg_alpha; end_update[] and alpha[] are written by ccg_alpha and read by ccg_update and ccg_beta; beta[] is
// written by ccg_beta and read by ccg_direction; <r,z> alternates between rz[0] and rz[1] (iteration it reads (it - 1) & 1 and writes it & 1).
// A column whose word is set is FROZEN: its x, r and p elements are stored back as they were loaded or not stored at all, its status,
// iterations and rr are not written again; a vector kernel returns at once when every column's word is set.  A frozen column is still
// multiplied (spmm runs all k); its q is ignored.
//
// The order of a column's dot is solve_common.hpp's over that column's m elements by ROW: one fp64 accumulator per (row position in the 1024-row
// step, column), ascending step, then (a0 + a1) + (a2 + a3) over the four positions 4u .. 4u + 3, the wave tree over 64 such sums, (w0 + w1) +
// (w2 + w3).  The lane mapping is another one: a step's rows 256 g .. 256 g + 255 (what wave g of cg.hpp owns) are 256 k contiguous elements
// of a compact vector, read by all 256 threads in flat order with 16-byte accesses -- thread t holds the elements 4 (256 i + t) .. + 3, i <
// kCcgSlots -- so each (position, column) keeps one lane and register through all steps; per g the accumulators go through LDS once
// (column-major, kCcgLd doubles per column) and wave w adds the columns w, w + 4, ... in the contract's tree.
#pragma once
#include "solve_common.hpp"

namespace spmv {

constexpr int kCcgMaxK = 16;            // SPMV_HIP_CG_COLUMNS_MAX
constexpr int kCcgSlots = kCcgMaxK / 4; // 16-byte groups of 4 flat elements a thread holds of one 256-row block
constexpr int kCcgRows = kCgChunk / 4;  // rows of a block: one wave's share of a step in cg.hpp
constexpr int kCcgLd = kCcgRows + 2;    // LDS: doubles per column (the pad spreads the columns over the banks, 16-byte alignment kept)

enum { kCcgVecR, kCcgVecP, kCcgVecQ, kCcgVectors };
// the partial arrays: array (a, column c) is entry a * k + c of kCgMaxParts doubles; entries behind the P in use stay +0.0 from the allocation on
enum { kCcgPartPQ, kCcgPartRZ, kCcgPartRR, kCcgPartBB, kCcgPartArrays };

struct ColsState {
    int end_update[kCcgMaxK], end_direction[kCcgMaxK];
    int status[kCcgMaxK], iterations[kCcgMaxK];
    double rr[kCcgMaxK], bb[kCcgMaxK];
    double rz[2][kCcgMaxK];
    double alpha[kCcgMaxK], beta[kCcgMaxK]; // already rounded to T
};

// spmv_solve.hip
hipError_t ccg_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream);  // ccg_init + ccg_begin; q holds A x0 when use_x0
hipError_t ccg_iteration_launch(const SolveArgs &a, int it, hipStream_t stream);   // the five kernels of iteration it >= 1; q holds A p

// true when the first k words are all set (an earlier launch's words: the same in every wave)
__device__ __forceinline__ bool ccg_all(const int *ended, int k)
{
    int all = 1;
    for (int c = 0; c < k; ++c) all &= ended[c] != 0;
    return all != 0;
}

// where a thread's elements of a 256-row block are: rc[i][e] = row in the block | column << 16 of flat element 4 (256 i + t) + e
struct CcgMap {
    int rc[kCcgSlots][4];
    int k, flat; // flat: this thread's first flat element of slot 0
    __device__ __forceinline__ explicit CcgMap(int kk) : k(kk), flat(4 * (int) threadIdx.x)
    {
#pragma unroll
        for (int i = 0; i < kCcgSlots; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int f = flat + 4 * kBlock * i + e;
                rc[i][e] = (f / k) | ((f % k) << 16);
            }
    }
    __device__ __forceinline__ bool have(int i) const { return flat + 4 * kBlock * i < kCcgRows * k; } // all 4 elements or none: 256 k is a multiple of 4
    __device__ __forceinline__ int row(int i, int e) const { return rc[i][e] & 0xffff; }
    __device__ __forceinline__ int col(int i, int e) const { return rc[i][e] >> 16; }
};

// the thread's 4 elements of slot i of the block that starts at row r0: from a compact vector (WIDE: index r0 k + flat, 16-byte accesses) or
// from the caller's array with leading dimension ld (element accesses); rows >= end read as 0
template <typename T, bool WIDE>
__device__ __forceinline__ void ccg_load4(const T *__restrict__ a, long long ld, long long r0, long long end, const CcgMap &mp, int i, T (&v)[4])
{
    if (WIDE) {
        cg_load4<T, true>(a, r0 * mp.k + mp.flat + 4 * kBlock * i, end * mp.k, v);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long r = r0 + mp.row(i, e);
            v[e] = r < end ? a[r * ld + mp.col(i, e)] : T(0);
        }
    }
}

// ... stored; `keep` (bit e): element e is not stored in the element form (a frozen column); the wide form stores all four, the frozen ones
// with the bits they were loaded with
template <typename T, bool WIDE>
__device__ __forceinline__ void ccg_store4(T *__restrict__ a, long long ld, long long r0, long long end, const CcgMap &mp, int i, const T (&v)[4], unsigned keep)
{
    if (WIDE) {
        cg_store4<T, true>(a, r0 * mp.k + mp.flat + 4 * kBlock * i, end * mp.k, v);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long r = r0 + mp.row(i, e);
            if (r < end && !((keep >> e) & 1u)) a[r * ld + mp.col(i, e)] = v[e];
        }
    }
}

// vz = Dinv[row] * vr for the thread's 4 elements of slot i, or vz = vr
template <typename T, bool DINV>
__device__ __forceinline__ void ccg_precondition4(const T *__restrict__ dinv, long long r0, long long end, const CcgMap &mp, int i, const T (&vr)[4], T (&vz)[4])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (DINV) {
            const long long r = r0 + mp.row(i, e);
            const T dv = r < end ? dinv[r] : T(0);
            vz[e] = dv * vr[e];
        } else {
            vz[e] = vr[e];
        }
    }
}

// block g's accumulators -> the k sums of wave g in cg.hpp's tree, into s_w[c][g].  s_t: kCcgMaxK * kCcgLd doubles, used again by every call
__device__ __forceinline__ void ccg_wave_tree(const double (&acc)[kCcgSlots][4], const CcgMap &mp, int g, double *s_t, double (*s_w)[kBlock / kWave])
{
#pragma clang fp contract(off)
    __syncthreads(); // the call before this one has read s_t
#pragma unroll
    for (int i = 0; i < kCcgSlots; ++i)
        if (mp.have(i))
#pragma unroll
            for (int e = 0; e < 4; ++e) s_t[mp.col(i, e) * kCcgLd + mp.row(i, e)] = acc[i][e];
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int c = wave; c < mp.k; c += kBlock / kWave) { // wave-uniform
        const double *a = s_t + c * kCcgLd + 4 * lane;
        double v = (a[0] + a[1]) + (a[2] + a[3]);
        v = group_sum_dpp<kWave>(v);
        if (lane == 0) s_w[c][g] = v;
    }
}

// the four wave sums of every column -> the workgroup's partial of array `id`
__device__ __forceinline__ void ccg_leave_partials(double (*s_w)[kBlock / kWave], int k, int id, double *__restrict__ part)
{
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    if (c < k) part[((size_t) id * k + c) * kCgMaxParts + blockIdx.x] = (s_w[c][0] + s_w[c][1]) + (s_w[c][2] + s_w[c][3]);
}

// r = b (x = 0 is written) or r = b - q with q = A x0; p = z = Dinv .* r; the partials of <r,z>, <r,r> and <b,b> of every column
template <typename T, bool WIDE, bool DINV, bool X0>
__global__ __launch_bounds__(kBlock) void ccg_init_kernel(int m, long long span, int k, const T *__restrict__ b, long long ldb, T *x, long long ldx, const T *__restrict__ q,
                                                          const T *__restrict__ dinv, T *__restrict__ r, T *__restrict__ p, double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double s_t[kCcgMaxK * kCcgLd];
    __shared__ double s_rz[kCcgMaxK][kBlock / kWave], s_rr[kCcgMaxK][kBlock / kWave], s_bb[kCcgMaxK][kBlock / kWave];
    const auto [begin, end] = cg_range(m, span);
    const CcgMap mp(k);
    for (int g = 0; g < kBlock / kWave; ++g) {
        double rz[kCcgSlots][4] = {}, rr[kCcgSlots][4] = {}, bb[kCcgSlots][4] = {};
        for (long long r0 = begin + kCcgRows * g; r0 < end; r0 += kCgChunk) {
#pragma unroll
            for (int i = 0; i < kCcgSlots; ++i) {
                if (!mp.have(i)) continue;
                T vb[4], vr[4], vz[4];
                ccg_load4<T, WIDE>(b, ldb, r0, end, mp, i, vb);
                if (X0) {
                    T vq[4];
                    ccg_load4<T, true>(q, k, r0, end, mp, i, vq);
#pragma unroll
                    for (int e = 0; e < 4; ++e) vr[e] = vb[e] - vq[e];
                } else {
                    const T zero[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
                    for (int e = 0; e < 4; ++e) vr[e] = vb[e];
                    ccg_store4<T, WIDE>(x, ldx, r0, end, mp, i, zero, 0u);
                }
                ccg_precondition4<T, DINV>(dinv, r0, end, mp, i, vr, vz);
                ccg_store4<T, true>(r, k, r0, end, mp, i, vr, 0u);
                ccg_store4<T, true>(p, k, r0, end, mp, i, vz, 0u);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    rz[i][e] += (double) vr[e] * (double) vz[e];
                    rr[i][e] += (double) vr[e] * (double) vr[e];
                    bb[i][e] += (double) vb[e] * (double) vb[e];
                }
            }
        }
        ccg_wave_tree(rz, mp, g, s_t, s_rz);
        ccg_wave_tree(rr, mp, g, s_t, s_rr);
        ccg_wave_tree(bb, mp, g, s_t, s_bb);
    }
    __syncthreads();
    ccg_leave_partials(s_rz, k, kCcgPartRZ, part);
    ccg_leave_partials(s_rr, k, kCcgPartRR, part);
    ccg_leave_partials(s_bb, k, kCcgPartBB, part);
}

// one workgroup per column: the state of iteration 0 (the host has zeroed it) from the partials ccg_init left; cg_begin_kernel's tests.  Writes
// end_direction[c]
template <bool HIST>
__global__ __launch_bounds__(kBlock) void ccg_begin_kernel(const double *__restrict__ part, int k, ColsState *st, double *__restrict__ hist, double rtol2, double atol2, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[3][kBlock / kWave];
    const int c = blockIdx.x;
    const int ids[3] = {kCcgPartRZ * k + c, kCcgPartRR * k + c, kCcgPartBB * k + c};
    double v[3];
    cg_final_sums<3>(part, ids, v, s_fin);
    if (threadIdx.x != 0) return;
    double rr = v[1];
    const double rz = v[0], bb = v[2];
    int status = -1;
    if (!nostop) {
        if (!cg_finite(bb) || !cg_finite(rr) || !cg_finite(rz)) status = 3;
        else if (bb == 0) { status = 0; rr = 0; } // the solution is x = 0: the host zeroes the column of X
        else if (rr <= __builtin_fmax(rtol2 * bb, atol2)) status = 0;
        else if (rz <= 0) status = 2;
    }
    st->iterations[c] = 0;
    st->rr[c] = rr;
    st->bb[c] = bb;
    st->rz[0][c] = rz;
    if (HIST) hist[c] = rr;
    if (status >= 0) { st->status[c] = status; st->end_direction[c] = 1; }
}

// the partials of <p,q> of every column; returns at once when every column has ended
template <typename T>
__global__ __launch_bounds__(kBlock) void ccg_dot_kernel(int m, long long span, int k, const T *__restrict__ p, const T *__restrict__ q, double *__restrict__ part, const ColsState *st)
{
#pragma clang fp contract(off)
    __shared__ double s_t[kCcgMaxK * kCcgLd];
    __shared__ double s_pq[kCcgMaxK][kBlock / kWave];
    if (ccg_all(st->end_direction, k)) return;
    const auto [begin, end] = cg_range(m, span);
    const CcgMap mp(k);
    for (int g = 0; g < kBlock / kWave; ++g) {
        double pq[kCcgSlots][4] = {};
        for (long long r0 = begin + kCcgRows * g; r0 < end; r0 += kCgChunk) {
#pragma unroll
            for (int i = 0; i < kCcgSlots; ++i) {
                if (!mp.have(i)) continue;
                T vp[4], vq[4];
                ccg_load4<T, true>(p, k, r0, end, mp, i, vp);
                ccg_load4<T, true>(q, k, r0, end, mp, i, vq);
#pragma unroll
                for (int e = 0; e < 4; ++e) pq[i][e] += (double) vp[e] * (double) vq[e];
            }
        }
        ccg_wave_tree(pq, mp, g, s_t, s_pq);
    }
    __syncthreads();
    ccg_leave_partials(s_pq, k, kCcgPartPQ, part);
}

// one workgroup per column, iteration it: alpha = <r,z>_old / <p,q> rounded to T once and cg_update_kernel's tests.  <p,q> <= 0 (breakdown) or
// a non-finite scalar: the column ends here and ccg_update does not touch it.  Writes end_update[c]
template <typename T>
__global__ __launch_bounds__(kBlock) void ccg_alpha_kernel(const double *__restrict__ part, int k, int it, ColsState *st, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[1][kBlock / kWave];
    const int c = blockIdx.x;
    if (st->end_direction[c]) { // an earlier launch's word
        if (threadIdx.x == 0) st->end_update[c] = 1;
        return;
    }
    const int ids[1] = {kCcgPartPQ * k + c};
    double v[1];
    cg_final_sums<1>(part, ids, v, s_fin);
    if (threadIdx.x != 0) return;
    const double rz = st->rz[(it - 1) & 1][c], pq = v[0];
    const double alpha64 = rz / pq;
    const T alpha = (T) alpha64;
    int status = -1;
    if (!nostop) {
        if (!cg_finite(pq) || !cg_finite(rz)) status = 3;
        else if (pq <= 0) status = 2;
        else if (!cg_finite((double) alpha)) status = 3;
    }
    if (status >= 0) { st->status[c] = status; st->end_update[c] = 1; }
    else st->alpha[c] = (double) alpha;
}

// iteration it: x = x + alpha p, r = r - alpha q in T (a multiply, then an add) for every column that has not ended; the partials of the new
// <r,z> and <r,r>
template <typename T, bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void ccg_update_kernel(int m, long long span, int k, const T *__restrict__ p, const T *__restrict__ q, T *__restrict__ x, long long ldx,
                                                            T *__restrict__ r, const T *__restrict__ dinv, double *__restrict__ part, const ColsState *st)
{
#pragma clang fp contract(off)
    __shared__ double s_t[kCcgMaxK * kCcgLd];
    __shared__ double s_rz[kCcgMaxK][kBlock / kWave], s_rr[kCcgMaxK][kBlock / kWave];
    if (ccg_all(st->end_update, k)) return;
    const auto [begin, end] = cg_range(m, span);
    const CcgMap mp(k);
    T al[kCcgSlots][4];
    unsigned frozen = 0; // bit 4 i + e
#pragma unroll
    for (int i = 0; i < kCcgSlots; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = mp.have(i) ? mp.col(i, e) : 0;
            al[i][e] = (T) st->alpha[c];
            if (st->end_update[c]) frozen |= 1u << (4 * i + e);
        }
    for (int g = 0; g < kBlock / kWave; ++g) {
        double rz[kCcgSlots][4] = {}, rr[kCcgSlots][4] = {};
        for (long long r0 = begin + kCcgRows * g; r0 < end; r0 += kCgChunk) {
#pragma unroll
            for (int i = 0; i < kCcgSlots; ++i) {
                if (!mp.have(i)) continue;
                const unsigned keep = (frozen >> (4 * i)) & 15u;
                T vp[4], vq[4], vx[4], vr[4], vz[4];
                ccg_load4<T, true>(p, k, r0, end, mp, i, vp);
                ccg_load4<T, true>(q, k, r0, end, mp, i, vq);
                ccg_load4<T, WIDE>(x, ldx, r0, end, mp, i, vx);
                ccg_load4<T, true>(r, k, r0, end, mp, i, vr);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const T ap = al[i][e] * vp[e], aq = al[i][e] * vq[e];
                    const T nx = vx[e] + ap, nr = vr[e] - aq;
                    if (!((keep >> e) & 1u)) { vx[e] = nx; vr[e] = nr; }
                }
                ccg_precondition4<T, DINV>(dinv, r0, end, mp, i, vr, vz);
                ccg_store4<T, WIDE>(x, ldx, r0, end, mp, i, vx, keep);
                ccg_store4<T, true>(r, k, r0, end, mp, i, vr, 0u);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    rz[i][e] += (double) vr[e] * (double) vz[e];
                    rr[i][e] += (double) vr[e] * (double) vr[e];
                }
            }
        }
        ccg_wave_tree(rz, mp, g, s_t, s_rz);
        ccg_wave_tree(rr, mp, g, s_t, s_rr);
    }
    __syncthreads();
    ccg_leave_partials(s_rz, k, kCcgPartRZ, part);
    ccg_leave_partials(s_rr, k, kCcgPartRR, part);
}

// one workgroup per column, iteration it: cg_direction_kernel's stop tests on the sums ccg_update left, beta = <r,z>_new / <r,z>_old rounded to T
// once; writes the column's iterations, rr and history entry.  Writes end_direction[c]
template <typename T>
__global__ __launch_bounds__(kBlock) void ccg_beta_kernel(const double *__restrict__ part, int k, int it, ColsState *st, double *__restrict__ hist, double rtol2, double atol2,
                                                          int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[2][kBlock / kWave];
    const int c = blockIdx.x;
    if (st->end_update[c]) { // written by ccg_alpha, this iteration's or an earlier one's
        if (threadIdx.x == 0) st->end_direction[c] = 1;
        return;
    }
    const int ids[2] = {kCcgPartRZ * k + c, kCcgPartRR * k + c};
    double v[2];
    cg_final_sums<2>(part, ids, v, s_fin);
    if (threadIdx.x != 0) return;
    const double rz = v[0], rr = v[1], rz_old = st->rz[(it - 1) & 1][c];
    const T beta = (T) (rz / rz_old);
    int status = -1;
    if (!nostop) {
        if (!cg_finite(rr) || !cg_finite(rz)) status = 3;
        else if (rr <= __builtin_fmax(rtol2 * st->bb[c], atol2)) status = 0;
        else if (rz <= 0) status = 2;
        else if (!cg_finite((double) beta)) status = 3;
    }
    st->iterations[c] = it;
    st->rr[c] = rr;
    st->rz[it & 1][c] = rz;
    if (hist) hist[(size_t) it * k + c] = rr;
    if (status >= 0) { st->status[c] = status; st->end_direction[c] = 1; }
    else st->beta[c] = (double) beta;
}

// iteration it: p = z + beta p in T for every column that has not ended (z recomputed from r, never stored)
template <typename T, bool DINV>
__global__ __launch_bounds__(kBlock) void ccg_direction_kernel(int m, long long span, int k, const T *__restrict__ r, const T *__restrict__ dinv, T *__restrict__ p,
                                                               const ColsState *st)
{
#pragma clang fp contract(off)
    if (ccg_all(st->end_direction, k)) return;
    const auto [begin, end] = cg_range(m, span);
    const CcgMap mp(k);
    T be[kCcgSlots][4];
    unsigned frozen = 0;
#pragma unroll
    for (int i = 0; i < kCcgSlots; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = mp.have(i) ? mp.col(i, e) : 0;
            be[i][e] = (T) st->beta[c];
            if (st->end_direction[c]) frozen |= 1u << (4 * i + e);
        }
    for (long long r0 = begin; r0 < end; r0 += kCcgRows) { // no sum here: the blocks in row order
#pragma unroll
        for (int i = 0; i < kCcgSlots; ++i) {
            if (!mp.have(i)) continue;
            T vr[4], vp[4], vz[4];
            ccg_load4<T, true>(r, k, r0, end, mp, i, vr);
            ccg_load4<T, true>(p, k, r0, end, mp, i, vp);
            ccg_precondition4<T, DINV>(dinv, r0, end, mp, i, vr, vz);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const T bp = be[i][e] * vp[e];
                const T np = vz[e] + bp;
                if (!((frozen >> (4 * i + e)) & 1u)) vp[e] = np;
            }
            ccg_store4<T, true>(p, k, r0, end, mp, i, vp, 0u);
        }
    }
}

} // namespace spmv
