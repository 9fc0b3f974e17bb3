// gmres.hpp -- the vector kernels of spmv_hip_gmres (right-preconditioned restarted GMRES(R) that stays on the device, classical Gram-Schmidt
// applied twice).  The workspace vectors are w, z and the basis v_1 .. v_(R+1); r lives in w between a restart and the scale that makes v_1.
// Behind the handle's own multiply w = A z (z = Dinv .* v_j; v_j itself without Dinv) step j of a cycle, global iteration k, is
//
//   gmres_dots      grid P   reads v_1..v_j, w          the partials of c_i = <v_i,w>, G basis vectors per trip over the workgroup's range
//   gmres_coeffs    grid j   reads those partials        workgroup i finishes c_i; a_i = T(c_i) into the state
//   gmres_sub_dots  grid P   reads v_1..v_j, w, a        w -= a_i v_i by ascending i; off the new w the partials of d_i = <v_i,w>
//   gmres_coeffs    grid j                               e_i = T(d_i)
//   gmres_sub_norm  grid P   reads v_1..v_j, w, e        w -= e_i v_i; the partials of <w,w>
//   gmres_rotate    grid 1   reads the state             the Hessenberg column, the rotations, g, the tests, the history; writes end_half
//   gmres_scale     grid P   reads w                     v_(j+1) = w * T(1 / hn); z = Dinv .* v_(j+1); passes an end on into end_update
//
// and at j = R the cycle ends and the next one starts:
//
//   gmres_solve     grid 1, one thread                   R y = g by back substitution
//   gmres_update_x  grid P   reads v_1..v_j, x, (Dinv)   u = sum y_i v_i, x = x + Dinv .* u
//   (w = A x)
//   gmres_residual  grid P   reads b, w                  r = b - w into w; the partials of <r,r>
//   gmres_cycle     grid 1                               beta = sqrt(<r,r>), g_1, 1 / beta, pending = 0; its tests; writes end_direction
//   gmres_scale                                          v_1 = r * T(1 / beta)
//
// Hand-off between workgroups is the kernel boundary and nothing else: no atomics, no in-launch flags, no fences, no spinning, no cooperative
// launch.  A thread of gmres_sub_dots reads again elements of w that IT has written, nothing another thread has.
//
// The state (GmresState, which begins with the SolveState the host's look reads): no kernel reads a word that its own launch writes.
//   end_direction  written by cg_begin and gmres_cycle   read by gmres_scale
//   end_half       written by gmres_rotate               read by gmres_scale, gmres_solve, gmres_update_x, gmres_residual, gmres_cycle
//   end_update     written by gmres_scale                read by gmres_dots, gmres_coeffs, gmres_sub_dots, gmres_sub_norm, gmres_rotate
// A kernel that finds the word it reads set passes the end on in the word it writes and returns, so from the launch that ends the loop on
// every later kernel of the batch returns at once.  `pending` counts the columns of the running cycle that x does not hold yet: gmres_rotate
// sets it to j when step j is applied, gmres_cycle to 0.  When the loop ends or the budget runs out with pending > 0 the host enqueues
// gmres_solve and gmres_update_x once more with `force` set: they ignore the end word and apply those columns.
//
// The order of a dot is solve_common.hpp's; every product, sum, quotient and square root is a separate operation: contraction is off in every
// function of this file AND spmv_solve.hip is compiled with -ffp-contract=off.
#pragma once
#include "solve_common.hpp"

namespace spmv {

constexpr int kGmresMaxRestart = 32; // SPMV_HIP_GMRES_RESTART_MAX
constexpr int kGmresGroup = 8;       // G: basis vectors per trip of gmres_dots: 8 G accumulator VGPRs; measured against 4

// the workspace vectors: SolveArgs::base + i * SolveArgs::stride; v_i (i >= 1) is vector kGmresVecV + i - 1
enum { kGmresVecW, kGmresVecZ, kGmresVecV, kGmresVectors = kGmresVecV + 1 }; // + restart
// the partial arrays: <v_i,w> in array i - 1; entries behind the P in use stay +0.0 from the allocation on
enum { kGmresPartWW = kGmresMaxRestart, kGmresPartRR, kGmresPartBB, kGmresPartArrays };

struct GmresState {
    SolveState s;                                   // what the host's look reads; s.rr: the estimate g_(j+1)^2 of the last step applied
    int pending;                                    // columns of the running cycle not yet in x
    int pad;
    double scale;                                   // 1 / beta or 1 / hn: what gmres_scale rounds to T
    double coef[2][kGmresMaxRestart];               // a_i and e_i, already rounded to T
    double c[kGmresMaxRestart], sn[kGmresMaxRestart]; // the rotations
    double g[kGmresMaxRestart + 1];
    double y[kGmresMaxRestart];                     // already rounded to T
    double r[kGmresMaxRestart][kGmresMaxRestart];   // r[col][row]: the rotated Hessenberg columns
};
constexpr size_t kGmresStateRoom = 10240;

// spmv_solve.hip
hipError_t gmres_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream);  // gmres_init + cg_begin + gmres_cycle + gmres_scale; w holds A x0 when use_x0
hipError_t gmres_step_launch(const SolveArgs &a, int k, int j, hipStream_t stream);  // step j of a cycle, iteration k >= 1; w holds A z
hipError_t gmres_apply_launch(const SolveArgs &a, int force, hipStream_t stream);    // gmres_solve + gmres_update_x
hipError_t gmres_restart_launch(const SolveArgs &a, hipStream_t stream);             // gmres_residual + gmres_cycle + gmres_scale; w holds A x
hipError_t gmres_sqrt_launch(const double *in, double *out, long long n, hipStream_t stream);

template <typename T>
__device__ __forceinline__ const T *gmres_v(const char *base, size_t stride, int i) { return reinterpret_cast<const T *>(base + (size_t) (kGmresVecV + i) * stride); }

// r = b (x = 0 is written) or r = b - w with w = A x0, into w; the partials of <r,r> and <b,b>
template <typename T, bool WIDE, bool X0>
__global__ __launch_bounds__(kBlock) void gmres_init_kernel(int m, long long span, const T *__restrict__ b, T *__restrict__ x, T *__restrict__ w, double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double s_own[2][kBlock / kWave];
    const auto [begin, end] = cg_range(m, span);
    double rr[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vb[4], vr[4];
        cg_load4<T, WIDE>(b, o, end, vb);
        if (X0) {
            T vw[4];
            cg_load4<T, true>(w, o, end, vw);
#pragma unroll
            for (int i = 0; i < 4; ++i) vr[i] = vb[i] - vw[i];
        } else {
            const T zero[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
            for (int i = 0; i < 4; ++i) vr[i] = vb[i];
            cg_store4<T, WIDE>(x, o, end, zero);
        }
        cg_store4<T, true>(w, o, end, vr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rr[i] += (double) vr[i] * (double) vr[i];
            bb[i] += (double) vb[i] * (double) vb[i];
        }
    }
    double own[2] = {cg_thread_sum(rr), cg_thread_sum(bb)};
    cg_block_tree<2>(own, s_own);
    if (threadIdx.x == 0) {
        part[(size_t) kGmresPartRR * kCgMaxParts + blockIdx.x] = own[0];
        part[(size_t) kGmresPartBB * kCgMaxParts + blockIdx.x] = own[1];
    }
}

// one workgroup: a cycle starts from the partials of <r,r>.  RESTART: the tests of a restart (at the start cg_begin has made them)
template <bool RESTART>
__global__ __launch_bounds__(kBlock) void gmres_cycle_kernel(const double *__restrict__ part, GmresState *st, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[1][kBlock / kWave];
    if (st->s.end_half) { // gmres_rotate's word: the columns it left pending are the host's to apply
        if (threadIdx.x == 0) st->s.end_direction = 1;
        return;
    }
    const int ids[1] = {kGmresPartRR};
    double v[1];
    cg_final_sums<1>(part, ids, v, s_fin);
    if (threadIdx.x != 0) return;
    const double rr = v[0];
    st->pending = 0;
    if (RESTART && !nostop) {
        int status = -1;
        if (!cg_finite(rr)) status = 3;
        else if (rr == 0) status = 0;
        if (status >= 0) { st->s.status = status; st->s.end_direction = 1; return; }
    }
    const double beta = __builtin_sqrt(rr);
    st->g[0] = beta;
    st->scale = 1.0 / beta;
}

// v_next = w * T(scale); z = Dinv .* v_next
template <typename T, bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void gmres_scale_kernel(int m, long long span, const T *__restrict__ w, T *__restrict__ v, const T *__restrict__ dinv, T *__restrict__ z,
                                                             GmresState *st)
{
#pragma clang fp contract(off)
    if (st->s.end_direction || st->s.end_half) { // earlier launches' words: the same in every wave
        if (blockIdx.x == 0 && threadIdx.x == 0) st->s.end_update = 1;
        return;
    }
    const T t = (T) st->scale;
    const auto [begin, end] = cg_range(m, span);
#pragma unroll 2
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vw[4], vz[4];
        cg_load4<T, true>(w, o, end, vw);
#pragma unroll
        for (int i = 0; i < 4; ++i) vw[i] = vw[i] * t;
        cg_store4<T, true>(v, o, end, vw);
        if (DINV) {
            cg_precondition4<T, WIDE, true>(dinv, o, end, vw, vz);
            cg_store4<T, true>(z, o, end, vz);
        }
    }
}

// w = w - coef_i v_i for i < j by ascending i at the 4 elements from `o`: a multiply, then a subtraction, in T
template <typename T>
__device__ __forceinline__ void gmres_sub4(const char *base, size_t stride, int j, const double *coef, long long o, long long end, T (&vw)[4])
{
#pragma clang fp contract(off)
    for (int i = 0; i < j; ++i) {
        const T a = (T) coef[i];
        T vv[4];
        cg_load4<T, true>(gmres_v<T>(base, stride, i), o, end, vv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const T av = a * vv[e];
            vw[e] = vw[e] - av;
        }
    }
}

// The partials of <v_i,w> for i < j, G basis vectors per trip over the workgroup's range (w is read again per trip): 4 G fp64 accumulators per
// thread, in the (thread, slot, step) order of the contract.  SUB: the first trip forms w = w - sum coef_i v_i before it multiplies, and
// stores it; the later trips read what this thread stored
template <typename T, int G, bool SUB>
__device__ __forceinline__ void gmres_dots_body(int m, long long span, const char *base, size_t stride, T *w, int j, const double *coef, double *__restrict__ part,
                                                double (*s_own)[kBlock / kWave])
{
#pragma clang fp contract(off)
    const auto [begin, end] = cg_range(m, span);
    for (int g0 = 0; g0 < j; g0 += G) {
        const int cnt = j - g0 < G ? j - g0 : G;
        double acc[G][4];
#pragma unroll
        for (int n = 0; n < G; ++n)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[n][e] = 0;
        for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
            T vw[4];
            cg_load4<T, true>((const T *) w, o, end, vw);
            if (SUB && g0 == 0) {
                gmres_sub4<T>(base, stride, j, coef, o, end, vw);
                cg_store4<T, true>(w, o, end, vw);
            }
#pragma unroll
            for (int n = 0; n < G; ++n) {
                if (n < cnt) { // uniform over the launch
                    T vv[4];
                    cg_load4<T, true>(gmres_v<T>(base, stride, g0 + n), o, end, vv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[n][e] += (double) vv[e] * (double) vw[e];
                }
            }
        }
        double own[G];
#pragma unroll
        for (int n = 0; n < G; ++n) own[n] = cg_thread_sum(acc[n]);
        if (g0 > 0) __syncthreads(); // the trip before this one has read s_own
        cg_block_tree<G>(own, s_own);
        if (threadIdx.x == 0)
#pragma unroll
            for (int n = 0; n < G; ++n)
                if (n < cnt) part[(size_t) (g0 + n) * kCgMaxParts + blockIdx.x] = own[n];
    }
}

template <typename T, int G>
__global__ __launch_bounds__(kBlock) void gmres_dots_kernel(int m, long long span, const char *base, size_t stride, int j, double *__restrict__ part, const GmresState *st)
{
    __shared__ double s_own[G][kBlock / kWave];
    if (st->s.end_update) return;
    gmres_dots_body<T, G, false>(m, span, base, stride, (T *) (base + (size_t) kGmresVecW * stride), j, nullptr, part, s_own);
}

template <typename T, int G>
__global__ __launch_bounds__(kBlock) void gmres_sub_dots_kernel(int m, long long span, char *base, size_t stride, int j, double *__restrict__ part, const GmresState *st)
{
    __shared__ double s_own[G][kBlock / kWave];
    if (st->s.end_update) return;
    gmres_dots_body<T, G, true>(m, span, base, stride, (T *) (base + (size_t) kGmresVecW * stride), j, st->coef[0], part, s_own);
}

// workgroup i finishes the sum of partial array i and leaves it, rounded to T, in coef[pass][i]
template <typename T>
__global__ __launch_bounds__(kBlock) void gmres_coeffs_kernel(const double *__restrict__ part, GmresState *st, int pass)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[1][kBlock / kWave];
    if (st->s.end_update) return;
    const int ids[1] = {(int) blockIdx.x};
    double v[1];
    cg_final_sums<1>(part, ids, v, s_fin);
    if (threadIdx.x == 0) st->coef[pass][blockIdx.x] = (double) (T) v[0];
}

// w = w - e_i v_i by ascending i; the partials of <w,w>
template <typename T>
__global__ __launch_bounds__(kBlock) void gmres_sub_norm_kernel(int m, long long span, char *base, size_t stride, int j, double *__restrict__ part, const GmresState *st)
{
#pragma clang fp contract(off)
    __shared__ double s_own[1][kBlock / kWave];
    if (st->s.end_update) return;
    T *w = (T *) (base + (size_t) kGmresVecW * stride);
    const auto [begin, end] = cg_range(m, span);
    double ww[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vw[4];
        cg_load4<T, true>((const T *) w, o, end, vw);
        gmres_sub4<T>(base, stride, j, st->coef[1], o, end, vw);
        cg_store4<T, true>(w, o, end, vw);
#pragma unroll
        for (int e = 0; e < 4; ++e) ww[e] += (double) vw[e] * (double) vw[e];
    }
    double own[1] = {cg_thread_sum(ww)};
    cg_block_tree<1>(own, s_own);
    if (threadIdx.x == 0) part[(size_t) kGmresPartWW * kCgMaxParts + blockIdx.x] = own[0];
}

// one workgroup finishes <w,w>; its thread 0 then does step j's scalar work (include/spmv_hip.h has the order): h_i = a_i + e_i, the earlier
// rotations, the new one, g, the tests.  An applied step leaves its column, its rotation, g, pending = j, iterations = k, rr = history[k] = est
template <bool HIST>
__global__ __launch_bounds__(kBlock) void gmres_rotate_kernel(const double *__restrict__ part, GmresState *st, int k, int j, double *__restrict__ hist, double rtol2,
                                                              double atol2, int nostop)
{
#pragma clang fp contract(off)
    __shared__ double s_fin[1][kBlock / kWave];
    if (st->s.end_update) { // gmres_scale's word
        if (threadIdx.x == 0) st->s.end_half = 1;
        return;
    }
    const int ids[1] = {kGmresPartWW};
    double v[1];
    cg_final_sums<1>(part, ids, v, s_fin);
    if (threadIdx.x != 0) return;
    const double ww = v[0], hn = __builtin_sqrt(ww);
    double *h = st->r[j - 1];
    bool finite = cg_finite(ww);
    for (int i = 0; i < j; ++i) {
        h[i] = st->coef[0][i] + st->coef[1][i];
        finite = finite && cg_finite(h[i]);
    }
    for (int i = 0; i + 1 < j; ++i) {
        const double c = st->c[i], s = st->sn[i], hi = h[i], hk = h[i + 1];
        const double t1 = c * hi, t2 = s * hk, t3 = s * hi, t4 = c * hk;
        h[i] = t1 + t2;
        h[i + 1] = t4 - t3;
        finite = finite && cg_finite(h[i]) && cg_finite(h[i + 1]);
    }
    const double hj = h[j - 1], hh = hj * hj, nn = hn * hn, sum = hh + nn, d = __builtin_sqrt(sum);
    finite = finite && cg_finite(d);
    int status = -1;
    if (!nostop) {
        if (!finite) status = 3;
        else if (d == 0) status = 2;
    }
    const double c = hj / d, s = hn / d, gj = st->g[j - 1], sg = s * gj, gn = -sg, gc = c * gj, est = gn * gn;
    if (!nostop && status < 0 && !(cg_finite(c) && cg_finite(s) && cg_finite(gc) && cg_finite(est))) status = 3;
    if (status >= 0) { // the step is not applied: x will be the iterate of the step before
        st->s.status = status;
        st->s.end_half = 1;
        return;
    }
    h[j - 1] = d;
    st->c[j - 1] = c;
    st->sn[j - 1] = s;
    st->g[j - 1] = gc;
    st->g[j] = gn;
    st->scale = 1.0 / hn;
    st->pending = j;
    st->s.iterations = k;
    st->s.rr = est;
    if (HIST) hist[k] = est;
    if (nostop) return;
    if (est <= __builtin_fmax(rtol2 * st->s.bb, atol2)) status = 0;
    else if (hn == 0) status = 2; // the space is exhausted and the estimate has not met the test: A Dinv is singular
    if (status >= 0) { st->s.status = status; st->s.end_half = 1; }
}

// one thread: R y = g over the pending columns, last row first, each row's sum from +0.0 by ascending column; y rounded to T for the update
template <typename T>
__global__ void gmres_solve_kernel(GmresState *st, int force)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0 || (!force && st->s.end_half)) return;
    const int n = st->pending;
    double y[kGmresMaxRestart];
    for (int i = n - 1; i >= 0; --i) {
        double sum = 0;
        for (int c = i + 1; c < n; ++c) {
            const double p = st->r[c][i] * y[c];
            sum = sum + p;
        }
        const double rest = st->g[i] - sum;
        y[i] = rest / st->r[i][i];
        st->y[i] = (double) (T) y[i];
    }
}

// u = y_1 v_1, then u = u + y_i v_i by ascending i; x = x + Dinv .* u.  u stays in registers
template <typename T, bool WIDE, bool DINV>
__global__ __launch_bounds__(kBlock) void gmres_update_x_kernel(int m, long long span, const char *base, size_t stride, T *__restrict__ x, const T *__restrict__ dinv,
                                                                const GmresState *st, int force)
{
#pragma clang fp contract(off)
    if (!force && st->s.end_half) return;
    const int n = st->pending;
    if (n <= 0) return;
    const auto [begin, end] = cg_range(m, span);
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vu[4], vx[4], vd[4];
        for (int i = 0; i < n; ++i) {
            const T y = (T) st->y[i];
            T vv[4];
            cg_load4<T, true>(gmres_v<T>(base, stride, i), o, end, vv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const T yv = y * vv[e];
                vu[e] = i == 0 ? yv : vu[e] + yv;
            }
        }
        cg_precondition4<T, WIDE, DINV>(dinv, o, end, vu, vd);
        cg_load4<T, WIDE>((const T *) x, o, end, vx);
#pragma unroll
        for (int e = 0; e < 4; ++e) vx[e] = vx[e] + vd[e];
        cg_store4<T, WIDE>(x, o, end, vx);
    }
}

// r = b - w with w = A x, into w; the partials of <r,r>
template <typename T, bool WIDE>
__global__ __launch_bounds__(kBlock) void gmres_residual_kernel(int m, long long span, const T *__restrict__ b, T *__restrict__ w, double *__restrict__ part, const GmresState *st)
{
#pragma clang fp contract(off)
    __shared__ double s_own[1][kBlock / kWave];
    if (st->s.end_half) return;
    const auto [begin, end] = cg_range(m, span);
    double rr[4] = {0, 0, 0, 0};
    for (long long o = begin + 4 * threadIdx.x; o < end; o += kCgChunk) {
        T vb[4], vw[4];
        cg_load4<T, WIDE>(b, o, end, vb);
        cg_load4<T, true>((const T *) w, o, end, vw);
#pragma unroll
        for (int i = 0; i < 4; ++i) vw[i] = vb[i] - vw[i];
        cg_store4<T, true>(w, o, end, vw);
#pragma unroll
        for (int i = 0; i < 4; ++i) rr[i] += (double) vw[i] * (double) vw[i];
    }
    double own[1] = {cg_thread_sum(rr)};
    cg_block_tree<1>(own, s_own);
    if (threadIdx.x == 0) part[(size_t) kGmresPartRR * kCgMaxParts + blockIdx.x] = own[0];
}

// out[i] = sqrt(in[i]): the square root gmres_cycle and gmres_rotate take, for the test that holds it against a correctly rounded one
template <typename D>
__global__ __launch_bounds__(kBlock) void gmres_sqrt_kernel(const D *__restrict__ in, D *__restrict__ out, long long n)
{
    const long long i = (long long) blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = __builtin_sqrt(in[i]);
}

} // namespace spmv
