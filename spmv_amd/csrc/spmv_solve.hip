// spmv_solve.hip -- translation unit of the vector kernels of the six device-resident solvers (kernels/cg.hpp, kernels/bicgstab.hpp,
// kernels/cg_columns.hpp, kernels/gmres.hpp, kernels/cg_mixed.hpp, kernels/lsqr.hpp, what they share in kernels/solve_common.hpp).  Launches only: the workspace, staging, the multiplies, the host's
// looks at the state and the error channel stay in spmv_shim.hip (shim/solve.hpp).  Per solve it calls cg_start_launch or bicg_start_launch
// once; per iteration cg_iteration_launch behind q = A p, or bicg_first_launch behind v = A ph and bicg_second_launch behind t = A sh;
// spmv_hip_cg_columns: ccg_start_launch, and ccg_iteration_launch behind q = A p for all k columns.  spmv_hip_gmres (kernels/gmres.hpp):
// gmres_start_launch, gmres_step_launch behind w = A z, and at a cycle's end gmres_apply_launch, then gmres_restart_launch behind w = A x.
// spmv_hip_cg_mixed (kernels/cg_mixed.hpp): mix_start_launch, mix_iteration_launch behind q = A_low p, and at a segment's end mix_try_launch,
// then mix_update_launch behind q64 = A_high xn.  spmv_hip_lsqr (kernels/lsqr.hpp): lsqr_init_launch, lsqr_first_launch behind v = A^T u, and per
// iteration lsqr_u_launch behind q = A v and lsqr_v_launch behind qt = A^T u.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/cg.hpp"
#include "kernels/bicgstab.hpp"
#include "kernels/cg_columns.hpp"
#include "kernels/gmres.hpp"
#include "kernels/cg_mixed.hpp"
#include "kernels/lsqr.hpp"

namespace spmv {

// cg_begin on the partial arrays rz / rr / bb; SPD: CG's <r,z> <= 0 test
template <bool SPD>
static void solve_begin(const SolveArgs &a, int rz, int rr, int bb, hipStream_t stream)
{
    if (a.hist) cg_begin_kernel<true, SPD><<<1, kBlock, 0, stream>>>(a.part, rz, rr, bb, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
    else cg_begin_kernel<false, SPD><<<1, kBlock, 0, stream>>>(a.part, rz, rr, bb, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void cg_start_t(const SolveArgs &a, bool use_x0, hipStream_t stream)
{
    const T *b = (const T *) a.b, *q = (const T *) a.vec[kCgVecQ], *dinv = (const T *) a.dinv;
    T *r = (T *) a.vec[kCgVecR], *p = (T *) a.vec[kCgVecP];
    if (use_x0) cg_init_kernel<T, WIDE, DINV, true><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, b, (T *) a.x, q, dinv, r, p, a.part);
    else cg_init_kernel<T, WIDE, DINV, false><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, b, (T *) a.x, q, dinv, r, p, a.part);
    solve_begin<true>(a, kCgPartRZ0, kCgPartRR, kCgPartBB, stream);
}

template <typename T, bool WIDE, bool DINV>
static void cg_iteration_t(const SolveArgs &a, int k, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    const T *dinv = (const T *) a.dinv;
    T *r = (T *) a.vec[kCgVecR], *p = (T *) a.vec[kCgVecP], *q = (T *) a.vec[kCgVecQ];
    cg_dot_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, p, q, a.part + (size_t) kCgPartPQ * kCgMaxParts, &a.state->end_direction);
    cg_update_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, p, q, (T *) a.x, r, dinv, a.part, a.state, a.nostop);
    cg_direction_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, r, dinv, p, a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void bicg_start_t(const SolveArgs &a, bool use_x0, hipStream_t stream)
{
    const T *b = (const T *) a.b, *v = (const T *) a.vec[kBicgVecV], *dinv = (const T *) a.dinv;
    T *r = (T *) a.vec[kBicgVecR], *rhat = (T *) a.vec[kBicgVecRhat], *p = (T *) a.vec[kBicgVecP], *y = (T *) a.vec[kBicgVecY];
    if (use_x0) bicg_init_kernel<T, WIDE, DINV, true><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, b, (T *) a.x, v, dinv, r, rhat, p, y, a.part);
    else bicg_init_kernel<T, WIDE, DINV, false><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, b, (T *) a.x, v, dinv, r, rhat, p, y, a.part);
    solve_begin<false>(a, kBicgPartRho0, kBicgPartRR, kBicgPartBB, stream);
}

template <typename T, bool WIDE, bool DINV>
static void bicg_first_t(const SolveArgs &a, int k, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    const T *rhat = (const T *) a.vec[kBicgVecRhat], *p = (const T *) a.vec[kBicgVecP], *v = (const T *) a.vec[kBicgVecV];
    cg_dot_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, rhat, v, a.part + (size_t) kBicgPartRV * kCgMaxParts, &a.state->end_direction);
    bicg_half_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, p, v, (T *) a.x, (T *) a.vec[kBicgVecR], (const T *) a.dinv, (T *) a.vec[kBicgVecY], a.part, a.state, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void bicg_second_t(const SolveArgs &a, int k, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    const T *rhat = (const T *) a.vec[kBicgVecRhat], *v = (const T *) a.vec[kBicgVecV], *t = (const T *) a.vec[kBicgVecT], *dinv = (const T *) a.dinv;
    T *r = (T *) a.vec[kBicgVecR], *p = (T *) a.vec[kBicgVecP], *y = (T *) a.vec[kBicgVecY];
    bicg_ts_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, t, r, a.part, a.state);
    bicg_update_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, t, r, y, (T *) a.x, rhat, a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
    bicg_direction_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, r, p, v, dinv, y, a.part, a.state, a.hist, a.rtol2, a.atol2, a.nostop);
}

static bool args_ok(const SolveArgs &a) { return a.m > 0 && a.parts >= 1 && a.parts <= kCgMaxParts && a.span * a.parts >= a.m; }

// the instantiation F<T, WIDE, DINV> that a.wide / a.dinv select
#define FORM_LAUNCH(F, T, ...)                                                                                       \
    do {                                                                                                             \
        if (a.wide) { if (a.dinv) F<T, true, true>(__VA_ARGS__); else F<T, true, false>(__VA_ARGS__); }              \
        else { if (a.dinv) F<T, false, true>(__VA_ARGS__); else F<T, false, false>(__VA_ARGS__); }                   \
    } while (0)

// the checked launch of the form of F that a.f64 / a.wide / a.dinv select; `ok`: what the call needs beyond args_ok
#define SOLVE_LAUNCH(F, ok, ...)                                                                                     \
    do {                                                                                                             \
        if (!args_ok(a) || !(ok)) return hipErrorInvalidValue;                                                       \
        if (a.f64) FORM_LAUNCH(F, double, __VA_ARGS__);                                                              \
        else FORM_LAUNCH(F, float, __VA_ARGS__);                                                                     \
        return hipGetLastError();                                                                                    \
    } while (0)

template <typename T, bool WIDE, bool DINV>
static void ccg_start_t(const SolveArgs &a, bool use_x0, hipStream_t stream)
{
    const T *b = (const T *) a.b, *q = (const T *) a.vec[kCcgVecQ], *dinv = (const T *) a.dinv;
    T *r = (T *) a.vec[kCcgVecR], *p = (T *) a.vec[kCcgVecP];
    if (use_x0) ccg_init_kernel<T, WIDE, DINV, true><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, a.k, b, a.ldb, (T *) a.x, a.ldx, q, dinv, r, p, a.part);
    else ccg_init_kernel<T, WIDE, DINV, false><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, a.k, b, a.ldb, (T *) a.x, a.ldx, q, dinv, r, p, a.part);
    if (a.hist) ccg_begin_kernel<true><<<(unsigned) a.k, kBlock, 0, stream>>>(a.part, a.k, a.cols, a.hist, a.rtol2, a.atol2, a.nostop);
    else ccg_begin_kernel<false><<<(unsigned) a.k, kBlock, 0, stream>>>(a.part, a.k, a.cols, a.hist, a.rtol2, a.atol2, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void ccg_iteration_t(const SolveArgs &a, int it, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts, cols = (unsigned) a.k;
    const T *dinv = (const T *) a.dinv;
    T *r = (T *) a.vec[kCcgVecR], *p = (T *) a.vec[kCcgVecP], *q = (T *) a.vec[kCcgVecQ];
    ccg_dot_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, a.k, p, q, a.part, a.cols);
    ccg_alpha_kernel<T><<<cols, kBlock, 0, stream>>>(a.part, a.k, it, a.cols, a.nostop);
    ccg_update_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, a.k, p, q, (T *) a.x, a.ldx, r, dinv, a.part, a.cols);
    ccg_beta_kernel<T><<<cols, kBlock, 0, stream>>>(a.part, a.k, it, a.cols, a.hist, a.rtol2, a.atol2, a.nostop);
    ccg_direction_kernel<T, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, a.k, r, dinv, p, a.cols);
}

static bool cols_ok(const SolveArgs &a) { return a.k >= 1 && a.k <= kCcgMaxK && a.ldb >= a.k && a.ldx >= a.k && a.cols != nullptr && (!a.wide || (a.ldb == a.k && a.ldx == a.k)); }

hipError_t ccg_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream) { SOLVE_LAUNCH(ccg_start_t, cols_ok(a), a, use_x0, stream); }
hipError_t ccg_iteration_launch(const SolveArgs &a, int it, hipStream_t stream) { SOLVE_LAUNCH(ccg_iteration_t, cols_ok(a) && it >= 1, a, it, stream); }
hipError_t cg_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream) { SOLVE_LAUNCH(cg_start_t, true, a, use_x0, stream); }
hipError_t cg_iteration_launch(const SolveArgs &a, int k, hipStream_t stream) { SOLVE_LAUNCH(cg_iteration_t, k >= 1, a, k, stream); }
hipError_t bicg_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream) { SOLVE_LAUNCH(bicg_start_t, true, a, use_x0, stream); }
hipError_t bicg_first_launch(const SolveArgs &a, int k, hipStream_t stream) { SOLVE_LAUNCH(bicg_first_t, k >= 1, a, k, stream); }
hipError_t bicg_second_launch(const SolveArgs &a, int k, hipStream_t stream) { SOLVE_LAUNCH(bicg_second_t, k >= 1, a, k, stream); }

// ---- spmv_hip_gmres
static GmresState *gmres_state(const SolveArgs &a) { return reinterpret_cast<GmresState *>(a.state); }
template <typename T> static T *gmres_vec(const SolveArgs &a, int i) { return (T *) (a.base + (size_t) i * a.stride); }

// v_i = w * T(scale) (i >= 1), z = Dinv .* v_i
template <typename T, bool WIDE, bool DINV>
static void gmres_scale_t(const SolveArgs &a, int i, hipStream_t stream)
{
    gmres_scale_kernel<T, WIDE, DINV><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, gmres_vec<T>(a, kGmresVecW), gmres_vec<T>(a, kGmresVecV + i - 1), (const T *) a.dinv,
                                                                                  gmres_vec<T>(a, kGmresVecZ), gmres_state(a));
}

template <typename T, bool WIDE, bool DINV>
static void gmres_start_t(const SolveArgs &a, bool use_x0, hipStream_t stream)
{
    T *w = gmres_vec<T>(a, kGmresVecW);
    if (use_x0) gmres_init_kernel<T, WIDE, true><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, (const T *) a.b, (T *) a.x, w, a.part);
    else gmres_init_kernel<T, WIDE, false><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, (const T *) a.b, (T *) a.x, w, a.part);
    solve_begin<false>(a, kGmresPartRR, kGmresPartRR, kGmresPartBB, stream);
    gmres_cycle_kernel<false><<<1, kBlock, 0, stream>>>(a.part, gmres_state(a), a.nostop);
    gmres_scale_t<T, WIDE, DINV>(a, 1, stream);
}

template <typename T, bool WIDE, bool DINV>
static void gmres_step_t(const SolveArgs &a, int k, int j, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    GmresState *st = gmres_state(a);
    gmres_dots_kernel<T, kGmresGroup><<<grid, kBlock, 0, stream>>>(a.m, a.span, a.base, a.stride, j, a.part, st);
    gmres_coeffs_kernel<T><<<(unsigned) j, kBlock, 0, stream>>>(a.part, st, 0);
    gmres_sub_dots_kernel<T, kGmresGroup><<<grid, kBlock, 0, stream>>>(a.m, a.span, a.base, a.stride, j, a.part, st);
    gmres_coeffs_kernel<T><<<(unsigned) j, kBlock, 0, stream>>>(a.part, st, 1);
    gmres_sub_norm_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, a.base, a.stride, j, a.part, st);
    if (a.hist) gmres_rotate_kernel<true><<<1, kBlock, 0, stream>>>(a.part, st, k, j, a.hist, a.rtol2, a.atol2, a.nostop);
    else gmres_rotate_kernel<false><<<1, kBlock, 0, stream>>>(a.part, st, k, j, a.hist, a.rtol2, a.atol2, a.nostop);
    if (j < a.restart) gmres_scale_t<T, WIDE, DINV>(a, j + 1, stream);
}

template <typename T, bool WIDE, bool DINV>
static void gmres_apply_t(const SolveArgs &a, int force, hipStream_t stream)
{
    gmres_solve_kernel<T><<<1, kWave, 0, stream>>>(gmres_state(a), force);
    gmres_update_x_kernel<T, WIDE, DINV><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, a.base, a.stride, (T *) a.x, (const T *) a.dinv, gmres_state(a), force);
}

template <typename T, bool WIDE, bool DINV>
static void gmres_restart_t(const SolveArgs &a, hipStream_t stream)
{
    gmres_residual_kernel<T, WIDE><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, (const T *) a.b, gmres_vec<T>(a, kGmresVecW), a.part, gmres_state(a));
    gmres_cycle_kernel<true><<<1, kBlock, 0, stream>>>(a.part, gmres_state(a), a.nostop);
    gmres_scale_t<T, WIDE, DINV>(a, 1, stream);
}

static bool gmres_ok(const SolveArgs &a) { return a.restart >= 1 && a.restart <= kGmresMaxRestart && a.base != nullptr && a.stride >= sizeof(double) && a.state != nullptr; }

hipError_t gmres_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream) { SOLVE_LAUNCH(gmres_start_t, gmres_ok(a), a, use_x0, stream); }
hipError_t gmres_step_launch(const SolveArgs &a, int k, int j, hipStream_t stream) { SOLVE_LAUNCH(gmres_step_t, gmres_ok(a) && k >= 1 && j >= 1 && j <= a.restart, a, k, j, stream); }
hipError_t gmres_apply_launch(const SolveArgs &a, int force, hipStream_t stream) { SOLVE_LAUNCH(gmres_apply_t, gmres_ok(a), a, force, stream); }
hipError_t gmres_restart_launch(const SolveArgs &a, hipStream_t stream) { SOLVE_LAUNCH(gmres_restart_t, gmres_ok(a), a, stream); }

hipError_t gmres_sqrt_launch(const double *in, double *out, long long n, hipStream_t stream)
{
    if (n <= 0 || !in || !out || (n + kBlock - 1) / kBlock > 0x7fffffffLL) return hipErrorInvalidValue;
    gmres_sqrt_kernel<double><<<(unsigned) ((n + kBlock - 1) / kBlock), kBlock, 0, stream>>>(in, out, n);
    return hipGetLastError();
}

// ---- spmv_hip_cg_mixed: T is float, the type of the iterations, whatever a.f64 says of the handle
static MixState *mix_state(const SolveArgs &a) { return reinterpret_cast<MixState *>(a.state); }
static double *mix_vec64(const SolveArgs &a, int i) { return (double *) a.vec[i]; }
template <typename T> static T *mix_vec(const SolveArgs &a, int i) { return (T *) a.vec[kMixVectors64 + i]; }

template <typename T, bool WIDE, bool DINV>
static void mix_start_t(const SolveArgs &a, bool use_x0, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    const double *b = (const double *) a.b;
    double *x = (double *) a.x, *q64 = mix_vec64(a, kMixVecQ64);
    const T *dinv = (const T *) a.dinv;
    T *r = mix_vec<T>(a, kMixVecR);
    if (use_x0) mix_residual_kernel<WIDE, DINV, 1><<<grid, kBlock, 0, stream>>>(a.m, a.span, 0, b, x, q64, dinv, r, a.part);
    else mix_residual_kernel<WIDE, DINV, 0><<<grid, kBlock, 0, stream>>>(a.m, a.span, 0, b, x, q64, dinv, r, a.part);
    mix_resume_kernel<WIDE, DINV, true><<<grid, kBlock, 0, stream>>>(a.m, a.span, 0, 0, a.budget, mix_vec64(a, kMixVecXn), x, r, dinv, mix_vec<T>(a, kMixVecP), mix_vec<T>(a, kMixVecY),
                                                                     a.part, mix_state(a), a.hist, a.rtol2, a.atol2, a.nostop);
}

// cg_dot<float> and cg_update<float> are spmv_hip_cg's own, on y in the place of x
template <typename T, bool WIDE, bool DINV>
static void mix_iteration_t(const SolveArgs &a, int k, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    const T *dinv = (const T *) a.dinv;
    T *r = mix_vec<T>(a, kMixVecR), *p = mix_vec<T>(a, kMixVecP), *q = mix_vec<T>(a, kMixVecQ);
    cg_dot_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, p, q, a.part + (size_t) kCgPartPQ * kCgMaxParts, &a.state->end_direction);
    cg_update_kernel<T, WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, p, q, mix_vec<T>(a, kMixVecY), r, dinv, a.part, a.state, a.nostop);
    mix_direction_kernel<WIDE, DINV><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, r, dinv, p, a.part, mix_state(a), a.hist, a.drop2, a.every, a.budget, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void mix_try_t(const SolveArgs &a, hipStream_t stream)
{
    mix_try_kernel<WIDE><<<(unsigned) a.parts, kBlock, 0, stream>>>(a.m, a.span, (const double *) a.x, mix_vec<T>(a, kMixVecY), mix_vec64(a, kMixVecXn), mix_state(a));
}

template <typename T, bool WIDE, bool DINV>
static void mix_update_t(const SolveArgs &a, int k, int update, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    double *x = (double *) a.x;
    const T *dinv = (const T *) a.dinv;
    T *r = mix_vec<T>(a, kMixVecR);
    mix_residual_kernel<WIDE, DINV, 2><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, (const double *) a.b, x, mix_vec64(a, kMixVecQ64), dinv, r, a.part);
    mix_resume_kernel<WIDE, DINV, false><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, update, a.budget, mix_vec64(a, kMixVecXn), x, r, dinv, mix_vec<T>(a, kMixVecP),
                                                                      mix_vec<T>(a, kMixVecY), a.part, mix_state(a), a.hist, a.rtol2, a.atol2, a.nostop);
}

static bool mix_ok(const SolveArgs &a)
{
    for (void *v : a.vec) if (!v) return false;
    return a.b && a.x && a.part && a.state;
}

// the checked launch of the float form of F that a.wide / a.dinv select
#define MIX_LAUNCH(F, ok, ...)                                                     \
    do {                                                                           \
        if (!args_ok(a) || !mix_ok(a) || !(ok)) return hipErrorInvalidValue;       \
        FORM_LAUNCH(F, float, __VA_ARGS__);                                        \
        return hipGetLastError();                                                  \
    } while (0)

hipError_t mix_start_launch(const SolveArgs &a, bool use_x0, hipStream_t stream) { MIX_LAUNCH(mix_start_t, true, a, use_x0, stream); }
hipError_t mix_iteration_launch(const SolveArgs &a, int k, hipStream_t stream) { MIX_LAUNCH(mix_iteration_t, k >= 1, a, k, stream); }
hipError_t mix_try_launch(const SolveArgs &a, hipStream_t stream) { MIX_LAUNCH(mix_try_t, true, a, stream); }
hipError_t mix_update_launch(const SolveArgs &a, int k, int update, hipStream_t stream) { MIX_LAUNCH(mix_update_t, k >= 1 && update >= 1, a, k, update, stream); }

// ---- spmv_hip_lsqr: vectors of two lengths, u and q over a.m (a.parts, a.span), v, w, qt and x over a.n (a.parts_n, a.span_n); no Dinv
static LsqrState *lsqr_state(const SolveArgs &a) { return reinterpret_cast<LsqrState *>(a.state); }

template <typename T, bool WIDE, bool DINV>
static void lsqr_init_t(const SolveArgs &a, bool use_x0, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    T *u = (T *) a.vec[kLsqrVecU];
    if (use_x0) lsqr_init_kernel<T, WIDE, true><<<grid, kBlock, 0, stream>>>(a.m, a.span, (const T *) a.b, (const T *) a.vec[kLsqrVecQ], u, a.part);
    else lsqr_init_kernel<T, WIDE, false><<<grid, kBlock, 0, stream>>>(a.m, a.span, (const T *) a.b, (const T *) a.vec[kLsqrVecQ], u, a.part);
    lsqr_unit_u_kernel<T, true><<<grid, kBlock, 0, stream>>>(a.m, a.span, u, a.part, lsqr_state(a), a.hist, a.rtol2, a.atol2, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void lsqr_first_t(const SolveArgs &a, bool use_x0, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts_n;
    T *v = (T *) a.vec[kLsqrVecV];
    if (use_x0) lsqr_vv_kernel<T, WIDE, true><<<grid, kBlock, 0, stream>>>(a.n, a.span_n, v, (T *) a.x, a.part, lsqr_state(a));
    else lsqr_vv_kernel<T, WIDE, false><<<grid, kBlock, 0, stream>>>(a.n, a.span_n, v, (T *) a.x, a.part, lsqr_state(a));
    lsqr_step_kernel<T, WIDE, true><<<grid, kBlock, 0, stream>>>(a.n, a.span_n, 0, v, (T *) a.vec[kLsqrVecW], (T *) a.x, a.part, lsqr_state(a), a.hist, a.rtol2, a.atol2, a.ls_tol,
                                                                 a.damp, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void lsqr_u_t(const SolveArgs &a, int k, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts;
    T *u = (T *) a.vec[kLsqrVecU];
    lsqr_u_kernel<T><<<grid, kBlock, 0, stream>>>(a.m, a.span, k, (const T *) a.vec[kLsqrVecQ], u, a.part, lsqr_state(a));
    lsqr_unit_u_kernel<T, false><<<grid, kBlock, 0, stream>>>(a.m, a.span, u, a.part, lsqr_state(a), a.hist, a.rtol2, a.atol2, a.nostop);
}

template <typename T, bool WIDE, bool DINV>
static void lsqr_v_t(const SolveArgs &a, int k, hipStream_t stream)
{
    const unsigned grid = (unsigned) a.parts_n;
    T *v = (T *) a.vec[kLsqrVecV];
    lsqr_v_kernel<T><<<grid, kBlock, 0, stream>>>(a.n, a.span_n, (const T *) a.vec[kLsqrVecQt], v, a.part, lsqr_state(a), a.nostop);
    lsqr_step_kernel<T, WIDE, false><<<grid, kBlock, 0, stream>>>(a.n, a.span_n, k, v, (T *) a.vec[kLsqrVecW], (T *) a.x, a.part, lsqr_state(a), a.hist, a.rtol2, a.atol2, a.ls_tol,
                                                                  a.damp, a.nostop);
}

static bool lsqr_ok(const SolveArgs &a)
{
    for (int i = 0; i < kLsqrVectors; ++i) if (!a.vec[i]) return false;
    return a.n >= 0 && a.parts_n >= 1 && a.parts_n <= kCgMaxParts && a.span_n * a.parts_n >= a.n && a.b && (a.x || a.n == 0) && a.part && a.state && !a.dinv;
}

hipError_t lsqr_init_launch(const SolveArgs &a, bool use_x0, hipStream_t stream) { SOLVE_LAUNCH(lsqr_init_t, lsqr_ok(a), a, use_x0, stream); }
hipError_t lsqr_first_launch(const SolveArgs &a, bool use_x0, hipStream_t stream) { SOLVE_LAUNCH(lsqr_first_t, lsqr_ok(a), a, use_x0, stream); }
hipError_t lsqr_u_launch(const SolveArgs &a, int k, hipStream_t stream) { SOLVE_LAUNCH(lsqr_u_t, lsqr_ok(a) && k >= 1, a, k, stream); }
hipError_t lsqr_v_launch(const SolveArgs &a, int k, hipStream_t stream) { SOLVE_LAUNCH(lsqr_v_t, lsqr_ok(a) && k >= 1, a, k, stream); }

} // namespace spmv
