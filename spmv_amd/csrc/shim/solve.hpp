// shim/solve.hpp -- part of spmv_shim.hip: the six solves on the RESIDENT matrix that stay on the device and their timer: conjugate gradients
// (spmv_hip_cg), BiCGStab (spmv_hip_bicgstab), conjugate gradients for k right-hand sides at once (spmv_hip_cg_columns), restarted GMRES
// (spmv_hip_gmres), mixed-precision conjugate gradients on a pair of handles (spmv_hip_cg_mixed) and LSQR for any m x n matrix
// (spmv_hip_lsqr).  The vector kernels are kernels/cg.hpp, bicgstab.hpp, cg_columns.hpp, gmres.hpp, cg_mixed.hpp and lsqr.hpp, launched from their own translation unit (spmv_solve.hip); the multiplies -- q = A p,
// or v = A ph and t = A sh -- are launch<T>() on workspace vectors: the launch spmv_shim_run makes, without its staging: the handle's own
// schedule, spmv()'s bits.  For k columns the multiply is spmm_panels() on the compact workspace vectors: the launches spmv_shim_spmm makes,
// without its staging: spmv_hip_spmm's bits.
//
// The host enqueues `check_every` iterations, copies the state back and synchronises ONCE; inside a batch nothing waits for the host: alpha,
// (omega,) beta and the stop tests are derived on the device (kernels/cg.hpp), and once the state says that the loop has ended every later
// kernel of the batch returns at once -- what is wasted is at most check_every - 1 multiplies into the scratch vector q (BiCGStab:
// 2 check_every - 1 into v and t).  The returned x, iterations and history therefore do not depend on check_every.  With k columns the state
// holds k of everything; the loop ends when every column has ended.
//
// Everything here is written once: one call struct (spmv_solve_call), one workspace rule, one loop (solve_run), one timer (solve_time).  A
// solver is a row of kSolvers: its sizes, its workspace, what its start and one iteration enqueue, how its state reads, and three hooks that
// most rows leave empty.  k, ldb and ldx are 1 for the single solves.  spmv_hip_gmres's workspace has `restart` vectors more than its fixed
// three, and it has a `finish`: the columns of an unfinished cycle are applied to x behind the last look.  spmv_hip_cg_mixed has vectors of
// two sizes, an `admit` (what its pair of handles must share) and a `resume`: a look that finds a segment ended enqueues the update, and the
// loop goes on.  spmv_hip_lsqr is the one solver whose matrix need not be square: its vectors have two LENGTHS (b, u and q m elements; x, v,
// w and qt n), each with its own geometry of the dots, and its second multiply is launch<T>() on the attached transpose: the launch
// spmv_hip_spmv_transpose makes, without its staging.
#pragma once

// what the host reads out of a solver's state, per column
struct SolveLook {
    bool done[kCcgMaxK];
    int status[kCcgMaxK], iterations[kCcgMaxK];
    double rr[kCcgMaxK], bb[kCcgMaxK];
    int updates;      // spmv_hip_cg_mixed: committed updates
    double ar, anorm; // spmv_hip_lsqr
};

// one solve or timing: the handle, spmv_hip_cg_mixed's fp32 one (nullptr otherwise), the device operands
struct SolveRun {
    spmv_dev *d, *low;
    SolveArgs a;
};

struct Solver {
    int id;                           // SPMV_SHIM_SOLVE_*: the row's index in kSolvers, and of its storage in spmv_dev::solve_ws
    const char *name;                 // in error texts
    int vectors, vectors4;            // workspace vectors of m k elements of the handle's type, and behind them of m k 4-byte elements
    int vectors_n;                    // spmv_hip_lsqr: behind those, workspace vectors of n elements of the handle's type; != 0: x has n elements and m != n is allowed
    int part_arrays;                  // partial arrays of kCgMaxParts doubles PER COLUMN
    int vectors_per_step;             // spmv_hip_gmres: further vectors per step of a cycle; its workspace is sized by `restart`, not by k (0: by k)
    int max_k;                        // most right-hand sides of a call
    int check_every;                  // iterations between two looks at the state when the caller leaves check_every at 0
    size_t state_bytes, state_room;   // the device state: what is zeroed and copied, and the bytes behind the partial arrays that hold it
    size_t dinv_size;                 // bytes of an element of Dinv; 0: the handle's
    int stage_b, stage_x;             // the stage buffers of host B and X
    int (*start)(const Solver &s, const SolveRun &r, bool use_x0); // behind the zeroed state: (A x0,) the init and begin kernels
    int (*iteration)(const Solver &s, const SolveRun &r, int k);   // iteration k >= 1: the multiplies and the vector kernels
    void (*look)(const void *state, int k, SolveLook &l);           // a host copy of the state -> what it says
    int (*finish)(const Solver &s, const SolveRun &r, const void *state); // nullptr, or what the last look's state still asks for
    // nullptr, or what a look that finds the loop ended may still enqueue: true when the loop goes on, from iteration it + 1; false with rc set on a failure
    bool (*resume)(const Solver &s, const SolveRun &r, const void *state, int &it, int &rc);
    int (*admit)(const Solver &s, const char *what, const spmv_dev *d, const spmv_dev *low); // nullptr, or the solver's own rules for its handles
};

static int solve_multiply(spmv_dev *d, const void *x, void *y)
{
    return d->vsize == sizeof(double) ? launch<double>(d, (const double *) x, (double *) y) : launch<float>(d, (const float *) x, (float *) y);
}

static int solve_launched(const Solver &s, hipError_t e)
{
    return e == hipSuccess ? SPMV_HIP_OK : fail(SPMV_HIP_E_RUNTIME, "%s: launch: %s", s.name, hipGetErrorString(e));
}

// (q = A x0,) cg_init + cg_begin
static int cg_start(const Solver &s, const SolveRun &r, bool use_x0)
{
    int rc;
    if (use_x0 && (rc = solve_multiply(r.d, r.a.x, r.a.vec[kCgVecQ]))) return rc;
    return solve_launched(s, cg_start_launch(r.a, use_x0, r.d->stream));
}

// q = A p, then the three vector kernels
static int cg_iteration(const Solver &s, const SolveRun &r, int k)
{
    const int rc = solve_multiply(r.d, r.a.vec[kCgVecP], r.a.vec[kCgVecQ]);
    return rc ? rc : solve_launched(s, cg_iteration_launch(r.a, k, r.d->stream));
}

// (v = A x0,) bicg_init + bicg_begin
static int bicg_start(const Solver &s, const SolveRun &r, bool use_x0)
{
    int rc;
    if (use_x0 && (rc = solve_multiply(r.d, r.a.x, r.a.vec[kBicgVecV]))) return rc;
    return solve_launched(s, bicg_start_launch(r.a, use_x0, r.d->stream));
}

// v = A ph, bicg_rv + bicg_half, t = A sh, bicg_ts + bicg_update + bicg_direction; without Dinv ph is p and sh is s, which is in r
static int bicg_iteration(const Solver &s, const SolveRun &r, int k)
{
    const SolveArgs &a = r.a;
    int rc;
    if ((rc = solve_multiply(r.d, a.vec[a.dinv ? kBicgVecY : kBicgVecP], a.vec[kBicgVecV])) || (rc = solve_launched(s, bicg_first_launch(a, k, r.d->stream)))) return rc;
    if ((rc = solve_multiply(r.d, a.vec[a.dinv ? kBicgVecY : kBicgVecR], a.vec[kBicgVecT]))) return rc;
    return solve_launched(s, bicg_second_launch(a, k, r.d->stream));
}

// (q = A X0 for all columns,) ccg_init + ccg_begin
static int ccg_start(const Solver &s, const SolveRun &r, bool use_x0)
{
    const SolveArgs &a = r.a;
    int rc;
    if (use_x0 && (rc = spmm_panels(r.d, a.k, (const char *) a.x, a.ldx, (char *) a.vec[kCcgVecQ], a.k))) return rc;
    return solve_launched(s, ccg_start_launch(a, use_x0, r.d->stream));
}

// q = A p for all columns in one pass over A, then the five vector kernels
static int ccg_iteration(const Solver &s, const SolveRun &r, int it)
{
    const SolveArgs &a = r.a;
    const int rc = spmm_panels(r.d, a.k, (const char *) a.vec[kCcgVecP], a.k, (char *) a.vec[kCcgVecQ], a.k);
    return rc ? rc : solve_launched(s, ccg_iteration_launch(a, it, r.d->stream));
}

// (w = A x0,) gmres_init + cg_begin + gmres_cycle + gmres_scale
static int gmres_start(const Solver &s, const SolveRun &r, bool use_x0)
{
    const SolveArgs &a = r.a;
    int rc;
    if (use_x0 && (rc = solve_multiply(r.d, a.x, a.base + kGmresVecW * a.stride))) return rc;
    return solve_launched(s, gmres_start_launch(a, use_x0, r.d->stream));
}

// step j = (k - 1) mod restart + 1 of its cycle: w = A z (z is v_j without Dinv), then the seven vector kernels, sized by j; at j = restart
// the cycle's end (gmres_solve + gmres_update_x) and the restart (w = A x, gmres_residual + gmres_cycle + gmres_scale) as well
static int gmres_iteration(const Solver &s, const SolveRun &r, int k)
{
    const SolveArgs &a = r.a;
    spmv_dev *d = r.d;
    const int j = (k - 1) % a.restart + 1;
    int rc;
    if ((rc = solve_multiply(d, a.base + (a.dinv ? (size_t) kGmresVecZ : (size_t) (kGmresVecV + j - 1)) * a.stride, a.base + kGmresVecW * a.stride))) return rc;
    if ((rc = solve_launched(s, gmres_step_launch(a, k, j, d->stream))) || j < a.restart) return rc;
    if ((rc = solve_launched(s, gmres_apply_launch(a, 0, d->stream))) || (rc = solve_multiply(d, a.x, a.base + kGmresVecW * a.stride))) return rc;
    return solve_launched(s, gmres_restart_launch(a, d->stream));
}

// the loop ended, or the budget ran out, in the middle of a cycle: the columns the state names go into x
static int gmres_finish(const Solver &s, const SolveRun &r, const void *state)
{
    return ((const GmresState *) state)->pending > 0 ? solve_launched(s, gmres_apply_launch(r.a, 1, r.d->stream)) : SPMV_HIP_OK;
}

// (q = A x0,) lsqr_init + lsqr_unit_u, v = A^T u, lsqr_vv + lsqr_step
static int lsqr_start(const Solver &s, const SolveRun &r, bool use_x0)
{
    const SolveArgs &a = r.a;
    int rc;
    if (use_x0 && (rc = solve_multiply(r.d, a.x, a.vec[kLsqrVecQ]))) return rc;
    if ((rc = solve_launched(s, lsqr_init_launch(a, use_x0, r.d->stream))) || (rc = solve_multiply(r.d->tr, a.vec[kLsqrVecU], a.vec[kLsqrVecV]))) return rc;
    return solve_launched(s, lsqr_first_launch(a, use_x0, r.d->stream));
}

// q = A v, lsqr_u + lsqr_unit_u, qt = A^T u, lsqr_v + lsqr_step: both multiplies are always enqueued
static int lsqr_iteration(const Solver &s, const SolveRun &r, int k)
{
    const SolveArgs &a = r.a;
    int rc;
    if ((rc = solve_multiply(r.d, a.vec[kLsqrVecV], a.vec[kLsqrVecQ])) || (rc = solve_launched(s, lsqr_u_launch(a, k, r.d->stream)))) return rc;
    if ((rc = solve_multiply(r.d->tr, a.vec[kLsqrVecU], a.vec[kLsqrVecQt]))) return rc;
    return solve_launched(s, lsqr_v_launch(a, k, r.d->stream));
}

static void single_look(const void *state, int, SolveLook &l)
{
    const SolveState &hs = *(const SolveState *) state;
    l.done[0] = hs.end_half || hs.end_update || hs.end_direction;
    l.status[0] = hs.status;
    l.iterations[0] = hs.iterations;
    l.rr[0] = hs.rr;
    l.bb[0] = hs.bb;
}

static void cols_look(const void *state, int k, SolveLook &l)
{
    const ColsState &hs = *(const ColsState *) state;
    for (int j = 0; j < k; ++j) {
        l.done[j] = hs.end_update[j] || hs.end_direction[j];
        l.status[j] = hs.status[j];
        l.iterations[j] = hs.iterations[j];
        l.rr[j] = hs.rr[j];
        l.bb[j] = hs.bb[j];
    }
}

static void lsqr_look(const void *state, int k, SolveLook &l)
{
    single_look(state, k, l);
    l.ar = ((const LsqrState *) state)->ar;
    l.anorm = ((const LsqrState *) state)->anorm;
}

// bytes of one workspace vector of m x k elements of `elem` bytes, and of one of spmv_hip_lsqr's of n elements
static size_t solve_vec_bytes(const spmv_dev *d, int k, size_t elem) { return (elem * (size_t) d->m * (size_t) k + 255) & ~(size_t) 255; }
static size_t solve_vecn_bytes(const spmv_dev *d) { return (d->vsize * (size_t) d->n + 255) & ~(size_t) 255; }
// the elements of a column of x: n for spmv_hip_lsqr, m (= n) for the others
static size_t solve_x_rows(const Solver &s, const spmv_dev *d) { return (size_t) (s.vectors_n ? d->n : d->m); }
// P and L of a dot over `len` >= 0 elements (include/spmv_hip.h); one empty workgroup for len = 0
static void solve_geometry(long long len, int &parts, long long &span)
{
    const long long chunks = (len + kCgChunk - 1) / kCgChunk;
    parts = (int) (chunks < 1 ? 1 : chunks < kCgMaxParts ? chunks : kCgMaxParts);
    span = (long long) kCgChunk * ((len + (long long) kCgChunk * parts - 1) / ((long long) kCgChunk * parts));
    if (span < kCgChunk) span = kCgChunk;
}
// what a workspace sized by n (k columns; spmv_hip_gmres: restart n) holds: the columns of a vector, the vectors of the handle's type, all the
// vectors' bytes, the bytes behind them
static int solve_cols(const Solver &s, int n) { return s.vectors_per_step ? 1 : n; }
static int solve_vectors(const Solver &s, int n) { return s.vectors + s.vectors_per_step * n; }
static size_t solve_vectors_bytes(const Solver &s, const spmv_dev *d, int n)
{
    return solve_vectors(s, n) * solve_vec_bytes(d, solve_cols(s, n), d->vsize) + s.vectors4 * solve_vec_bytes(d, solve_cols(s, n), 4) + s.vectors_n * solve_vecn_bytes(d);
}
static size_t solve_tail_bytes(const Solver &s, int n) { return sizeof(double) * s.part_arrays * (size_t) solve_cols(s, n) * kCgMaxParts + s.state_room; }

// the vectors, the partial arrays (zeroed once: the entries behind the P in use stay +0.0) and the state: allocated at the solver's first solve --
// s.vectors * solve_vec_bytes(k, vsize) + s.vectors4 * solve_vec_bytes(k, 4) + s.vectors_n * solve_vecn_bytes() + 8 * s.part_arrays * k * 1024 + s.state_room bytes -- and given
// back and allocated anew when a call has more columns than it holds (spmv_hip_gmres: a larger restart; its vectors are restart + 3 of m elements)
static int solve_workspace(const Solver &s, spmv_dev *d, int n)
{
    static_assert(sizeof(SolveState) <= 256 && sizeof(ColsState) <= 1024 && sizeof(GmresState) <= kGmresStateRoom && sizeof(MixState) <= 256 && sizeof(LsqrState) <= 256,
                  "the state's room behind the partial arrays");
    spmv_dev::SolveWs &w = d->solve_ws[s.id];
    if (w.n >= n) return SPMV_HIP_OK;
    if (w.p) {
        quiesce(d);
        (void) pool_free(w.p);
        d->device_bytes -= (long long) (solve_vectors_bytes(s, d, w.n) + solve_tail_bytes(s, w.n));
        w.p = nullptr;
        w.n = 0;
    }
    const size_t vecs = solve_vectors_bytes(s, d, n), tail = solve_tail_bytes(s, n);
    ALLOC_TRY(d, &w.p, vecs + tail, false);
    w.n = n;
    HIP_TRY(hipMemsetAsync((char *) w.p + vecs, 0, tail, d->stream));
    return SPMV_HIP_OK;
}

// One solve's device operands: the workspace carved up (by the columns it HOLDS, so that a partial array never lies where a vector did), host
// B / X / Dinv staged (X's copy-back registered with the stager; the initial guess copied in when it is wanted; the single solves share their
// stage buffers, and all five Dinv's: the calls are synchronous, so they never hold them at the same time), the history block, the geometry
// of the dots (spmv_hip_lsqr: both).  m > 0.
static int solve_prepare(const Solver &s, spmv_dev *d, Stager &stg, const spmv_solve_call &c, size_t hist_entries, int nostop, SolveArgs &a)
{
    int rc = solve_workspace(s, d, s.vectors_per_step ? c.restart : c.k);
    if (rc) return rc;
    spmv_dev::SolveWs &w = d->solve_ws[s.id];
    const int cols = solve_cols(s, w.n), vectors = solve_vectors(s, w.n), k = c.k;
    const size_t vec = solve_vec_bytes(d, cols, d->vsize), vec4 = solve_vec_bytes(d, cols, 4), vecn = solve_vecn_bytes(d), m = (size_t) d->m, xrows = solve_x_rows(s, d);
    char *ws = (char *) w.p, *ws4 = ws + vectors * vec, *wsn = ws4 + s.vectors4 * vec4;
    a.m = d->m;
    a.k = k;
    a.restart = c.restart;
    a.base = ws;
    a.stride = vec;
    solve_geometry(d->m, a.parts, a.span);
    a.n = d->n;
    solve_geometry(d->n, a.parts_n, a.span_n);
    const int slots = (int) (sizeof(a.vec) / sizeof(a.vec[0]));
    for (int i = 0; i < vectors && i < slots; ++i) a.vec[i] = ws + i * vec;
    for (int i = 0; i < s.vectors4 && vectors + i < slots; ++i) a.vec[vectors + i] = ws4 + i * vec4;
    for (int i = 0; i < s.vectors_n && vectors + s.vectors4 + i < slots; ++i) a.vec[vectors + s.vectors4 + i] = wsn + i * vecn;
    a.part = (double *) (wsn + s.vectors_n * vecn);
    void *state = a.part + s.part_arrays * (size_t) cols * kCgMaxParts;
    if (s.max_k > 1) a.cols = (ColsState *) state;
    else a.state = (SolveState *) state;
    a.rtol2 = c.opt.rtol * c.opt.rtol;
    a.atol2 = c.opt.atol * c.opt.atol;
    const double drop = c.update_drop > 0 ? c.update_drop : SPMV_HIP_CG_MIXED_UPDATE_DROP;
    a.drop2 = drop * drop;
    a.every = c.update_every;
    a.ls_tol = c.ls_tol;
    a.damp = c.damp;
    a.budget = c.opt.max_iterations;
    a.nostop = nostop;
    a.f64 = d->vsize == sizeof(double);
    a.b = c.b;
    a.dinv = c.opt.Dinv;
    a.x = c.x;
    a.ldb = c.ldb;
    a.ldx = c.ldx;
    long long ld = 1;
    if ((rc = stg.in(d->stage[s.stage_b], a.b, a.ldb, m, k)) || (rc = stg.in(d->stage[STAGE_CG_DINV], a.dinv, ld, m, 1, s.dinv_size)) || (rc = stg.out(d->stage[s.stage_x], a.x, a.ldx, xrows, k)))
        return rc;
    if (a.x != c.x && c.opt.use_x0) HIP_TRY(stg.copy(a.x, (size_t) k, c.x, (size_t) c.ldx, xrows, (size_t) k, hipMemcpyHostToDevice, d->vsize));
    // 16-byte accesses: B and X compact and aligned; the single solves' kernels read Dinv that way too, the k-column ones by element
    a.wide = a.ldb == k && a.ldx == k && wide_ok(a.b, 1, 16) && wide_ok(a.x, 1, 16) && (s.max_k > 1 || !a.dinv || wide_ok(a.dinv, 1, 16));
    a.hist = nullptr;
    if (hist_entries > 0) {
        if ((rc = stg.reserve(w.hist, sizeof(double) * hist_entries))) return rc;
        a.hist = (double *) w.hist.p;
    }
    return SPMV_HIP_OK;
}

static void *solve_state(const Solver &s, const SolveArgs &a) { return s.max_k > 1 ? (void *) a.cols : (void *) a.state; }

// the state zeroed, then the solver's start
static int solve_start(const Solver &s, const SolveRun &r, bool use_x0)
{
    HIP_TRY(hipMemsetAsync(solve_state(s, r.a), 0, s.state_bytes, r.d->stream));
    return s.start(s, r, use_x0);
}

// what a solve and its timer refuse alike: the code already reported, or SPMV_HIP_OK
static int solve_admit(const Solver &s, const char *pre, const spmv_dev *d, const spmv_solve_call &c)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "%s%s: schedule not built", pre, s.name);
    if (s.admit) if (const int rc = s.admit(s, pre, d, c.low)) return rc;
    if (c.k < 1 || c.k > s.max_k || c.ldb < c.k || c.ldx < c.k) return fail(SPMV_HIP_E_ARG, "%s%s: need 1 <= k <= %d, ldb >= k, ldx >= k", pre, s.name, s.max_k);
    if (s.vectors_per_step && (c.restart < 1 || c.restart > kGmresMaxRestart)) return fail(SPMV_HIP_E_ARG, "%s%s: need 1 <= restart <= %d", pre, s.name, kGmresMaxRestart);
    if (c.update_every < 0) return fail(SPMV_HIP_E_ARG, "%s%s: need update_every >= 0", pre, s.name);
    if (!s.vectors_n && d->m != d->n) return fail(SPMV_HIP_E_ARG, "%s%s: the matrix is %d x %d, not square", pre, s.name, d->m, d->n);
    if ((d->m > 0 && !c.b) || (solve_x_rows(s, d) > 0 && !c.x)) return fail(SPMV_HIP_E_ARG, "%s%s: B or X is NULL", pre, s.name);
    if (s.vectors_n && !(c.ls_tol >= 0 && c.damp >= 0)) return fail(SPMV_HIP_E_ARG, "%s%s: ls_tol and damp must be >= 0 (and not NaN)", pre, s.name);
    if (s.vectors_n && c.opt.Dinv) return fail(SPMV_HIP_E_ARG, "%s%s: there is no Dinv", pre, s.name);
    if (s.vectors_n && (!d->tr || !d->tr->built || d->tr_gen != d->val_gen)) return fail(SPMV_HIP_E_NOSTATE, "%s%s: the transpose is not attached, not built or not refreshed", pre, s.name);
    if (s.max_k > 1 && d->nnz > 0 && !d->colidx) return fail(SPMV_HIP_E_NOSTATE, "%s%s: the resident column indices were released (spmv_shim_restore_columns first)", pre, s.name);
    return SPMV_HIP_OK;
}

// history (k > 1): entry [it * k + j] is column j's rr after iteration it, written for it <= that column's iterations
static int solve_run(const Solver &s, spmv_dev *d, const spmv_solve_call &c)
{
    const spmv_hip_cg_options &opt = c.opt;
    spmv_hip_cg_result *res = c.res;
    const int k = c.k;
    if (!res) return fail(SPMV_HIP_E_ARG, "%s: res is NULL", s.name);
    int rc = solve_admit(s, "", d, c);
    if (rc) return rc;
    for (int j = 0; j < k; ++j) {
        res[j].status = SPMV_HIP_CG_CONVERGED;
        res[j].iterations = 0;
        res[j].rr = res[j].bb = 0;
    }
    if (c.updates) *c.updates = 0;
    if (c.ar) *c.ar = 0;
    if (c.anorm) *c.anorm = 0;
    if (d->m == 0 && solve_x_rows(s, d) == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    if (d->m == 0) { // spmv_hip_lsqr without rows: B is empty, bb = 0, x = 0
        if (!is_device_ptr(c.x)) { memset(c.x, 0, d->vsize * (size_t) d->n); return SPMV_HIP_OK; }
        HIP_TRY(hipMemsetAsync(c.x, 0, d->vsize * (size_t) d->n, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        return SPMV_HIP_OK;
    }
    if (s.vectors_n) d->tr->stream = d->stream; // the transpose launches on the parent's stream, as the halves of a split do
    if (s.max_k > 1 && (rc = spmm_plan(d))) return rc;
    Stager stg{d};
    SolveRun r{d, c.low, {}};
    const SolveArgs &a = r.a;
    rc = solve_prepare(s, d, stg, c, opt.history ? ((size_t) opt.max_iterations + 1) * (size_t) k : 0, 0, r.a);
    if (rc || (rc = solve_start(s, r, opt.use_x0 != 0))) return rc;
    const int every = opt.check_every > 0 ? opt.check_every : s.check_every;
    alignas(8) unsigned char hs[sizeof(GmresState) > sizeof(ColsState) ? sizeof(GmresState) : sizeof(ColsState)];
    static_assert(sizeof(hs) >= sizeof(SolveState) && sizeof(hs) >= sizeof(MixState) && sizeof(hs) >= sizeof(LsqrState), "the largest state");
    SolveLook l = {};
    // every look but the last is followed by an applied iteration or by what a resume enqueued
    int it = 0;
    for (long long looks = 0;; ++looks) {
        HIP_TRY(hipMemcpyAsync(hs, solve_state(s, a), s.state_bytes, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        s.look(hs, k, l);
        bool done = true;
        for (int j = 0; j < k; ++j) done = done && l.done[j];
        // the resume comes before the budget test: what it enqueued is looked at again even when the budget is spent, and it says where `it` goes on
        if (done ? !(s.resume && s.resume(s, r, hs, it, rc)) : it >= opt.max_iterations) break;
        if (looks > 2ll * opt.max_iterations + 2) return fail(SPMV_HIP_E_RUNTIME, "%s: the device's state does not advance", s.name);
        const int stop = opt.max_iterations - it < every ? opt.max_iterations : it + every;
        while (it < stop)
            if ((rc = s.iteration(s, r, ++it))) return rc;
    }
    if (rc || (s.finish && (rc = s.finish(s, r, hs)))) return rc;
    int longest = 0;
    for (int j = 0; j < k; ++j) {
        res[j].status = l.done[j] ? l.status[j] : SPMV_HIP_CG_MAX_ITERATIONS;
        res[j].iterations = l.iterations[j];
        res[j].rr = l.rr[j];
        res[j].bb = l.bb[j];
        if (l.iterations[j] > longest) longest = l.iterations[j];
        if (!(l.done[j] && l.status[j] == SPMV_HIP_CG_CONVERGED && l.bb[j] == 0)) continue;
        // B = 0: x = 0
        if (k == 1 && a.ldx == 1) HIP_TRY(hipMemsetAsync(a.x, 0, d->vsize * solve_x_rows(s, d), d->stream));
        else HIP_TRY(hipMemset2DAsync((char *) a.x + d->vsize * (size_t) j, d->vsize * (size_t) a.ldx, 0, d->vsize, (size_t) d->m, d->stream));
    }
    if (c.updates) *c.updates = l.updates;
    if (c.ar) *c.ar = l.ar;
    if (c.anorm) *c.anorm = l.anorm;
    std::vector<double> hist;
    if (opt.history && k == 1) HIP_TRY(hipMemcpyAsync(opt.history, a.hist, sizeof(double) * ((size_t) longest + 1), hipMemcpyDeviceToHost, d->stream));
    if (opt.history && k > 1) {
        hist.resize(((size_t) longest + 1) * (size_t) k);
        HIP_TRY(hipMemcpyAsync(hist.data(), a.hist, sizeof(double) * hist.size(), hipMemcpyDeviceToHost, d->stream));
    }
    if ((rc = stg.finish())) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream)); // the call is synchronous whatever the handle's async setting
    for (size_t i = 0; i < hist.size(); ++i) // the entries behind a column's end stay the caller's
        if ((int) (i / (size_t) k) <= l.iterations[i % (size_t) k]) opt.history[i] = hist[i];
    return SPMV_HIP_OK;
}

// `warmup` untimed + `iters` timed RUNS of opt.max_iterations iterations each, the stop tests disabled: every run starts again from B (and
// X when use_x0), its iterations are enqueued back to back and bracketed by two events on the handle's stream (the start is outside them:
// not state.hpp's time_events, which brackets a whole call).  ms_out[i] (may be NULL): run i.  Mean ms per run, < 0 on failure.  Device pointers only.
static double solve_time(const Solver &s, spmv_dev *d, const spmv_solve_call &c, int warmup, int iters, float *ms_out)
{
    const spmv_hip_cg_options &opt = c.opt;
    if (!d || !d->built || iters <= 0 || warmup < 0 || opt.max_iterations < 1 || d->m <= 0) { fail(SPMV_HIP_E_ARG, "time_%s: bad arguments", s.name); return -1.0; }
    if (solve_admit(s, "time_", d, c)) return -1.0;
    if (!is_device_ptr(c.b) || !is_device_ptr(c.x) || (opt.Dinv && !is_device_ptr(opt.Dinv))) { fail(SPMV_HIP_E_ARG, "time_%s: B, X and Dinv must be device pointers", s.name); return -1.0; }
    DeviceGuard guard(d->device);
    if (!guard.ok) { fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device); return -1.0; }
    if (s.max_k > 1 && spmm_plan(d)) return -1.0;
    if (s.vectors_n) d->tr->stream = d->stream;
    Stager stg{d};
    SolveRun r{d, c.low, {}};
    if (solve_prepare(s, d, stg, c, 0, 1, r.a)) return -1.0;
    Events ev(2 * iters);
    if (!ev.ok) { fail(SPMV_HIP_E_RUNTIME, "hipEventCreate"); return -1.0; }
    int rc = SPMV_HIP_OK;
    for (int run = -warmup; run < iters && !rc; ++run) {
        rc = solve_start(s, r, opt.use_x0 != 0);
        if (run >= 0) (void) hipEventRecord(ev[2 * run], d->stream);
        for (int it = 1; it <= opt.max_iterations && !rc; ++it) rc = s.iteration(s, r, it);
        if (run >= 0) (void) hipEventRecord(ev[2 * run + 1], d->stream);
    }
    const hipError_t e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) fail(SPMV_HIP_E_RUNTIME, "time_%s: %s", s.name, hipGetErrorString(e));
    if (rc || e != hipSuccess) return -1.0;
    double tot = 0;
    for (int i = 0; i < iters; ++i) {
        float ms = 0;
        (void) hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
        if (ms_out) ms_out[i] = ms;
        tot += ms;
    }
    return tot / iters;
}

// out[i] = the square root spmv_hip_gmres's kernels take of in[i]; n doubles each, device pointers; synchronous, on the null stream
extern "C" int spmv_shim_gmres_sqrt(const double *in, double *out, long long n)
{
    if (n == 0) return SPMV_HIP_OK;
    if (n < 0 || !in || !out || !is_device_ptr(in) || !is_device_ptr(out)) return fail(SPMV_HIP_E_ARG, "gmres_sqrt: need n >= 0 and device pointers");
    const hipError_t e = gmres_sqrt_launch(in, out, n, nullptr);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "gmres_sqrt: launch: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return SPMV_HIP_OK;
}

// ------------------------------------------------------------------------------------ spmv_hip_cg_mixed
// Conjugate gradients with reliable updates on a PAIR of handles (kernels/cg_mixed.hpp): the iterations are spmv_hip_cg's in float, on `low`'s
// multiply and on the partial solution y; when a segment ends, x + y goes through the fp64 handle's multiply and the TRUE residual replaces the
// recurrence's.  A look that finds a segment's end enqueues the update (mix_try, the fp64 multiply, mix_residual, mix_resume) and the loop
// enqueues the next batch behind it with no look in between; mix_resume re-arms the loop on the device, or ends the solve, in which case that
// batch's kernels return at once.  The iterations are numbered from the APPLIED count of the look (the arrays of <r,z> alternate by it), and so
// is the budget.  The workspace is the fp64 handle's: two vectors of m doubles, four of m floats; `low` is only multiplied with.
static int mix_admit(const Solver &s, const char *pre, const spmv_dev *hi, const spmv_dev *lo)
{
    if (!lo || !lo->built) return fail(SPMV_HIP_E_NOSTATE, "%s%s: schedule not built", pre, s.name);
    const char *why = nullptr;
    if (hi->vsize != sizeof(double) || lo->vsize != sizeof(float)) why = "`high` must be an fp64 handle and `low` an fp32 one";
    else if (hi->m != lo->m || hi->n != lo->n || hi->nnz != lo->nnz) why = "m, n or nnz differ between the two handles";
    else if (hi->device != lo->device) why = "the two handles are on different devices";
    else if (hi->stream != lo->stream) why = "the two handles are on different streams";
    return why ? fail(SPMV_HIP_E_ARG, "%s%s: %s", pre, s.name, why) : SPMV_HIP_OK;
}

// (q64 = A_high x0,) mix_residual + mix_resume
static int mix_start(const Solver &s, const SolveRun &r, bool use_x0)
{
    int rc;
    if (use_x0 && (rc = solve_multiply(r.d, r.a.x, r.a.vec[kMixVecQ64]))) return rc;
    return solve_launched(s, mix_start_launch(r.a, use_x0, r.d->stream));
}

// behind iteration k: xn = x + y, q64 = A_high xn, mix_residual + mix_resume
static int mix_update(const Solver &s, const SolveRun &r, int k, int update)
{
    int rc;
    if ((rc = solve_launched(s, mix_try_launch(r.a, r.d->stream))) || (rc = solve_multiply(r.d, r.a.vec[kMixVecXn], r.a.vec[kMixVecQ64]))) return rc;
    return solve_launched(s, mix_update_launch(r.a, k, update, r.d->stream));
}

// q = A_low p, then cg_dot, cg_update and mix_direction.  The timer (nostop), where no test ends a segment: update k / update_every behind every
// update_every-th iteration (none at 0), so that what is enqueued does not depend on the data; every update is committed
static int mix_iteration(const Solver &s, const SolveRun &r, int k)
{
    const SolveArgs &a = r.a;
    int rc;
    if ((rc = solve_multiply(r.low, a.vec[kMixVectors64 + kMixVecP], a.vec[kMixVectors64 + kMixVecQ])) || (rc = solve_launched(s, mix_iteration_launch(a, k, r.d->stream)))) return rc;
    return a.nostop && a.every > 0 && k % a.every == 0 ? mix_update(s, r, k, k / a.every) : SPMV_HIP_OK;
}

static void mix_look(const void *state, int k, SolveLook &l)
{
    single_look(state, k, l);
    l.updates = ((const MixState *) state)->updates;
}

// a segment's end: the update behind the applied iterations, and the loop goes on from them; mix_resume writes a final status only behind it
static bool mix_resume(const Solver &s, const SolveRun &r, const void *state, int &it, int &rc)
{
    const MixState &hs = *(const MixState *) state;
    if (!hs.segment_end) return false;
    it = hs.s.iterations;
    return !(rc = mix_update(s, r, it, hs.updates + 1));
}

// ------------------------------------------------------------------------------------ the six rows
// indexed by the solver ids of spmv_shim.h.  check_every: DESIGN 3.26 for CG.  BiCGStab's is from the sweep of tools/bicgstab_bench.py (DESIGN
// 3.27): a look costs 23-31 us; at 8 an iteration is within 3 % of the best figure of the sweep (32) on the 1e6-row case and within 0.3 % on the
// 1e7-row band, and what a larger value saves per iteration it loses again behind convergence, where on average check_every - 1 multiplies are wasted.
// The k-column solve and the mixed one keep CG's 8; spmv_hip_lsqr's is from the sweep of tools/lsqr_bench.py
static const Solver kSolvers[SPMV_SHIM_SOLVE_COUNT] = {
    {SPMV_SHIM_SOLVE_CG, "cg", kCgVectors, 0, 0, kCgPartArrays, 0, 1, 8, sizeof(SolveState), 256, 0, STAGE_CG_B, STAGE_CG_X, cg_start, cg_iteration, single_look, nullptr, nullptr, nullptr},
    {SPMV_SHIM_SOLVE_BICGSTAB, "bicgstab", kBicgVectors, 0, 0, kBicgPartArrays, 0, 1, 8, sizeof(SolveState), 256, 0, STAGE_CG_B, STAGE_CG_X, bicg_start, bicg_iteration, single_look, nullptr,
     nullptr, nullptr},
    {SPMV_SHIM_SOLVE_CG_COLUMNS, "cg_columns", kCcgVectors, 0, 0, kCcgPartArrays, 0, kCcgMaxK, 8, sizeof(ColsState), 1024, 0, STAGE_CGC_B, STAGE_CGC_X, ccg_start, ccg_iteration, cols_look,
     nullptr, nullptr, nullptr},
    {SPMV_SHIM_SOLVE_GMRES, "gmres", kGmresVectors, 0, 0, kGmresPartArrays, 1, 1, 8, sizeof(GmresState), kGmresStateRoom, 0, STAGE_CG_B, STAGE_CG_X, gmres_start, gmres_iteration, single_look,
     gmres_finish, nullptr, nullptr},
    {SPMV_SHIM_SOLVE_CG_MIXED, "cg_mixed", kMixVectors64, kMixVectors32, 0, kMixPartArrays, 0, 1, 8, sizeof(MixState), 256, sizeof(float), STAGE_CG_B, STAGE_CG_X, mix_start, mix_iteration,
     mix_look, nullptr, mix_resume, mix_admit},
    {SPMV_SHIM_SOLVE_LSQR, "lsqr", kLsqrVectorsM, 0, kLsqrVectorsN, kLsqrPartArrays, 0, 1, 8, sizeof(LsqrState), 256, 0, STAGE_CG_B, STAGE_CG_X, lsqr_start, lsqr_iteration, lsqr_look, nullptr,
     nullptr, nullptr},
};

static const Solver *solve_row(const spmv_solve_call *c)
{
    if (c && c->solver >= 0 && c->solver < SPMV_SHIM_SOLVE_COUNT) return &kSolvers[c->solver];
    fail(SPMV_HIP_E_ARG, "solve: no call, or no such solver");
    return nullptr;
}

extern "C" int spmv_shim_solve(spmv_dev *d, const spmv_solve_call *c)
{
    const Solver *s = solve_row(c);
    return s ? solve_run(*s, d, *c) : SPMV_HIP_E_ARG;
}

extern "C" double spmv_shim_time_solve(spmv_dev *d, const spmv_solve_call *c, int warmup, int iters, float *ms_out)
{
    const Solver *s = solve_row(c);
    return s ? solve_time(*s, d, *c, warmup, iters, ms_out) : -1.0;
}
