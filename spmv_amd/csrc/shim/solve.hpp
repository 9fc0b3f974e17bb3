// shim/solve.hpp -- part of spmv_shim.hip: the solves on the RESIDENT matrix that stay on the device, conjugate gradients (spmv_hip_cg),
// BiCGStab (spmv_hip_bicgstab) and conjugate gradients for k right-hand sides at once (spmv_hip_cg_columns), and their timers.  The vector
// kernels are kernels/cg.hpp, kernels/bicgstab.hpp and kernels/cg_columns.hpp, launched from their own translation unit (spmv_solve.hip); the
// multiplies -- q = A p, or v = A ph and t = A sh -- are launch<T>() on workspace vectors: the launch spmv_shim_run makes, without its staging:
// the handle's own schedule, spmv()'s bits.  For k columns the multiply is spmm_panels() on the compact workspace vectors: the launches
// spmv_shim_spmm makes, without its staging: spmv_hip_spmm's bits.
//
// The host enqueues `check_every` iterations, copies the state back and synchronises ONCE; inside a batch nothing waits for the host: alpha,
// (omega,) beta and the stop tests are derived on the device (kernels/cg.hpp), and once the state says that the loop has ended every later
// kernel of the batch returns at once -- what is wasted is at most check_every - 1 multiplies into the scratch vector q (BiCGStab:
// 2 check_every - 1 into v and t).  The returned x, iterations and history therefore do not depend on check_every.  With k columns the state
// holds k of everything; the loop ends when every column has ended.
//
// Everything here is written once; a solver is a Solver: its sizes, its workspace, what its start and one iteration enqueue and how its
// state reads.  k, ldb and ldx are 1 for the single solves.  spmv_hip_gmres (kernels/gmres.hpp) is the fourth: its workspace has `restart`
// vectors more than its fixed three, and it alone has a `finish`: the columns of an unfinished cycle are applied to x behind the last look.
// spmv_hip_cg_mixed (kernels/cg_mixed.hpp), at the end of this file, is not a Solver: it solves on a pair of handles with vectors of two types.
#pragma once

// what the host reads out of a solver's state, per column
struct SolveLook {
    bool done[kCcgMaxK];
    int status[kCcgMaxK], iterations[kCcgMaxK];
    double rr[kCcgMaxK], bb[kCcgMaxK];
};

struct Solver {
    const char *name;                 // in error texts
    int vectors, part_arrays;         // workspace vectors of m k elements; partial arrays of kCgMaxParts doubles PER COLUMN
    int vectors_per_step;             // spmv_hip_gmres: further vectors per step of a cycle; its workspace is sized by `restart`, not by k (0: by k)
    int check_every;                  // iterations between two looks at the state when the caller leaves check_every at 0
    size_t state_bytes, state_room;   // the device state: what is zeroed and copied, and the bytes behind the partial arrays that hold it
    void *spmv_dev::*ws;              // the workspace: the vectors, the partial arrays, the state
    int spmv_dev::*ws_k;              // the columns that workspace holds; nullptr: the solver has one column
    StageBuf spmv_dev::*hist;         // the history block
    int stage_b, stage_x;             // the stage buffers of host B and X
    int (*start)(const Solver &s, spmv_dev *d, const SolveArgs &a, bool use_x0); // behind the zeroed state: (A x0,) the init and begin kernels
    int (*iteration)(const Solver &s, spmv_dev *d, const SolveArgs &a, int k);   // iteration k >= 1: the multiplies and the vector kernels
    void (*look)(const void *state, int k, SolveLook &l);                         // a host copy of the state -> what it says
    int (*finish)(const Solver &s, spmv_dev *d, const SolveArgs &a, const void *state); // nullptr, or what the last look's state still asks for
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
static int cg_start(const Solver &s, spmv_dev *d, const SolveArgs &a, bool use_x0)
{
    int rc;
    if (use_x0 && (rc = solve_multiply(d, a.x, a.vec[kCgVecQ]))) return rc;
    return solve_launched(s, cg_start_launch(a, use_x0, d->stream));
}

// q = A p, then the three vector kernels
static int cg_iteration(const Solver &s, spmv_dev *d, const SolveArgs &a, int k)
{
    const int rc = solve_multiply(d, a.vec[kCgVecP], a.vec[kCgVecQ]);
    return rc ? rc : solve_launched(s, cg_iteration_launch(a, k, d->stream));
}

// (v = A x0,) bicg_init + bicg_begin
static int bicg_start(const Solver &s, spmv_dev *d, const SolveArgs &a, bool use_x0)
{
    int rc;
    if (use_x0 && (rc = solve_multiply(d, a.x, a.vec[kBicgVecV]))) return rc;
    return solve_launched(s, bicg_start_launch(a, use_x0, d->stream));
}

// v = A ph, bicg_rv + bicg_half, t = A sh, bicg_ts + bicg_update + bicg_direction; without Dinv ph is p and sh is s, which is in r
static int bicg_iteration(const Solver &s, spmv_dev *d, const SolveArgs &a, int k)
{
    int rc;
    if ((rc = solve_multiply(d, a.vec[a.dinv ? kBicgVecY : kBicgVecP], a.vec[kBicgVecV])) || (rc = solve_launched(s, bicg_first_launch(a, k, d->stream)))) return rc;
    if ((rc = solve_multiply(d, a.vec[a.dinv ? kBicgVecY : kBicgVecR], a.vec[kBicgVecT]))) return rc;
    return solve_launched(s, bicg_second_launch(a, k, d->stream));
}

// (q = A X0 for all columns,) ccg_init + ccg_begin
static int ccg_start(const Solver &s, spmv_dev *d, const SolveArgs &a, bool use_x0)
{
    int rc;
    if (use_x0 && (rc = spmm_panels(d, a.k, (const char *) a.x, a.ldx, (char *) a.vec[kCcgVecQ], a.k))) return rc;
    return solve_launched(s, ccg_start_launch(a, use_x0, d->stream));
}

// q = A p for all columns in one pass over A, then the five vector kernels
static int ccg_iteration(const Solver &s, spmv_dev *d, const SolveArgs &a, int it)
{
    const int rc = spmm_panels(d, a.k, (const char *) a.vec[kCcgVecP], a.k, (char *) a.vec[kCcgVecQ], a.k);
    return rc ? rc : solve_launched(s, ccg_iteration_launch(a, it, d->stream));
}

// (w = A x0,) gmres_init + cg_begin + gmres_cycle + gmres_scale
static int gmres_start(const Solver &s, spmv_dev *d, const SolveArgs &a, bool use_x0)
{
    int rc;
    if (use_x0 && (rc = solve_multiply(d, a.x, a.base + kGmresVecW * a.stride))) return rc;
    return solve_launched(s, gmres_start_launch(a, use_x0, d->stream));
}

// step j = (k - 1) mod restart + 1 of its cycle: w = A z (z is v_j without Dinv), then the seven vector kernels, sized by j; at j = restart
// the cycle's end (gmres_solve + gmres_update_x) and the restart (w = A x, gmres_residual + gmres_cycle + gmres_scale) as well
static int gmres_iteration(const Solver &s, spmv_dev *d, const SolveArgs &a, int k)
{
    const int j = (k - 1) % a.restart + 1;
    int rc;
    if ((rc = solve_multiply(d, a.base + (a.dinv ? (size_t) kGmresVecZ : (size_t) (kGmresVecV + j - 1)) * a.stride, a.base + kGmresVecW * a.stride))) return rc;
    if ((rc = solve_launched(s, gmres_step_launch(a, k, j, d->stream))) || j < a.restart) return rc;
    if ((rc = solve_launched(s, gmres_apply_launch(a, 0, d->stream))) || (rc = solve_multiply(d, a.x, a.base + kGmresVecW * a.stride))) return rc;
    return solve_launched(s, gmres_restart_launch(a, d->stream));
}

// the loop ended, or the budget ran out, in the middle of a cycle: the columns the state names go into x
static int gmres_finish(const Solver &s, spmv_dev *d, const SolveArgs &a, const void *state)
{
    return ((const GmresState *) state)->pending > 0 ? solve_launched(s, gmres_apply_launch(a, 1, d->stream)) : SPMV_HIP_OK;
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

// indexed by the solver ids of spmv_shim.h.  check_every: DESIGN 3.26 for CG.  BiCGStab's is from the sweep of tools/bicgstab_bench.py (DESIGN
// 3.27): a look costs 23-31 us; at 8 an iteration is within 3 % of the best figure of the sweep (32) on the 1e6-row case and within 0.3 % on the
// 1e7-row band, and what a larger value saves per iteration it loses again behind convergence, where on average check_every - 1 multiplies are wasted.
// The k-column solve keeps CG's 8
static const Solver kSolvers[] = {
    {"cg", kCgVectors, kCgPartArrays, 0, 8, sizeof(SolveState), 256, &spmv_dev::cg_ws, nullptr, &spmv_dev::cg_hist, STAGE_CG_B, STAGE_CG_X, cg_start, cg_iteration, single_look, nullptr},
    {"bicgstab", kBicgVectors, kBicgPartArrays, 0, 8, sizeof(SolveState), 256, &spmv_dev::bicg_ws, nullptr, &spmv_dev::bicg_hist, STAGE_CG_B, STAGE_CG_X, bicg_start, bicg_iteration,
     single_look, nullptr},
    {"cg_columns", kCcgVectors, kCcgPartArrays, 0, 8, sizeof(ColsState), 1024, &spmv_dev::cgc_ws, &spmv_dev::cgc_k, &spmv_dev::cgc_hist, STAGE_CGC_B, STAGE_CGC_X, ccg_start,
     ccg_iteration, cols_look, nullptr},
    {"gmres", kGmresVectors, kGmresPartArrays, 1, 8, sizeof(GmresState), kGmresStateRoom, &spmv_dev::gmres_ws, &spmv_dev::gmres_restart, &spmv_dev::gmres_hist, STAGE_CG_B,
     STAGE_CG_X, gmres_start, gmres_iteration, single_look, gmres_finish},
};
static const Solver *solver_of(int id) { return id == SPMV_SHIM_SOLVE_CG || id == SPMV_SHIM_SOLVE_BICGSTAB ? &kSolvers[id] : nullptr; }
// a solver with k columns (its workspace is sized by k; spmv_hip_gmres's by restart)
static bool solve_has_columns(const Solver &s) { return s.ws_k && !s.vectors_per_step; }

// bytes of one workspace vector of m x k elements
static size_t solve_vec_bytes(const spmv_dev *d, int k) { return (d->vsize * (size_t) d->m * (size_t) k + 255) & ~(size_t) 255; }
// what a workspace sized by n (k columns; spmv_hip_gmres: restart n) holds: the columns of a vector, the vectors, the bytes behind them
static int solve_cols(const Solver &s, int n) { return s.vectors_per_step ? 1 : n; }
static int solve_vectors(const Solver &s, int n) { return s.vectors + s.vectors_per_step * n; }
static size_t solve_tail_bytes(const Solver &s, int n) { return sizeof(double) * s.part_arrays * (size_t) solve_cols(s, n) * kCgMaxParts + s.state_room; }
// the size n the solver's workspace was built for (0: none yet)
static int solve_ws_columns(const Solver &s, const spmv_dev *d) { return !(d->*s.ws) ? 0 : s.ws_k ? d->*s.ws_k : 1; }

// the vectors, the partial arrays (zeroed once: the entries behind the P in use stay +0.0) and the state: allocated at the solver's first solve --
// s.vectors * solve_vec_bytes(k) + 8 * s.part_arrays * k * 1024 + s.state_room bytes -- and, for a solver with columns, given back and
// allocated anew when a call has more columns than it holds (spmv_hip_gmres: a larger restart; its vectors are restart + 3 of m elements)
static int solve_workspace(const Solver &s, spmv_dev *d, int k)
{
    static_assert(sizeof(SolveState) <= 256 && sizeof(ColsState) <= 1024 && sizeof(GmresState) <= kGmresStateRoom, "the state's room behind the partial arrays");
    const int have = solve_ws_columns(s, d);
    if (have >= k) return SPMV_HIP_OK;
    if (have) {
        quiesce(d);
        (void) pool_free(d->*s.ws);
        d->device_bytes -= (long long) (solve_vectors(s, have) * solve_vec_bytes(d, solve_cols(s, have)) + solve_tail_bytes(s, have));
        d->*s.ws = nullptr;
    }
    const size_t vec = solve_vec_bytes(d, solve_cols(s, k)), tail = solve_tail_bytes(s, k);
    ALLOC_TRY(d, &(d->*s.ws), solve_vectors(s, k) * vec + tail, false);
    if (s.ws_k) d->*s.ws_k = k;
    HIP_TRY(hipMemsetAsync((char *) (d->*s.ws) + solve_vectors(s, k) * vec, 0, tail, d->stream));
    return SPMV_HIP_OK;
}

// One solve's device operands: the workspace carved up (by the columns it HOLDS, so that a partial array never lies where a vector did), host
// B / X / Dinv staged (X's copy-back registered with the stager; the initial guess copied in when it is wanted; the single solves share their
// stage buffers, and all three Dinv's: the calls are synchronous, so they never hold them at the same time), the history block, the geometry
// of the dots.  m > 0.
static int solve_prepare(const Solver &s, spmv_dev *d, Stager &stg, int k, int restart, const void *b, long long ldb, void *x, long long ldx, const spmv_hip_cg_options *opt,
                         size_t hist_entries, int nostop, SolveArgs &a)
{
    int rc = solve_workspace(s, d, s.vectors_per_step ? restart : k);
    if (rc) return rc;
    const int held = solve_ws_columns(s, d), vectors = solve_vectors(s, held);
    const size_t vec = solve_vec_bytes(d, solve_cols(s, held)), m = (size_t) d->m;
    char *ws = (char *) (d->*s.ws);
    a.m = d->m;
    a.k = k;
    a.restart = restart;
    a.base = ws;
    a.stride = vec;
    const long long chunks = ((long long) d->m + kCgChunk - 1) / kCgChunk;
    a.parts = (int) (chunks < kCgMaxParts ? chunks : kCgMaxParts);
    a.span = (long long) kCgChunk * (((long long) d->m + (long long) kCgChunk * a.parts - 1) / ((long long) kCgChunk * a.parts));
    for (int i = 0; i < vectors && i < (int) (sizeof(a.vec) / sizeof(a.vec[0])); ++i) a.vec[i] = ws + i * vec;
    a.part = (double *) (ws + vectors * vec);
    void *state = ws + vectors * vec + sizeof(double) * s.part_arrays * (size_t) solve_cols(s, held) * kCgMaxParts;
    if (solve_has_columns(s)) a.cols = (ColsState *) state;
    else a.state = (SolveState *) state;
    a.rtol2 = opt->rtol * opt->rtol;
    a.atol2 = opt->atol * opt->atol;
    a.nostop = nostop;
    a.f64 = d->vsize == sizeof(double);
    a.b = b;
    a.dinv = opt->Dinv;
    a.x = x;
    a.ldb = ldb;
    a.ldx = ldx;
    long long ld = 1;
    if ((rc = stg.in(d->stage[s.stage_b], a.b, a.ldb, m, k)) || (rc = stg.in(d->stage[STAGE_CG_DINV], a.dinv, ld, m, 1)) || (rc = stg.out(d->stage[s.stage_x], a.x, a.ldx, m, k))) return rc;
    if (a.x != x && opt->use_x0) HIP_TRY(stg.copy(a.x, (size_t) k, x, (size_t) ldx, m, (size_t) k, hipMemcpyHostToDevice, d->vsize));
    // 16-byte accesses: B and X compact and aligned; the single solves' kernels read Dinv that way too, the k-column ones by element
    a.wide = a.ldb == k && a.ldx == k && wide_ok(a.b, 1, 16) && wide_ok(a.x, 1, 16) && (solve_has_columns(s) || !a.dinv || wide_ok(a.dinv, 1, 16));
    a.hist = nullptr;
    if (hist_entries > 0) {
        if ((rc = stg.reserve(d->*s.hist, sizeof(double) * hist_entries))) return rc;
        a.hist = (double *) (d->*s.hist).p;
    }
    return SPMV_HIP_OK;
}

static void *solve_state(const Solver &s, const SolveArgs &a) { return solve_has_columns(s) ? (void *) a.cols : (void *) a.state; }

// the state zeroed, then the solver's start
static int solve_start(const Solver &s, spmv_dev *d, const SolveArgs &a, bool use_x0)
{
    HIP_TRY(hipMemsetAsync(solve_state(s, a), 0, s.state_bytes, d->stream));
    return s.start(s, d, a, use_x0);
}

// res: k entries.  history (k > 1): entry [it * k + j] is column j's rr after iteration it, written for it <= that column's iterations
static int solve_run(const Solver &s, spmv_dev *d, int k, int restart, const void *b, long long ldb, void *x, long long ldx, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "%s: schedule not built", s.name);
    if (!opt || !res) return fail(SPMV_HIP_E_ARG, "%s: opt or res is NULL", s.name);
    const bool cols = solve_has_columns(s);
    if (k < 1 || k > (cols ? kCcgMaxK : 1) || ldb < k || ldx < k) return fail(SPMV_HIP_E_ARG, "%s: need 1 <= k <= %d, ldb >= k, ldx >= k", s.name, cols ? kCcgMaxK : 1);
    if (s.vectors_per_step && (restart < 1 || restart > kGmresMaxRestart)) return fail(SPMV_HIP_E_ARG, "%s: need 1 <= restart <= %d", s.name, kGmresMaxRestart);
    if (d->m != d->n) return fail(SPMV_HIP_E_ARG, "%s: the matrix is %d x %d, not square", s.name, d->m, d->n);
    if (d->m > 0 && (!b || !x)) return fail(SPMV_HIP_E_ARG, "%s: B or X is NULL", s.name);
    if (cols && d->nnz > 0 && !d->colidx) return fail(SPMV_HIP_E_NOSTATE, "%s: the resident column indices were released (spmv_shim_restore_columns first)", s.name);
    for (int j = 0; j < k; ++j) {
        res[j].status = SPMV_HIP_CG_CONVERGED;
        res[j].iterations = 0;
        res[j].rr = res[j].bb = 0;
    }
    if (d->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    int rc;
    if (cols && (rc = spmm_plan(d))) return rc;
    Stager stg{d};
    SolveArgs a;
    rc = solve_prepare(s, d, stg, k, restart, b, ldb, x, ldx, opt, opt->history ? ((size_t) opt->max_iterations + 1) * (size_t) k : 0, 0, a);
    if (rc || (rc = solve_start(s, d, a, opt->use_x0 != 0))) return rc;
    const int every = opt->check_every > 0 ? opt->check_every : s.check_every;
    alignas(8) unsigned char hs[sizeof(GmresState) > sizeof(ColsState) ? sizeof(GmresState) : sizeof(ColsState)];
    static_assert(sizeof(hs) >= sizeof(SolveState), "the largest state");
    SolveLook l;
    for (int it = 0;;) {
        HIP_TRY(hipMemcpyAsync(hs, solve_state(s, a), s.state_bytes, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        s.look(hs, k, l);
        bool done = true;
        for (int j = 0; j < k; ++j) done = done && l.done[j];
        if (done || it >= opt->max_iterations) break;
        const int stop = opt->max_iterations - it < every ? opt->max_iterations : it + every;
        while (it < stop)
            if ((rc = s.iteration(s, d, a, ++it))) return rc;
    }
    if (s.finish && (rc = s.finish(s, d, a, hs))) return rc;
    int longest = 0;
    for (int j = 0; j < k; ++j) {
        res[j].status = l.done[j] ? l.status[j] : SPMV_HIP_CG_MAX_ITERATIONS;
        res[j].iterations = l.iterations[j];
        res[j].rr = l.rr[j];
        res[j].bb = l.bb[j];
        if (l.iterations[j] > longest) longest = l.iterations[j];
        if (!(l.done[j] && l.status[j] == SPMV_HIP_CG_CONVERGED && l.bb[j] == 0)) continue;
        // B = 0: x = 0
        if (k == 1 && a.ldx == 1) HIP_TRY(hipMemsetAsync(a.x, 0, d->vsize * (size_t) d->m, d->stream));
        else HIP_TRY(hipMemset2DAsync((char *) a.x + d->vsize * (size_t) j, d->vsize * (size_t) a.ldx, 0, d->vsize, (size_t) d->m, d->stream));
    }
    std::vector<double> hist;
    if (opt->history && k == 1) HIP_TRY(hipMemcpyAsync(opt->history, a.hist, sizeof(double) * ((size_t) longest + 1), hipMemcpyDeviceToHost, d->stream));
    if (opt->history && k > 1) {
        hist.resize(((size_t) longest + 1) * (size_t) k);
        HIP_TRY(hipMemcpyAsync(hist.data(), a.hist, sizeof(double) * hist.size(), hipMemcpyDeviceToHost, d->stream));
    }
    if ((rc = stg.finish())) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream)); // the call is synchronous whatever the handle's async setting
    for (size_t i = 0; i < hist.size(); ++i) // the entries behind a column's end stay the caller's
        if ((int) (i / (size_t) k) <= l.iterations[i % (size_t) k]) opt->history[i] = hist[i];
    return SPMV_HIP_OK;
}

// `warmup` untimed + `iters` timed RUNS of opt->max_iterations iterations each, the stop tests disabled: every run starts again from B (and
// X when use_x0), its iterations are enqueued back to back and bracketed by two events on the handle's stream (the start is outside them:
// not state.hpp's time_events, which brackets a whole call).  ms_out[i] (may be NULL): run i.  Mean ms per run, < 0 on failure.  Device pointers only.
static double solve_time(const Solver &s, spmv_dev *d, int k, int restart, const void *b, long long ldb, void *x, long long ldx, const spmv_hip_cg_options *opt, int warmup, int iters,
                         float *ms_out)
{
    if (!d || !d->built || !opt || iters <= 0 || warmup < 0 || opt->max_iterations < 1 || d->m != d->n || d->m <= 0 || k < 1 || k > (solve_has_columns(s) ? kCcgMaxK : 1) || ldb < k || ldx < k ||
        (s.vectors_per_step && (restart < 1 || restart > kGmresMaxRestart))) {
        fail(SPMV_HIP_E_ARG, "time_%s: bad arguments", s.name);
        return -1.0;
    }
    if (!is_device_ptr(b) || !is_device_ptr(x) || (opt->Dinv && !is_device_ptr(opt->Dinv))) { fail(SPMV_HIP_E_ARG, "time_%s: B, X and Dinv must be device pointers", s.name); return -1.0; }
    if (solve_has_columns(s) && d->nnz > 0 && !d->colidx) { fail(SPMV_HIP_E_NOSTATE, "time_%s: the resident column indices were released", s.name); return -1.0; }
    DeviceGuard guard(d->device);
    if (!guard.ok) { fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device); return -1.0; }
    if (solve_has_columns(s) && spmm_plan(d)) return -1.0;
    Stager stg{d};
    SolveArgs a;
    if (solve_prepare(s, d, stg, k, restart, b, ldb, x, ldx, opt, 0, 1, a)) return -1.0;
    Events ev(2 * iters);
    if (!ev.ok) { fail(SPMV_HIP_E_RUNTIME, "hipEventCreate"); return -1.0; }
    int rc = SPMV_HIP_OK;
    for (int run = -warmup; run < iters && !rc; ++run) {
        rc = solve_start(s, d, a, opt->use_x0 != 0);
        if (run >= 0) (void) hipEventRecord(ev[2 * run], d->stream);
        for (int it = 1; it <= opt->max_iterations && !rc; ++it) rc = s.iteration(s, d, a, it);
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

extern "C" int spmv_shim_solve(int solver, spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    const Solver *s = solver_of(solver);
    return s ? solve_run(*s, d, 1, 0, b, 1, x, 1, opt, res) : fail(SPMV_HIP_E_ARG, "solve: no solver %d", solver);
}

extern "C" double spmv_shim_time_solve(int solver, spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out)
{
    const Solver *s = solver_of(solver);
    if (!s) { fail(SPMV_HIP_E_ARG, "time_solve: no solver %d", solver); return -1.0; }
    return solve_time(*s, d, 1, 0, b, 1, x, 1, opt, warmup, iters, ms_out);
}

extern "C" int spmv_shim_solve_columns(spmv_dev *d, int k, const void *b, long long ldb, void *x, long long ldx, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    return solve_run(kSolvers[SPMV_SHIM_SOLVE_CG_COLUMNS], d, k, 0, b, ldb, x, ldx, opt, res);
}

extern "C" double spmv_shim_time_solve_columns(spmv_dev *d, int k, const void *b, long long ldb, void *x, long long ldx, const spmv_hip_cg_options *opt, int warmup, int iters,
                                               float *ms_out)
{
    return solve_time(kSolvers[SPMV_SHIM_SOLVE_CG_COLUMNS], d, k, 0, b, ldb, x, ldx, opt, warmup, iters, ms_out);
}

extern "C" int spmv_shim_solve_gmres(spmv_dev *d, int restart, const void *b, void *x, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    return solve_run(kSolvers[SPMV_SHIM_SOLVE_GMRES], d, 1, restart, b, 1, x, 1, opt, res);
}

extern "C" double spmv_shim_time_solve_gmres(spmv_dev *d, int restart, const void *b, void *x, const spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out)
{
    return solve_time(kSolvers[SPMV_SHIM_SOLVE_GMRES], d, 1, restart, b, 1, x, 1, opt, warmup, iters, ms_out);
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
// Conjugate gradients with reliable updates on a PAIR of handles (kernels/cg_mixed.hpp): the iterations are spmv_hip_cg's in float, on `lo`'s
// multiply and on the partial solution y; when a segment ends, x + y goes through `hi`'s fp64 multiply and the TRUE residual replaces the
// recurrence's.  The loop is solve_run's -- check_every iterations, one look -- with one thing more: a look that finds a segment's end enqueues
// the update (mix_try, hi's multiply, mix_residual, mix_resume) and the next batch behind it with no look in between; mix_resume re-arms the
// loop on the device, or ends the solve, in which case that batch's kernels return at once.  The iterations are numbered from the APPLIED
// count of the look (the arrays of <r,z> alternate by it), and so is the budget.  The workspace is hi's, of this solver's own; lo is only
// multiplied with.

// bytes of the workspace: two vectors of m doubles, four of m floats, the partial arrays, the state
static size_t mix_vec_bytes(const spmv_dev *d, size_t elem) { return (elem * (size_t) d->m + 255) & ~(size_t) 255; }
static size_t mix_tail_bytes() { return sizeof(double) * kMixPartArrays * kCgMaxParts + 256; }

static const char *mix_pair_error(const spmv_dev *hi, const spmv_dev *lo)
{
    if (hi->vsize != sizeof(double) || lo->vsize != sizeof(float)) return "`high` must be an fp64 handle and `low` an fp32 one";
    if (hi->m != lo->m || hi->n != lo->n || hi->nnz != lo->nnz) return "m, n or nnz differ between the two handles";
    if (hi->m != hi->n) return "the matrix is not square";
    if (hi->device != lo->device) return "the two handles are on different devices";
    if (hi->stream != lo->stream) return "the two handles are on different streams";
    return nullptr;
}

static int mix_prepare(spmv_dev *hi, Stager &stg, const double *b, double *x, const spmv_hip_cg_mixed_options *opt, size_t hist_entries, int nostop, MixArgs &a)
{
    static_assert(sizeof(MixState) <= 256, "the state's room behind the partial arrays");
    const size_t v64 = mix_vec_bytes(hi, sizeof(double)), v32 = mix_vec_bytes(hi, sizeof(float)), m = (size_t) hi->m;
    if (!hi->mix_ws) {
        ALLOC_TRY(hi, &hi->mix_ws, kMixVectors64 * v64 + kMixVectors32 * v32 + mix_tail_bytes(), false);
        HIP_TRY(hipMemsetAsync((char *) hi->mix_ws + kMixVectors64 * v64 + kMixVectors32 * v32, 0, mix_tail_bytes(), hi->stream));
    }
    char *ws = (char *) hi->mix_ws, *w32 = ws + kMixVectors64 * v64;
    a.m = hi->m;
    const long long chunks = ((long long) hi->m + kCgChunk - 1) / kCgChunk;
    a.parts = (int) (chunks < kCgMaxParts ? chunks : kCgMaxParts);
    a.span = (long long) kCgChunk * (((long long) hi->m + (long long) kCgChunk * a.parts - 1) / ((long long) kCgChunk * a.parts));
    a.xn = (double *) (ws + kMixVecXn * v64);
    a.q64 = (double *) (ws + kMixVecQ64 * v64);
    a.r = (float *) (w32 + kMixVecR * v32);
    a.p = (float *) (w32 + kMixVecP * v32);
    a.q = (float *) (w32 + kMixVecQ * v32);
    a.y = (float *) (w32 + kMixVecY * v32);
    a.part = (double *) (w32 + kMixVectors32 * v32);
    a.state = (MixState *) (a.part + (size_t) kMixPartArrays * kCgMaxParts);
    a.rtol2 = opt->rtol * opt->rtol;
    a.atol2 = opt->atol * opt->atol;
    const double drop = opt->update_drop > 0 ? opt->update_drop : SPMV_HIP_CG_MIXED_UPDATE_DROP;
    a.drop2 = drop * drop;
    a.every = opt->update_every;
    a.budget = opt->max_iterations;
    a.nostop = nostop;
    a.b = b;
    a.x = x;
    a.dinv = opt->Dinv;
    int rc;
    long long ld = 1, ldb = 1, ldx = 1;
    if ((rc = stg.in(hi->stage[STAGE_CG_B], a.b, ldb, m, 1)) || (rc = stg.in(hi->stage[STAGE_CG_DINV], a.dinv, ld, m, 1, sizeof(float))) || (rc = stg.out(hi->stage[STAGE_CG_X], a.x, ldx, m, 1)))
        return rc;
    if (a.x != x && opt->use_x0) HIP_TRY(hipMemcpyAsync(a.x, x, sizeof(double) * m, hipMemcpyHostToDevice, hi->stream));
    a.wide = wide_ok(a.b, 1, 16) && wide_ok(a.x, 1, 16) && (!a.dinv || wide_ok(a.dinv, 1, 16));
    a.hist = nullptr;
    if (hist_entries > 0) {
        if ((rc = stg.reserve(hi->mix_hist, sizeof(double) * hist_entries))) return rc;
        a.hist = (double *) hi->mix_hist.p;
    }
    return SPMV_HIP_OK;
}

static int mix_launched(hipError_t e) { return e == hipSuccess ? SPMV_HIP_OK : fail(SPMV_HIP_E_RUNTIME, "cg_mixed: launch: %s", hipGetErrorString(e)); }

// the state zeroed, (q64 = A_high x0,) mix_residual + mix_resume
static int mix_start(spmv_dev *hi, const MixArgs &a, bool use_x0)
{
    int rc;
    HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(MixState), hi->stream));
    if (use_x0 && (rc = launch<double>(hi, a.x, a.q64))) return rc;
    return mix_launched(mix_start_launch(a, use_x0, hi->stream));
}

// q = A_low p, then cg_dot, cg_update and mix_direction
static int mix_iteration(spmv_dev *hi, spmv_dev *lo, const MixArgs &a, int k)
{
    const int rc = launch<float>(lo, a.p, a.q);
    return rc ? rc : mix_launched(mix_iteration_launch(a, k, hi->stream));
}

// behind iteration k: xn = x + y, q64 = A_high xn, mix_residual + mix_resume
static int mix_update(spmv_dev *hi, const MixArgs &a, int k, int update)
{
    int rc;
    if ((rc = mix_launched(mix_try_launch(a, hi->stream))) || (rc = launch<double>(hi, a.xn, a.q64))) return rc;
    return mix_launched(mix_update_launch(a, k, update, hi->stream));
}

extern "C" int spmv_shim_solve_mixed(spmv_dev *hi, spmv_dev *lo, const double *b, double *x, const spmv_hip_cg_mixed_options *opt, spmv_hip_cg_mixed_result *res)
{
    if (!hi || !hi->built || !lo || !lo->built) return fail(SPMV_HIP_E_NOSTATE, "cg_mixed: schedule not built");
    if (!opt || !res) return fail(SPMV_HIP_E_ARG, "cg_mixed: opt or res is NULL");
    if (const char *why = mix_pair_error(hi, lo)) return fail(SPMV_HIP_E_ARG, "cg_mixed: %s", why);
    if (hi->m > 0 && (!b || !x)) return fail(SPMV_HIP_E_ARG, "cg_mixed: B or X is NULL");
    res->status = SPMV_HIP_CG_CONVERGED;
    res->iterations = res->updates = 0;
    res->rr = res->bb = 0;
    if (hi->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(hi->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", hi->device);
    Stager stg{hi};
    MixArgs a;
    int rc = mix_prepare(hi, stg, b, x, opt, opt->history ? (size_t) opt->max_iterations + 1 : 0, 0, a);
    if (rc || (rc = mix_start(hi, a, opt->use_x0 != 0))) return rc;
    const int every = opt->check_every > 0 ? opt->check_every : 8;
    MixState hs;
    // every look but the last is followed by an applied iteration or by an update
    for (long long looks = 0;; ++looks) {
        HIP_TRY(hipMemcpyAsync(&hs, a.state, sizeof hs, hipMemcpyDeviceToHost, hi->stream));
        HIP_TRY(hipStreamSynchronize(hi->stream));
        const bool ended = hs.s.end_update || hs.s.end_direction;
        int k = hs.s.iterations;
        if ((ended && !hs.segment_end) || (!ended && k >= opt->max_iterations)) break;
        if (looks > 2ll * opt->max_iterations + 2) return fail(SPMV_HIP_E_RUNTIME, "cg_mixed: the device's state does not advance");
        if (ended && (rc = mix_update(hi, a, k, hs.updates + 1))) return rc;
        const int stop = opt->max_iterations - k < every ? opt->max_iterations : k + every;
        while (k < stop)
            if ((rc = mix_iteration(hi, lo, a, ++k))) return rc;
    }
    const bool ended = hs.s.end_update || hs.s.end_direction;
    res->status = ended ? hs.s.status : SPMV_HIP_CG_MAX_ITERATIONS;
    res->iterations = hs.s.iterations;
    res->updates = hs.updates;
    res->rr = hs.s.rr;
    res->bb = hs.s.bb;
    if (ended && hs.s.status == SPMV_HIP_CG_CONVERGED && hs.s.bb == 0) HIP_TRY(hipMemsetAsync(a.x, 0, sizeof(double) * (size_t) hi->m, hi->stream)); // B = 0: x = 0
    if (opt->history) HIP_TRY(hipMemcpyAsync(opt->history, a.hist, sizeof(double) * ((size_t) hs.s.iterations + 1), hipMemcpyDeviceToHost, hi->stream));
    if ((rc = stg.finish())) return rc;
    HIP_TRY(hipStreamSynchronize(hi->stream)); // the call is synchronous whatever the handle's async setting
    return SPMV_HIP_OK;
}

// solve_time for the pair: the stop tests off, an update behind every opt->update_every-th iteration (none when that is 0), so that what is
// enqueued does not depend on the data; every update is committed
extern "C" double spmv_shim_time_solve_mixed(spmv_dev *hi, spmv_dev *lo, const double *b, double *x, const spmv_hip_cg_mixed_options *opt, int warmup, int iters, float *ms_out)
{
    if (!hi || !hi->built || !lo || !lo->built || !opt || iters <= 0 || warmup < 0 || opt->max_iterations < 1 || hi->m <= 0 || opt->update_every < 0) {
        fail(SPMV_HIP_E_ARG, "time_cg_mixed: bad arguments");
        return -1.0;
    }
    if (const char *why = mix_pair_error(hi, lo)) { fail(SPMV_HIP_E_ARG, "time_cg_mixed: %s", why); return -1.0; }
    if (!is_device_ptr(b) || !is_device_ptr(x) || (opt->Dinv && !is_device_ptr(opt->Dinv))) { fail(SPMV_HIP_E_ARG, "time_cg_mixed: B, X and Dinv must be device pointers"); return -1.0; }
    DeviceGuard guard(hi->device);
    if (!guard.ok) { fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", hi->device); return -1.0; }
    Stager stg{hi};
    MixArgs a;
    if (mix_prepare(hi, stg, b, x, opt, 0, 1, a)) return -1.0;
    Events ev(2 * iters);
    if (!ev.ok) { fail(SPMV_HIP_E_RUNTIME, "hipEventCreate"); return -1.0; }
    int rc = SPMV_HIP_OK;
    for (int run = -warmup; run < iters && !rc; ++run) {
        rc = mix_start(hi, a, opt->use_x0 != 0);
        if (run >= 0) (void) hipEventRecord(ev[2 * run], hi->stream);
        for (int it = 1, updates = 0; it <= opt->max_iterations && !rc; ++it) {
            rc = mix_iteration(hi, lo, a, it);
            if (!rc && opt->update_every > 0 && it % opt->update_every == 0) rc = mix_update(hi, a, it, ++updates);
        }
        if (run >= 0) (void) hipEventRecord(ev[2 * run + 1], hi->stream);
    }
    const hipError_t e = hipStreamSynchronize(hi->stream);
    if (e != hipSuccess) fail(SPMV_HIP_E_RUNTIME, "time_cg_mixed: %s", hipGetErrorString(e));
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
