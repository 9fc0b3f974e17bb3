// shim/solve.hpp -- part of spmv_shim.hip: the solves on the RESIDENT matrix that stay on the device, conjugate gradients (spmv_hip_cg) and
// BiCGStab (spmv_hip_bicgstab), and their timers.  The vector kernels are kernels/cg.hpp and kernels/bicgstab.hpp, launched from their own
// translation unit (spmv_solve.hip); the multiplies -- q = A p, or v = A ph and t = A sh -- are launch<T>() on workspace vectors: the launch
// spmv_shim_run makes, without its staging: the handle's own schedule, spmv()'s bits.
//
// The host enqueues `check_every` iterations, copies the state back and synchronises ONCE; inside a batch nothing waits for the host: alpha,
// (omega,) beta and the stop tests are derived on the device by every workgroup (kernels/cg.hpp), and once the state says that the loop has ended
// every later kernel of the batch returns at once -- what is wasted is at most check_every - 1 multiplies into the scratch vector q (BiCGStab:
// 2 check_every - 1 into v and t).  The returned x, iterations and history therefore do not depend on check_every.
//
// Everything here is written once; a solver is a Solver: its sizes, its workspace and what its start and one iteration enqueue.
#pragma once

struct Solver {
    const char *name;                 // in error texts
    int vectors, part_arrays;         // workspace vectors of m elements; partial arrays of kCgMaxParts doubles
    int check_every;                  // iterations between two looks at the state when the caller leaves check_every at 0
    void *spmv_dev::*ws;              // the workspace: the vectors, the partial arrays, the state
    StageBuf spmv_dev::*hist;         // the history block
    int (*start)(const Solver &s, spmv_dev *d, const SolveArgs &a, bool use_x0); // behind the zeroed state: (A x0,) the init and begin kernels
    int (*iteration)(const Solver &s, spmv_dev *d, const SolveArgs &a, int k);   // iteration k >= 1: the multiplies and the vector kernels
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

// indexed by the solver ids of spmv_shim.h.  check_every: DESIGN 3.26 for CG.  BiCGStab's is from the sweep of tools/bicgstab_bench.py (DESIGN
// 3.27): a look costs 23-31 us; at 8 an iteration is within 3 % of the best figure of the sweep (32) on the 1e6-row case and within 0.3 % on the
// 1e7-row band, and what a larger value saves per iteration it loses again behind convergence, where on average check_every - 1 multiplies are wasted
static const Solver kSolvers[] = {
    {"cg", kCgVectors, kCgPartArrays, 8, &spmv_dev::cg_ws, &spmv_dev::cg_hist, cg_start, cg_iteration},
    {"bicgstab", kBicgVectors, kBicgPartArrays, 8, &spmv_dev::bicg_ws, &spmv_dev::bicg_hist, bicg_start, bicg_iteration},
};
static const Solver *solver_of(int id) { return id == SPMV_SHIM_SOLVE_CG || id == SPMV_SHIM_SOLVE_BICGSTAB ? &kSolvers[id] : nullptr; }

static size_t solve_vec_bytes(const spmv_dev *d) { return (d->vsize * (size_t) d->m + 255) & ~(size_t) 255; }

// the vectors, the partial arrays (zeroed once: the entries behind the P in use stay +0.0) and the state: allocated at the solver's first solve
static int solve_workspace(const Solver &s, spmv_dev *d)
{
    static_assert(sizeof(SolveState) <= 256, "the state has 256 bytes behind the partial arrays");
    if (d->*s.ws) return SPMV_HIP_OK;
    const size_t vec = solve_vec_bytes(d), tail = sizeof(double) * s.part_arrays * kCgMaxParts + 256;
    ALLOC_TRY(d, &(d->*s.ws), s.vectors * vec + tail, false);
    HIP_TRY(hipMemsetAsync((char *) (d->*s.ws) + s.vectors * vec, 0, tail, d->stream));
    return SPMV_HIP_OK;
}

// One solve's device operands: the workspace carved up, host B / X / Dinv staged (X's copy-back registered with the stager; the initial
// guess copied in when it is wanted; the solvers share the stage buffers: both calls are synchronous, so they never hold them at the same
// time), the history block, the geometry of the dots.  m > 0.
static int solve_prepare(const Solver &s, spmv_dev *d, Stager &stg, const void *b, void *x, const spmv_hip_cg_options *opt, size_t hist_entries, int nostop, SolveArgs &a)
{
    int rc = solve_workspace(s, d);
    if (rc) return rc;
    const size_t vec = solve_vec_bytes(d), m = (size_t) d->m;
    char *ws = (char *) (d->*s.ws);
    a.m = d->m;
    const long long chunks = ((long long) d->m + kCgChunk - 1) / kCgChunk;
    a.parts = (int) (chunks < kCgMaxParts ? chunks : kCgMaxParts);
    a.span = (long long) kCgChunk * (((long long) d->m + (long long) kCgChunk * a.parts - 1) / ((long long) kCgChunk * a.parts));
    for (int i = 0; i < s.vectors; ++i) a.vec[i] = ws + i * vec;
    a.part = (double *) (ws + s.vectors * vec);
    a.state = (SolveState *) (ws + s.vectors * vec + sizeof(double) * s.part_arrays * kCgMaxParts);
    a.rtol2 = opt->rtol * opt->rtol;
    a.atol2 = opt->atol * opt->atol;
    a.nostop = nostop;
    a.f64 = d->vsize == sizeof(double);
    a.b = b;
    a.dinv = opt->Dinv;
    a.x = x;
    long long ld = 1;
    if ((rc = stg.in(d->stage[STAGE_CG_B], a.b, ld, m, 1)) || (rc = stg.in(d->stage[STAGE_CG_DINV], a.dinv, ld, m, 1)) || (rc = stg.out(d->stage[STAGE_CG_X], a.x, ld, m, 1))) return rc;
    if (a.x != x && opt->use_x0) HIP_TRY(hipMemcpyAsync(a.x, x, d->vsize * m, hipMemcpyHostToDevice, d->stream));
    a.wide = wide_ok(a.b, 1, 16) && wide_ok(a.x, 1, 16) && (!a.dinv || wide_ok(a.dinv, 1, 16));
    a.hist = nullptr;
    if (hist_entries > 0) {
        if ((rc = stg.reserve(d->*s.hist, sizeof(double) * hist_entries))) return rc;
        a.hist = (double *) (d->*s.hist).p;
    }
    return SPMV_HIP_OK;
}

// the state zeroed, then the solver's start
static int solve_start(const Solver &s, spmv_dev *d, const SolveArgs &a, bool use_x0)
{
    HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(SolveState), d->stream));
    return s.start(s, d, a, use_x0);
}

static int solve_run(const Solver &s, spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "%s: schedule not built", s.name);
    if (!opt || !res) return fail(SPMV_HIP_E_ARG, "%s: opt or res is NULL", s.name);
    if (d->m != d->n) return fail(SPMV_HIP_E_ARG, "%s: the matrix is %d x %d, not square", s.name, d->m, d->n);
    if (d->m > 0 && (!b || !x)) return fail(SPMV_HIP_E_ARG, "%s: B or X is NULL", s.name);
    res->status = SPMV_HIP_CG_CONVERGED;
    res->iterations = 0;
    res->rr = res->bb = 0;
    if (d->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    Stager stg{d};
    SolveArgs a;
    int rc = solve_prepare(s, d, stg, b, x, opt, opt->history ? (size_t) opt->max_iterations + 1 : 0, 0, a);
    if (rc || (rc = solve_start(s, d, a, opt->use_x0 != 0))) return rc;
    const int every = opt->check_every > 0 ? opt->check_every : s.check_every;
    SolveState hs;
    bool done = false;
    for (int k = 0;;) {
        HIP_TRY(hipMemcpyAsync(&hs, a.state, sizeof hs, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        done = hs.end_half || hs.end_update || hs.end_direction;
        if (done || k >= opt->max_iterations) break;
        const int stop = opt->max_iterations - k < every ? opt->max_iterations : k + every;
        while (k < stop)
            if ((rc = s.iteration(s, d, a, ++k))) return rc;
    }
    res->status = done ? hs.status : SPMV_HIP_CG_MAX_ITERATIONS;
    res->iterations = hs.iterations;
    res->rr = hs.rr;
    res->bb = hs.bb;
    if (done && hs.status == SPMV_HIP_CG_CONVERGED && hs.bb == 0) HIP_TRY(hipMemsetAsync(a.x, 0, d->vsize * (size_t) d->m, d->stream)); // B = 0: x = 0
    if (opt->history) HIP_TRY(hipMemcpyAsync(opt->history, a.hist, sizeof(double) * ((size_t) hs.iterations + 1), hipMemcpyDeviceToHost, d->stream));
    if ((rc = stg.finish())) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream)); // the call is synchronous whatever the handle's async setting
    return SPMV_HIP_OK;
}

// `warmup` untimed + `iters` timed RUNS of opt->max_iterations iterations each, the stop tests disabled: every run starts again from B (and
// X when use_x0), its iterations are enqueued back to back and bracketed by two events on the handle's stream (the start is outside them:
// not state.hpp's time_events, which brackets a whole call).  ms_out[i] (may be NULL): run i.  Mean ms per run, < 0 on failure.  Device pointers only.
static double solve_time(const Solver &s, spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || !opt || iters <= 0 || warmup < 0 || opt->max_iterations < 1 || d->m != d->n || d->m <= 0) { fail(SPMV_HIP_E_ARG, "time_%s: bad arguments", s.name); return -1.0; }
    if (!is_device_ptr(b) || !is_device_ptr(x) || (opt->Dinv && !is_device_ptr(opt->Dinv))) { fail(SPMV_HIP_E_ARG, "time_%s: B, X and Dinv must be device pointers", s.name); return -1.0; }
    DeviceGuard guard(d->device);
    if (!guard.ok) { fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device); return -1.0; }
    Stager stg{d};
    SolveArgs a;
    if (solve_prepare(s, d, stg, b, x, opt, 0, 1, a)) return -1.0;
    std::vector<hipEvent_t> ev;
    auto done = [&](double mean) {
        for (hipEvent_t e : ev) (void) hipEventDestroy(e);
        return mean;
    };
    for (int i = 0; i < 2 * iters; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) { (void) hipGetLastError(); fail(SPMV_HIP_E_RUNTIME, "hipEventCreate"); return done(-1.0); }
        ev.push_back(e);
    }
    int rc = SPMV_HIP_OK;
    for (int run = -warmup; run < iters && !rc; ++run) {
        rc = solve_start(s, d, a, opt->use_x0 != 0);
        if (run >= 0) (void) hipEventRecord(ev[2 * run], d->stream);
        for (int k = 1; k <= opt->max_iterations && !rc; ++k) rc = s.iteration(s, d, a, k);
        if (run >= 0) (void) hipEventRecord(ev[2 * run + 1], d->stream);
    }
    const hipError_t e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) fail(SPMV_HIP_E_RUNTIME, "time_%s: %s", s.name, hipGetErrorString(e));
    if (rc || e != hipSuccess) return done(-1.0);
    double tot = 0;
    for (int i = 0; i < iters; ++i) {
        float ms = 0;
        (void) hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
        if (ms_out) ms_out[i] = ms;
        tot += ms;
    }
    return done(tot / iters);
}

extern "C" int spmv_shim_solve(int solver, spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    const Solver *s = solver_of(solver);
    return s ? solve_run(*s, d, b, x, opt, res) : fail(SPMV_HIP_E_ARG, "solve: no solver %d", solver);
}

extern "C" double spmv_shim_time_solve(int solver, spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out)
{
    const Solver *s = solver_of(solver);
    if (!s) { fail(SPMV_HIP_E_ARG, "time_solve: no solver %d", solver); return -1.0; }
    return solve_time(*s, d, b, x, opt, warmup, iters, ms_out);
}
