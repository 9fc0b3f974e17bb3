// shim/cg.hpp -- part of spmv_shim.hip: the conjugate-gradient solve on the RESIDENT matrix (spmv_hip_cg) and its timer.  The vector kernels
// are kernels/cg.hpp, launched from their own translation unit (spmv_cg.hip: cg_start_launch, cg_iteration_launch); the multiply q = A p is
// launch<T>() on workspace vectors -- the launch spmv_shim_run makes, without its staging: the handle's own schedule, spmv()'s bits.
//
// The host enqueues `check_every` iterations, copies the state back and synchronises ONCE; inside a batch nothing waits for the host: alpha,
// beta and the stop test are derived on the device by every workgroup (kernels/cg.hpp), and once the state says that the loop has ended every later kernel of
// the batch returns at once -- what is wasted is at most check_every - 1 multiplies into the scratch vector q.  The returned x, iterations
// and history therefore do not depend on check_every.
#pragma once

constexpr int kCgCheckEvery = 8; // iterations between two looks at the state when the caller leaves check_every at 0

static size_t cg_vec_bytes(const spmv_dev *d) { return (d->vsize * (size_t) d->m + 255) & ~(size_t) 255; }

// r, p, q, the partial arrays (zeroed once: the entries behind the P in use stay +0.0) and the state: allocated at the first solve
static int cg_workspace(spmv_dev *d)
{
    if (d->cg_ws) return SPMV_HIP_OK;
    const size_t vec = cg_vec_bytes(d), tail = sizeof(double) * kCgPartArrays * kCgMaxParts + 256;
    ALLOC_TRY(d, &d->cg_ws, 3 * vec + tail, false);
    HIP_TRY(hipMemsetAsync((char *) d->cg_ws + 3 * vec, 0, tail, d->stream));
    return SPMV_HIP_OK;
}

// One solve's device operands: the workspace carved up, host B / X / Dinv staged (X's copy-back registered with the stager; the initial
// guess copied in when it is wanted), the history block, the geometry of the dots.  m > 0.
static int cg_prepare(spmv_dev *d, Stager &stg, const void *b, void *x, const spmv_hip_cg_options *opt, size_t hist_entries, int nostop, CgArgs &a)
{
    int rc = cg_workspace(d);
    if (rc) return rc;
    const size_t vec = cg_vec_bytes(d), m = (size_t) d->m;
    char *ws = (char *) d->cg_ws;
    a.m = d->m;
    const long long chunks = ((long long) d->m + kCgChunk - 1) / kCgChunk;
    a.parts = (int) (chunks < kCgMaxParts ? chunks : kCgMaxParts);
    a.span = (long long) kCgChunk * (((long long) d->m + (long long) kCgChunk * a.parts - 1) / ((long long) kCgChunk * a.parts));
    a.r = ws;
    a.p = ws + vec;
    a.q = ws + 2 * vec;
    a.part = (double *) (ws + 3 * vec);
    a.state = (CgState *) (ws + 3 * vec + sizeof(double) * kCgPartArrays * kCgMaxParts);
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
        if ((rc = stg.reserve(d->cg_hist, sizeof(double) * hist_entries))) return rc;
        a.hist = (double *) d->cg_hist.p;
    }
    return SPMV_HIP_OK;
}

static int cg_multiply(spmv_dev *d, const void *x, void *y)
{
    return d->vsize == sizeof(double) ? launch<double>(d, (const double *) x, (double *) y) : launch<float>(d, (const float *) x, (float *) y);
}

// state zeroed, (q = A x0,) cg_init + cg_begin
static int cg_start(spmv_dev *d, const CgArgs &a, bool use_x0)
{
    int rc;
    HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(CgState), d->stream));
    if (use_x0 && (rc = cg_multiply(d, a.x, a.q))) return rc;
    const hipError_t e = cg_start_launch(a, use_x0, d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "cg: launch: %s", hipGetErrorString(e));
    return SPMV_HIP_OK;
}

// iteration k >= 1: q = A p, then the three vector kernels
static int cg_iteration(spmv_dev *d, const CgArgs &a, int k)
{
    const int rc = cg_multiply(d, a.p, a.q);
    if (rc) return rc;
    const hipError_t e = cg_iteration_launch(a, k, d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "cg: launch: %s", hipGetErrorString(e));
    return SPMV_HIP_OK;
}

extern "C" int spmv_shim_cg(spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "cg: schedule not built");
    if (!opt || !res) return fail(SPMV_HIP_E_ARG, "cg: opt or res is NULL");
    if (d->m != d->n) return fail(SPMV_HIP_E_ARG, "cg: the matrix is %d x %d, not square", d->m, d->n);
    if (d->m > 0 && (!b || !x)) return fail(SPMV_HIP_E_ARG, "cg: B or X is NULL");
    res->status = SPMV_HIP_CG_CONVERGED;
    res->iterations = 0;
    res->rr = res->bb = 0;
    if (d->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    Stager stg{d};
    CgArgs a;
    int rc = cg_prepare(d, stg, b, x, opt, opt->history ? (size_t) opt->max_iterations + 1 : 0, 0, a);
    if (rc || (rc = cg_start(d, a, opt->use_x0 != 0))) return rc;
    const int every = opt->check_every > 0 ? opt->check_every : kCgCheckEvery;
    CgState hs;
    bool done = false;
    for (int k = 0;;) {
        HIP_TRY(hipMemcpyAsync(&hs, a.state, sizeof hs, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        done = hs.end_update || hs.end_direction;
        if (done || k >= opt->max_iterations) break;
        const int stop = opt->max_iterations - k < every ? opt->max_iterations : k + every;
        while (k < stop)
            if ((rc = cg_iteration(d, a, ++k))) return rc;
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
// X when use_x0), its iterations are enqueued back to back and bracketed by two events on the handle's stream (the start is outside them).
// ms_out[i] (may be NULL): run i.  Mean ms per run, < 0 on failure.  Device pointers only.
extern "C" double spmv_shim_time_cg(spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || !opt || iters <= 0 || warmup < 0 || opt->max_iterations < 1 || d->m != d->n || d->m <= 0) { fail(SPMV_HIP_E_ARG, "time_cg: bad arguments"); return -1.0; }
    if (!is_device_ptr(b) || !is_device_ptr(x) || (opt->Dinv && !is_device_ptr(opt->Dinv))) { fail(SPMV_HIP_E_ARG, "time_cg: B, X and Dinv must be device pointers"); return -1.0; }
    DeviceGuard guard(d->device);
    if (!guard.ok) { fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device); return -1.0; }
    Stager stg{d};
    CgArgs a;
    if (cg_prepare(d, stg, b, x, opt, 0, 1, a)) return -1.0;
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
        rc = cg_start(d, a, opt->use_x0 != 0);
        if (run >= 0) (void) hipEventRecord(ev[2 * run], d->stream);
        for (int k = 1; k <= opt->max_iterations && !rc; ++k) rc = cg_iteration(d, a, k);
        if (run >= 0) (void) hipEventRecord(ev[2 * run + 1], d->stream);
    }
    const hipError_t e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) fail(SPMV_HIP_E_RUNTIME, "time_cg: %s", hipGetErrorString(e));
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
