// shim/bicgstab.hpp -- part of spmv_shim.hip, behind shim/cg.hpp: the BiCGStab solve on the RESIDENT matrix (spmv_hip_bicgstab) and its timer.
// The vector kernels are kernels/bicgstab.hpp, launched from their own translation unit (spmv_bicgstab.hip); the two multiplies of an
// iteration, v = A ph and t = A sh, are launch<T>() on workspace vectors (cg_multiply): the handle's own schedule, spmv()'s bits.
//
// The host loop is spmv_hip_cg's: enqueue `check_every` iterations, copy the state back and synchronise ONCE.  alpha, omega, beta and the
// stop tests are derived on the device by every workgroup, and once the state says that the loop has ended every later kernel of the batch
// returns at once -- what is wasted is at most 2 check_every - 1 multiplies into the scratch vectors v and t.  The returned x, iterations and
// history therefore do not depend on check_every.
#pragma once

// iterations between two looks at the state when the caller leaves check_every at 0.  From the sweep of tools/bicgstab_bench.py: a
// look costs 23-31 us; at 8 an iteration is within 3 % of the best figure of the sweep (32) on the 1e6-row case and within 0.3 % on the 1e7-row
// band, and what a larger value saves per iteration it loses again behind convergence, where on average check_every - 1 multiplies are wasted
constexpr int kBicgCheckEvery = 8;

constexpr int kBicgVectors = 6; // r, rhat, p, v, t, y

// the six vectors, the partial arrays (zeroed once: the entries behind the P in use stay +0.0) and the state: allocated at the first solve
static int bicg_workspace(spmv_dev *d)
{
    if (d->bicg_ws) return SPMV_HIP_OK;
    const size_t vec = cg_vec_bytes(d), tail = sizeof(double) * kBicgPartArrays * kCgMaxParts + 256;
    ALLOC_TRY(d, &d->bicg_ws, kBicgVectors * vec + tail, false);
    HIP_TRY(hipMemsetAsync((char *) d->bicg_ws + kBicgVectors * vec, 0, tail, d->stream));
    return SPMV_HIP_OK;
}

// One solve's device operands, as cg_prepare: the workspace carved up, host B / X / Dinv staged through spmv_hip_cg's stage buffers (both calls
// are synchronous, so they never hold them at the same time), the history block, the geometry of the dots.  m > 0.
static int bicg_prepare(spmv_dev *d, Stager &stg, const void *b, void *x, const spmv_hip_cg_options *opt, size_t hist_entries, int nostop, BicgArgs &a)
{
    static_assert(sizeof(BicgState) <= 256, "the state has 256 bytes behind the partial arrays");
    int rc = bicg_workspace(d);
    if (rc) return rc;
    const size_t vec = cg_vec_bytes(d), m = (size_t) d->m;
    char *ws = (char *) d->bicg_ws;
    a.m = d->m;
    const long long chunks = ((long long) d->m + kCgChunk - 1) / kCgChunk;
    a.parts = (int) (chunks < kCgMaxParts ? chunks : kCgMaxParts);
    a.span = (long long) kCgChunk * (((long long) d->m + (long long) kCgChunk * a.parts - 1) / ((long long) kCgChunk * a.parts));
    a.r = ws;
    a.rhat = ws + vec;
    a.p = ws + 2 * vec;
    a.v = ws + 3 * vec;
    a.t = ws + 4 * vec;
    a.y = ws + 5 * vec;
    a.part = (double *) (ws + kBicgVectors * vec);
    a.state = (BicgState *) (ws + kBicgVectors * vec + sizeof(double) * kBicgPartArrays * kCgMaxParts);
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
        if ((rc = stg.reserve(d->bicg_hist, sizeof(double) * hist_entries))) return rc;
        a.hist = (double *) d->bicg_hist.p;
    }
    return SPMV_HIP_OK;
}

// state zeroed, (v = A x0,) bicg_init + bicg_begin
static int bicg_start(spmv_dev *d, const BicgArgs &a, bool use_x0)
{
    int rc;
    HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(BicgState), d->stream));
    if (use_x0 && (rc = cg_multiply(d, a.x, a.v))) return rc;
    const hipError_t e = bicg_start_launch(a, use_x0, d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "bicgstab: launch: %s", hipGetErrorString(e));
    return SPMV_HIP_OK;
}

// iteration k >= 1: v = A ph, bicg_rv + bicg_half, t = A sh, bicg_ts + bicg_update + bicg_direction; without Dinv ph is p and sh is s, which is in r
static int bicg_iteration(spmv_dev *d, const BicgArgs &a, int k)
{
    int rc = cg_multiply(d, a.dinv ? a.y : a.p, a.v);
    if (rc) return rc;
    hipError_t e = bicg_first_launch(a, k, d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "bicgstab: launch: %s", hipGetErrorString(e));
    if ((rc = cg_multiply(d, a.dinv ? a.y : a.r, a.t))) return rc;
    e = bicg_second_launch(a, k, d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "bicgstab: launch: %s", hipGetErrorString(e));
    return SPMV_HIP_OK;
}

extern "C" int spmv_shim_bicgstab(spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "bicgstab: schedule not built");
    if (!opt || !res) return fail(SPMV_HIP_E_ARG, "bicgstab: opt or res is NULL");
    if (d->m != d->n) return fail(SPMV_HIP_E_ARG, "bicgstab: the matrix is %d x %d, not square", d->m, d->n);
    if (d->m > 0 && (!b || !x)) return fail(SPMV_HIP_E_ARG, "bicgstab: B or X is NULL");
    res->status = SPMV_HIP_CG_CONVERGED;
    res->iterations = 0;
    res->rr = res->bb = 0;
    if (d->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    Stager stg{d};
    BicgArgs a;
    int rc = bicg_prepare(d, stg, b, x, opt, opt->history ? (size_t) opt->max_iterations + 1 : 0, 0, a);
    if (rc || (rc = bicg_start(d, a, opt->use_x0 != 0))) return rc;
    const int every = opt->check_every > 0 ? opt->check_every : kBicgCheckEvery;
    BicgState hs;
    bool done = false;
    for (int k = 0;;) {
        HIP_TRY(hipMemcpyAsync(&hs, a.state, sizeof hs, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        done = hs.end_half || hs.end_update || hs.end_direction;
        if (done || k >= opt->max_iterations) break;
        const int stop = opt->max_iterations - k < every ? opt->max_iterations : k + every;
        while (k < stop)
            if ((rc = bicg_iteration(d, a, ++k))) return rc;
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

// As spmv_shim_time_cg: `warmup` untimed + `iters` timed RUNS of opt->max_iterations iterations each, the stop tests disabled; every run starts
// again from B (and X when use_x0), its iterations are enqueued back to back and bracketed by two events on the handle's stream (the start is
// outside them).  ms_out[i] (may be NULL): run i.  Mean ms per run, < 0 on failure.  Device pointers only.
extern "C" double spmv_shim_time_bicgstab(spmv_dev *d, const void *b, void *x, const spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || !opt || iters <= 0 || warmup < 0 || opt->max_iterations < 1 || d->m != d->n || d->m <= 0) { fail(SPMV_HIP_E_ARG, "time_bicgstab: bad arguments"); return -1.0; }
    if (!is_device_ptr(b) || !is_device_ptr(x) || (opt->Dinv && !is_device_ptr(opt->Dinv))) { fail(SPMV_HIP_E_ARG, "time_bicgstab: B, X and Dinv must be device pointers"); return -1.0; }
    DeviceGuard guard(d->device);
    if (!guard.ok) { fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device); return -1.0; }
    Stager stg{d};
    BicgArgs a;
    if (bicg_prepare(d, stg, b, x, opt, 0, 1, a)) return -1.0;
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
        rc = bicg_start(d, a, opt->use_x0 != 0);
        if (run >= 0) (void) hipEventRecord(ev[2 * run], d->stream);
        for (int k = 1; k <= opt->max_iterations && !rc; ++k) rc = bicg_iteration(d, a, k);
        if (run >= 0) (void) hipEventRecord(ev[2 * run + 1], d->stream);
    }
    const hipError_t e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) fail(SPMV_HIP_E_RUNTIME, "time_bicgstab: %s", hipGetErrorString(e));
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
