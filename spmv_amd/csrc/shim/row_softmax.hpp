// shim/row_softmax.hpp -- part of spmv_shim.hip: the row softmax over the RESIDENT row structure and its backward (spmv_hip_row_softmax,
// spmv_hip_row_softmax_backward).  The kernels are kernels/row_softmax.hpp, launched from their own translation unit (spmv_softmax.hip,
// row_reduce_launch); this side owns the tables -- spmm's batch table and long-row list (spmm_plan: RowPtr alone is read, the resident
// ColIdx is neither needed nor restored) --, the HBM staging of host arrays and the error channel.
#pragma once

// a: S (forward) or P (backward); g: G (backward only); nnz elements each, host or device
static int row_reduce_run(spmv_dev *d, const char *what, bool backward, const void *a, const void *g, void *out)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "%s: schedule not built", what);
    if (d->nnz > 0 && (!a || !out || (backward && !g))) return fail(SPMV_HIP_E_ARG, "%s: a NULL array", what);
    if (d->nnz == 0 || d->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    int rc = spmm_plan(d);
    if (rc) return rc;
    const size_t bytes = d->vsize * (size_t) d->nnz;
    const bool adev = is_device_ptr(a), gdev = !backward || is_device_ptr(g), odev = is_device_ptr(out);
    RowReduceArgs r;
    r.m = d->m;
    r.nb = d->spmm_nb;
    r.nlong = d->spmm_nlong;
    r.cus = d->cus;
    r.split = d->spmm_split;
    r.longs = d->spmm_longs;
    r.rowptr = d->rowptr;
    r.a = a;
    r.g = backward ? g : nullptr;
    r.out = out;
    r.backward = backward;
    if (!adev) {
        if ((rc = spmm_stage_buffer(d, &d->rowred_a, &d->rowred_a_bytes, bytes))) return rc;
        HIP_TRY(hipMemcpyAsync(d->rowred_a, a, bytes, hipMemcpyHostToDevice, d->stream));
        r.a = d->rowred_a;
    }
    if (!gdev) {
        if ((rc = spmm_stage_buffer(d, &d->rowred_g, &d->rowred_g_bytes, bytes))) return rc;
        HIP_TRY(hipMemcpyAsync(d->rowred_g, g, bytes, hipMemcpyHostToDevice, d->stream));
        r.g = d->rowred_g;
    }
    if (!odev) { // empty rows hold no element: every element of the staging buffer is written before it is copied back
        if ((rc = spmm_stage_buffer(d, &d->rowred_o, &d->rowred_o_bytes, bytes))) return rc;
        r.out = d->rowred_o;
    }
    const hipError_t e = row_reduce_launch(r, d->vsize == sizeof(double), d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "%s: launch: %s", what, hipGetErrorString(e));
    if (!odev) HIP_TRY(hipMemcpyAsync(out, d->rowred_o, bytes, hipMemcpyDeviceToHost, d->stream));
    if (!d->async || !adev || !gdev || !odev) HIP_TRY(hipStreamSynchronize(d->stream));
    return SPMV_HIP_OK;
}

extern "C" int spmv_shim_row_softmax(spmv_dev *d, const void *s, void *out) { return row_reduce_run(d, "row_softmax", false, s, nullptr, out); }

extern "C" int spmv_shim_row_softmax_backward(spmv_dev *d, const void *p, const void *g, void *out) { return row_reduce_run(d, "row_softmax_backward", true, p, g, out); }

extern "C" double spmv_shim_time_row_softmax(spmv_dev *d, const void *s, void *out, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || iters <= 0) { fail(SPMV_HIP_E_ARG, "time_row_softmax: bad arguments"); return -1.0; }
    if (!is_device_ptr(s) || !is_device_ptr(out)) { fail(SPMV_HIP_E_ARG, "time_row_softmax: S and Out must be device pointers"); return -1.0; }
    const int keep_async = d->async;
    d->async = 1;
    std::vector<hipEvent_t> ev((size_t) iters + 1);
    for (auto &e : ev) if (hipEventCreate(&e) != hipSuccess) { d->async = keep_async; fail(SPMV_HIP_E_RUNTIME, "hipEventCreate"); return -1.0; }
    int rc = SPMV_HIP_OK;
    for (int i = 0; i < warmup && !rc; ++i) rc = spmv_shim_row_softmax(d, s, out);
    for (int i = 0; i < iters && !rc; ++i) {
        (void) hipEventRecord(ev[i], d->stream);
        rc = spmv_shim_row_softmax(d, s, out);
    }
    (void) hipEventRecord(ev[iters], d->stream);
    hipError_t e = hipStreamSynchronize(d->stream);
    d->async = keep_async;
    double mean = -1.0;
    if (!rc && e == hipSuccess) {
        double tot = 0;
        for (int i = 0; i < iters; ++i) {
            float ms = 0;
            (void) hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            if (ms_out) ms_out[i] = ms;
            tot += ms;
        }
        mean = tot / iters;
    } else if (e != hipSuccess) {
        fail(SPMV_HIP_E_RUNTIME, "time_row_softmax: %s", hipGetErrorString(e));
    }
    for (auto &v : ev) (void) hipEventDestroy(v);
    return mean;
}
