// shim/row_softmax.hpp -- part of spmv_shim.hip: the row softmax over the RESIDENT row structure and its backward (spmv_hip_row_softmax,
// spmv_hip_row_softmax_backward).  The kernels are kernels/row_softmax.hpp, launched from their own translation unit (spmv_softmax.hip,
// row_reduce_launch); the tables are spmm's batch table and long-row list (spmm_plan: RowPtr alone is read, the resident ColIdx is neither
// needed nor restored).
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
    const size_t nnz = (size_t) d->nnz;
    Stager stg{d};
    long long ld = 1;
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
    // empty rows hold no element: every element of a staged result is written before it is copied back
    if ((rc = stg.in(d->stage[STAGE_ROWRED_A], r.a, ld, nnz, 1)) || (backward && (rc = stg.in(d->stage[STAGE_ROWRED_G], r.g, ld, nnz, 1))) ||
        (rc = stg.out(d->stage[STAGE_ROWRED_O], r.out, ld, nnz, 1))) return rc;
    const hipError_t e = row_reduce_launch(r, d->vsize == sizeof(double), d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "%s: launch: %s", what, hipGetErrorString(e));
    return stg.finish();
}

extern "C" int spmv_shim_row_softmax(spmv_dev *d, const void *s, void *out) { return row_reduce_run(d, "row_softmax", false, s, nullptr, out); }

extern "C" int spmv_shim_row_softmax_backward(spmv_dev *d, const void *p, const void *g, void *out) { return row_reduce_run(d, "row_softmax_backward", true, p, g, out); }

extern "C" double spmv_shim_time_row_softmax(spmv_dev *d, const void *s, void *out, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || iters <= 0) { fail(SPMV_HIP_E_ARG, "time_row_softmax: bad arguments"); return -1.0; }
    if (!is_device_ptr(s) || !is_device_ptr(out)) { fail(SPMV_HIP_E_ARG, "time_row_softmax: S and Out must be device pointers"); return -1.0; }
    return time_events(d, "time_row_softmax", warmup, iters, ms_out, [&] { return spmv_shim_row_softmax(d, s, out); });
}
