// shim/sddmm.hpp -- part of spmv_shim.hip: Out[p] = sum_c U[row(p), c] V[col(p), c] over the RESIDENT pattern (spmv_hip_sddmm).  The kernel is
// kernels/sddmm.hpp, launched from its own translation unit (spmv_sddmm.hip, sddmm_launch); this side owns the plan (one launch: the entries
// are split evenly, nothing is built per matrix), the HBM staging of host U / V / Out and the error channel.
#pragma once

extern "C" int spmv_shim_sddmm(spmv_dev *d, int k, const void *u, long long ldu, const void *v, long long ldv, void *out)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "sddmm: schedule not built");
    if (k < 1 || ldu < k || ldv < k) return fail(SPMV_HIP_E_ARG, "sddmm: need k >= 1, ldu >= k, ldv >= k (k = %d, ldu = %lld, ldv = %lld)", k, ldu, ldv);
    if (d->nnz > 0 && (!u || !v || !out)) return fail(SPMV_HIP_E_ARG, "sddmm: U, V or Out is NULL");
    if (d->nnz > 0 && !d->colidx) return fail(SPMV_HIP_E_NOSTATE, "sddmm: the resident column indices were released (spmv_shim_restore_columns first)");
    if (d->nnz == 0 || d->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    const size_t s = d->vsize;
    const bool udev = is_device_ptr(u), vdev = is_device_ptr(v), odev = is_device_ptr(out);
    int rc;
    SddmmArgs a;
    a.m = d->m;
    a.k = k;
    a.nnz = d->nnz;
    a.rowptr = d->rowptr;
    a.colidx = d->colidx;
    a.u = u; a.ldu = ldu;
    a.v = v; a.ldv = ldv;
    a.out = out;
    if (!udev) { // host U: its k columns packed into HBM (the padding is not copied)
        if ((rc = spmm_stage_buffer(d, &d->sddmm_u, &d->sddmm_u_bytes, s * (size_t) k * (size_t) d->m))) return rc;
        HIP_TRY(hipMemcpy2DAsync(d->sddmm_u, s * (size_t) k, u, s * (size_t) ldu, s * (size_t) k, (size_t) d->m, hipMemcpyHostToDevice, d->stream));
        a.u = d->sddmm_u; a.ldu = k;
    }
    if (!vdev) {
        if ((rc = spmm_stage_buffer(d, &d->sddmm_v, &d->sddmm_v_bytes, s * (size_t) k * (size_t) d->n))) return rc;
        HIP_TRY(hipMemcpy2DAsync(d->sddmm_v, s * (size_t) k, v, s * (size_t) ldv, s * (size_t) k, (size_t) d->n, hipMemcpyHostToDevice, d->stream));
        a.v = d->sddmm_v; a.ldv = k;
    }
    if (!odev) {
        if ((rc = spmm_stage_buffer(d, &d->sddmm_o, &d->sddmm_o_bytes, s * (size_t) d->nnz))) return rc;
        a.out = d->sddmm_o;
    }
    // the load width changes no bit (kernels/sddmm.hpp): chosen per call from what the addresses allow
    a.vec = ((uintptr_t) a.u & 15) == 0 && ((uintptr_t) a.v & 15) == 0 && ((size_t) a.ldu * s) % 16 == 0 && ((size_t) a.ldv * s) % 16 == 0;
    const hipError_t e = sddmm_launch(a, s == sizeof(double), d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "sddmm: launch: %s", hipGetErrorString(e));
    if (!odev) HIP_TRY(hipMemcpyAsync(out, d->sddmm_o, s * (size_t) d->nnz, hipMemcpyDeviceToHost, d->stream));
    if (!d->async || !udev || !vdev || !odev) HIP_TRY(hipStreamSynchronize(d->stream));
    return SPMV_HIP_OK;
}

extern "C" double spmv_shim_time_sddmm(spmv_dev *d, int k, const void *u, long long ldu, const void *v, long long ldv, void *out, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || iters <= 0) { fail(SPMV_HIP_E_ARG, "time_sddmm: bad arguments"); return -1.0; }
    if (!is_device_ptr(u) || !is_device_ptr(v) || !is_device_ptr(out)) { fail(SPMV_HIP_E_ARG, "time_sddmm: U, V and Out must be device pointers"); return -1.0; }
    const int keep_async = d->async;
    d->async = 1;
    std::vector<hipEvent_t> ev((size_t) iters + 1);
    for (auto &e : ev) if (hipEventCreate(&e) != hipSuccess) { d->async = keep_async; fail(SPMV_HIP_E_RUNTIME, "hipEventCreate"); return -1.0; }
    int rc = SPMV_HIP_OK;
    for (int i = 0; i < warmup && !rc; ++i) rc = spmv_shim_sddmm(d, k, u, ldu, v, ldv, out);
    for (int i = 0; i < iters && !rc; ++i) {
        (void) hipEventRecord(ev[i], d->stream);
        rc = spmv_shim_sddmm(d, k, u, ldu, v, ldv, out);
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
        fail(SPMV_HIP_E_RUNTIME, "time_sddmm: %s", hipGetErrorString(e));
    }
    for (auto &v2 : ev) (void) hipEventDestroy(v2);
    return mean;
}
