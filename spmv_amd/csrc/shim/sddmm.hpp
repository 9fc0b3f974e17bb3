// shim/sddmm.hpp -- part of spmv_shim.hip: Out[p] = sum_c U[row(p), c] V[col(p), c] over the RESIDENT pattern (spmv_hip_sddmm).  The kernel is
// kernels/sddmm.hpp, launched from its own translation unit (spmv_sddmm.hip, sddmm_launch); this side owns the plan (one launch: the entries
// are split evenly, nothing is built per matrix).
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
    Stager stg{d};
    long long ldo = 1;
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
    if ((rc = stg.in(d->stage[STAGE_SDDMM_U], a.u, a.ldu, (size_t) d->m, k)) || (rc = stg.in(d->stage[STAGE_SDDMM_V], a.v, a.ldv, (size_t) d->n, k)) ||
        (rc = stg.out(d->stage[STAGE_SDDMM_O], a.out, ldo, (size_t) d->nnz, 1))) return rc;
    // the load width changes no bit (kernels/sddmm.hpp): chosen per call from what the addresses allow
    a.vec = wide_ok(a.u, a.ldu, s) && wide_ok(a.v, a.ldv, s);
    const hipError_t e = sddmm_launch(a, s == sizeof(double), d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "sddmm: launch: %s", hipGetErrorString(e));
    return stg.finish();
}

extern "C" double spmv_shim_time_sddmm(spmv_dev *d, int k, const void *u, long long ldu, const void *v, long long ldv, void *out, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || iters <= 0) { fail(SPMV_HIP_E_ARG, "time_sddmm: bad arguments"); return -1.0; }
    if (!is_device_ptr(u) || !is_device_ptr(v) || !is_device_ptr(out)) { fail(SPMV_HIP_E_ARG, "time_sddmm: U, V and Out must be device pointers"); return -1.0; }
    return time_events(d, "time_sddmm", warmup, iters, ms_out, [&] { return spmv_shim_sddmm(d, k, u, ldu, v, ldv, out); });
}
