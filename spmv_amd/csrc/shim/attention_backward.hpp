// shim/attention_backward.hpp -- part of spmv_shim.hip: dQ, dK, dV of O = softmax_rows(scale * Q K^T on the RESIDENT pattern) V in two passes
// (spmv_hip_attention_backward).  The kernels are kernels/attention_backward.hpp, launched from their own translation unit
// (spmv_attention_backward.hip, attention_backward_launch); the tables are spmm's batch table and long-row list of the resident matrix
// and, when dK or dV is wanted, those of the attached transpose.  This side adds the two nnz-sized arrays the passes share.
#pragma once

// attb_p / attb_ds: P and dS in CSR order, allocated once per resident matrix
static int attention_backward_plan(spmv_dev *d)
{
    if (d->attb_p && d->attb_ds) return SPMV_HIP_OK;
    const size_t bytes = d->vsize * (size_t) d->nnz;
    int rc;
    if (!d->attb_p && (rc = dev_alloc(d, &d->attb_p, bytes, false))) return rc;
    if (!d->attb_ds && (rc = dev_alloc(d, &d->attb_ds, bytes, false))) return rc;
    return SPMV_HIP_OK;
}

// dq / dk / dv: NULL = not wanted.  When dk or dv is wanted the transpose must be attached with its column indices resident
// (spmv_shim_transpose, spmv_shim_transpose_restore_columns); its values are not read.
extern "C" int spmv_shim_attention_backward(spmv_dev *d, int k, int dv, double scale, const void *q, long long ldq, const void *kk, long long ldk, const void *v,
                                            long long ldv, const void *g, long long ldg, void *dq, long long lddq, void *dk, long long lddk, void *dvo, long long lddv)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "attention_backward: schedule not built");
    if (k < 1 || dv < 1 || ldq < k || ldk < k || ldv < dv || ldg < dv || (dq && lddq < k) || (dk && lddk < k) || (dvo && lddv < dv))
        return fail(SPMV_HIP_E_ARG, "attention_backward: need k >= 1, dv >= 1, ldq, ldk >= k, ldv, ldg >= dv, lddq, lddk >= k, lddv >= dv (k = %d, dv = %d)", k, dv);
    if (d->m > 0 && (!q || !kk || !v || !g)) return fail(SPMV_HIP_E_ARG, "attention_backward: Q, K, V or G is NULL");
    if (!dq && !dk && !dvo) return SPMV_HIP_OK;
    if (d->nnz > 0 && !d->colidx) return fail(SPMV_HIP_E_NOSTATE, "attention_backward: the resident column indices were released (spmv_shim_restore_columns first)");
    const bool cols = (dk || dvo) && d->n > 0;
    spmv_dev *t = d->tr;
    if (cols && (!t || !d->tr_perm || (t->nnz > 0 && !t->colidx))) return fail(SPMV_HIP_E_NOSTATE, "attention_backward: the transpose is not attached with its column indices");
    if (d->m == 0 && !cols) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    int rc;
    if ((rc = spmm_plan(d)) || (rc = attention_backward_plan(d)) || (cols && (rc = spmm_plan(t)))) return rc;
    const size_t s = d->vsize;
    Stager stg{d};
    AttentionBwdArgs a;
    a.m = d->m;
    a.k = k;
    a.dv = dv;
    a.cus = d->cus;
    a.nb = d->spmm_nb;
    a.nlong = d->spmm_nlong;
    a.split = d->spmm_split;
    a.longs = d->spmm_longs;
    a.rowptr = d->rowptr;
    a.colidx = d->colidx;
    if (cols) {
        a.t_rows = t->m;
        a.t_nb = t->spmm_nb;
        a.t_nlong = t->spmm_nlong;
        a.t_split = t->spmm_split;
        a.t_longs = t->spmm_longs;
        a.t_rowptr = t->rowptr;
        a.t_colidx = t->colidx;
        a.perm = d->tr_perm;
    }
    a.p = d->attb_p;
    a.ds = d->attb_ds;
    a.scale = scale;
    a.q = q; a.ldq = ldq;
    a.kk = kk; a.ldk = ldk;
    a.v = v; a.ldv = ldv;
    a.g = g; a.ldg = ldg;
    a.dq = d->m > 0 ? dq : nullptr; a.lddq = lddq;
    a.dk = cols ? dk : nullptr; a.lddk = lddk;
    a.dvo = cols ? dvo : nullptr; a.lddv = lddv;
    // every row of a wanted output gets its elements, empty rows and columns their zeros: a staged result is written completely before it is copied back
    if ((rc = stg.in(d->stage[STAGE_ATTB_Q], a.q, a.ldq, (size_t) d->m, k)) || (rc = stg.in(d->stage[STAGE_ATTB_K], a.kk, a.ldk, (size_t) d->n, k)) ||
        (rc = stg.in(d->stage[STAGE_ATTB_V], a.v, a.ldv, (size_t) d->n, dv)) || (rc = stg.in(d->stage[STAGE_ATTB_G], a.g, a.ldg, (size_t) d->m, dv)) ||
        (a.dq && (rc = stg.out(d->stage[STAGE_ATTB_DQ], a.dq, a.lddq, (size_t) d->m, k))) || (a.dk && (rc = stg.out(d->stage[STAGE_ATTB_DK], a.dk, a.lddk, (size_t) d->n, k))) ||
        (a.dvo && (rc = stg.out(d->stage[STAGE_ATTB_DV], a.dvo, a.lddv, (size_t) d->n, dv)))) return rc;
    // the access width changes no bit (kernels/attention_backward.hpp): chosen per call from what the addresses allow
    a.vec = wide_ok(a.q, a.ldq, s) && wide_ok(a.kk, a.ldk, s) && wide_ok(a.v, a.ldv, s) && wide_ok(a.g, a.ldg, s) && (!a.dq || wide_ok(a.dq, a.lddq, s)) &&
            (!a.dk || wide_ok(a.dk, a.lddk, s)) && (!a.dvo || wide_ok(a.dvo, a.lddv, s));
    const hipError_t e = attention_backward_launch(a, s == sizeof(double), d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "attention_backward: launch: %s", hipGetErrorString(e));
    return stg.finish();
}

extern "C" double spmv_shim_time_attention_backward(spmv_dev *d, int k, int dv, double scale, const void *q, long long ldq, const void *kk, long long ldk, const void *v,
                                                    long long ldv, const void *g, long long ldg, void *dq, long long lddq, void *dk, long long lddk, void *dvo, long long lddv,
                                                    int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || iters <= 0) { fail(SPMV_HIP_E_ARG, "time_attention_backward: bad arguments"); return -1.0; }
    if (!is_device_ptr(q) || !is_device_ptr(kk) || !is_device_ptr(v) || !is_device_ptr(g) || (dq && !is_device_ptr(dq)) || (dk && !is_device_ptr(dk)) || (dvo && !is_device_ptr(dvo))) {
        fail(SPMV_HIP_E_ARG, "time_attention_backward: Q, K, V, G and the outputs must be device pointers");
        return -1.0;
    }
    return time_events(d, "time_attention_backward", warmup, iters, ms_out,
                       [&] { return spmv_shim_attention_backward(d, k, dv, scale, q, ldq, kk, ldk, v, ldv, g, ldg, dq, lddq, dk, lddk, dvo, lddv); });
}
