// shim/spmm.hpp -- part of spmv_shim.hip: Y = A X for k right-hand sides over the RESIDENT CSR (spmv_hip_spmm).  The executors are
// kernels/spmm.hpp, launched from their own translation unit (spmv_spmm.hip, spmm_launch); this side owns the batch table and the long-row list.
#pragma once

// equal-nnz row batches (one wave each) and the rows longer than kSpmmLongThr (a workgroup each): built once per resident matrix
static int spmm_plan(spmv_dev *d)
{
    if (d->spmm_planned) return SPMV_HIP_OK;
    const int m = d->m;
    int nb = (int) ((d->nnz + kSpmmBatchNnz - 1) / kSpmmBatchNnz);
    if (m > 0 && nb < 1) nb = 1;
    int *split = nullptr, *longs = nullptr, *cnt = nullptr;
    const size_t split_bytes = sizeof(int) * ((size_t) nb + 1);
    size_t longs_bytes = 0;
    int nlong = 0, rc = SPMV_HIP_OK;
    auto bail = [&](int code) {
        quiesce(d);
        if (split) { (void) pool_free(split); d->device_bytes -= (long long) split_bytes; }
        if (longs) { (void) pool_free(longs); d->device_bytes -= (long long) longs_bytes; }
        if (cnt) (void) pool_free(cnt);
        return code;
    };
    if ((rc = dev_alloc(d, (void **) &split, split_bytes, false))) return rc;
    if (nb > 0) rowblock_split_kernel<<<grid_for((long long) nb + 1, kBlock, INT_MAX), kBlock, 0, d->stream>>>(m, (int) d->nnz, nb, kSpmmBatchNnz, d->rowptr, split);
    if (hipGetLastError() != hipSuccess) return bail(fail(SPMV_HIP_E_RUNTIME, "spmm: batch split launch failed"));
    if (d->stats.max_row_len > kSpmmLongThr) {
        if (pool_malloc((void **) &cnt, sizeof(int)) != hipSuccess) { (void) hipGetLastError(); return bail(fail(SPMV_HIP_E_ALLOC, "spmm: pool_malloc(count)")); }
        hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int), d->stream);
        if (e == hipSuccess) {
            count_longer_kernel<<<grid_for(m, kBlock, d->cus * 8), kBlock, 0, d->stream>>>(m, kSpmmLongThr, d->rowptr, cnt);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&nlong, cnt, sizeof(int), hipMemcpyDeviceToHost, d->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) { (void) hipGetLastError(); return bail(fail(SPMV_HIP_E_RUNTIME, "spmm: long-row count: %s", hipGetErrorString(e))); }
        longs_bytes = sizeof(int) * (size_t) (nlong > 0 ? nlong : 4);
        if ((rc = dev_alloc(d, (void **) &longs, longs_bytes, false))) return bail(rc);
        e = hipMemsetAsync(cnt, 0, sizeof(int), d->stream);
        if (e == hipSuccess) {
            spmm_long_list_kernel<<<grid_for(m, kBlock, d->cus * 8), kBlock, 0, d->stream>>>(m, kSpmmLongThr, d->rowptr, longs, cnt);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) { (void) hipGetLastError(); return bail(fail(SPMV_HIP_E_RUNTIME, "spmm: long-row list: %s", hipGetErrorString(e))); }
        (void) pool_free(cnt);
    }
    d->spmm_split = split;
    d->spmm_longs = longs;
    d->spmm_nb = nb;
    d->spmm_nlong = nlong;
    d->spmm_planned = true;
    return SPMV_HIP_OK;
}

// Y = A X on DEVICE operands, one pass over A per panel of KP columns; the batch table and the long-row list are built (spmm_plan).  What
// spmv_shim_spmm launches behind its staging, and what spmv_hip_cg_columns multiplies its workspace vectors with (shim/solve.hpp)
static int spmm_panels(spmv_dev *d, int k, const char *xd, long long lx, char *yd, long long ly)
{
    const size_t s = d->vsize;
    const bool f64 = s == sizeof(double);
    const int KP = f64 ? SpmmShape<double>::KP : SpmmShape<float>::KP;
    for (int c = 0; c < k; c += KP) { // one pass over A per panel
        SpmmArgs a;
        a.m = d->m;
        a.nb = d->spmm_nb;
        a.nlong = d->spmm_nlong;
        a.kc = k - c < KP ? k - c : KP;
        a.cus = d->cus;
        a.split = d->spmm_split;
        a.longs = d->spmm_longs;
        a.rowptr = d->rowptr;
        a.colidx = d->colidx;
        a.val = d->val;
        a.x = xd + s * (size_t) c;
        a.y = yd + s * (size_t) c;
        a.ldx = lx;
        a.ldy = ly;
        a.vec = wide_ok(a.x, lx, s) && wide_ok(a.y, ly, s);
        const hipError_t e = spmm_launch(a, f64, d->stream);
        if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "spmm: launch: %s", hipGetErrorString(e));
    }
    return SPMV_HIP_OK;
}

extern "C" int spmv_shim_spmm(spmv_dev *d, int k, const void *x, long long ldx, void *y, long long ldy)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "spmm: schedule not built");
    if (k < 1 || ldx < k || ldy < k) return fail(SPMV_HIP_E_ARG, "spmm: need k >= 1, ldx >= k, ldy >= k (k = %d, ldx = %lld, ldy = %lld)", k, ldx, ldy);
    if (d->m > 0 && (!x || !y)) return fail(SPMV_HIP_E_ARG, "spmm: X or Y is NULL");
    if (d->nnz > 0 && !d->colidx) return fail(SPMV_HIP_E_NOSTATE, "spmm: the resident column indices were released (spmv_shim_restore_columns first)");
    if (d->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    int rc = spmm_plan(d);
    if (rc) return rc;
    Stager stg{d};
    const char *xd = (const char *) x;
    char *yd = (char *) y;
    long long lx = ldx, ly = ldy;
    if ((rc = stg.in(d->stage[STAGE_SPMM_X], xd, lx, (size_t) d->n, k)) || (rc = stg.out(d->stage[STAGE_SPMM_Y], yd, ly, (size_t) d->m, k))) return rc;
    if ((rc = spmm_panels(d, k, xd, lx, yd, ly))) return rc;
    return stg.finish();
}

// The create-time ColIdx again in HBM after spmv_shim_release_columns gave the resident copy back: copied as is, or -- perm_host given (option
// "reorder": the resident matrix is P A P^T) -- permuted like the values were at create (rcm_permute_kernel over the caller's RowPtr / ColIdx).
extern "C" int spmv_shim_restore_columns(spmv_dev *d, const int *rowptr, const int *colidx, const int *perm_host)
{
    if (!d) return fail(SPMV_HIP_E_ARG, "restore_columns: NULL");
    if (d->colidx || d->nnz == 0) return SPMV_HIP_OK;
    if (!colidx || (perm_host && !rowptr)) return fail(SPMV_HIP_E_ARG, "restore_columns: the resident column indices were released and ColIdx / RowPtr is NULL");
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    const int m = d->m;
    const long long nnz = d->nnz;
    const size_t ci_bytes = sizeof(int) * ((size_t) nnz + kStreamPad);
    int *ci = nullptr;
    int rc = dev_alloc(d, (void **) &ci, ci_bytes, false);
    if (rc) return rc;
    std::vector<void *> tmp; // scratch returned to the pool on every path
    auto scratch = [&](void **p, size_t bytes) { const hipError_t e = pool_malloc(p, bytes ? bytes : 16); if (e == hipSuccess) tmp.push_back(*p); return e; };
    auto finish = [&](int code) {
        (void) hipStreamSynchronize(d->stream);
        (void) hipGetLastError();
        for (void *p : tmp) (void) pool_free(p);
        if (code) { (void) pool_free(ci); d->device_bytes -= (long long) ci_bytes; }
        else d->colidx = ci;
        return code;
    };
    hipError_t e = hipMemsetAsync(ci + nnz, 0, sizeof(int) * kStreamPad, d->stream);
    if (e == hipSuccess && !perm_host) {
        e = hipMemcpyAsync(ci, colidx, sizeof(int) * (size_t) nnz, hipMemcpyDefault, d->stream);
    } else if (e == hipSuccess) {
        std::vector<int> inv((size_t) m);
        for (int i = 0; i < m; ++i) {
            if (perm_host[i] < 0 || perm_host[i] >= m) return finish(fail(SPMV_HIP_E_ARG, "restore_columns: permutation entry %d out of range", perm_host[i]));
            inv[(size_t) perm_host[i]] = i;
        }
        int *dperm = nullptr, *dinv = nullptr, *drp = (int *) rowptr, *dci = (int *) colidx;
        if (scratch((void **) &dperm, sizeof(int) * (size_t) m) != hipSuccess || scratch((void **) &dinv, sizeof(int) * (size_t) m) != hipSuccess ||
            (!is_device_ptr(rowptr) && scratch((void **) &drp, sizeof(int) * ((size_t) m + 1)) != hipSuccess) ||
            (!is_device_ptr(colidx) && scratch((void **) &dci, sizeof(int) * (size_t) nnz) != hipSuccess))
            return finish(fail(SPMV_HIP_E_ALLOC, "restore_columns: scratch"));
        e = hipMemcpyAsync(dperm, perm_host, sizeof(int) * (size_t) m, hipMemcpyHostToDevice, d->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dinv, inv.data(), sizeof(int) * (size_t) m, hipMemcpyHostToDevice, d->stream);
        if (e == hipSuccess && drp != rowptr) e = hipMemcpyAsync(drp, rowptr, sizeof(int) * ((size_t) m + 1), hipMemcpyHostToDevice, d->stream);
        if (e == hipSuccess && dci != colidx) e = hipMemcpyAsync(dci, colidx, sizeof(int) * (size_t) nnz, hipMemcpyHostToDevice, d->stream);
        // the same kernel that built the resident P A P^T at create, here for the columns only (val / va2 NULL)
        if (e == hipSuccess) {
            rcm_permute_kernel<float><<<grid_for(m, kBlock / kWave, d->cus * 32), kBlock, 0, d->stream>>>(m, dperm, dinv, drp, dci, nullptr, d->rowptr, ci, nullptr);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) return finish(fail(SPMV_HIP_E_RUNTIME, "restore_columns: %s", hipGetErrorString(e)));
    // every index must address X before a kernel gathers with it (the array may have been changed since create)
    int host2[2] = {INT_MAX, INT_MIN};
    int *mnmx = nullptr;
    if (scratch((void **) &mnmx, sizeof host2) != hipSuccess) return finish(fail(SPMV_HIP_E_ALLOC, "restore_columns: scratch"));
    e = hipMemcpy(mnmx, host2, sizeof host2, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        colidx_range_kernel<<<grid_for(nnz, kBlock * 16, d->cus * 8), kBlock, 0, d->stream>>>(nnz, ci, mnmx);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host2, mnmx, sizeof host2, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) return finish(fail(SPMV_HIP_E_RUNTIME, "restore_columns: range check: %s", hipGetErrorString(e)));
    if (host2[0] < 0 || host2[1] >= d->n) return finish(fail(SPMV_HIP_E_ARG, "restore_columns: ColIdx out of range: min %d, max %d, n = %d", host2[0], host2[1], d->n));
    return finish(SPMV_HIP_OK);
}

extern "C" double spmv_shim_time_spmm(spmv_dev *d, int k, const void *x, long long ldx, void *y, long long ldy, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || iters <= 0) { fail(SPMV_HIP_E_ARG, "time_spmm: bad arguments"); return -1.0; }
    if (!is_device_ptr(x) || !is_device_ptr(y)) { fail(SPMV_HIP_E_ARG, "time_spmm: X and Y must be device pointers"); return -1.0; }
    return time_events(d, "time_spmm", warmup, iters, ms_out, [&] { return spmv_shim_spmm(d, k, x, ldx, y, ldy); });
}
