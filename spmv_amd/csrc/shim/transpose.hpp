// shim/transpose.hpp -- part of spmv_shim.hip: A^T of the resident CSR as a matrix of its own (spmv_hip_spmv_transpose).  The kernels are
// kernels/transpose.hpp, launched from their own translation unit (spmv_transpose.hip).  The host C side (spmv_api.c) plans and builds the child
// exactly as create() plans a matrix, then attaches it -- the protocol of the split halves (shim/split.hpp).
#pragma once

// Build A^T (n x m): an unplanned matrix that owns rowptr_T / colidx_T / val_T, and perm (device, nnz ints: perm[p] = our CSR index of its
// entry p).  Needs the resident ColIdx (spmv_shim_restore_columns after spmv_shim_release_columns).
extern "C" int spmv_shim_transpose(spmv_dev *d, spmv_dev **out, int **perm_out)
{
    if (!d || !out || !perm_out) return fail(SPMV_HIP_E_ARG, "transpose: NULL");
    *out = nullptr;
    *perm_out = nullptr;
    if (d->nnz > 0 && !d->colidx) return fail(SPMV_HIP_E_NOSTATE, "transpose: the resident column indices were released (spmv_shim_restore_columns first)");
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    const int m = d->m, n = d->n;
    const long long nnz = d->nnz;
    const int tiles = (int) ((nnz + kTrTile - 1) / kTrTile);
    int bits = 0; // columns are < n: bits of n - 1
    while (bits < 31 && ((long long) n - 1) >> bits > 0) ++bits;
    const int passes = nnz > 0 ? std::max(1, (bits + kTrBits - 1) / kTrBits) : 0;
    spmv_dev *c = new spmv_dev();
    c->device = d->device; c->cus = d->cus; c->m = n; c->n = m; c->vsize = d->vsize; c->stream = d->stream; c->async = d->async;
    c->col_min = 0; c->col_max = m - 1;
    int *perm = nullptr;
    std::vector<void *> tmp; // scratch returned to the pool on every path
    auto scratch = [&](void **p, size_t bytes) { const hipError_t e = pool_malloc(p, bytes ? bytes : 16); if (e == hipSuccess) tmp.push_back(*p); else (void) hipGetLastError(); return e; };
    auto finish = [&](int code) {
        (void) hipStreamSynchronize(d->stream);
        (void) hipGetLastError();
        for (void *p : tmp) (void) pool_free(p);
        if (code) { if (perm) (void) pool_free(perm); spmv_shim_matrix_destroy(c); }
        return code;
    };
    if (pool_malloc((void **) &perm, sizeof(int) * (size_t) (nnz > 0 ? nnz : 1)) != hipSuccess) { (void) hipGetLastError(); perm = nullptr; return finish(fail(SPMV_HIP_E_ALLOC, "transpose: perm")); }
    int rc = dev_alloc(c, (void **) &c->rowptr, sizeof(int) * ((size_t) n + 1), false);
    if (!rc) rc = dev_alloc(c, (void **) &c->colidx, sizeof(int) * ((size_t) nnz + kStreamPad), false); // padded like any resident CSR
    if (!rc) rc = dev_alloc(c, &c->val, d->vsize * ((size_t) nnz + kStreamPad), false);
    if (rc) return finish(rc);
    hipError_t e = hipMemsetAsync(c->colidx + nnz, 0, sizeof(int) * kStreamPad, d->stream);
    if (e == hipSuccess) e = hipMemsetAsync((char *) c->val + d->vsize * (size_t) nnz, 0, d->vsize * kStreamPad, d->stream);
    if (e == hipSuccess && nnz == 0) e = hipMemsetAsync(c->rowptr, 0, sizeof(int) * ((size_t) n + 1), d->stream);
    if (e == hipSuccess && nnz > 0) {
        const long long len = (long long) kTrDigits * tiles; // digit-major (digit, tile) counts
        const int nb = (int) ((len + kScanTile - 1) / kScanTile);
        int *keys[2] = {nullptr, nullptr}, *vtmp = nullptr, *cnt = nullptr, *offs = nullptr, *sums = nullptr, *total = nullptr;
        if (scratch((void **) &keys[0], sizeof(int) * (size_t) nnz) != hipSuccess || scratch((void **) &keys[1], sizeof(int) * (size_t) nnz) != hipSuccess ||
            (passes > 1 && scratch((void **) &vtmp, sizeof(int) * (size_t) nnz) != hipSuccess) || scratch((void **) &cnt, sizeof(int) * (size_t) len) != hipSuccess ||
            scratch((void **) &offs, sizeof(int) * (size_t) len) != hipSuccess || scratch((void **) &sums, sizeof(int) * (size_t) nb) != hipSuccess ||
            scratch((void **) &total, sizeof(int)) != hipSuccess)
            return finish(fail(SPMV_HIP_E_ALLOC, "transpose: sort scratch (%lld entries)", nnz));
        // the values ping-pong so that the last pass writes perm itself
        auto vals_out = [&](int p) { return ((passes - 1 - p) & 1) == 0 ? perm : vtmp; };
        for (int p = 0; p < passes && e == hipSuccess; ++p) {
            const int *kin = p == 0 ? d->colidx : keys[(p - 1) & 1];
            const int *vin = p == 0 ? nullptr : vals_out(p - 1);
            e = tr_hist_launch(nnz, tiles, p * kTrBits, kin, cnt, d->stream);
            if (e == hipSuccess) {
                scan_block_sums_kernel<<<nb, kBlock, 0, d->stream>>>(len, cnt, sums);
                scan_sums_inplace_kernel<<<1, kBlock, 0, d->stream>>>(nb, sums, total);
                scan_apply_kernel<<<nb, kBlock, 0, d->stream>>>(len, cnt, sums, offs, nullptr, nullptr);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = tr_scatter_launch(nnz, tiles, p * kTrBits, kin, vin, offs, keys[p & 1], vals_out(p), d->stream);
        }
        const int *sorted = keys[(passes - 1) & 1];
        int *row_of = keys[passes & 1]; // the other key buffer is free now
        if (e == hipSuccess) e = tr_rowptr_launch(n, nnz, sorted, c->rowptr, d->cus, d->stream);
        if (e == hipSuccess) e = tr_rows_launch(m, d->rowptr, row_of, d->cus, d->stream);
        if (e == hipSuccess) e = tr_columns_launch(nnz, perm, row_of, c->colidx, d->cus, d->stream);
        if (e == hipSuccess) e = tr_gather_launch(nnz, perm, d->val, c->val, d->vsize == sizeof(double), d->cus, d->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) return finish(fail(SPMV_HIP_E_RUNTIME, "transpose: %s", hipGetErrorString(e)));
    if ((rc = matrix_row_stats(c))) return finish(rc);
    if (c->nnz != nnz) return finish(fail(SPMV_HIP_E_RUNTIME, "transpose: %lld entries, expected %lld", c->nnz, nnz));
    finish(SPMV_HIP_OK);
    *out = c;
    *perm_out = perm;
    return SPMV_HIP_OK;
}

// Hand A^T (planned and built) and perm to the parent, which owns and counts them from now on -- or, with NULLs, destroy them.
extern "C" int spmv_shim_attach_transpose(spmv_dev *d, spmv_dev *child, int *perm)
{
    if (!d) return fail(SPMV_HIP_E_ARG, "attach_transpose: NULL");
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    quiesce(d);
    if (d->tr && d->tr != child) spmv_shim_matrix_destroy(d->tr);
    if (d->tr_perm && d->tr_perm != perm) {
        (void) pool_free(d->tr_perm);
        d->device_bytes -= (long long) d->tr_perm_bytes;
        d->tr_perm_bytes = 0;
    }
    if (perm && perm != d->tr_perm) {
        d->tr_perm_bytes = sizeof(int) * (size_t) (d->nnz > 0 ? d->nnz : 1);
        d->device_bytes += (long long) d->tr_perm_bytes;
    }
    d->tr = child;
    d->tr_perm = perm;
    d->tr_gen = d->val_gen;
    return SPMV_HIP_OK;
}

extern "C" spmv_dev *spmv_shim_transpose_of(const spmv_dev *d) { return d ? d->tr : nullptr; }

// HBM held by the attached transpose: its arrays and schedule (split halves included); perm is in the parent's own count
static long long transpose_bytes(const spmv_dev *d)
{
    const spmv_dev *t = d->tr;
    if (!t) return 0;
    return t->device_bytes + (t->sp_near ? t->sp_near->device_bytes : 0) + (t->sp_far ? t->sp_far->device_bytes : 0);
}

// The parent's values changed since A^T was built or last refreshed (spmv_shim_update_values counts them): gather them into val_T and let the
// child's own refresh re-permute them into its schedule.
extern "C" int spmv_shim_transpose_refresh(spmv_dev *d)
{
    if (!d || !d->tr) return fail(SPMV_HIP_E_NOSTATE, "transpose: not built");
    if (d->tr_gen == d->val_gen) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    spmv_dev *t = d->tr;
    HIP_TRY(tr_gather_launch(d->nnz, d->tr_perm, d->val, t->val, d->vsize == sizeof(double), d->cus, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream)); // the child refreshes on its own stream (the same one unless a set_stream is in between)
    const int rc = spmv_shim_update_values(t, t->val);
    if (!rc) d->tr_gen = d->val_gen;
    return rc;
}

// spmv_shim_spmm on the child gathers through the child's global column indices, which the child's own spmv_shim_release_columns may have
// given back at the end of its build.  No create-time array exists for them: they are rebuilt from what the parent keeps, exactly as
// spmv_shim_transpose made them -- colidx_T[p] = row of A holding entry perm[p].  Counted in the child's device_bytes (hence the parent's info).
extern "C" int spmv_shim_transpose_restore_columns(spmv_dev *d)
{
    if (!d || !d->tr) return fail(SPMV_HIP_E_NOSTATE, "transpose: not built");
    spmv_dev *t = d->tr;
    if (t->colidx || t->nnz == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    const long long nnz = d->nnz;
    const size_t ci_bytes = sizeof(int) * ((size_t) nnz + kStreamPad);
    int *ci = nullptr, *row_of = nullptr;
    int rc = dev_alloc(t, (void **) &ci, ci_bytes, false);
    if (rc) return rc;
    auto finish = [&](int code) {
        (void) hipStreamSynchronize(d->stream);
        (void) hipGetLastError();
        if (row_of) (void) pool_free(row_of);
        if (code) { (void) pool_free(ci); t->device_bytes -= (long long) ci_bytes; }
        else t->colidx = ci;
        return code;
    };
    if (pool_malloc((void **) &row_of, sizeof(int) * (size_t) nnz) != hipSuccess) { (void) hipGetLastError(); row_of = nullptr; return finish(fail(SPMV_HIP_E_ALLOC, "transpose: row scratch (%lld entries)", nnz)); }
    hipError_t e = hipMemsetAsync(ci + nnz, 0, sizeof(int) * kStreamPad, d->stream);
    if (e == hipSuccess) e = tr_rows_launch(d->m, d->rowptr, row_of, d->cus, d->stream);
    if (e == hipSuccess) e = tr_columns_launch(nnz, d->tr_perm, row_of, ci, d->cus, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) return finish(fail(SPMV_HIP_E_RUNTIME, "transpose: restore columns: %s", hipGetErrorString(e)));
    return finish(SPMV_HIP_OK);
}

// tools / tests: the built map on the host (rowptr_T: n + 1 ints, perm: nnz ints; either may be NULL)
extern "C" int spmv_shim_transpose_map(spmv_dev *d, int *rowptr_t, int *perm)
{
    if (!d || !d->tr) return fail(SPMV_HIP_E_NOSTATE, "transpose_map: not built");
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    HIP_TRY(hipStreamSynchronize(d->stream));
    if (rowptr_t) HIP_TRY(hipMemcpy(rowptr_t, d->tr->rowptr, sizeof(int) * ((size_t) d->n + 1), hipMemcpyDeviceToHost));
    if (perm && d->nnz > 0) HIP_TRY(hipMemcpy(perm, d->tr_perm, sizeof(int) * (size_t) d->nnz, hipMemcpyDeviceToHost));
    return SPMV_HIP_OK;
}
