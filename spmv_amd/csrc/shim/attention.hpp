// shim/attention.hpp -- part of spmv_shim.hip: O = softmax_rows(scale * Q K^T on the RESIDENT pattern) V in one pass.  One entry point,
// spmv_shim_attention, and its timer serve every public variant -- one head, `heads` heads side by side in the rows, an additive bias per head and
// entry, fewer K / V heads than query heads, the rows' log-sum-exps, 16-bit operands: spmv_api.c passes them all as one spmv_attention_call
// (spmv_shim.h), a variant without a feature with that feature's neutral value.  The merge of two partial results is here too.  The
// kernels are kernels/attention.hpp, launched from their own translation unit (spmv_attention.hip, attention_launch: compiled in one part per
// element type of Q, K and V); the tables are spmm's batch table and long-row list (spmm_plan).  This side adds what the long rows need: where
// each one parks its scores.
#pragma once

// long_off[i] = first element of long row i of spmm's list in att_park (sum of the long rows' lengths elements): built once per resident matrix
static int attention_plan(spmv_dev *d)
{
    if (d->att_planned) return SPMV_HIP_OK;
    const int nlong = d->spmm_nlong;
    if (nlong > 0) {
        const size_t off_bytes = sizeof(int) * ((size_t) nlong + 1);
        int *off = nullptr;
        void *park = nullptr;
        int rc = dev_alloc(d, (void **) &off, off_bytes, false);
        if (rc) return rc;
        auto bail = [&](int code) {
            quiesce(d);
            (void) pool_free(off);
            d->device_bytes -= (long long) off_bytes;
            return code;
        };
        std::vector<int> host((size_t) nlong + 1, 0);
        attention_long_len_kernel<<<grid_for(nlong, kBlock, d->cus * 8), kBlock, 0, d->stream>>>(nlong, d->spmm_longs, d->rowptr, off);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(host.data(), off, sizeof(int) * (size_t) nlong, hipMemcpyDeviceToHost, d->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) { (void) hipGetLastError(); return bail(fail(SPMV_HIP_E_RUNTIME, "attention: long-row lengths: %s", hipGetErrorString(e))); }
        long long total = 0; // at most nnz < INT_MAX
        for (int i = 0; i <= nlong; ++i) {
            const int len = host[(size_t) i];
            host[(size_t) i] = (int) total;
            total += len;
        }
        e = hipMemcpyAsync(off, host.data(), off_bytes, hipMemcpyHostToDevice, d->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) { (void) hipGetLastError(); return bail(fail(SPMV_HIP_E_RUNTIME, "attention: long-row offsets: %s", hipGetErrorString(e))); }
        if ((rc = dev_alloc(d, &park, d->vsize * (size_t) total, false))) return bail(rc);
        d->att_off = off;
        d->att_park = park;
    }
    d->att_planned = true;
    return SPMV_HIP_OK;
}

// A host bias: `planes` planes of nnz elements, ld apart, packed into the handle's buffer `b` (Stager::in with a plane as a row); a shared plane
// (ld = 0) is one row and stays shared.  nnz > 0.
static int attention_stage_bias(Stager &stg, StageBuf &b, const void *&bias, long long &ldb, int heads)
{
    const bool shared = ldb == 0;
    long long ld = shared ? stg.d->nnz : ldb;
    const int rc = stg.in(b, bias, ld, shared ? (size_t) 1 : (size_t) heads, (int) stg.d->nnz);
    if (!shared) ldb = ld;
    return rc;
}

// The one place of the type rules on this side (spmv_api.c states them ahead of its gate from the public handle's data_size), for the forward (one
// output type, out2 = out1) and the backward: io_type HANDLE is the handle-precision path and has no other output type; F16 or BF16 needs a float
// handle and output types HANDLE or io_type.
static bool attention_types_ok(const spmv_dev *d, int io_type, int out1, int out2)
{
    if (io_type == SPMV_HIP_T_HANDLE) return out1 == SPMV_HIP_T_HANDLE && out2 == SPMV_HIP_T_HANDLE;
    return (io_type == SPMV_HIP_T_F16 || io_type == SPMV_HIP_T_BF16) && (out1 == SPMV_HIP_T_HANDLE || out1 == io_type) && (out2 == SPMV_HIP_T_HANDLE || out2 == io_type) &&
           (!d || d->vsize == sizeof(float));
}

// The operands: spmv_attention_call (spmv_shim.h).  With lse NULL the launches are those without a log-sum-exp.  io_type F16 or BF16: a host
// operand is staged at its own element size; attention_launch finds the kernels of every io_type.
extern "C" int spmv_shim_attention(spmv_dev *d, const spmv_attention_call *c)
{
    const int heads = c->heads, kv_heads = c->kv_heads, k = c->k, dv = c->dv, io_type = c->io_type, o_type = c->o_type;
    if (!attention_types_ok(d, io_type, o_type, o_type))
        return fail(SPMV_HIP_E_ARG, "attention: 16-bit operands need a float handle, io_type F16 or BF16 and o_type HANDLE or io_type (io_type = %d, o_type = %d)", io_type, o_type);
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "attention: schedule not built");
    if (kv_heads < 1 || heads < 1 || heads % kv_heads != 0) return fail(SPMV_HIP_E_ARG, "attention: need kv_heads >= 1 and heads a multiple of it (heads = %d, kv_heads = %d)", heads, kv_heads);
    const long long wk = (long long) heads * k, wv = (long long) heads * dv;
    const long long gk = (long long) kv_heads * k, gv = (long long) kv_heads * dv; // K's and V's widths
    if (heads < 1 || k < 1 || dv < 1 || wk > INT_MAX || wv > INT_MAX || c->ldq < wk || c->ldk < gk || c->ldv < gv || c->ldo < wv)
        return fail(SPMV_HIP_E_ARG, "attention: need heads, k, dv >= 1, heads * k and heads * dv within int, ldq >= heads * k, ldk >= kv_heads * k, ldv >= kv_heads * dv, ldo >= heads * dv (heads = %d, kv_heads = %d, k = %d, dv = %d, ld = %lld, %lld, %lld, %lld)",
                    heads, kv_heads, k, dv, c->ldq, c->ldk, c->ldv, c->ldo);
    if (c->bias && (c->ldb < 0 || (c->ldb > 0 && c->ldb < d->nnz)))
        return fail(SPMV_HIP_E_ARG, "attention: the bias planes need ldb = 0 (one plane for all heads) or ldb >= nnz (ldb = %lld, nnz = %lld)", c->ldb, d->nnz);
    if (c->lse && c->ldl < d->m) return fail(SPMV_HIP_E_ARG, "attention: the log-sum-exp planes need ldl >= m (ldl = %lld, m = %d)", c->ldl, d->m);
    if (d->m > 0 && (!c->q || !c->kk || !c->v || !c->o)) return fail(SPMV_HIP_E_ARG, "attention: Q, K, V or O is NULL");
    if (d->nnz > 0 && !d->colidx) return fail(SPMV_HIP_E_NOSTATE, "attention: the resident column indices were released (spmv_shim_restore_columns first)");
    if (d->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    int rc;
    if ((rc = spmm_plan(d)) || (rc = attention_plan(d))) return rc;
    const size_t s = d->vsize;
    const size_t si = io_type ? 2 : s, so = o_type ? 2 : s; // element sizes of Q / K / V and of O
    Stager stg{d};
    AttentionArgs a;
    a.m = d->m;
    a.heads = heads;
    a.io_type = io_type;
    a.o_type = o_type;
    a.gs = heads / kv_heads;
    a.k = k;
    a.dv = dv;
    a.nb = d->spmm_nb;
    a.nlong = d->spmm_nlong;
    a.cus = d->cus;
    a.split = d->spmm_split;
    a.longs = d->spmm_longs;
    a.rowptr = d->rowptr;
    a.colidx = d->colidx;
    a.long_off = d->att_off;
    a.park = d->att_park;
    a.scale = c->scale;
    a.q = c->q; a.ldq = c->ldq;
    a.kk = c->kk; a.ldk = c->ldk;
    a.v = c->v; a.ldv = c->ldv;
    a.o = c->o; a.ldo = c->ldo;
    a.bias = d->nnz > 0 ? c->bias : nullptr; a.ldb = a.bias ? c->ldb : 0; // no entry: no bias is read
    a.lse = c->lse; a.ldl = a.lse ? c->ldl : 0;
    // every row of O gets its heads * dv elements, empty rows their zeros: a staged result is written completely before it is copied back
    if ((rc = stg.in(d->stage[STAGE_ATT_Q], a.q, a.ldq, (size_t) d->m, (int) wk, si)) || (rc = stg.in(d->stage[STAGE_ATT_K], a.kk, a.ldk, (size_t) d->n, (int) gk, si)) ||
        (rc = stg.in(d->stage[STAGE_ATT_V], a.v, a.ldv, (size_t) d->n, (int) gv, si)) || (rc = stg.out(d->stage[STAGE_ATT_O], a.o, a.ldo, (size_t) d->m, (int) wv, so)) ||
        (a.bias && (rc = attention_stage_bias(stg, d->stage[STAGE_ATT_B], a.bias, a.ldb, heads))) ||
        (a.lse && (rc = stg.out(d->stage[STAGE_ATT_L], a.lse, a.ldl, (size_t) heads, d->m)))) return rc; // every row of every plane is written
    // the access width changes no bit (kernels/attention.hpp): chosen per call from what the addresses allow -- with more than one head, every
    // head's first column has to allow whole segments as well (seg_ok, state.hpp: 16 bytes, 8 of a 16-bit operand)
    a.vec = seg_ok(a.q, a.ldq, si) && seg_ok(a.kk, a.ldk, si) && seg_ok(a.v, a.ldv, si) && seg_ok(a.o, a.ldo, so) &&
            (heads == 1 || (seg_cols_ok(k, si) && seg_cols_ok(dv, si) && seg_cols_ok(dv, so)));
    const hipError_t e = attention_launch(a, s == sizeof(double), d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "attention: launch: %s", hipGetErrorString(e));
    return stg.finish();
}

// one timer preamble: what is given must be a device pointer, and Q, K, V and O must be given (is_device_ptr(NULL) is false)
extern "C" double spmv_shim_time_attention(spmv_dev *d, const spmv_attention_call *c, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || iters <= 0) { fail(SPMV_HIP_E_ARG, "time_attention: bad arguments"); return -1.0; }
    if (!is_device_ptr(c->q) || !is_device_ptr(c->kk) || !is_device_ptr(c->v) || !is_device_ptr(c->o) || (c->bias && !is_device_ptr(c->bias)) || (c->lse && !is_device_ptr(c->lse))) {
        fail(SPMV_HIP_E_ARG, "time_attention: Q, K, V, O, the bias and L must be device pointers");
        return -1.0;
    }
    return time_events(d, "time_attention", warmup, iters, ms_out, [&] { return spmv_shim_attention(d, c); });
}

// O and L of two partial results merged by their log-sum-exps (spmv_hip_attention_merge; kernels/attention_merge.hpp): the matrix is not read,
// only the handle's m, precision, stream and staging.  o may be o1 and l may be l1; l NULL: the merged log-sum-exp is not wanted.
extern "C" int spmv_shim_attention_merge(spmv_dev *d, int heads, int dv, const void *o1, long long ldo1, const void *l1, long long ldl1, const void *o2, long long ldo2,
                                         const void *l2, long long ldl2, void *o, long long ldo, void *l, long long ldl)
{
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "attention_merge: schedule not built");
    const long long wv = (long long) heads * dv;
    if (heads < 1 || dv < 1 || wv > INT_MAX || ldo1 < wv || ldo2 < wv || ldo < wv)
        return fail(SPMV_HIP_E_ARG, "attention_merge: need heads, dv >= 1, heads * dv within int and ldo1, ldo2, ldo >= heads * dv (heads = %d, dv = %d, ld = %lld, %lld, %lld)", heads,
                    dv, ldo1, ldo2, ldo);
    if (ldl1 < d->m || ldl2 < d->m || (l && ldl < d->m))
        return fail(SPMV_HIP_E_ARG, "attention_merge: the log-sum-exp planes need ldl1, ldl2, ldl >= m (ld = %lld, %lld, %lld, m = %d)", ldl1, ldl2, ldl, d->m);
    if (d->m > 0 && (!o1 || !l1 || !o2 || !l2 || !o)) return fail(SPMV_HIP_E_ARG, "attention_merge: O1, L1, O2, L2 or O is NULL");
    if (d->m == 0) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    const size_t s = d->vsize;
    Stager stg{d};
    AttentionMergeArgs a;
    a.m = d->m;
    a.heads = heads;
    a.dv = dv;
    a.cus = d->cus;
    a.o1 = o1; a.ldo1 = ldo1;
    a.l1 = l1; a.ldl1 = ldl1;
    a.o2 = o2; a.ldo2 = ldo2;
    a.l2 = l2; a.ldl2 = ldl2;
    a.o = o; a.ldo = ldo;
    a.l = l; a.ldl = l ? ldl : 0;
    int rc;
    // a host accumulator (o == o1, l == l1) is read through one buffer and written through another: the copies keep the in-place rule
    if ((rc = stg.in(d->stage[STAGE_MRG_O1], a.o1, a.ldo1, (size_t) d->m, (int) wv)) || (rc = stg.in(d->stage[STAGE_MRG_L1], a.l1, a.ldl1, (size_t) heads, d->m)) ||
        (rc = stg.in(d->stage[STAGE_MRG_O2], a.o2, a.ldo2, (size_t) d->m, (int) wv)) || (rc = stg.in(d->stage[STAGE_MRG_L2], a.l2, a.ldl2, (size_t) heads, d->m)) ||
        (rc = stg.out(d->stage[STAGE_MRG_O], a.o, a.ldo, (size_t) d->m, (int) wv)) || (a.l && (rc = stg.out(d->stage[STAGE_MRG_L], a.l, a.ldl, (size_t) heads, d->m)))) return rc;
    // the access width changes no bit (kernels/attention_merge.hpp): with more than one head, every head's first column has to be 16-byte aligned as well
    a.vec = wide_ok(a.o1, a.ldo1, s) && wide_ok(a.o2, a.ldo2, s) && wide_ok(a.o, a.ldo, s) && (heads == 1 || ((size_t) dv * s) % 16 == 0);
    const hipError_t e = attention_merge_launch(a, s == sizeof(double), d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "attention_merge: launch: %s", hipGetErrorString(e));
    return stg.finish();
}

extern "C" double spmv_shim_time_attention_merge(spmv_dev *d, int heads, int dv, const void *o1, long long ldo1, const void *l1, long long ldl1, const void *o2, long long ldo2,
                                                 const void *l2, long long ldl2, void *o, long long ldo, void *l, long long ldl, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || iters <= 0) { fail(SPMV_HIP_E_ARG, "time_attention_merge: bad arguments"); return -1.0; }
    if (!is_device_ptr(o1) || !is_device_ptr(l1) || !is_device_ptr(o2) || !is_device_ptr(l2) || !is_device_ptr(o) || (l && !is_device_ptr(l))) {
        fail(SPMV_HIP_E_ARG, "time_attention_merge: the operands must be device pointers");
        return -1.0;
    }
    return time_events(d, "time_attention_merge", warmup, iters, ms_out,
                       [&] { return spmv_shim_attention_merge(d, heads, dv, o1, ldo1, l1, ldl1, o2, ldo2, l2, ldl2, o, ldo, l, ldl); });
}

