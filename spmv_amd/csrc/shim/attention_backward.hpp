// shim/attention_backward.hpp -- part of spmv_shim.hip: dQ, dK, dV and dB of O = softmax_rows(scale * Q K^T on the RESIDENT pattern) V in two
// passes per round of up to hg heads.  One entry point, spmv_shim_attention_backward, and its timer serve every public variant (one head, heads,
// bias, GQA, driven by the final O and log-sum-exp, 16-bit operands): spmv_api.c passes them all as one spmv_attention_backward_call (spmv_shim.h).
// The kernels are kernels/attention_backward.hpp, launched from their own translation unit (spmv_attention_backward.hip,
// attention_backward_launch: compiled in one part per element type of Q, K, V and G); the tables are spmm's batch table and long-row list of the
// resident matrix and, when dK or dV is wanted, those of the attached transpose.  This side adds the two nnz-sized arrays the passes share.
#pragma once

// attb_p / attb_ds: `planes` planes of nnz elements each, plane g one head's P / dS in CSR order.  Allocated at the first call that needs them,
// grown (never shrunk) when a later call needs more planes; nothing in them outlives a call, so growing copies nothing.
static int attention_backward_plan(spmv_dev *d, int planes)
{
    if (d->attb_p && d->attb_ds && d->attb_planes >= planes) return SPMV_HIP_OK;
    const size_t bytes = d->vsize * (size_t) d->nnz * (size_t) planes;
    quiesce(d); // an asynchronous call may still read the arrays that go back to the pool
    auto drop = [&](void *&p) {
        if (!p) return;
        (void) pool_free(p);
        p = nullptr;
        d->device_bytes -= (long long) d->attb_bytes; // what dev_alloc counted for it
    };
    drop(d->attb_p);
    drop(d->attb_ds);
    d->attb_planes = 0;
    d->attb_bytes = bytes ? bytes : 16;
    int rc;
    if ((rc = dev_alloc(d, &d->attb_p, bytes, false))) return rc;
    if ((rc = dev_alloc(d, &d->attb_ds, bytes, false))) { drop(d->attb_p); return rc; }
    d->attb_planes = planes;
    return SPMV_HIP_OK;
}

// heads per round (the planes a call needs): at most `limit` when limit > 0 (option "attention_backward_heads"); limit = 0: the most for which
// the two arrays, 2 * hg * s * nnz bytes, stay within an eighth of the device's memory -- the pool's default share (pool_cap), used as a bound
// on memory, not as a measured optimum; one head at the least.  Changes no bit: only memory and the number of rounds.
// gs (query heads per K / V head): the default is rounded down to a multiple of gs when it is at least gs, so that no round of the default path
// starts inside a group (the column pass then never reads dK / dV back); an explicit limit is taken as it is.
static int attention_backward_group(const spmv_dev *d, int heads, int limit, int gs = 1)
{
    if (limit > 0) return heads < limit ? heads : limit;
    static long long eighth = -1; // of the first device asked about: the devices of one process are alike
    if (eighth < 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); total_b = (size_t) 64 << 30; }
        eighth = (long long) (total_b / 8);
    }
    const long long per_head = 2 * (long long) d->vsize * d->nnz;
    const long long fit = per_head > 0 ? eighth / per_head : heads;
    const int hg = fit >= heads ? heads : (fit < 1 ? 1 : (int) fit);
    return hg >= gs ? hg - hg % gs : hg;
}

// The operands: spmv_attention_backward_call (spmv_shim.h).  When dk or dvo is wanted the transpose must be attached with its column indices
// resident (spmv_shim_transpose, spmv_shim_transpose_restore_columns); its values are not read.  db is written by the row pass alone: with only db
// wanted the column pass does not run and the transpose is not looked at.  The planes, bias and db are per QUERY head.
// io_type F16 or BF16: a host operand is staged at its own element size (attention_backward_launch finds the kernels of every io_type); with
// kv_heads < heads a 16-bit dk / dvo is summed in the handle's float arrays attb_nk / attb_nv (n x kv_heads * k, n x kv_heads * dv; allocated at
// the first such call, grown when a call needs more, counted in device_bytes) and rounded once into the caller's arrays by the call's last launch.
extern "C" int spmv_shim_attention_backward(spmv_dev *d, const spmv_attention_backward_call *c)
{
    const int heads = c->heads, kv_heads = c->kv_heads, k = c->k, dv = c->dv, io_type = c->io_type, dq_type = c->dq_type, dkv_type = c->dkv_type;
    if (!attention_types_ok(d, io_type, dq_type, dkv_type))
        return fail(SPMV_HIP_E_ARG, "attention_backward: 16-bit operands need a float handle, io_type F16 or BF16 and dq_type, dkv_type HANDLE or io_type (io_type = %d, dq_type = %d, dkv_type = %d)",
                    io_type, dq_type, dkv_type);
    if (io_type != SPMV_HIP_T_HANDLE && d && d->m > 0 && (c->o == nullptr) != (c->lse == nullptr))
        return fail(SPMV_HIP_E_ARG, "attention_backward: O and L are given together or not at all");
    const bool stats = c->stats != 0; // else o and lse are not looked at
    const void *o = stats ? c->o : nullptr, *lse = stats ? c->lse : nullptr;
    if (!d || !d->built) return fail(SPMV_HIP_E_NOSTATE, "attention_backward: schedule not built");
    if (kv_heads < 1 || heads < 1 || heads % kv_heads != 0)
        return fail(SPMV_HIP_E_ARG, "attention_backward: need kv_heads >= 1 and heads a multiple of it (heads = %d, kv_heads = %d)", heads, kv_heads);
    const long long wk = (long long) heads * k, wv = (long long) heads * dv;
    const long long gk = (long long) kv_heads * k, gv = (long long) kv_heads * dv; // the widths of K and dK, of V and dV
    if (heads < 1 || k < 1 || dv < 1 || wk > INT_MAX || wv > INT_MAX || c->max_heads < 0 || c->ldq < wk || c->ldk < gk || c->ldv < gv || c->ldg < wv || (c->dq && c->lddq < wk) ||
        (c->dk && c->lddk < gk) || (c->dvo && c->lddv < gv))
        return fail(SPMV_HIP_E_ARG, "attention_backward: need heads, k, dv >= 1, heads * k and heads * dv within int, ldq >= heads * k, ldk >= kv_heads * k, ldv >= kv_heads * dv, ldg >= heads * dv, lddq >= heads * k, lddk >= kv_heads * k, lddv >= kv_heads * dv (heads = %d, kv_heads = %d, k = %d, dv = %d)",
                    heads, kv_heads, k, dv);
    if (d->m > 0 && (!c->q || !c->kk || !c->v || !c->g)) return fail(SPMV_HIP_E_ARG, "attention_backward: Q, K, V or G is NULL");
    if (stats && ((d->m > 0 && (!o || !lse)) || c->ldo < wv || c->ldl < d->m))
        return fail(SPMV_HIP_E_ARG, "attention_backward: the final O and L are needed, with ldo >= heads * dv and ldl >= m (ldo = %lld, ldl = %lld, m = %d)", c->ldo, c->ldl, d->m);
    if ((c->bias && (c->ldb < 0 || (c->ldb > 0 && c->ldb < d->nnz))) || (c->db && c->lddb < d->nnz))
        return fail(SPMV_HIP_E_ARG, "attention_backward: the bias planes need ldb = 0 (one plane for all heads) or ldb >= nnz, those of dB lddb >= nnz (ldb = %lld, lddb = %lld, nnz = %lld)",
                    c->ldb, c->lddb, d->nnz);
    if (!c->dq && !c->dk && !c->dvo && !c->db) return SPMV_HIP_OK;
    if (d->nnz > 0 && !d->colidx) return fail(SPMV_HIP_E_NOSTATE, "attention_backward: the resident column indices were released (spmv_shim_restore_columns first)");
    void *const db = d->nnz > 0 ? c->db : nullptr; // no entry: dB has no element
    const bool cols = (c->dk || c->dvo) && d->n > 0;
    spmv_dev *t = d->tr;
    if (cols && (!t || !d->tr_perm || (t->nnz > 0 && !t->colidx))) return fail(SPMV_HIP_E_NOSTATE, "attention_backward: the transpose is not attached with its column indices");
    if ((d->m == 0 || (!c->dq && !db)) && !cols) return SPMV_HIP_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(SPMV_HIP_E_RUNTIME, "hipSetDevice(%d) failed", d->device);
    int rc;
    const int hg = attention_backward_group(d, heads, c->max_heads, heads / kv_heads);
    if ((rc = spmm_plan(d)) || (rc = attention_backward_plan(d, hg)) || (cols && (rc = spmm_plan(t)))) return rc;
    const size_t s = d->vsize;
    const size_t si = io_type ? 2 : s, sq = dq_type ? 2 : s, so = dkv_type ? 2 : s; // element sizes of Q / K / V / G, of dQ and of dK / dV
    Stager stg{d};
    AttentionBwdArgs a;
    a.m = d->m;
    a.n = d->n;
    a.kv_heads = kv_heads;
    a.io_type = io_type;
    a.dq_type = dq_type;
    a.dkv_type = dkv_type;
    a.heads = heads;
    a.hg = hg;
    a.gs = heads / kv_heads;
    a.plane = d->nnz;
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
    a.scale = c->scale;
    a.q = c->q; a.ldq = c->ldq;
    a.kk = c->kk; a.ldk = c->ldk;
    a.v = c->v; a.ldv = c->ldv;
    a.g = c->g; a.ldg = c->ldg;
    a.dq = d->m > 0 ? c->dq : nullptr; a.lddq = c->lddq;
    a.dk = cols ? c->dk : nullptr; a.lddk = c->lddk;
    a.dvo = cols ? c->dvo : nullptr; a.lddv = c->lddv;
    a.bias = d->nnz > 0 ? c->bias : nullptr; a.ldb = a.bias ? c->ldb : 0; // no entry: no bias is read
    a.db = db; a.lddb = c->lddb;
    if (stats && d->m > 0) { a.o = o; a.ldo = c->ldo; a.lse = lse; a.ldl = c->ldl; }
    // every row of a wanted output gets its elements, empty rows and columns their zeros: a staged result is written completely before it is copied back
    if ((rc = stg.in(d->stage[STAGE_ATTB_Q], a.q, a.ldq, (size_t) d->m, (int) wk, si)) || (rc = stg.in(d->stage[STAGE_ATTB_K], a.kk, a.ldk, (size_t) d->n, (int) gk, si)) ||
        (rc = stg.in(d->stage[STAGE_ATTB_V], a.v, a.ldv, (size_t) d->n, (int) gv, si)) || (rc = stg.in(d->stage[STAGE_ATTB_G], a.g, a.ldg, (size_t) d->m, (int) wv, si)) ||
        (a.dq && (rc = stg.out(d->stage[STAGE_ATTB_DQ], a.dq, a.lddq, (size_t) d->m, (int) wk, sq))) ||
        (a.dk && (rc = stg.out(d->stage[STAGE_ATTB_DK], a.dk, a.lddk, (size_t) d->n, (int) gk, so))) ||
        (a.dvo && (rc = stg.out(d->stage[STAGE_ATTB_DV], a.dvo, a.lddv, (size_t) d->n, (int) gv, so))) ||
        (a.bias && (rc = attention_stage_bias(stg, d->stage[STAGE_ATT_B], a.bias, a.ldb, heads))) ||
        (a.db && (rc = stg.out(d->stage[STAGE_ATT_DB], a.db, a.lddb, (size_t) heads, (int) d->nnz))) || // every entry of every plane is written
        (a.o && ((rc = stg.in(d->stage[STAGE_ATTB_O], a.o, a.ldo, (size_t) d->m, (int) wv)) || (rc = stg.in(d->stage[STAGE_ATTB_L], a.lse, a.ldl, (size_t) heads, d->m))))) return rc;
    // a 16-bit dK / dV over groups of heads is never a partial sum: the column pass adds in the handle's float arrays, the narrowing rounds once
    if (a.gs > 1 && dkv_type != SPMV_HIP_T_HANDLE && (a.dk || a.dvo)) {
        if (a.dk) {
            if ((rc = stg.reserve(d->attb_nk, sizeof(float) * (size_t) d->n * (size_t) gk))) return rc;
            a.nar_dk = a.dk; a.nar_lddk = a.lddk;
            a.dk = d->attb_nk.p; a.lddk = gk;
        }
        if (a.dvo) {
            if ((rc = stg.reserve(d->attb_nv, sizeof(float) * (size_t) d->n * (size_t) gv))) return rc;
            a.nar_dv = a.dvo; a.nar_lddv = a.lddv;
            a.dvo = d->attb_nv.p; a.lddv = gv;
        }
        a.dkv_type = SPMV_HIP_T_HANDLE;
    }
    // the access width changes no bit (kernels/attention_backward.hpp): chosen per call from what the addresses allow -- with more than one head,
    // every head's first column has to allow whole segments as well (seg_ok, state.hpp: 16 bytes, 8 of a 16-bit operand).  A call's element sizes
    // are s alone, or 2 and 4, which ask the same of a head's width (a multiple of 4): Q's size stands for every operand's there
    const size_t sk = a.dkv_type ? 2 : s; // dK's and dV's as the kernels write them
    a.vec = seg_ok(a.q, a.ldq, si) && seg_ok(a.kk, a.ldk, si) && seg_ok(a.v, a.ldv, si) && seg_ok(a.g, a.ldg, si) && (!a.dq || seg_ok(a.dq, a.lddq, sq)) &&
            (!a.dk || seg_ok(a.dk, a.lddk, sk)) && (!a.dvo || seg_ok(a.dvo, a.lddv, sk)) && (!a.o || seg_ok(a.o, a.ldo, s)) &&
            (heads == 1 || (seg_cols_ok(k, si) && seg_cols_ok(dv, si)));
    const hipError_t e = attention_backward_launch(a, s == sizeof(double), d->stream);
    if (e != hipSuccess) return fail(SPMV_HIP_E_RUNTIME, "attention_backward: launch: %s", hipGetErrorString(e));
    return stg.finish();
}

// one timer preamble: what is given must be a device pointer, and Q, K, V, G and -- when they drive the row pass -- O and L must be given
// (is_device_ptr(NULL) is false)
extern "C" double spmv_shim_time_attention_backward(spmv_dev *d, const spmv_attention_backward_call *c, int warmup, int iters, float *ms_out)
{
    if (!d || !d->built || iters <= 0) { fail(SPMV_HIP_E_ARG, "time_attention_backward: bad arguments"); return -1.0; }
    auto dev_or_null = [](const void *p) { return !p || is_device_ptr(p); };
    if (!is_device_ptr(c->q) || !is_device_ptr(c->kk) || !is_device_ptr(c->v) || !is_device_ptr(c->g) || (c->stats && (!c->o || !c->lse)) || !dev_or_null(c->o) || !dev_or_null(c->lse) ||
        !dev_or_null(c->bias) || !dev_or_null(c->dq) || !dev_or_null(c->dk) || !dev_or_null(c->dvo) || !dev_or_null(c->db)) {
        fail(SPMV_HIP_E_ARG, "time_attention_backward: Q, K, V, G, O, L, the bias and the outputs must be device pointers");
        return -1.0;
    }
    return time_events(d, "time_attention_backward", warmup, iters, ms_out, [&] { return spmv_shim_attention_backward(d, c); });
}
