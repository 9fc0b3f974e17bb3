/*
 * spmv_api.c -- host side of the drop-in API, plain C11 (north_star: "host code stays C").
 *
 * Replaces the reference's handle + dispatch layer, src/src_spmv/common.c:
 *   gemv_Handle_init / gemv_create_handle / handle_init_common_parameters   common.c:18-29, 63-83
 *   spmv_create_handle_all_in_one                                           common.c:123-190
 *   spmv (indirect call through spmv_functions[])                           common.c:278-304, 85-94
 *   spmv_clear_handle / spmv_destory_handle                                 common.c:31-71
 *   Methods_names / Vectorized_names / funcNames                            common.c:306-339
 *
 * What is different by design: the per-method "get_handle" inspectors and "_Selected" executors
 * of the reference (serial_spmv.c ... csr5_spmv.cpp) are CPU code; here create() asks the
 * planner (spmv_plan.c) for a GPU schedule and hands it to the HIP shim (spmv_shim.hip), and
 * spmv() forwards to the shim.  Without a working HIP device every call reports SPMV_HIP_E_NODEVICE
 * and computes nothing.  The one piece of host arithmetic (host_rows.c: VECTOR_NONE + Method_Serial /
 * Method_Parallel, BASELINE config 1) runs only when option "host_rows" switches it on -- it is a
 * configuration the caller asks for, never a fallback.
 */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spmv.h"
#include "spmv_hip.h"
#include "spmv_hip_tools.h"
#include "spmv_internal.h"
#include "spmv_shim.h"
#include "reorder/rcm.h"

/* ---------------------------------------------------------------- name tables (ABI data symbols) */
const char *Methods_names[] = {
    "Method_Serial", "Method_Parallel", "Method_Balanced", "Method_Balanced2",
    "Method_BalancedYid", "Method_SellCSigma", "Method_Csr5Spmv",
};
const char *Vectorized_names[] = {
    "VECTOR_NONE", "VECTOR_AVX2", "VECTOR_AVX512", "VECTOR_HIP",
};
#define FN4(m) m "_VECTOR_NONE", m "_VECTOR_AVX2", m "_VECTOR_AVX512", m "_VECTOR_HIP"
const char *funcNames[] = {
    FN4("Method_Serial"), FN4("Method_Parallel"), FN4("Method_Balanced"), FN4("Method_Balanced2"),
    FN4("Method_BalancedYid"), FN4("Method_SellCSigma"), FN4("Method_Csr5Spmv"),
};

/* ---------------------------------------------------------------- error channel (thread-local) */
static _Thread_local int g_err_code = 0;
static _Thread_local char g_err_text[512] = "";

void spmv_set_error(int code, const char *where, const char *what)
{
    g_err_code = code;
    snprintf(g_err_text, sizeof g_err_text, "%s: %s", where, what ? what : "");
    if (!getenv("SPMV_HIP_QUIET")) fprintf(stderr, "[spmv_hip] error %d in %s\n", code, g_err_text);
    /* the API is all-void like the reference's (which checks nothing, not even malloc): a caller that cannot poll
     * spmv_hip_last_error() may ask for the process to stop at the first failure instead of computing on */
    if (getenv("SPMV_HIP_ABORT_ON_ERROR")) abort();
}
int spmv_hip_last_error(void) { return g_err_code; }
const char *spmv_hip_last_error_string(void) { return g_err_text; }
void spmv_hip_clear_error(void) { g_err_code = 0; g_err_text[0] = 0; }
int spmv_hip_device_count(void) { return spmv_shim_device_count(); }
void spmv_hip_trim_pool(void) { spmv_shim_trim_pool(); }

/* the shim's code goes out with the shim's text; `refuse` is the same for a rule of this file; a timer's failure is a negative time */
static int report(int rc, const char *where)
{
    if (rc) spmv_set_error(rc, where, spmv_shim_error_text());
    return rc;
}
static double report_time(double ms, const char *where)
{
    if (ms < 0) spmv_set_error(SPMV_HIP_E_RUNTIME, where, spmv_shim_error_text());
    return ms;
}
static int refuse(int code, const char *where, const char *what)
{
    spmv_set_error(code, where, what);
    return code;
}
static size_t value_size(spmv_Handle_t h) { return h->data_size == sizeof(double) ? sizeof(double) : sizeof(float); } /* serial_spmv.c:48-54 */
static long long alg_bytes(long long m, long long n, long long nnz, long long s) { return 4ll * (m + 1) + nnz * (4 + s) + s * n + s * m; } /* SURVEY 8d */

/* ---------------------------------------------------------------- handle life-cycle */
static void handle_reset(spmv_Handle_t h) /* common.c:18-29 */
{
    h->spmvMethod = Method_Serial;
    h->data_size = 0;
    h->nthreads = 0;
    h->vectorizedWay = VECTOR_NONE;
    h->Level_3_opt_used = 0;
    h->RowPtr = NULL;
    h->ColIdx = NULL;
    h->index = NULL;
    h->Matrix_Val = NULL;
    h->Y_temp = NULL;
    h->extraHandle = NULL;
}

static void index_free(spmv_Handle_t h)
{
    if (h->Level_3_opt_used && h->index) free(h->index); /* the permutation is owned by the handle (common.c:44-50) */
    h->index = NULL;
    h->Level_3_opt_used = 0;
}

static void state_free(spmv_Handle_t h)
{
    index_free(h);
    spmv_hip_state *st = (spmv_hip_state *) h->extraHandle;
    if (st) {
        if (st->dev) spmv_shim_matrix_destroy(st->dev);
        if (st->multi) spmv_shim_multi_destroy(st->multi);
        free(st);
        h->extraHandle = NULL;
    }
}

void spmv_clear_handle(spmv_Handle_t h) /* common.c:31-52, 69-71 */
{
    if (!h) return;
    state_free(h);
    handle_reset(h);
}

void spmv_destory_handle(spmv_Handle_t h) /* common.c:54-61 */
{
    if (!h) return;
    state_free(h);
    free(h);
}

/* Option "reorder" (SURVEY 8f f-4): RCM on host copies of the pattern, B = P A P^T uploaded instead
 * of A, the permutation published in handle->index -- the protocol of the reference's OPT_LEVEL 3
 * path (common.c:144-156: permuted copy + index; test_spmv.c:95-101,130-137: the caller gathers
 * XX[i] = X[index[i]] before spmv() and scatters Y[index[i]] = YY[i] after).  Returns 0 when the
 * permuted matrix is resident, non-zero to fall back to the unpermuted upload. */
/* ---------------------------------------------------------------- values changed in place
 * The reference multiplies the arrays passed to THIS call (common.c:286-298); this library multiplies its HBM-resident copy.  Option
 * "check_values" closes the gap: at create a checksum of Matrix_Val is kept, spmv() recomputes it and refreshes the resident copies when
 * it differs.  Mode 1: the full position-weighted sum (shim; host loop or one device reduction).  Mode 2 (default, HOST arrays -- the
 * reference's only mode, where a call already moves x and y over PCIe): the same sum over a SAMPLE -- every 64th 32-bit word (at most
 * 65536 of them) plus the first and last 1024 words -- certain to see an update that touches the whole array (a Newton or time step),
 * blind to most single-entry edits (spmv_hip_update_values or mode 1 are for those). */
static unsigned long long sampled_host_checksum(const void *val, long long words)
{
    const unsigned *w = (const unsigned *) val;
    unsigned long long s = 0;
    long long i;
    const long long edge = words < 2048 ? words : 1024;
    for (i = 0; i < edge; ++i) s += ((unsigned long long) w[i] + 0x9E3779B97F4A7C15ull) * (2ull * (unsigned long long) i + 1ull);
    if (words >= 2048) {
        /* every 64th word, but never more than 65536 samples: a 2.56 GB value array (config 2) costs 65 k cache lines per call, under a millisecond */
        const long long stride = (words - 2048) / 65536 > 64 ? (words - 2048) / 65536 : 64;
        for (i = words - 1024; i < words; ++i) s += ((unsigned long long) w[i] + 0x9E3779B97F4A7C15ull) * (2ull * (unsigned long long) i + 1ull);
        for (i = 1024; i < words - 1024; i += stride) s += ((unsigned long long) w[i] + 0x9E3779B97F4A7C15ull) * (2ull * (unsigned long long) i + 1ull);
    }
    return s;
}

/* take the checksum the handle's options ask for (create, re-inspection, update_values) */
static void watch_values(spmv_Handle_t h, spmv_hip_state *st, const void *Val, long long nnz)
{
    const long mode = st->opts.v[SPMV_OPT_CHECK_VALUES];
    st->val_sum_valid = 0;
    st->val_words = nnz * (long long) (value_size(h) / 4);
    if (!Val || st->val_words <= 0 || mode == 0) return;
    if (mode == 1) {
        if (spmv_shim_checksum_words(Val, st->val_words, &st->val_sum) == SPMV_HIP_OK) st->val_sum_valid = 1;
    } else if (!spmv_shim_is_device_ptr(Val)) {
        st->val_sum = sampled_host_checksum(Val, st->val_words);
        st->val_sum_valid = 2;
    }
}

/* host copies of P A P^T and the permutation (all malloc'ed; 0 on success) */
static int reorder_on_host(size_t vs, int m, const int *RowPtr, const int *ColIdx, const void *Val, int **rp2, int **ci2, void **va2, int **perm_out)
{
    int *rp = (int *) malloc(sizeof(int) * ((size_t) m + 1)), *ci = NULL, *perm = NULL;
    void *va = NULL;
    int rc = 1, nnz;
    *rp2 = *ci2 = NULL; *va2 = NULL; *perm_out = NULL;
    if (!rp || spmv_shim_copy_to_host(rp, RowPtr, sizeof(int) * ((size_t) m + 1))) goto out;
    nnz = rp[m];
    if (rp[0] != 0 || nnz < 0) goto out;
    { /* RowPtr must be monotone within [0, nnz] before anything indexes ColIdx/Val with it */
        int i;
        for (i = 0; i < m; ++i)
            if (rp[i] > rp[i + 1] || rp[i + 1] > nnz) goto out;
    }
    ci = (int *) malloc(sizeof(int) * (size_t) (nnz ? nnz : 1));
    va = malloc(vs * (size_t) (nnz ? nnz : 1));
    perm = (int *) malloc(sizeof(int) * (size_t) m);
    if (!ci || !va || !perm) goto out;
    if (spmv_shim_copy_to_host(ci, ColIdx, sizeof(int) * (size_t) nnz) || spmv_shim_copy_to_host(va, Val, vs * (size_t) nnz)) goto out;
    if (spmv_rcm_order(m, rp, ci, perm) || spmv_permute_csr(m, rp, ci, va, vs, perm, rp2, ci2, va2)) goto out;
    *perm_out = perm;
    perm = NULL;
    rc = 0;
out:
    free(rp); free(ci); free(va); free(perm);
    return rc;
}

static int upload_reordered(spmv_Handle_t h, spmv_hip_state *st, int m, int n, const int *RowPtr,
                            const int *ColIdx, const void *Val)
{
    const size_t vs = value_size(h);
    int *rp2 = NULL, *ci2 = NULL, *perm = NULL;
    void *va2 = NULL;
    int rc = 1;
    if (reorder_on_host(vs, m, RowPtr, ColIdx, Val, &rp2, &ci2, &va2, &perm)) goto out;
    if (spmv_shim_matrix_create(&st->dev, m, n, rp2, ci2, va2, vs) != SPMV_HIP_OK) goto out;
    h->index = perm;
    h->Level_3_opt_used = 1;
    perm = NULL;
    rc = 0;
out:
    free(perm); free(rp2); free(ci2); free(va2);
    return rc;
}

/* Option "gpus" > 0: row blocks over the GPUs of this process (shim/multi.hpp; BASELINE config 5, SURVEY 8e, the GPU
 * analogue of numa.c:277-304).  Every shard is planned from ITS row statistics and built on its device. */
/* plan + inspect every shard (and its boundary sub-matrix, if the range exchange split one off) of a multi-GPU state */
static int multi_plan_shards(spmv_Handle_t h, spmv_hip_state *st, SPMV_METHODS *actual)
{
    const int G = spmv_shim_multi_count(st->multi);
    int g, part, rc = SPMV_HIP_OK;
    for (g = 0; g < G && !rc; ++g)
        for (part = 0; part < 2 && !rc; ++part) {
            spmv_dev *dev = part == 0 ? spmv_shim_multi_shard(st->multi, g) : spmv_shim_multi_boundary(st->multi, g);
            spmv_stats stats;
            spmv_plan plan;
            SPMV_METHODS a = st->requested;
            if (!dev) continue;
            rc = spmv_shim_matrix_stats(dev, &stats);
            if (!rc) {
                spmv_plan_choose(st->requested, &stats, (size_t) h->data_size, &st->opts, &plan, &a, 1);
                rc = spmv_shim_build(dev, &plan);
            }
            if (!rc && g == 0 && part == 0) { *actual = a; st->plan = plan; }
        }
    if (rc) {
        spmv_set_error(rc, "create/multi shard", spmv_shim_error_text());
        spmv_shim_multi_destroy(st->multi);
        st->multi = NULL;
    }
    return rc;
}

static int state_build_multi(spmv_Handle_t h, spmv_hip_state *st, int m, int n, const int *RowPtr,
                             const int *ColIdx, const void *Val)
{
    SPMV_METHODS actual = st->requested;
    int rc;
    if (st->multi) { spmv_shim_multi_destroy(st->multi); st->multi = NULL; }
    index_free(h);
    rc = -1;
    if (st->opts.v[SPMV_OPT_REORDER] >= 1 && m == n && m > 1 && RowPtr && ColIdx && Val) {
        /* Option "reorder" on a multi-GPU handle: P A P^T is what gets cut into equal-nnz row blocks -- the reason a partitioner exists in the
         * reference at all (fewer off-block columns: HyperGraphInterface.cpp:60-147 feeding the NUMA row blocks, numa.c:277-304).  The
         * caller-side protocol is the single-GPU one: XX[i] = X[index[i]], Y[index[i]] = YY[i] (test_spmv.c:95-101, 130-137). */
        const size_t vs = h->data_size == sizeof(double) ? sizeof(double) : sizeof(float);
        int *rp2 = NULL, *ci2 = NULL, *perm = NULL;
        void *va2 = NULL;
        spmv_dev *tmp = NULL;
        if (st->opts.v[SPMV_OPT_REORDER] == 1 && (perm = (int *) malloc(sizeof(int) * (size_t) m)) != NULL &&
            spmv_shim_matrix_create(&tmp, m, n, RowPtr, ColIdx, Val, vs) == SPMV_HIP_OK && spmv_shim_reorder_rcm(tmp, perm) == SPMV_HIP_OK) {
            /* reorder = 1: on the device (kernels/rcm.hpp) -- the whole matrix on the current device for a moment, P A P^T handed to the sharding as device arrays */
            const int *drp = NULL, *dci = NULL;
            const void *dva = NULL;
            spmv_shim_matrix_arrays(tmp, &drp, &dci, &dva);
            rc = spmv_shim_multi_create(&st->multi, (int) st->opts.v[SPMV_OPT_GPUS], (int) st->opts.v[SPMV_OPT_X_EXCHANGE], m, n, drp, dci, dva, vs);
            if (rc == SPMV_HIP_OK) { h->index = perm; h->Level_3_opt_used = 1; perm = NULL; }
        } else if ((free(perm), perm = NULL, spmv_hip_clear_error(), 1) && reorder_on_host(vs, m, RowPtr, ColIdx, Val, &rp2, &ci2, &va2, &perm) == 0) {
            rc = spmv_shim_multi_create(&st->multi, (int) st->opts.v[SPMV_OPT_GPUS], (int) st->opts.v[SPMV_OPT_X_EXCHANGE], m, n, rp2, ci2, va2, vs);
            if (rc == SPMV_HIP_OK) { h->index = perm; h->Level_3_opt_used = 1; perm = NULL; }
        } else {
            /* never silently: the caller asked for a permutation and will gather x / scatter y by handle->index -- which stays NULL, i.e. identity */
            spmv_set_error(SPMV_HIP_E_ARG, "create/multi", "option reorder: the matrix could not be reordered (bad RowPtr or out of host memory); created unpermuted, handle->index = NULL");
        }
        if (tmp) spmv_shim_matrix_destroy(tmp);
        free(perm); free(rp2); free(ci2); free(va2);
    }
    if (rc != SPMV_HIP_OK)
        rc = spmv_shim_multi_create(&st->multi, (int) st->opts.v[SPMV_OPT_GPUS], (int) st->opts.v[SPMV_OPT_X_EXCHANGE], m, n, RowPtr, ColIdx, Val,
                                    (size_t) h->data_size);
    if (rc) { spmv_set_error(rc, "create/multi", spmv_shim_error_text()); return rc; }
    rc = multi_plan_shards(h, st, &actual);
    if (rc) return rc;
    st->m = m;
    st->n = n;
    watch_values(h, st, Val, spmv_shim_multi_nnz(st->multi));
    st->from_blocks = 0;
    h->spmvMethod = actual; /* shard 0's: the shards of a skewed matrix may differ (Balanced vs Balanced2) */
    h->RowPtr = (BASIC_INT_TYPE *) RowPtr;
    h->ColIdx = (BASIC_INT_TYPE *) ColIdx;
    h->Matrix_Val = (void *) Val;
    return SPMV_HIP_OK;
}

/* Extension: a multi-GPU handle from row blocks that already exist separately -- block g: rows[g] rows, LOCAL 0-based int32 RowPtr,
 * GLOBAL column indices in [0, n), values; host or device pointers -- the way the reference's NUMA experiment hands every node its
 * block (src/samples/numa.c:277-304, 129-158).  No monolithic CSR exists, so BASELINE config 5 (8 x 1e7 rows x 32 = 2.56e9
 * non-zeros, beyond one int32 RowPtr) is expressible through the C API.  Block g lives on device g; x_exchange as for option "gpus".
 * spmv() on such a handle takes full-length X / Y and IGNORES its CSR arguments (pass NULL). */
void spmv_hip_create_handle_from_blocks(spmv_Handle_t *Handle, int blocks, const BASIC_INT_TYPE *rows, BASIC_INT_TYPE n,
                                        BASIC_INT_TYPE *const *RowPtr, BASIC_INT_TYPE *const *ColIdx, void *const *Matrix_Val,
                                        SPMV_METHODS Function, BASIC_SIZE_TYPE size)
{
    spmv_Handle_t h;
    spmv_hip_state *st;
    SPMV_METHODS actual;
    int rc;
    if (!Handle) { spmv_set_error(SPMV_HIP_E_ARG, "create_from_blocks", "Handle is NULL"); return; }
    h = (spmv_Handle_t) malloc(sizeof(spmv_Handle));
    *Handle = h;
    if (!h) { spmv_set_error(SPMV_HIP_E_ALLOC, "create_from_blocks", "malloc(handle)"); return; }
    handle_reset(h);
    if ((int) Function < (int) Method_Serial || (int) Function >= (int) Method_Total_Size) Function = Method_Serial;
    h->nthreads = 1;
    h->vectorizedWay = VECTOR_HIP;
    h->data_size = size;
    h->spmvMethod = Function;
    st = (spmv_hip_state *) calloc(1, sizeof *st);
    if (!st) { spmv_set_error(SPMV_HIP_E_ALLOC, "create_from_blocks", "malloc(state)"); return; }
    st->requested = actual = Function;
    spmv_options_snapshot(&st->opts);
    rc = spmv_shim_multi_create_blocks(&st->multi, blocks, (int) st->opts.v[SPMV_OPT_X_EXCHANGE], rows, n, (const int *const *) RowPtr,
                                       (const int *const *) ColIdx, (const void *const *) Matrix_Val, (size_t) size);
    if (rc) { spmv_set_error(rc, "create_from_blocks", spmv_shim_error_text()); free(st); return; }
    if (multi_plan_shards(h, st, &actual) != SPMV_HIP_OK) { free(st); return; }
    st->m = spmv_shim_multi_rows(st->multi);
    st->n = n;
    st->from_blocks = 1;
    h->spmvMethod = actual;
    h->extraHandle = st;
}

/* A matrix with locality in PART of its entries (every tenth row random; web graphs: 90 % of a row near the diagonal, 10 % on hub
 * columns) stages no x window -- one stray entry per tile is enough -- and the blocked executor pays for the local entries too.  When
 * the shim's sample says a real part of the entries, but not all, lies near its tile's centre column, the matrix is split once into
 * A_near + A_far (csrc/kernels/split.hpp), each half planned and inspected like any matrix -- near: the method's tile schedule, every
 * tile staged by construction, never the blocked executor; far: always the blocked executor, accumulating into y -- and the pair is
 * timed against the schedule as built; the faster stays (spmv_hip_info.split_ms, far_nnz). */
static void try_split(spmv_Handle_t h, spmv_hip_state *st, spmv_dev *dev, SPMV_METHODS actual)
{
    spmv_dev *halves[2] = {NULL, NULL};
    double t_built, t_split = -1.0;
    int k, ok = 1;
    if (st->opts.v[SPMV_OPT_SPLIT] != 1 || !spmv_shim_split_candidate(dev)) return;
    t_built = spmv_shim_time_self(dev, 5);
    if (t_built <= 0.0 || spmv_shim_split(dev, &halves[0], &halves[1]) != SPMV_HIP_OK) return;
    for (k = 0; k < 2 && ok; ++k) {
        spmv_stats stats;
        spmv_plan plan;
        spmv_options o = st->opts;
        SPMV_METHODS a = actual;
        o.v[SPMV_OPT_CACHE_BLOCK] = k == 0 ? 0 : 2;
        /* the near half of a CSR-vector request: rows that lost entries to the far half are no longer regular (every tenth row empty:
         * 57 % of CSR-vector's 8-row steps run masked, 0.89 vs 0.55 ms under CSR5) -- let the row statistics choose, as auto_method = 1 does */
        if (k == 0 && actual == Method_Parallel && o.v[SPMV_OPT_AUTO_METHOD] < 1) o.v[SPMV_OPT_AUTO_METHOD] = 1;
        ok = spmv_shim_matrix_stats(halves[k], &stats) == SPMV_HIP_OK;
        if (ok) {
            spmv_plan_choose(actual == Method_Serial ? Method_Parallel : actual, &stats, (size_t) h->data_size, &o, &plan, &a, k == 0 && actual == Method_Parallel);
            ok = spmv_shim_build(halves[k], &plan) == SPMV_HIP_OK;
        }
    }
    if (ok && getenv("SPMV_HIP_SPLIT_DEBUG")) {
        spmv_hip_info a, b;
        double tn = spmv_shim_time_self(halves[0], 5), tf = spmv_shim_time_self(halves[1], 5);
        (void) spmv_shim_info(halves[0], &a);
        (void) spmv_shim_info(halves[1], &b);
        fprintf(stderr, "[spmv_hip] split: as built %.4f ms; near %lld nnz %s %.4f ms; far %lld nnz %s %.4f ms (inspect %.1f / %.1f ms)\n", t_built, a.nnz, a.kernel_name,
                tn, b.nnz, b.kernel_name, tf, a.inspect_ms, b.inspect_ms);
    }
    if (ok && spmv_shim_attach_split(dev, halves[0], halves[1], 0) == SPMV_HIP_OK) {
        t_split = spmv_shim_time_self(dev, 5);
        if (t_split > 0.0 && t_split < 0.9 * t_built) (void) spmv_shim_attach_split(dev, halves[0], halves[1], 1); /* keep: drop the unsplit schedule */
        else (void) spmv_shim_attach_split(dev, NULL, NULL, 0);                                                    /* destroys the halves */
    } else {
        if (halves[0]) spmv_shim_matrix_destroy(halves[0]);
        if (halves[1]) spmv_shim_matrix_destroy(halves[1]);
    }
    spmv_shim_note_split_ms(dev, t_built, t_split);
    spmv_hip_clear_error();
}

/* Plan + inspect one uploaded matrix as create() does: row statistics -> spmv_plan_choose -> spmv_shim_build, the measured choice
 * (auto_method = 2), the near / far split, the release of the column copy, the handle's stream and async setting.  Used for the handle's
 * matrix (state_build) and for its transpose (transpose_ready), with the handle's requested method and options.  *plan and *actual receive
 * what was chosen, *nnz the matrix's non-zeros.  A failure is reported; the matrix is the caller's to destroy. */
static int plan_and_build(spmv_Handle_t h, spmv_hip_state *st, spmv_dev *dev, spmv_plan *plan_out, SPMV_METHODS *actual_out, long long *nnz_out)
{
    spmv_stats stats;
    spmv_plan plan;
    SPMV_METHODS actual = st->requested;
    int rc = spmv_shim_matrix_stats(dev, &stats);
    if (rc) { spmv_set_error(rc, "create/stats", spmv_shim_error_text()); return rc; }
    spmv_plan_choose(st->requested, &stats, (size_t) h->data_size, &st->opts, &plan, &actual, 1);
    rc = spmv_shim_build(dev, &plan);
    if (rc) { spmv_set_error(rc, "create/inspect", spmv_shim_error_text()); return rc; }
    /* A schedule that could not stage a single x window on a matrix whose x is far larger than an L2 is
     * switched to the row-block x column-slab executor INSIDE spmv_shim_build (option "cache_block", default
     * automatic) -- whatever the method, so Method_Parallel / Method_CSR5SPMV requests on matrices without
     * column locality no longer run the gather-bound tile kernels. */
    /* automatic choice, measured (auto_method = 2): the rules above pick from row statistics; which schedule is
     * fastest also depends on the columns and, by a few percent, on the device.  For matrices
     * large enough to be worth it, every candidate schedule is built and timed on scratch vectors and the
     * fastest is kept (the rule-based choice stays on a tie within 2 %). */
    if (st->opts.v[SPMV_OPT_AUTO_METHOD] == 2 && stats.nnz >= (1ll << 20)) {
        static const SPMV_METHODS cand[] = {Method_Parallel, Method_CSR5SPMV, Method_SellCSigma, Method_Balanced_Yid, Method_Balanced};
        spmv_plan best_plan = plan;
        SPMV_METHODS best_method = actual;
        double best_ms = spmv_shim_time_self(dev, 5);
        unsigned k, j, nseen = 1;
        spmv_plan seen[1 + sizeof cand / sizeof cand[0]]; /* schedules already built and timed: several methods may plan the same one (short heavy-tailed rows) */
        int current_is_best = best_ms >= 0.0;
        seen[0] = plan;
        for (k = 0; k < sizeof cand / sizeof cand[0] && best_ms >= 0.0; ++k) {
            spmv_plan p;
            SPMV_METHODS a = cand[k];
            double ms;
            int dup = 0;
            spmv_plan_choose(cand[k], &stats, (size_t) h->data_size, &st->opts, &p, &a, 0);
            for (j = 0; j < nseen; ++j) /* the same schedule with the same shape is the same multiply whatever the method is called: timing noise must not choose */
                if (seen[j].sched == p.sched && seen[j].lanes_per_row == p.lanes_per_row && seen[j].long_thr == p.long_thr && seen[j].sell_sigma == p.sell_sigma &&
                    seen[j].sell_long_thr == p.sell_long_thr && seen[j].csr5_sigma == p.csr5_sigma && seen[j].rowblock_nnz == p.rowblock_nnz) dup = 1;
            if (dup) continue;
            seen[nseen++] = p;
            if (spmv_shim_build(dev, &p) != SPMV_HIP_OK) { current_is_best = 0; continue; }
            current_is_best = 0;
            ms = spmv_shim_time_self(dev, 5);
            if (ms >= 0.0 && ms < 0.98 * best_ms) { best_ms = ms; best_plan = p; best_method = a; current_is_best = 1; }
        }
        if (!current_is_best) {
            rc = spmv_shim_build(dev, &best_plan);
            if (rc) { spmv_set_error(rc, "create/inspect", spmv_shim_error_text()); return rc; }
        }
        plan = best_plan;
        actual = best_method;
    }
    try_split(h, st, dev, actual);
    if (st->opts.v[SPMV_OPT_KEEP_COLUMNS] == 0) (void) spmv_shim_release_columns(dev); /* the last build of this create is done */
    if (st->stream_set) spmv_shim_set_stream(dev, st->stream);
    spmv_shim_set_async(dev, st->async);
    *plan_out = plan;
    *actual_out = actual;
    *nnz_out = stats.nnz;
    return SPMV_HIP_OK;
}

/* Upload + plan + inspect.  Used by create and by spmv() when it is handed another matrix. */
static int state_build(spmv_Handle_t h, spmv_hip_state *st, int m, int n, const int *RowPtr,
                       const int *ColIdx, const void *Val)
{
    long long nnz = 0;
    SPMV_METHODS actual = st->requested;
    int rc;
    if (st->opts.v[SPMV_OPT_GPUS] > 0) return state_build_multi(h, st, m, n, RowPtr, ColIdx, Val);
    if (st->dev) { spmv_shim_matrix_destroy(st->dev); st->dev = NULL; }
    if (m < 0 || n < 0 || (m > 0 && !RowPtr)) {
        spmv_set_error(SPMV_HIP_E_ARG, "create", "negative size or NULL RowPtr");
        return SPMV_HIP_E_ARG;
    }
    index_free(h);
    rc = -1;
    if (st->opts.v[SPMV_OPT_REORDER] == 2 && m == n && m > 1 && RowPtr && ColIdx && Val)
        rc = upload_reordered(h, st, m, n, RowPtr, ColIdx, Val); /* the host BFS of round 1 (reorder/rcm.c), kept for comparison; 0 = uploaded the permuted matrix */
    if (rc != 0) rc = spmv_shim_matrix_create(&st->dev, m, n, RowPtr, ColIdx, Val, (size_t) h->data_size);
    if (rc) { spmv_set_error(rc, "create/upload", spmv_shim_error_text()); return rc; }
    if (st->opts.v[SPMV_OPT_REORDER] == 1 && m == n && m > 1) {
        /* reverse Cuthill-McKee ON THE DEVICE over the matrix just uploaded (kernels/rcm.hpp): P A P^T replaces it, handle->index = the
         * permutation (test_spmv.c:95-101, 130-137: the caller gathers x and scatters y).  A failure leaves the unpermuted matrix resident
         * and index NULL -- and says so. */
        int *perm = (int *) malloc(sizeof(int) * (size_t) m);
        if (perm && spmv_shim_reorder_rcm(st->dev, perm) == SPMV_HIP_OK) {
            h->index = perm;
            h->Level_3_opt_used = 1;
        } else {
            free(perm);
            spmv_set_error(SPMV_HIP_E_RUNTIME, "create/reorder", perm ? spmv_shim_error_text() : "malloc(perm)");
        }
    }
    rc = plan_and_build(h, st, st->dev, &st->plan, &actual, &nnz);
    if (rc) {
        spmv_shim_matrix_destroy(st->dev);
        st->dev = NULL;
        return rc;
    }
    st->m = m;
    st->n = n;
    watch_values(h, st, Val, nnz);
    h->spmvMethod = actual;
    h->RowPtr = (BASIC_INT_TYPE *) RowPtr;
    h->ColIdx = (BASIC_INT_TYPE *) ColIdx;
    h->Matrix_Val = (void *) Val;
    return SPMV_HIP_OK;
}

void spmv_create_handle_all_in_one(spmv_Handle_t *Handle, BASIC_INT_TYPE m, BASIC_INT_TYPE n,
                                   BASIC_INT_TYPE *RowPtr, BASIC_INT_TYPE *ColIdx, void *Matrix_Val,
                                   BASIC_SIZE_TYPE nthreads, SPMV_METHODS Function, BASIC_SIZE_TYPE size,
                                   VECTORIZED_WAY vectorizedWay, const char *MtxToken)
{
    spmv_Handle_t h;
    spmv_hip_state *st;
    (void) MtxToken; /* the reference uses it for METIS cache file names only (common.c:152-154) */
    if (!Handle) { spmv_set_error(SPMV_HIP_E_ARG, "create", "Handle is NULL"); return; }
    h = (spmv_Handle_t) malloc(sizeof(spmv_Handle)); /* common.c:63-67 */
    *Handle = h;
    if (!h) { spmv_set_error(SPMV_HIP_E_ALLOC, "create", "malloc(handle)"); return; }
    handle_reset(h);
    if ((int) Function < (int) Method_Serial || (int) Function >= (int) Method_Total_Size)
        Function = Method_Serial; /* common.c:136 */
    /* common.c:74-83 */
    h->nthreads = nthreads;
    h->vectorizedWay = vectorizedWay;
    h->data_size = size;
    h->spmvMethod = Function;

    st = (spmv_hip_state *) calloc(1, sizeof *st);
    if (!st) { spmv_set_error(SPMV_HIP_E_ALLOC, "create", "malloc(state)"); return; }
    st->requested = Function;
    spmv_options_snapshot(&st->opts);
    h->extraHandle = st;
    /* BASELINE config 1 ("reference plumbing, no GPU"): VECTOR_NONE + Method_Serial / Method_Parallel run
     * the plain-C row loop of host_rows.c on the caller's arrays, which are BORROWED like the reference
     * does (common.c:157-159) -- but only when option "host_rows" asks for it. */
    if (st->opts.v[SPMV_OPT_HOST_ROWS] == 1 && vectorizedWay == VECTOR_NONE &&
        (Function == Method_Serial || Function == Method_Parallel)) {
        if (spmv_shim_is_device_ptr(RowPtr) || spmv_shim_is_device_ptr(ColIdx) || spmv_shim_is_device_ptr(Matrix_Val)) {
            spmv_set_error(SPMV_HIP_E_ARG, "create(host_rows)", "the host row loop needs HOST arrays; device pointers were passed");
            free(st);
            h->extraHandle = NULL;
            return;
        }
        if (m < 0 || n < 0 || (m > 0 && (!RowPtr || (RowPtr[m] > 0 && (!ColIdx || !Matrix_Val))))) {
            spmv_set_error(SPMV_HIP_E_ARG, "create(host_rows)", "negative size or NULL CSR array");
            free(st);
            h->extraHandle = NULL;
            return;
        }
        st->host_rows = 1;
        st->m = m;
        st->n = n;
        h->RowPtr = RowPtr;
        h->ColIdx = ColIdx;
        h->Matrix_Val = Matrix_Val;
        return;
    }
    if (state_build(h, st, m, n, RowPtr, ColIdx, Matrix_Val) != SPMV_HIP_OK) {
        /* keep a valid handle whose spmv() is a reported no-op */
        free(st);
        h->extraHandle = NULL;
    }
}

/* The prologue of every multiply (spmv, spmv_hip_spmm): the CSR arguments of THIS call against the resident matrix -- re-inspection
 * for another matrix, refresh of values changed in place (option "check_values").  0, or the code already reported. */
static int refresh_resident(spmv_Handle_t handle, spmv_hip_state *st, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr,
                            const BASIC_INT_TYPE *ColIdx, const void *Matrix_Val)
{
    int rc;
    /* The reference re-reads the CSR arguments on every call (common.c:286-298).  Same pointers
     * and m as at create -> the HBM-resident matrix; anything else -> re-inspect that matrix. */
    if (st->from_blocks) {
        /* created from row blocks: there is no monolithic CSR the arguments could name; they are ignored */
    } else if (m != st->m || RowPtr != handle->RowPtr || ColIdx != handle->ColIdx ||
               Matrix_Val != handle->Matrix_Val) {
        if (!st->warned_rebuild && !getenv("SPMV_HIP_QUIET")) {
            fprintf(stderr, "[spmv_hip] spmv(): CSR arguments differ from create(); re-inspecting "
                            "(slow path, DESIGN.md \"CSR arguments\")\n");
            st->warned_rebuild = 1;
        }
        if ((rc = state_build(handle, st, m, st->n, RowPtr, ColIdx, Matrix_Val)) != SPMV_HIP_OK) return rc;
    } else if (st->val_sum_valid) {
        /* option "check_values": the reference re-reads Matrix_Val on every call, so a caller may change the
         * values in place between calls (Newton steps, time stepping).  Detect that by checksum and refresh
         * the resident copies (no re-inspection: the pattern is the same). */
        unsigned long long sum = 0;
        int have = 1;
        if (st->val_sum_valid == 2) sum = sampled_host_checksum(Matrix_Val, st->val_words);
        else have = spmv_shim_checksum_words(Matrix_Val, st->val_words, &sum) == SPMV_HIP_OK;
        if (have && sum != st->val_sum) {
            if (st->multi && !handle->Level_3_opt_used) { /* every shard refreshes its slice of the values in place */
                if ((rc = report(spmv_shim_multi_update_values(st->multi, Matrix_Val), "spmv/refresh values"))) return rc;
                st->val_sum = sum;
            } else if (handle->Level_3_opt_used) {
                /* option "reorder": the resident matrix is P A P^T, whose value order is not the caller's -- the values
                 * cannot be refreshed in place; upload, reorder and inspect the caller's matrix again (state_build
                 * takes a new checksum) */
                if ((rc = state_build(handle, st, m, st->n, RowPtr, ColIdx, Matrix_Val)) != SPMV_HIP_OK) return rc;
            } else {
                if ((rc = report(spmv_shim_update_values(st->dev, Matrix_Val), "spmv/refresh values"))) return rc;
                st->val_sum = sum;
            }
        }
    }
    return SPMV_HIP_OK;
}

void spmv(const spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr,
          const BASIC_INT_TYPE *ColIdx, const void *Matrix_Val, const void *X, void *Y)
{
    spmv_hip_state *st;
    if (handle == NULL) return; /* common.c:285 */
    st = (spmv_hip_state *) handle->extraHandle;
    if (st && st->host_rows) { /* the arguments of THIS call are what is multiplied (common.c:286-298) */
        if (m > 0 && (!RowPtr || !Y || (RowPtr[m] > 0 && (!ColIdx || !Matrix_Val || !X)))) {
            spmv_set_error(SPMV_HIP_E_ARG, "spmv(host_rows)", "NULL argument");
            return;
        }
        spmv_host_rows(m, RowPtr, ColIdx, Matrix_Val, (size_t) handle->data_size, X, Y,
                       handle->spmvMethod == Method_Parallel ? (int) (handle->nthreads > 0 ? handle->nthreads : 1) : 1);
        return;
    }
    if (!st || (!st->dev && !st->multi)) {
        spmv_set_error(SPMV_HIP_E_NOSTATE, "spmv", "handle has no device state (create failed?)");
        return;
    }
    if (refresh_resident(handle, st, m, RowPtr, ColIdx, Matrix_Val) != SPMV_HIP_OK) return;
    (void) report(st->multi ? spmv_shim_multi_run(st->multi, X, Y) : spmv_shim_run(st->dev, X, Y), "spmv");
}

/* ---------------------------------------------------------------- extensions */
static spmv_hip_state *state_of(spmv_Handle_t h, const char *where)
{
    spmv_hip_state *st = h ? (spmv_hip_state *) h->extraHandle : NULL;
    if (st && st->multi && !st->dev) {
        spmv_set_error(SPMV_HIP_E_ARG, where, "not available on a multi-GPU handle (option \"gpus\"): it owns one stream per device");
        return NULL;
    }
    if (!st || !st->dev) {
        spmv_set_error(SPMV_HIP_E_NOSTATE, where, "handle has no device state");
        return NULL;
    }
    return st;
}

static spmv_multi *multi_of(spmv_Handle_t h, const char *where)
{
    spmv_hip_state *st = h ? (spmv_hip_state *) h->extraHandle : NULL;
    if (!st || !st->multi) {
        spmv_set_error(SPMV_HIP_E_NOSTATE, where, "not a multi-GPU handle (create it with option \"gpus\" > 0)");
        return NULL;
    }
    return st->multi;
}

/* Number of GPUs the handle's row blocks live on (0: not a multi-GPU handle). */
int spmv_hip_multi_gpus(spmv_Handle_t h)
{
    spmv_hip_state *st = h ? (spmv_hip_state *) h->extraHandle : NULL;
    return st && st->multi ? spmv_shim_multi_count(st->multi) : 0;
}

int spmv_hip_multi_uses_rccl(spmv_Handle_t h)
{
    spmv_hip_state *st = h ? (spmv_hip_state *) h->extraHandle : NULL;
    return st && st->multi ? spmv_shim_multi_uses_rccl(st->multi) : 0;
}

/* one shim call on the multi-GPU state, reported */
static int multi_call(spmv_Handle_t h, const char *where, int (*call)(spmv_multi *))
{
    spmv_multi *mt = multi_of(h, where);
    return mt ? report(call(mt), where) : SPMV_HIP_E_NOSTATE;
}

int spmv_hip_multi_slices(spmv_Handle_t h, int gpu, void **x_slice, long long *x_first, long long *x_count,
                          void **y_block, long long *y_first, long long *y_count, int *device)
{
    spmv_multi *mt = multi_of(h, "multi_slices");
    return mt ? report(spmv_shim_multi_slices(mt, gpu, x_slice, x_first, x_count, y_block, y_first, y_count, device), "multi_slices") : SPMV_HIP_E_NOSTATE;
}

int spmv_hip_multi_step(spmv_Handle_t h) { return multi_call(h, "multi_step", spmv_shim_multi_step); }
int spmv_hip_multi_step_async(spmv_Handle_t h) { return multi_call(h, "multi_step_async", spmv_shim_multi_step_async); }
int spmv_hip_multi_synchronize(spmv_Handle_t h) { return multi_call(h, "multi_synchronize", spmv_shim_multi_sync); }

int spmv_hip_set_stream(spmv_Handle_t h, void *stream)
{
    spmv_hip_state *st = state_of(h, "set_stream");
    if (!st) return SPMV_HIP_E_NOSTATE;
    st->stream = stream;
    st->stream_set = 1;
    return spmv_shim_set_stream(st->dev, stream);
}

int spmv_hip_set_async(spmv_Handle_t h, int async)
{
    spmv_hip_state *st = state_of(h, "set_async");
    if (!st) return SPMV_HIP_E_NOSTATE;
    st->async = async != 0;
    return spmv_shim_set_async(st->dev, st->async);
}

int spmv_hip_synchronize(spmv_Handle_t h)
{
    spmv_hip_state *st = state_of(h, "synchronize");
    return st ? report(spmv_shim_sync(st->dev), "synchronize") : SPMV_HIP_E_NOSTATE;
}

int spmv_hip_get_info(spmv_Handle_t h, spmv_hip_info *out)
{
    spmv_hip_state *st = h ? (spmv_hip_state *) h->extraHandle : NULL;
    if (st && st->host_rows && out) { /* no device state: describe the host loop */
        memset(out, 0, sizeof *out);
        out->device = -1;
        out->schedule = SPMV_SCHED_HOST_ROWS;
        out->m = st->m;
        out->n = st->n;
        out->nnz = out->stored_nnz = st->m > 0 ? h->RowPtr[st->m] : 0;
        out->mean_row_len = st->m > 0 ? (double) out->nnz / st->m : 0.0;
        out->alg_bytes = alg_bytes(st->m, st->n, out->nnz, (long long) value_size(h));
        out->stream_bytes = out->alg_bytes;
        out->schedule_name = "host-rows";
        out->kernel_name = "spmv_host_rows";
        return SPMV_HIP_OK;
    }
    if (st && st->multi && out) { /* shard 0 names the schedule; sizes, byte counts and stored entries are summed over the
                                   * shards (inspect_ms: the slowest shard), so that rates derived from the struct are the whole matrix's */
        int rc = spmv_shim_info(spmv_shim_multi_shard(st->multi, 0), out), g;
        const int G = spmv_shim_multi_count(st->multi);
        for (g = 1; g < G && rc == SPMV_HIP_OK; ++g) {
            spmv_hip_info o;
            rc = spmv_shim_info(spmv_shim_multi_shard(st->multi, g), &o);
            if (rc != SPMV_HIP_OK) break;
            out->stream_bytes += o.stream_bytes;
            out->x_bytes += o.x_bytes;
            out->stored_nnz += o.stored_nnz;
            out->device_bytes += o.device_bytes;
            out->empty_rows += o.empty_rows;
            out->x_groups += o.x_groups;
            out->x_groups_staged += o.x_groups_staged;
            out->run_nnz += o.run_nnz;
            if (o.inspect_ms > out->inspect_ms) out->inspect_ms = o.inspect_ms;
            if (o.max_row_len > out->max_row_len) out->max_row_len = o.max_row_len;
            if (o.min_row_len < out->min_row_len) out->min_row_len = o.min_row_len;
        }
        if (rc == SPMV_HIP_OK) {
            out->m = st->m; out->n = st->n; out->nnz = spmv_shim_multi_nnz(st->multi);
            out->mean_row_len = st->m > 0 ? (double) out->nnz / st->m : 0.0;
            out->alg_bytes = alg_bytes(st->m, st->n, out->nnz, (long long) value_size(h));
        }
        return rc;
    }
    st = state_of(h, "get_info");
    if (!st || !out) return SPMV_HIP_E_NOSTATE;
    return spmv_shim_info(st->dev, out);
}

/* New values behind the pattern the handle was created with: Val (host or device, nnz entries in CSR order)
 * is copied to HBM and re-permuted into the schedule's private layouts (SELL slabs, CSR5 tiles, long-row
 * sub-matrix, row-block x column-slab streams) by device kernels; RowPtr / ColIdx, descriptors, x windows
 * and the autotune result are kept.  Cost: one pass over the values (config 2: ~1 ms against ~30 ms of
 * clear + create).  handle->Matrix_Val is set to Val, so later spmv() calls may pass either pointer. */
int spmv_hip_update_values(spmv_Handle_t h, const void *Val)
{
    spmv_hip_state *st = h ? (spmv_hip_state *) h->extraHandle : NULL;
    int rc;
    if (st && st->host_rows) { h->Matrix_Val = (void *) Val; return SPMV_HIP_OK; } /* borrowed arrays: nothing resident */
    if (!(st && st->multi) && !(st = state_of(h, "update_values"))) return SPMV_HIP_E_NOSTATE;
    if (!Val) return refuse(SPMV_HIP_E_ARG, "update_values", "Val is NULL");
    if (h->Level_3_opt_used) /* the resident matrix is P A P^T: its value order is not the caller's */
        return refuse(SPMV_HIP_E_ARG, "update_values", "not available on a reordered handle (option \"reorder\")");
    if ((rc = report(st->multi ? spmv_shim_multi_update_values(st->multi, Val) : spmv_shim_update_values(st->dev, Val), "update_values"))) return rc;
    h->Matrix_Val = (void *) Val;
    watch_values(h, st, Val, st->multi ? spmv_shim_multi_nnz(st->multi) : st->val_words / (long long) (value_size(h) / 4));
    return SPMV_HIP_OK;
}

long spmv_hip_get_handle_option(spmv_Handle_t h, const char *key)
{
    spmv_hip_state *st = h ? (spmv_hip_state *) h->extraHandle : NULL;
    return st ? spmv_options_get(&st->opts, key) : -1;
}

double spmv_hip_time_launches(spmv_Handle_t h, const void *x, void *y, int warmup, int iters, float *ms_out)
{
    spmv_hip_state *st = state_of(h, "time_launches");
    return st ? report_time(spmv_shim_time(st->dev, x, y, warmup, iters, ms_out), "time_launches") : -1.0;
}

/* ---------------------------------------------------------------- operations on the resident matrix: one gate, one prologue
 * spmm, the transposed multiplies, sddmm, the row softmax, the fused attention and their timers work on the single-GPU resident matrix.  An entry point is: its own
 * argument rules -- a NULL handle and a bad k / ld are E_ARG before the handle's state is looked at --, the gate or the prologue, the tables it
 * needs (columns, transpose), the shim call through report().  Where an entry point checks its operands for NULL is its own business and differs. */
#define RESIDENT_NOT_REORDERED 1 /* the entries are addressed in the caller's CSR order: the resident P A P^T of option "reorder" has another */

/* The gate: 0 and *out = the single-GPU device state, or the code already reported. */
static int resident_state(spmv_Handle_t h, const char *where, int flags, spmv_hip_state **out)
{
    spmv_hip_state *st = h ? (spmv_hip_state *) h->extraHandle : NULL;
    *out = NULL;
    if (!h) return refuse(SPMV_HIP_E_ARG, where, "handle is NULL");
    if (st && st->host_rows) return refuse(SPMV_HIP_E_ARG, where, "not available on a host_rows handle");
    if (st && st->multi) return refuse(SPMV_HIP_E_ARG, where, "not available on a multi-GPU handle (option \"gpus\", create_handle_from_blocks)");
    if (!st || !st->dev) return refuse(SPMV_HIP_E_NOSTATE, where, "handle has no device state (create failed or handle cleared)");
    if ((flags & RESIDENT_NOT_REORDERED) && h->Level_3_opt_used) return refuse(SPMV_HIP_E_ARG, where, "not available on a reordered handle (option \"reorder\")");
    *out = st;
    return SPMV_HIP_OK;
}

/* The prologue of an operation that takes the CSR arguments like spmv(): the gate, this call's arguments against the resident matrix
 * (refresh_resident), and what a re-inspection may have changed -- the device state, the reordering -- looked at again. */
static int resident_prologue(spmv_Handle_t h, const char *where, int flags, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                             const void *Matrix_Val, spmv_hip_state **out)
{
    int rc = resident_state(h, where, flags, out);
    if (rc || (rc = refresh_resident(h, *out, m, RowPtr, ColIdx, Matrix_Val)) != SPMV_HIP_OK) return rc;
    if (!(*out)->dev) return refuse(SPMV_HIP_E_NOSTATE, where, "handle has no device state");
    if ((flags & RESIDENT_NOT_REORDERED) && h->Level_3_opt_used) return refuse(SPMV_HIP_E_ARG, where, "not available on a reordered handle (option \"reorder\")");
    return SPMV_HIP_OK;
}

/* option keep_columns = 0 may have released the resident ColIdx at create; the handle's ColIdx is the create-time array (pointer rule) */
static int spmm_columns(spmv_Handle_t h, spmv_hip_state *st, const char *where)
{
    return report(spmv_shim_restore_columns(st->dev, h->RowPtr, h->ColIdx, h->Level_3_opt_used ? h->index : NULL), where);
}

/* ---------------------------------------------------------------- k right-hand sides */
/* the argument rules ahead of the gate: spmv_hip_spmm; its timer with m = 1 (X and Y are always needed); spmv_hip_spmm_transpose with m = 0 (it checks X and Y behind the gate) */
static int spmm_args(spmv_Handle_t h, const char *where, int k, const void *X, long long ldx, const void *Y, long long ldy, int m)
{
    if (!h) return refuse(SPMV_HIP_E_ARG, where, "handle is NULL");
    if (k < 1 || ldx < k || ldy < k) return refuse(SPMV_HIP_E_ARG, where, "need k >= 1, ldx >= k and ldy >= k");
    if (m > 0 && (!X || !Y)) return refuse(SPMV_HIP_E_ARG, where, "X or Y is NULL");
    return SPMV_HIP_OK;
}

int spmv_hip_spmm(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                  const void *Matrix_Val, int k, const void *X, long long ldx, void *Y, long long ldy)
{
    spmv_hip_state *st;
    int rc;
    if ((rc = spmm_args(handle, "spmm", k, X, ldx, Y, ldy, m)) || (rc = resident_prologue(handle, "spmm", 0, m, RowPtr, ColIdx, Matrix_Val, &st))) return rc;
    if (k == 1 && ldx == 1 && ldy == 1) return report(spmv_shim_run(st->dev, X, Y), "spmm"); /* one vector: the handle's own spmv schedule, bit-identical to spmv() */
    if ((rc = spmm_columns(handle, st, "spmm"))) return rc;
    return report(spmv_shim_spmm(st->dev, k, X, ldx, Y, ldy), "spmm");
}

double spmv_hip_time_spmm_launches(spmv_Handle_t h, int k, const void *X, long long ldx, void *Y, long long ldy, int warmup, int iters, float *ms_out)
{
    const char *where = "time_spmm_launches";
    spmv_hip_state *st;
    if (spmm_args(h, where, k, X, ldx, Y, ldy, 1) || resident_state(h, where, 0, &st) || spmm_columns(h, st, where)) return -1.0;
    return report_time(spmv_shim_time_spmm(st->dev, k, X, ldx, Y, ldy, warmup, iters, ms_out), where);
}

/* ---------------------------------------------------------------- y = A^T x */
/* A^T of the resident matrix: built on the device once per resident matrix, planned and inspected by the code path of create() with the
 * handle's requested method and options, attached to the resident matrix; afterwards its values are gathered again whenever A's changed.
 * When create() released the resident ColIdx, it is restored for the build and released again, so the forward multiply is unchanged. */
static int transpose_built(spmv_Handle_t h, spmv_hip_state *st, const char *where)
{
    int rc;
    if (!spmv_shim_transpose_of(st->dev)) {
        const int *ci = NULL;
        spmv_dev *child = NULL;
        int *perm = NULL;
        long long nnz = 0;
        SPMV_METHODS actual = st->requested;
        spmv_plan plan;
        int released;
        spmv_shim_matrix_arrays(st->dev, NULL, &ci, NULL);
        released = ci == NULL;
        if ((rc = spmm_columns(h, st, where)) != SPMV_HIP_OK) return rc;
        rc = spmv_shim_transpose(st->dev, &child, &perm);
        if (released) (void) spmv_shim_release_columns(st->dev);
        if (report(rc, where)) return rc;
        if ((rc = report(spmv_shim_attach_transpose(st->dev, child, perm), where)) != SPMV_HIP_OK) {
            spmv_shim_matrix_destroy(child);
            return rc;
        }
        if ((rc = plan_and_build(h, st, child, &plan, &actual, &nnz)) != SPMV_HIP_OK) {
            (void) spmv_shim_attach_transpose(st->dev, NULL, NULL); /* destroys child and perm */
            return rc;
        }
        st->tplan = plan;
        st->tmethod = actual;
    }
    return SPMV_HIP_OK;
}

/* ... and its values those of A as they are now */
static int transpose_ready(spmv_Handle_t h, spmv_hip_state *st, const char *where)
{
    const int rc = transpose_built(h, st, where);
    return rc ? rc : report(spmv_shim_transpose_refresh(st->dev), where);
}

static const char transpose_not_built[] = "the transpose is not built (spmv_hip_prepare_transpose, or a first spmv_hip_spmv_transpose)";

int spmv_hip_spmv_transpose(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                            const void *Matrix_Val, const void *X, void *Y)
{
    spmv_hip_state *st;
    int rc = resident_state(handle, "spmv_transpose", 0, &st); /* ahead of the prologue: the operands are checked behind the gate, before the refresh */
    if (rc) return rc;
    if ((m > 0 && !X) || (st->n > 0 && !Y)) return refuse(SPMV_HIP_E_ARG, "spmv_transpose", "X or Y is NULL");
    if ((rc = resident_prologue(handle, "spmv_transpose", 0, m, RowPtr, ColIdx, Matrix_Val, &st)) || (rc = transpose_ready(handle, st, "spmv_transpose"))) return rc;
    return report(spmv_shim_run(spmv_shim_transpose_of(st->dev), X, Y), "spmv_transpose");
}

int spmv_hip_prepare_transpose(spmv_Handle_t handle)
{
    spmv_hip_state *st;
    int rc = resident_state(handle, "prepare_transpose", 0, &st);
    return rc ? rc : transpose_ready(handle, st, "prepare_transpose");
}

int spmv_hip_get_transpose_info(spmv_Handle_t handle, spmv_hip_info *out)
{
    spmv_hip_state *st;
    int rc = resident_state(handle, "get_transpose_info", 0, &st);
    if (rc) return rc;
    if (!out) return refuse(SPMV_HIP_E_ARG, "get_transpose_info", "out is NULL");
    if (!spmv_shim_transpose_of(st->dev)) return refuse(SPMV_HIP_E_NOSTATE, "get_transpose_info", transpose_not_built);
    return report(spmv_shim_info(spmv_shim_transpose_of(st->dev), out), "get_transpose_info");
}

double spmv_hip_time_transpose_launches(spmv_Handle_t h, const void *x, void *y, int warmup, int iters, float *ms_out)
{
    const char *where = "time_transpose_launches";
    spmv_hip_state *st;
    if (resident_state(h, where, 0, &st) || transpose_ready(h, st, where)) return -1.0;
    return report_time(spmv_shim_time(spmv_shim_transpose_of(st->dev), x, y, warmup, iters, ms_out), where);
}

int spmv_hip_transpose_map(spmv_Handle_t h, int *rowptr_t, int *perm)
{
    spmv_hip_state *st;
    int rc = resident_state(h, "transpose_map", 0, &st);
    if (rc) return rc;
    if (!spmv_shim_transpose_of(st->dev)) return refuse(SPMV_HIP_E_NOSTATE, "transpose_map", transpose_not_built);
    return report(spmv_shim_transpose_map(st->dev, rowptr_t, perm), "transpose_map");
}

/* ---------------------------------------------------------------- Y = A^T X for k right-hand sides */
/* the attached transpose with its own column indices resident: what spmv_shim_spmm on the child gathers through */
static int transpose_columns(spmv_hip_state *st, const char *where)
{
    return report(spmv_shim_transpose_restore_columns(st->dev), where);
}

int spmv_hip_spmm_transpose(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                            const void *Matrix_Val, int k, const void *X, long long ldx, void *Y, long long ldy)
{
    const char *where = "spmm_transpose";
    spmv_hip_state *st;
    int rc;
    if ((rc = spmm_args(handle, where, k, NULL, ldx, NULL, ldy, 0)) || (rc = resident_state(handle, where, 0, &st))) return rc; /* the operands: behind the gate, before the refresh */
    if ((m > 0 || st->n > 0) && (!X || !Y)) return refuse(SPMV_HIP_E_ARG, where, "X or Y is NULL");
    if ((rc = resident_prologue(handle, where, 0, m, RowPtr, ColIdx, Matrix_Val, &st)) || (rc = transpose_ready(handle, st, where))) return rc;
    if (k == 1 && ldx == 1 && ldy == 1) return report(spmv_shim_run(spmv_shim_transpose_of(st->dev), X, Y), where); /* one vector: A^T's own schedule, bit-identical to spmv_hip_spmv_transpose */
    if ((rc = transpose_columns(st, where))) return rc;
    return report(spmv_shim_spmm(spmv_shim_transpose_of(st->dev), k, X, ldx, Y, ldy), where);
}

double spmv_hip_time_spmm_transpose_launches(spmv_Handle_t h, int k, const void *X, long long ldx, void *Y, long long ldy, int warmup, int iters, float *ms_out)
{
    const char *where = "time_spmm_transpose_launches";
    spmv_hip_state *st;
    if (!h || k < 1 || ldx < k || ldy < k || !X || !Y) {
        (void) refuse(SPMV_HIP_E_ARG, where, !h ? "handle is NULL" : "need k >= 1, ldx >= k, ldy >= k, X and Y");
        return -1.0;
    }
    if (resident_state(h, where, 0, &st) || transpose_ready(h, st, where) || transpose_columns(st, where)) return -1.0;
    return report_time(spmv_shim_time_spmm(spmv_shim_transpose_of(st->dev), k, X, ldx, Y, ldy, warmup, iters, ms_out), where);
}

/* ---------------------------------------------------------------- the operations over A's pattern: sddmm, row softmax and its backward */
int spmv_hip_sddmm(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                   const void *Matrix_Val, int k, const void *U, long long ldu, const void *V, long long ldv, void *Out)
{
    spmv_hip_state *st;
    spmv_hip_info info;
    int rc;
    if (!handle || k < 1 || ldu < k || ldv < k) return refuse(SPMV_HIP_E_ARG, "sddmm", !handle ? "handle is NULL" : "need k >= 1, ldu >= k and ldv >= k");
    if ((rc = resident_prologue(handle, "sddmm", RESIDENT_NOT_REORDERED, m, RowPtr, ColIdx, Matrix_Val, &st)) || (rc = report(spmv_shim_info(st->dev, &info), "sddmm"))) return rc;
    if (info.nnz == 0 || info.m == 0) return SPMV_HIP_OK; /* nothing stored: nothing written */
    if (!U || !V || !Out) return refuse(SPMV_HIP_E_ARG, "sddmm", "U, V or Out is NULL");
    if ((rc = spmm_columns(handle, st, "sddmm"))) return rc;
    return report(spmv_shim_sddmm(st->dev, k, U, ldu, V, ldv, Out), "sddmm");
}

double spmv_hip_time_sddmm_launches(spmv_Handle_t h, int k, const void *U, long long ldu, const void *V, long long ldv, void *Out, int warmup, int iters, float *ms_out)
{
    const char *where = "time_sddmm_launches";
    spmv_hip_state *st;
    if (!h || k < 1 || ldu < k || ldv < k) {
        (void) refuse(SPMV_HIP_E_ARG, where, !h ? "handle is NULL" : "need k >= 1, ldu >= k and ldv >= k");
        return -1.0;
    }
    if (resident_state(h, where, RESIDENT_NOT_REORDERED, &st) || spmm_columns(h, st, where)) return -1.0;
    return report_time(spmv_shim_time_sddmm(st->dev, k, U, ldu, V, ldv, Out, warmup, iters, ms_out), where);
}

/* P: S (forward) or P (backward); G: NULL for the forward */
static int row_softmax_call(spmv_Handle_t handle, const char *where, int backward, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                            const void *Matrix_Val, const void *P, const void *G, void *Out)
{
    spmv_hip_state *st;
    spmv_hip_info info;
    int rc;
    if ((rc = resident_prologue(handle, where, RESIDENT_NOT_REORDERED, m, RowPtr, ColIdx, Matrix_Val, &st)) || (rc = report(spmv_shim_info(st->dev, &info), where))) return rc;
    if (info.nnz == 0 || info.m == 0) return SPMV_HIP_OK; /* nothing stored: nothing written */
    if (!P || !Out || (backward && !G)) return refuse(SPMV_HIP_E_ARG, where, "a NULL array");
    /* RowPtr alone is read: a released resident ColIdx copy stays released */
    return report(backward ? spmv_shim_row_softmax_backward(st->dev, P, G, Out) : spmv_shim_row_softmax(st->dev, P, Out), where);
}

int spmv_hip_row_softmax(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                         const void *Matrix_Val, const void *S, void *Out)
{
    return row_softmax_call(handle, "row_softmax", 0, m, RowPtr, ColIdx, Matrix_Val, S, NULL, Out);
}

int spmv_hip_row_softmax_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                  const void *Matrix_Val, const void *P, const void *G, void *Out)
{
    return row_softmax_call(handle, "row_softmax_backward", 1, m, RowPtr, ColIdx, Matrix_Val, P, G, Out);
}

double spmv_hip_time_row_softmax_launches(spmv_Handle_t h, const void *S, void *Out, int warmup, int iters, float *ms_out)
{
    spmv_hip_state *st;
    if (resident_state(h, "time_row_softmax_launches", RESIDENT_NOT_REORDERED, &st)) return -1.0;
    return report_time(spmv_shim_time_row_softmax(st->dev, S, Out, warmup, iters, ms_out), "time_row_softmax_launches");
}

/* ---------------------------------------------------------------- O = softmax_rows(scale * Q K^T on A's pattern) V in one pass: one path for every variant
 * An entry point -- one head, `heads` heads side by side, with a bias, with fewer K / V heads (GQA, MQA), with the rows' log-sum-exps, on 16-bit
 * operands -- fills a spmv_attention_call (spmv_shim.h; what it has no argument for: heads = kv_heads = 1, no bias, no L, the handle's types), names
 * itself and takes the one path of calls or the one of timers. */
#define ATTENTION_16 1    /* an entry point with type arguments: the type rules are stated here, from the public handle's data_size */
#define ATTENTION_TIMER 2 /* a timer: ldl is left to the shim, which knows the handle's m */

/* the argument rules ahead of the gate, in this order: the calls with their m, the timers with m = 1 (the operands are always needed) */
static int attention_rules(spmv_Handle_t h, const char *where, int flags, const spmv_attention_call *c, BASIC_INT_TYPE m)
{
    const long long wk = (long long) c->heads * c->k, wv = (long long) c->heads * c->dv, gk = (long long) c->kv_heads * c->k, gv = (long long) c->kv_heads * c->dv;
    if (!h) return refuse(SPMV_HIP_E_ARG, where, "handle is NULL");
    if (c->heads < 1 || c->kv_heads < 1 || c->k < 1 || c->dv < 1) return refuse(SPMV_HIP_E_ARG, where, "need heads >= 1, kv_heads >= 1, k >= 1 and dv >= 1");
    if (c->heads % c->kv_heads != 0) return refuse(SPMV_HIP_E_ARG, where, "heads must be a multiple of kv_heads");
    if (wk > INT_MAX || wv > INT_MAX || gk > INT_MAX || gv > INT_MAX) return refuse(SPMV_HIP_E_ARG, where, "heads * k, heads * dv, kv_heads * k or kv_heads * dv does not fit an int");
    if (c->ldq < wk || c->ldk < gk || c->ldv < gv || c->ldo < wv)
        return refuse(SPMV_HIP_E_ARG, where, "need ldq >= heads * k, ldk >= kv_heads * k, ldv >= kv_heads * dv and ldo >= heads * dv");
    if (m > 0 && (!c->q || !c->kk || !c->v || !c->o)) return refuse(SPMV_HIP_E_ARG, where, "Q, K, V or O is NULL");
    if (c->bias && c->ldb < 0) return refuse(SPMV_HIP_E_ARG, where, "need ldb >= 0"); /* 0 < ldb < nnz: refused by the shim, nothing written */
    if (!(flags & ATTENTION_TIMER) && c->lse && c->ldl < (long long) m) return refuse(SPMV_HIP_E_ARG, where, "need ldl >= m");
    if (flags & ATTENTION_16) {
        /* data_size is in the public handle, so a handle whose create failed answers the type rules too (a cleared handle holds no precision any
         * more, data_size 0: it gets as far as the gate and is SPMV_HIP_E_NOSTATE there, like in every other call) */
        if (h->data_size != sizeof(float) && h->data_size != 0) return refuse(SPMV_HIP_E_ARG, where, "16-bit operands need an fp32 handle");
        if (c->io_type != SPMV_HIP_T_F16 && c->io_type != SPMV_HIP_T_BF16) return refuse(SPMV_HIP_E_ARG, where, "io_type must be SPMV_HIP_T_F16 or SPMV_HIP_T_BF16");
        if (c->o_type != SPMV_HIP_T_HANDLE && c->o_type != c->io_type) return refuse(SPMV_HIP_E_ARG, where, "o_type must be SPMV_HIP_T_HANDLE or equal to io_type");
    }
    return SPMV_HIP_OK;
}

static int attention_call(spmv_Handle_t h, const char *where, int flags, const spmv_attention_call *c, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr,
                          const BASIC_INT_TYPE *ColIdx, const void *Matrix_Val)
{
    spmv_hip_state *st;
    int rc;
    if ((rc = attention_rules(h, where, flags, c, m)) || (rc = resident_prologue(h, where, RESIDENT_NOT_REORDERED, m, RowPtr, ColIdx, Matrix_Val, &st)) ||
        (rc = spmm_columns(h, st, where))) return rc;
    return report(spmv_shim_attention(st->dev, c), where);
}

static double attention_time(spmv_Handle_t h, const char *where, int flags, const spmv_attention_call *c, int warmup, int iters, float *ms_out)
{
    spmv_hip_state *st;
    if (attention_rules(h, where, flags | ATTENTION_TIMER, c, 1) || resident_state(h, where, RESIDENT_NOT_REORDERED, &st) || spmm_columns(h, st, where)) return -1.0;
    return report_time(spmv_shim_time_attention(st->dev, c, warmup, iters, ms_out), where);
}

int spmv_hip_attention(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                       const void *Matrix_Val, int k, int dv, double scale,
                       const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                       void *O, long long ldo)
{
    const spmv_attention_call c = {.heads = 1, .kv_heads = 1, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv, .o = O, .ldo = ldo};
    return attention_call(handle, "attention", 0, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_launches(spmv_Handle_t h, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                        void *O, long long ldo, int warmup, int iters, float *ms_out)
{
    const spmv_attention_call c = {.heads = 1, .kv_heads = 1, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv, .o = O, .ldo = ldo};
    return attention_time(h, "time_attention_launches", 0, &c, warmup, iters, ms_out);
}

int spmv_hip_attention_heads(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                             const void *Matrix_Val, int heads, int k, int dv, double scale,
                             const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                             void *O, long long ldo)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                   .o = O, .ldo = ldo};
    return attention_call(handle, "attention_heads", 0, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_heads_launches(spmv_Handle_t h, int heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk, const void *V,
                                              long long ldv, void *O, long long ldo, int warmup, int iters, float *ms_out)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                   .o = O, .ldo = ldo};
    return attention_time(h, "time_attention_heads_launches", 0, &c, warmup, iters, ms_out);
}

int spmv_hip_attention_bias(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                            const void *Matrix_Val, int heads, int k, int dv, double scale,
                            const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                            const void *B, long long ldb, void *O, long long ldo)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                   .bias = B, .ldb = ldb, .o = O, .ldo = ldo};
    return attention_call(handle, "attention_bias", 0, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_bias_launches(spmv_Handle_t h, int heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk,
                                             const void *V, long long ldv, const void *B, long long ldb, void *O, long long ldo, int warmup, int iters, float *ms_out)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                   .bias = B, .ldb = ldb, .o = O, .ldo = ldo};
    return attention_time(h, "time_attention_bias_launches", 0, &c, warmup, iters, ms_out);
}

int spmv_hip_attention_gqa(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                           const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                           const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                           const void *B, long long ldb, void *O, long long ldo)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                   .bias = B, .ldb = ldb, .o = O, .ldo = ldo};
    return attention_call(handle, "attention_gqa", 0, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_gqa_launches(spmv_Handle_t h, int heads, int kv_heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk,
                                            const void *V, long long ldv, const void *B, long long ldb, void *O, long long ldo, int warmup, int iters, float *ms_out)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                   .bias = B, .ldb = ldb, .o = O, .ldo = ldo};
    return attention_time(h, "time_attention_gqa_launches", 0, &c, warmup, iters, ms_out);
}

int spmv_hip_attention_gqa_lse(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                               const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                               const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                               const void *B, long long ldb, void *O, long long ldo, void *L, long long ldl)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                   .bias = B, .ldb = ldb, .o = O, .ldo = ldo, .lse = L, .ldl = ldl};
    return attention_call(handle, "attention_gqa_lse", 0, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_gqa_lse_launches(spmv_Handle_t h, int heads, int kv_heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk,
                                                const void *V, long long ldv, const void *B, long long ldb, void *O, long long ldo, void *L, long long ldl, int warmup, int iters,
                                                float *ms_out)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                   .bias = B, .ldb = ldb, .o = O, .ldo = ldo, .lse = L, .ldl = ldl};
    return attention_time(h, "time_attention_gqa_lse_launches", 0, &c, warmup, iters, ms_out);
}

int spmv_hip_attention_gqa_lse_16(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                  const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale, int io_type,
                                  const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                  const void *B, long long ldb, void *O, long long ldo, int o_type, void *L, long long ldl)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .io_type = io_type, .o_type = o_type, .q = Q, .ldq = ldq,
                                   .kk = K, .ldk = ldk, .v = V, .ldv = ldv, .bias = B, .ldb = ldb, .o = O, .ldo = ldo, .lse = L, .ldl = ldl};
    return attention_call(handle, "attention_gqa_lse_16", ATTENTION_16, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_gqa_lse_16_launches(spmv_Handle_t h, int heads, int kv_heads, int k, int dv, double scale, int io_type, const void *Q, long long ldq,
                                                   const void *K, long long ldk, const void *V, long long ldv, const void *B, long long ldb, void *O, long long ldo, int o_type,
                                                   void *L, long long ldl, int warmup, int iters, float *ms_out)
{
    const spmv_attention_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .io_type = io_type, .o_type = o_type, .q = Q, .ldq = ldq,
                                   .kk = K, .ldk = ldk, .v = V, .ldv = ldv, .bias = B, .ldb = ldb, .o = O, .ldo = ldo, .lse = L, .ldl = ldl};
    return attention_time(h, "time_attention_gqa_lse_16_launches", ATTENTION_16, &c, warmup, iters, ms_out);
}

/* ---------------------------------------------------------------- two partial results merged by their log-sum-exps */

/* m is the handle's: whether an operand is NULL while m > 0, and the plane strides against m, are looked at behind the gate (nothing written) */
static int attention_merge_args(spmv_Handle_t h, const char *where, int heads, int dv, long long ldo1, long long ldo2, long long ldo)
{
    long long wv;
    if (!h) return refuse(SPMV_HIP_E_ARG, where, "handle is NULL");
    if (heads < 1 || dv < 1) return refuse(SPMV_HIP_E_ARG, where, "need heads >= 1 and dv >= 1");
    wv = (long long) heads * dv;
    if (wv > INT_MAX) return refuse(SPMV_HIP_E_ARG, where, "heads * dv does not fit an int");
    if (ldo1 < wv || ldo2 < wv || ldo < wv) return refuse(SPMV_HIP_E_ARG, where, "need ldo1, ldo2 and ldo >= heads * dv");
    return SPMV_HIP_OK;
}

int spmv_hip_attention_merge(spmv_Handle_t handle, int heads, int dv, const void *O1, long long ldo1, const void *L1, long long ldl1,
                             const void *O2, long long ldo2, const void *L2, long long ldl2, void *O, long long ldo, void *L, long long ldl)
{
    const char *where = "attention_merge";
    spmv_hip_state *st;
    int rc;
    if ((rc = attention_merge_args(handle, where, heads, dv, ldo1, ldo2, ldo))) return rc;
    if (ldl1 < 0 || ldl2 < 0 || (L && ldl < 0)) return refuse(SPMV_HIP_E_ARG, where, "need ldl1, ldl2 and ldl >= m");
    if ((rc = resident_state(handle, where, RESIDENT_NOT_REORDERED, &st))) return rc;
    return report(spmv_shim_attention_merge(st->dev, heads, dv, O1, ldo1, L1, ldl1, O2, ldo2, L2, ldl2, O, ldo, L, ldl), where);
}

double spmv_hip_time_attention_merge_launches(spmv_Handle_t h, int heads, int dv, const void *O1, long long ldo1, const void *L1, long long ldl1, const void *O2, long long ldo2,
                                              const void *L2, long long ldl2, void *O, long long ldo, void *L, long long ldl, int warmup, int iters, float *ms_out)
{
    const char *where = "time_attention_merge_launches";
    spmv_hip_state *st;
    if (attention_merge_args(h, where, heads, dv, ldo1, ldo2, ldo) || resident_state(h, where, RESIDENT_NOT_REORDERED, &st)) return -1.0;
    return report_time(spmv_shim_time_attention_merge(st->dev, heads, dv, O1, ldo1, L1, ldl1, O2, ldo2, L2, ldl2, O, ldo, L, ldl, warmup, iters, ms_out), where);
}

/* ---------------------------------------------------------------- dQ, dK, dV and dB of the fused attention in two passes over A: one path for every variant
 * Like the forward: an entry point fills a spmv_attention_backward_call, names itself and takes the path of calls or that of timers. */
#define ATTENTION_GATE_FIRST 4 /* spmv_hip_attention_backward alone: with nothing wanted it still runs the prologue, so a handle without state is
                                * SPMV_HIP_E_NOSTATE there, where every later entry point returns 0 before the handle's state is looked at */

/* the argument rules ahead of the gate, in this order: the calls with their m, the timers with m = 1.  The strides of outputs that are not wanted
 * are not looked at. */
static int attention_backward_rules(spmv_Handle_t h, const char *where, int flags, const spmv_attention_backward_call *c, BASIC_INT_TYPE m)
{
    const long long wk = (long long) c->heads * c->k, wv = (long long) c->heads * c->dv, gk = (long long) c->kv_heads * c->k, gv = (long long) c->kv_heads * c->dv;
    if (!h) return refuse(SPMV_HIP_E_ARG, where, "handle is NULL");
    if (c->heads < 1 || c->kv_heads < 1 || c->k < 1 || c->dv < 1) return refuse(SPMV_HIP_E_ARG, where, "need heads >= 1, kv_heads >= 1, k >= 1 and dv >= 1");
    if (c->heads % c->kv_heads != 0) return refuse(SPMV_HIP_E_ARG, where, "heads must be a multiple of kv_heads");
    if (wk > INT_MAX || wv > INT_MAX || gk > INT_MAX || gv > INT_MAX) return refuse(SPMV_HIP_E_ARG, where, "heads * k, heads * dv, kv_heads * k or kv_heads * dv does not fit an int");
    if (c->ldq < wk || c->ldk < gk || c->ldv < gv || c->ldg < wv || (c->dq && c->lddq < wk) || (c->dk && c->lddk < gk) || (c->dvo && c->lddv < gv))
        return refuse(SPMV_HIP_E_ARG, where, "need ldq >= heads * k, ldk >= kv_heads * k, ldv >= kv_heads * dv, ldg >= heads * dv and, for the requested outputs, lddq >= heads * k, lddk >= kv_heads * k, lddv >= kv_heads * dv");
    if (m > 0 && (!c->q || !c->kk || !c->v || !c->g)) return refuse(SPMV_HIP_E_ARG, where, "Q, K, V or G is NULL");
    if ((c->bias && c->ldb < 0) || (c->db && c->lddb < 0)) return refuse(SPMV_HIP_E_ARG, where, "need ldb >= 0 and lddb >= 0"); /* a plane stride below nnz: refused by the shim, nothing written */
    if ((flags & ATTENTION_16) && m > 0 && (c->o == NULL) != (c->lse == NULL)) return refuse(SPMV_HIP_E_ARG, where, "O and L are given together or not at all");
    if (c->stats) {
        if (c->ldo < wv) return refuse(SPMV_HIP_E_ARG, where, "need ldo >= heads * dv");
        if (c->ldl < (long long) m) return refuse(SPMV_HIP_E_ARG, where, "need ldl >= m");
        if (m > 0 && (!c->o || !c->lse)) return refuse(SPMV_HIP_E_ARG, where, "O or L is NULL");
    }
    if (flags & ATTENTION_16) { /* from the public handle's data_size, like the forward's */
        if (h->data_size != sizeof(float) && h->data_size != 0) return refuse(SPMV_HIP_E_ARG, where, "16-bit operands need an fp32 handle");
        if (c->io_type != SPMV_HIP_T_F16 && c->io_type != SPMV_HIP_T_BF16) return refuse(SPMV_HIP_E_ARG, where, "io_type must be SPMV_HIP_T_F16 or SPMV_HIP_T_BF16");
        if (c->dq_type != SPMV_HIP_T_HANDLE && c->dq_type != c->io_type) return refuse(SPMV_HIP_E_ARG, where, "dq_type must be SPMV_HIP_T_HANDLE or equal to io_type");
        if (c->dkv_type != SPMV_HIP_T_HANDLE && c->dkv_type != c->io_type) return refuse(SPMV_HIP_E_ARG, where, "dkv_type must be SPMV_HIP_T_HANDLE or equal to io_type");
    }
    return SPMV_HIP_OK;
}

/* behind the gate: A's columns and, when dK or dV is wanted, the transpose (its values are not read: no refresh) with its columns; the heads per round */
static int attention_backward_tables(spmv_Handle_t h, spmv_hip_state *st, const char *where, spmv_attention_backward_call *c)
{
    int rc = spmm_columns(h, st, where);
    if (!rc && (c->dk || c->dvo) && !(rc = transpose_built(h, st, where))) rc = transpose_columns(st, where); /* only dB (or dQ) wanted: no transpose */
    c->max_heads = (int) st->opts.v[SPMV_OPT_ATTENTION_BACKWARD_HEADS];
    return rc;
}

static int attention_backward_call(spmv_Handle_t h, const char *where, int flags, spmv_attention_backward_call *c, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr,
                                   const BASIC_INT_TYPE *ColIdx, const void *Matrix_Val)
{
    const int wanted = c->dq || c->dk || c->dvo || c->db;
    spmv_hip_state *st;
    int rc;
    if ((rc = attention_backward_rules(h, where, flags, c, m))) return rc;
    if (!wanted && !(flags & ATTENTION_GATE_FIRST)) return SPMV_HIP_OK; /* nothing wanted: no work, the handle's state is not looked at */
    if ((rc = resident_prologue(h, where, RESIDENT_NOT_REORDERED, m, RowPtr, ColIdx, Matrix_Val, &st))) return rc;
    if (!wanted) return SPMV_HIP_OK;
    if ((rc = attention_backward_tables(h, st, where, c))) return rc;
    return report(spmv_shim_attention_backward(st->dev, c), where);
}

static double attention_backward_time(spmv_Handle_t h, const char *where, int flags, spmv_attention_backward_call *c, int warmup, int iters, float *ms_out)
{
    spmv_hip_state *st;
    if (attention_backward_rules(h, where, flags, c, 1) || resident_state(h, where, RESIDENT_NOT_REORDERED, &st) || attention_backward_tables(h, st, where, c)) return -1.0;
    return report_time(spmv_shim_time_attention_backward(st->dev, c, warmup, iters, ms_out), where);
}

int spmv_hip_attention_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                const void *Matrix_Val, int k, int dv, double scale,
                                const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                const void *G, long long ldg, void *dQ, long long lddq, void *dK, long long lddk, void *dV, long long lddv)
{
    spmv_attention_backward_call c = {.heads = 1, .kv_heads = 1, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv, .g = G, .ldg = ldg,
                                      .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv};
    return attention_backward_call(handle, "attention_backward", ATTENTION_GATE_FIRST, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_backward_launches(spmv_Handle_t h, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk,
                                                 const void *V, long long ldv, const void *G, long long ldg, void *dQ, long long lddq, void *dK, long long lddk,
                                                 void *dV, long long lddv, int warmup, int iters, float *ms_out)
{
    spmv_attention_backward_call c = {.heads = 1, .kv_heads = 1, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv, .g = G, .ldg = ldg,
                                      .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv};
    return attention_backward_time(h, "time_attention_backward_launches", 0, &c, warmup, iters, ms_out);
}

int spmv_hip_attention_heads_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                      const void *Matrix_Val, int heads, int k, int dv, double scale,
                                      const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                      const void *G, long long ldg, void *dQ, long long lddq, void *dK, long long lddk, void *dV, long long lddv)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                      .g = G, .ldg = ldg, .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv};
    return attention_backward_call(handle, "attention_heads_backward", 0, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_heads_backward_launches(spmv_Handle_t h, int heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk,
                                                       const void *V, long long ldv, const void *G, long long ldg, void *dQ, long long lddq, void *dK, long long lddk,
                                                       void *dV, long long lddv, int warmup, int iters, float *ms_out)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                      .g = G, .ldg = ldg, .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv};
    return attention_backward_time(h, "time_attention_heads_backward_launches", 0, &c, warmup, iters, ms_out);
}

int spmv_hip_attention_bias_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                     const void *Matrix_Val, int heads, int k, int dv, double scale,
                                     const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                     const void *B, long long ldb, const void *G, long long ldg, void *dQ, long long lddq, void *dK, long long lddk,
                                     void *dV, long long lddv, void *dB, long long lddb)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                      .bias = B, .ldb = ldb, .g = G, .ldg = ldg, .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv, .db = dB, .lddb = lddb};
    return attention_backward_call(handle, "attention_bias_backward", 0, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_bias_backward_launches(spmv_Handle_t h, int heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                                      long long ldk, const void *V, long long ldv, const void *B, long long ldb, const void *G, long long ldg, void *dQ,
                                                      long long lddq, void *dK, long long lddk, void *dV, long long lddv, void *dB, long long lddb, int warmup, int iters,
                                                      float *ms_out)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                      .bias = B, .ldb = ldb, .g = G, .ldg = ldg, .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv, .db = dB, .lddb = lddb};
    return attention_backward_time(h, "time_attention_bias_backward_launches", 0, &c, warmup, iters, ms_out);
}

int spmv_hip_attention_gqa_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                    const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                                    const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                    const void *B, long long ldb, const void *G, long long ldg, void *dQ, long long lddq, void *dK, long long lddk,
                                    void *dV, long long lddv, void *dB, long long lddb)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                      .bias = B, .ldb = ldb, .g = G, .ldg = ldg, .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv, .db = dB, .lddb = lddb};
    return attention_backward_call(handle, "attention_gqa_backward", 0, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_gqa_backward_launches(spmv_Handle_t h, int heads, int kv_heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                                     long long ldk, const void *V, long long ldv, const void *B, long long ldb, const void *G, long long ldg, void *dQ,
                                                     long long lddq, void *dK, long long lddk, void *dV, long long lddv, void *dB, long long lddb, int warmup, int iters,
                                                     float *ms_out)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                      .bias = B, .ldb = ldb, .g = G, .ldg = ldg, .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv, .db = dB, .lddb = lddb};
    return attention_backward_time(h, "time_attention_gqa_backward_launches", 0, &c, warmup, iters, ms_out);
}

int spmv_hip_attention_gqa_backward_lse(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                        const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                                        const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                        const void *B, long long ldb, const void *G, long long ldg, const void *O, long long ldo, const void *L, long long ldl,
                                        void *dQ, long long lddq, void *dK, long long lddk, void *dV, long long lddv, void *dB, long long lddb)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                      .bias = B, .ldb = ldb, .g = G, .ldg = ldg, .stats = 1, .o = O, .ldo = ldo, .lse = L, .ldl = ldl,
                                      .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv, .db = dB, .lddb = lddb};
    return attention_backward_call(handle, "attention_gqa_backward_lse", 0, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_gqa_backward_lse_launches(spmv_Handle_t h, int heads, int kv_heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                                         long long ldk, const void *V, long long ldv, const void *B, long long ldb, const void *G, long long ldg, const void *O,
                                                         long long ldo, const void *L, long long ldl, void *dQ, long long lddq, void *dK, long long lddk, void *dV, long long lddv,
                                                         void *dB, long long lddb, int warmup, int iters, float *ms_out)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv,
                                      .bias = B, .ldb = ldb, .g = G, .ldg = ldg, .stats = 1, .o = O, .ldo = ldo, .lse = L, .ldl = ldl,
                                      .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv, .db = dB, .lddb = lddb};
    return attention_backward_time(h, "time_attention_gqa_backward_lse_launches", 0, &c, warmup, iters, ms_out);
}

/* O and L: both given, the row pass is driven by them; both NULL, it normalises by itself; one of the two while m > 0 is refused by the rules */
int spmv_hip_attention_gqa_backward_16(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                       const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale, int io_type,
                                       const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                       const void *B, long long ldb, const void *G, long long ldg, const void *O, long long ldo, const void *L, long long ldl,
                                       int dq_type, void *dQ, long long lddq, int dkv_type, void *dK, long long lddk, void *dV, long long lddv, void *dB, long long lddb)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .io_type = io_type, .dq_type = dq_type, .dkv_type = dkv_type,
                                      .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv, .bias = B, .ldb = ldb, .g = G, .ldg = ldg,
                                      .stats = O && L, .o = O, .ldo = ldo, .lse = L, .ldl = ldl,
                                      .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv, .db = dB, .lddb = lddb};
    return attention_backward_call(handle, "attention_gqa_backward_16", ATTENTION_16, &c, m, RowPtr, ColIdx, Matrix_Val);
}

double spmv_hip_time_attention_gqa_backward_16_launches(spmv_Handle_t h, int heads, int kv_heads, int k, int dv, double scale, int io_type, const void *Q, long long ldq,
                                                        const void *K, long long ldk, const void *V, long long ldv, const void *B, long long ldb, const void *G, long long ldg,
                                                        const void *O, long long ldo, const void *L, long long ldl, int dq_type, void *dQ, long long lddq, int dkv_type, void *dK,
                                                        long long lddk, void *dV, long long lddv, void *dB, long long lddb, int warmup, int iters, float *ms_out)
{
    spmv_attention_backward_call c = {.heads = heads, .kv_heads = kv_heads, .k = k, .dv = dv, .scale = scale, .io_type = io_type, .dq_type = dq_type, .dkv_type = dkv_type,
                                      .q = Q, .ldq = ldq, .kk = K, .ldk = ldk, .v = V, .ldv = ldv, .bias = B, .ldb = ldb, .g = G, .ldg = ldg,
                                      .stats = O && L, .o = O, .ldo = ldo, .lse = L, .ldl = ldl,
                                      .dq = dQ, .lddq = lddq, .dk = dK, .lddk = lddk, .dvo = dV, .lddv = lddv, .db = dB, .lddb = lddb};
    return attention_backward_time(h, "time_attention_gqa_backward_16_launches", ATTENTION_16, &c, warmup, iters, ms_out);
}

/* ---------------------------------------------------------------- the six solves on the device: one gate, one call struct
 * conjugate gradients, BiCGStab (a matrix that need not be symmetric), restarted GMRES, conjugate gradients for k right-hand sides,
 * mixed-precision conjugate gradients on a pair of handles and LSQR (a matrix that need not be square).  An entry point fills a spmv_solve_call and goes through solve_call or solve_time. */
typedef struct solve_csr { BASIC_INT_TYPE m; const BASIC_INT_TYPE *RowPtr, *ColIdx; const void *Val; } solve_csr; /* the CSR arguments of a solve that takes them */

static spmv_solve_call solve_fill(int solver, int k, int restart, const void *B, long long ldb, void *X, long long ldx, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    spmv_solve_call c = {.solver = solver, .k = k, .restart = restart, .b = B, .ldb = ldb, .x = X, .ldx = ldx, .res = res};
    if (opt) c.opt = *opt;
    return c;
}

/* Every argument rule, once, ahead of the gate (a refusal here is E_ARG whatever the handle's state); then the gate -- spmv_hip_cg_mixed: both
 * handles', addressed in the caller's order, and c->low filled; the prologue for a solve with the CSR arguments; the plain gate for a timer --
 * and what needs the state: the square matrix, and the columns of spmv_hip_cg_columns, which with one compact vector is spmv_hip_cg, its
 * workspace and bits.  given: opt and res are there.  m: the solve's; 1 for a timer (B and X are always needed); 0 for spmv_hip_cg_mixed, whose
 * m is the resident matrix's: the shim checks its B and X.  spmv_hip_lsqr: X has n elements, known behind the gate; the entries are addressed in the
 * caller's order (no reordered handle); the transpose is built at the first call and its values are A's as they are now (transpose_ready) */
static int solve_gate(const char *where, spmv_Handle_t h, spmv_Handle_t low, int given, spmv_solve_call *c, const solve_csr *csr, int m, spmv_hip_state **st)
{
    const int mixed = c->solver == SPMV_SHIM_SOLVE_CG_MIXED, lsqr = c->solver == SPMV_SHIM_SOLVE_LSQR, kmax = c->solver == SPMV_SHIM_SOLVE_CG_COLUMNS ? SPMV_HIP_CG_COLUMNS_MAX : 1;
    spmv_hip_state *lo = NULL;
    int rc;
    if (!h || (mixed && !low)) return refuse(SPMV_HIP_E_ARG, where, "handle is NULL");
    if (!given) return refuse(SPMV_HIP_E_ARG, where, "opt or res is NULL");
    if (m > 0 && (!c->b || (!lsqr && !c->x))) return refuse(SPMV_HIP_E_ARG, where, "B or X is NULL");
    if (c->opt.max_iterations < 0 || c->opt.check_every < 0) return refuse(SPMV_HIP_E_ARG, where, "need max_iterations >= 0 and check_every >= 0");
    if (!(c->opt.rtol >= 0) || !(c->opt.atol >= 0)) return refuse(SPMV_HIP_E_ARG, where, "rtol and atol must be >= 0 (and not NaN)");
    if (c->solver == SPMV_SHIM_SOLVE_GMRES && (c->restart < 1 || c->restart > SPMV_HIP_GMRES_RESTART_MAX))
        return refuse(SPMV_HIP_E_ARG, where, "need 1 <= restart <= SPMV_HIP_GMRES_RESTART_MAX");
    if (c->k < 1 || c->k > kmax || c->ldb < c->k || c->ldx < c->k) return refuse(SPMV_HIP_E_ARG, where, "need 1 <= k <= SPMV_HIP_CG_COLUMNS_MAX, ldb >= k and ldx >= k");
    if (!(c->update_drop >= 0) || !(c->update_drop < 1)) return refuse(SPMV_HIP_E_ARG, where, "need 0 <= update_drop < 1 (0: the default)");
    if (c->update_every < 0) return refuse(SPMV_HIP_E_ARG, where, "need update_every >= 0");
    if (lsqr) {
        if (!(c->ls_tol >= 0) || !(c->damp >= 0)) return refuse(SPMV_HIP_E_ARG, where, "ls_tol and damp must be >= 0 (and not NaN)");
        if ((rc = resident_state(h, where, RESIDENT_NOT_REORDERED, st))) return rc;
        if ((*st)->n > 0 && !c->x) return refuse(SPMV_HIP_E_ARG, where, "B or X is NULL");
        if (csr && (rc = resident_prologue(h, where, RESIDENT_NOT_REORDERED, csr->m, csr->RowPtr, csr->ColIdx, csr->Val, st))) return rc;
        return transpose_ready(h, *st, where);
    }
    if (mixed) {
        if ((rc = resident_state(h, where, RESIDENT_NOT_REORDERED, st)) || (rc = resident_state(low, where, RESIDENT_NOT_REORDERED, &lo))) return rc;
    } else if ((rc = csr ? resident_prologue(h, where, 0, csr->m, csr->RowPtr, csr->ColIdx, csr->Val, st) : resident_state(h, where, 0, st))) return rc;
    c->low = lo ? lo->dev : NULL;
    if ((*st)->m != (*st)->n) return refuse(SPMV_HIP_E_ARG, where, "the matrix is not square (m != n at create)");
    if (c->solver == SPMV_SHIM_SOLVE_CG_COLUMNS && c->k == 1 && c->ldb == 1 && c->ldx == 1) c->solver = SPMV_SHIM_SOLVE_CG;
    return c->solver == SPMV_SHIM_SOLVE_CG_COLUMNS ? spmm_columns(h, *st, where) : SPMV_HIP_OK;
}

static int solve_call(const char *where, spmv_Handle_t h, spmv_Handle_t low, int given, spmv_solve_call *c, const solve_csr *csr)
{
    spmv_hip_state *st;
    const int rc = solve_gate(where, h, low, given, c, csr, csr ? csr->m : 0, &st);
    return rc ? rc : report(spmv_shim_solve(st->dev, c), where);
}

static double solve_time(const char *where, spmv_Handle_t h, spmv_Handle_t low, int given, spmv_solve_call *c, int warmup, int iters, float *ms_out)
{
    spmv_hip_state *st;
    if (solve_gate(where, h, low, given, c, NULL, 1, &st)) return -1.0;
    return report_time(spmv_shim_time_solve(st->dev, c, warmup, iters, ms_out), where);
}

int spmv_hip_cg(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                const void *Matrix_Val, const void *B, void *X, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_CG, 1, 0, B, 1, X, 1, opt, res);
    return solve_call("cg", handle, NULL, opt && res, &c, &(solve_csr){m, RowPtr, ColIdx, Matrix_Val});
}

int spmv_hip_bicgstab(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                      const void *Matrix_Val, const void *B, void *X, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_BICGSTAB, 1, 0, B, 1, X, 1, opt, res);
    return solve_call("bicgstab", handle, NULL, opt && res, &c, &(solve_csr){m, RowPtr, ColIdx, Matrix_Val});
}

double spmv_hip_time_cg_iterations(spmv_Handle_t h, const void *B, void *X, const spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_CG, 1, 0, B, 1, X, 1, opt, NULL);
    return solve_time("time_cg_iterations", h, NULL, opt != NULL, &c, warmup, iters, ms_out);
}

double spmv_hip_time_bicgstab_iterations(spmv_Handle_t h, const void *B, void *X, const spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_BICGSTAB, 1, 0, B, 1, X, 1, opt, NULL);
    return solve_time("time_bicgstab_iterations", h, NULL, opt != NULL, &c, warmup, iters, ms_out);
}

int spmv_hip_gmres(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx, const void *Matrix_Val, const void *B, void *X, int restart,
                   const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_GMRES, 1, restart, B, 1, X, 1, opt, res);
    return solve_call("gmres", handle, NULL, opt && res, &c, &(solve_csr){m, RowPtr, ColIdx, Matrix_Val});
}

double spmv_hip_time_gmres_iterations(spmv_Handle_t h, const void *B, void *X, int restart, const spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_GMRES, 1, restart, B, 1, X, 1, opt, NULL);
    return solve_time("time_gmres_iterations", h, NULL, opt != NULL, &c, warmup, iters, ms_out);
}

int spmv_hip_gmres_device_sqrt(const double *in, double *out, long long n)
{
    return report(spmv_shim_gmres_sqrt(in, out, n), "gmres_device_sqrt");
}

int spmv_hip_cg_columns(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx, const void *Matrix_Val, int k, const void *B,
                        long long ldb, void *X, long long ldx, const spmv_hip_cg_options *opt, spmv_hip_cg_result *res)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_CG_COLUMNS, k, 0, B, ldb, X, ldx, opt, res);
    return solve_call("cg_columns", handle, NULL, opt && res, &c, &(solve_csr){m, RowPtr, ColIdx, Matrix_Val});
}

double spmv_hip_time_cg_columns_iterations(spmv_Handle_t h, int k, const void *B, long long ldb, void *X, long long ldx, const spmv_hip_cg_options *opt, int warmup, int iters,
                                           float *ms_out)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_CG_COLUMNS, k, 0, B, ldb, X, ldx, opt, NULL);
    return solve_time("time_cg_columns_iterations", h, NULL, opt != NULL, &c, warmup, iters, ms_out);
}

/* the mixed solve's options are a struct of their own: the common fields copied one by one; what a pair must share is the shim's to check */
static spmv_solve_call mixed_fill(const double *B, double *X, const spmv_hip_cg_mixed_options *opt, spmv_hip_cg_result *res, int *updates)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_CG_MIXED, 1, 0, B, 1, X, 1, NULL, res);
    c.updates = updates;
    if (!opt) return c;
    c.opt.rtol = opt->rtol;
    c.opt.atol = opt->atol;
    c.opt.max_iterations = opt->max_iterations;
    c.opt.check_every = opt->check_every;
    c.opt.use_x0 = opt->use_x0;
    c.opt.Dinv = opt->Dinv;
    c.opt.history = opt->history;
    c.update_drop = opt->update_drop;
    c.update_every = opt->update_every;
    return c;
}

int spmv_hip_cg_mixed(spmv_Handle_t high, spmv_Handle_t low, const double *B, double *X, const spmv_hip_cg_mixed_options *opt, spmv_hip_cg_mixed_result *res)
{
    spmv_hip_cg_result r = {0};
    int updates = 0;
    spmv_solve_call c = mixed_fill(B, X, opt, &r, &updates);
    const int rc = solve_call("cg_mixed", high, low, opt && res, &c, NULL);
    if (rc == SPMV_HIP_OK) *res = (spmv_hip_cg_mixed_result){.status = r.status, .iterations = r.iterations, .updates = updates, .rr = r.rr, .bb = r.bb};
    return rc;
}

double spmv_hip_time_cg_mixed_iterations(spmv_Handle_t high, spmv_Handle_t low, const double *B, double *X, const spmv_hip_cg_mixed_options *opt, int warmup, int iters,
                                         float *ms_out)
{
    spmv_solve_call c = mixed_fill(B, X, opt, NULL, NULL);
    return solve_time("time_cg_mixed_iterations", high, low, opt != NULL, &c, warmup, iters, ms_out);
}

/* LSQR's options and result are structs of their own: the common fields copied one by one; there is no Dinv */
static spmv_solve_call lsqr_fill(const void *B, void *X, const spmv_hip_lsqr_options *opt, spmv_hip_cg_result *res, double *ar, double *anorm)
{
    spmv_solve_call c = solve_fill(SPMV_SHIM_SOLVE_LSQR, 1, 0, B, 1, X, 1, NULL, res);
    c.ar = ar;
    c.anorm = anorm;
    if (!opt) return c;
    c.opt.rtol = opt->rtol;
    c.opt.atol = opt->atol;
    c.opt.max_iterations = opt->max_iterations;
    c.opt.check_every = opt->check_every;
    c.opt.use_x0 = opt->use_x0;
    c.opt.history = opt->history;
    c.ls_tol = opt->ls_tol;
    c.damp = opt->damp;
    return c;
}

int spmv_hip_lsqr(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx, const void *Matrix_Val, const void *B, void *X,
                  const spmv_hip_lsqr_options *opt, spmv_hip_lsqr_result *res)
{
    spmv_hip_cg_result r = {0};
    double ar = 0, anorm = 0;
    spmv_solve_call c = lsqr_fill(B, X, opt, &r, &ar, &anorm);
    const int rc = solve_call("lsqr", handle, NULL, opt && res, &c, &(solve_csr){m, RowPtr, ColIdx, Matrix_Val});
    if (rc == SPMV_HIP_OK) *res = (spmv_hip_lsqr_result){.status = r.status, .iterations = r.iterations, .rr = r.rr, .bb = r.bb, .ar = ar, .anorm = anorm};
    return rc;
}

double spmv_hip_time_lsqr_iterations(spmv_Handle_t h, const void *B, void *X, const spmv_hip_lsqr_options *opt, int warmup, int iters, float *ms_out)
{
    spmv_solve_call c = lsqr_fill(B, X, opt, NULL, NULL, NULL);
    return solve_time("time_lsqr_iterations", h, NULL, opt != NULL, &c, warmup, iters, ms_out);
}
