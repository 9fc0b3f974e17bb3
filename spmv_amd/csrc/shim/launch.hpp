// shim/launch.hpp -- part of the single translation unit spmv_shim.hip: the EXECUTORS' launchers (which
// kernel form, which template arguments, grid and LDS size per schedule), the create-time autotune of the
// CSR-vector forms, and launch<T>() = one y = A x on the handle's stream.
//
// The create-time choices.  Which form of a kernel is fastest differs between MI355X boxes by a few percent, so create() times the applicable
// ones once on the resident matrix and the handle launches the winner from then on.  autotune_vector, build_packed_values, autotune_blocked, autotune_rows
// and time_schedule are each a gate in front of ONE race, race_forms: it ends with no room for its scratch vectors (the default stays, nothing is wrong),
// failed (the choice goes back to the default) or timed.  What a form's code means, the candidates, the round counts, the 0.95 guard and what is done with
// the times are shim/tune.hpp: a table and pure functions that a host program runs without a device.  Option vector_form forces a form (tests, A/B runs).
#pragma once

// ------------------------------------------------------------------------------------ executors
// The launch of the CSR-vector family (kernels/csr_vector_tile.hpp) that a built CSR-vector or Balanced schedule makes: the one place that
// decides the kernel and its form (from tune.hpp's table).  launch(), the autotune, spmv_shim_release_columns and spmv_shim_info all read it.
static VecArgs vector_args(const spmv_dev *d)
{
    VecArgs a;
    const bool f64 = d->vsize == sizeof(double);
    if (d->plan.sched == SPMV_SCHED_ROWBLOCK || d->vt_wide) {
        // the rows kernel: Balanced's equal-nnz row blocks (split), or CSR-vector's wide form (uniform blocks).  Steps in flight: what option
        // vector_form names (5 / 12: two, 10 / 11: four), what create() measured (rows_depth, autotune_rows), else the dtype's default
        a.kernel = kVecRowsKernel;
        a.depth = rows_depth_of(d->plan.vector_form, d->rows_depth, f64);
        a.wide = d->vt_wide;
        a.split = d->plan.sched == SPMV_SCHED_ROWBLOCK ? d->rb_split : nullptr;
    } else {
        // tile kernel where most x tiles fit LDS or a tile form is named (unstaged tiles gather from L1/L2), else the pipe kernel
        const VecForm f = vector_form_of(d->plan.vector_form ? d->plan.vector_form : d->vec_choice, f64, d->vt_tiles > 0, d->vt_staged * 2 >= d->vt_tiles);
        if (f.tile) { a.kernel = kVecTileKernel; a.depth = f.depth; a.pre = f.pre; }
    }
    a.lanes = d->plan.lanes_per_row; a.m = d->m; a.long_thr = d->long_thr; a.tiles = d->vt_tiles; a.maxspan = d->vt_maxspan; a.rows = d->vt_rows;
    a.rowptr = d->rowptr; a.colidx = d->colidx; a.val = d->val; a.wins = d->vt_wins;
    a.col = d->vt_col; a.rowslot = d->vt_rowslot; a.tmpl = d->vt_tmpl; a.col8 = d->vt_col8; a.rowtid = d->vt_rowtid;
    a.device = d->device; a.stream = d->stream;
    if (d->pk_use && a.kernel == kVecTileKernel && a.depth != 8) { // packed planes: the same kernel, PACK flag (two or four steps in flight)
        a.pk_lo = d->pk_lo; a.pk_hi = d->pk_hi; a.pk_e = d->pk_e;
        if (d->pk_depth) a.depth = d->pk_depth;
    }
    return a;
}

// One CSR-vector-family launch as vector_args resolves it (spmv_vector.hip).
template <typename T>
static hipError_t launch_vector(const spmv_dev *d, const T *x, T *y)
{
    const VecArgs a = vector_args(d);
    return a.kernel == kVecRowsKernel ? rows_launch(a, x, y) : vector_launch(a, x, y);
}

// The race of every create-time choice: scratch x = 1 and y from the pool, two events, set(k); launch(x, y) once per candidate to warm it, then `rounds`
// interleaved rounds (one process, same clocks) of one launch per sample -- the forms differ by whole percents where they differ, events resolve a
// microsecond -- and tmin[k] = the minimum.  kRaceFailed: hipEventCreate or a launch returned an error (the race ends there), or the runtime holds one at the end.
enum RaceEnd { kRaceNoRoom, kRaceFailed, kRaceTimed };
template <typename T, class Set, class Launch>
static RaceEnd race_forms(spmv_dev *d, int ncand, int rounds, float *tmin, Set set, Launch launch)
{
    for (int k = 0; k < ncand; ++k) tmin[k] = kNotTimed;
    T *x = nullptr, *y = nullptr;
    if (pool_malloc((void **) &x, sizeof(T) * (size_t) (d->n > 0 ? d->n : 1)) != hipSuccess || pool_malloc((void **) &y, sizeof(T) * (size_t) (d->m > 0 ? d->m : 1)) != hipSuccess) {
        (void) hipGetLastError();
        if (x) (void) pool_free(x);
        return kRaceNoRoom;
    }
    fill_value_kernel<T><<<grid_for(d->n, kBlock, d->cus * 8), kBlock, 0, d->stream>>>(d->n, x, T(1));
    int rc = 0;
    {
        Events ev(2);
        rc = ev.ok ? 0 : 1;
        for (int k = 0; k < ncand && !rc; ++k) { set(k); rc = launch(x, y); } // warm every form once
        for (int round = 0; round < rounds && !rc; ++round)
            for (int k = 0; k < ncand && !rc; ++k) {
                set(k);
                (void) hipEventRecord(ev[0], d->stream);
                rc = launch(x, y);
                (void) hipEventRecord(ev[1], d->stream);
                (void) hipEventSynchronize(ev[1]);
                float ms = 0;
                (void) hipEventElapsedTime(&ms, ev[0], ev[1]);
                if (ms < tmin[k]) tmin[k] = ms;
            }
    }
    (void) pool_free(x);
    (void) pool_free(y);
    const bool clean = hipGetLastError() == hipSuccess;
    return rc || !clean ? kRaceFailed : kRaceTimed;
}

// Time the applicable CSR-vector forms on the resident matrix and keep the fastest (tune.hpp: vector_rule).
template <typename T>
static int autotune_vector(spmv_dev *d)
{
    d->vec_choice = VEC_AUTO;
    if (d->nnz < (1ll << 24) || d->plan.forced || d->vt_tiles <= 0) return SPMV_HIP_OK;
    if (d->vt_wide || d->vt_staged * 2 < d->vt_tiles) return SPMV_HIP_OK; // wide form: one kernel form; x windows not staged: the pipe form runs, nothing to choose (and 45 gather-bound launches would cost ~0.3 s)
    // (nearly) every tile staged: the pipe form (4-byte columns, gathers through L1 / L2) has nothing to win and is not timed -- on config 2 its nine
    // launches were a quarter of the inspector's 26 ms
    const int ncand = (long long) d->vt_staged * 100 >= (long long) d->vt_tiles * 99 ? kVectorCands - 1 : kVectorCands;
    float tmin[kVectorCands] = {};
    const RaceEnd end = race_forms<T>(d, ncand, kVectorRounds, tmin, [&](int k) { d->vec_choice = kVectorCand[k]; }, [&](const T *x, T *y) { return (int) launch_vector<T>(d, x, y); });
    d->vec_choice = VEC_AUTO;
    if (end == kRaceNoRoom) return SPMV_HIP_OK; // no room to tune: keep the default
    // the pipe form (int32 columns, global gathers) only on a clear win: a noisy sample -- e.g. another process on the device during create -- must not
    // cost 30 % on every later launch
    const int best = vector_rule(tmin, ncand, d->tune_ms);
    if (end == kRaceTimed) d->vec_choice = best;
    return SPMV_HIP_OK;
}

// PACKED tiles (option pack_values; kernels/csr_vector_tile.hpp): fp64 values of the narrow tile form streamed as 7 bytes from planes the library
// keeps beside val.  1: every qualifying tile is packed and the planes are used, no timing (tests, A/B).  2 (default): only where autotune_vector
// has just timed the plain forms and at least half of the tiles qualify (otherwise nothing is allocated); the packed kernel is timed at the
// winner's PRE setting with 4 and 2 steps in flight, interleaved with the plain winner, min of three, and stays only below 0.95 x the plain best --
// the guard the pipe form has in autotune_vector, for the same reason: a noisy sample must not decide.  A loser's planes are freed.
static void free_packed_values(spmv_dev *d)
{
    quiesce(d);
    for (void *p : {(void *) d->pk_lo, (void *) d->pk_hi, (void *) d->pk_e, (void *) d->pk_cnt}) if (p) sched_free(d, p);
    d->pk_lo = nullptr; d->pk_hi = nullptr; d->pk_e = nullptr; d->pk_cnt = nullptr;
    d->pk_tiles = d->pk_nnz = 0; d->pk_use = false; d->pk_depth = 0;
}

static int build_packed_values(spmv_dev *d)
{
    const int mode = d->plan.pack_values;
    d->pack_ms[0] = d->pack_ms[1] = 0;
    if (mode == 0 || d->vsize != sizeof(double) || d->plan.sched != SPMV_SCHED_CSR_VECTOR || d->vt_wide || d->vt_tiles <= 0 || d->nnz == 0) return SPMV_HIP_OK;
    const VecArgs plain = vector_args(d);
    if (plain.kernel != kVecTileKernel || plain.depth == 8) return SPMV_HIP_OK; // pipe form, or a forced form the packed kernel does not have
    const bool timed = d->vec_choice != VEC_AUTO; // autotune_vector ran (nnz >= 2^24, nothing forced)
    if (mode == 2 && !timed) return SPMV_HIP_OK;
    int rc = SPMV_HIP_OK;
    ALLOC_TRY(d, &d->pk_e, sizeof(int) * (size_t) d->vt_tiles, true);
    ALLOC_TRY(d, &d->pk_cnt, 2 * sizeof(unsigned long long), true);
    if (mode == 2) { // the gate alone first: nothing large is allocated for a matrix that does not qualify
        rc = pack_tiles_run(d, false);
        if (rc || d->pk_tiles * 2 < d->vt_tiles) { free_packed_values(d); return rc; }
    }
    // planes padded like val: a lane's tail read behind the last row stays inside
    if ((rc = dev_alloc(d, (void **) &d->pk_lo, sizeof(unsigned) * ((size_t) d->nnz + kStreamPad), true)) ||
        (rc = dev_alloc(d, (void **) &d->pk_hi, 3 * ((size_t) d->nnz + kStreamPad) + 4, true))) {
        (void) hipGetLastError();
        free_packed_values(d);
        return mode == 2 ? SPMV_HIP_OK : rc; // no room: the 8-byte stream stays
    }
    HIP_TRY(hipMemsetAsync(d->pk_lo + d->nnz, 0, sizeof(unsigned) * kStreamPad, d->stream));
    HIP_TRY(hipMemsetAsync(d->pk_hi + 3 * (size_t) d->nnz, 0, 3 * (size_t) kStreamPad + 4, d->stream));
    rc = pack_tiles_run(d, true);
    if (rc || d->pk_tiles == 0) { free_packed_values(d); return rc; }
    if (mode == 1) { d->pk_use = true; return SPMV_HIP_OK; }
    auto depth = [](int k) { return k > 0 ? vec_form(kPackedCand[k])->depth : 0; }; // candidate 0: the plain winner
    float tmin[kPackedCands];
    const RaceEnd end = race_forms<double>(d, kPackedCands, kPackedRounds, tmin, [&](int k) { d->pk_use = k > 0; d->pk_depth = depth(k); },
                                           [&](const double *x, double *y) { return (int) launch_vector<double>(d, x, y); });
    if (end == kRaceNoRoom) { free_packed_values(d); return SPMV_HIP_OK; } // no room to time: the 8-byte stream stays
    const int best = packed_rule(tmin, d->tune_ms, d->pack_ms);
    if (end != kRaceTimed || !best) { free_packed_values(d); return SPMV_HIP_OK; }
    d->pk_use = true;
    d->pk_depth = depth(best);
    return SPMV_HIP_OK;
}

// Row blocks x column slabs (kernels/blocked.hpp).  One-wave form: a single-wave workgroup per row block, two per CU; wide form
// (S.waves = 4 / 8): one workgroup of that many waves per block, one block per CU, the waves taking turns at adding (S.ordered) or
// not.  Forms = groups per pipeline step (S.form 0 / 1, chosen by autotune_blocked; option blk_groups forces one): 8 / 12 with one
// or four waves, 6 / 8 with eight (256 registers per wave).  All forms of one layout add the same products; the one-wave forms and
// the ordered wide forms each in a fixed order (tests compare their bits).
static void blocked_forms(const BlkSet &S, int un[2])
{
    un[0] = S.waves == 8 ? 6 : 8;
    un[1] = S.waves == 8 ? 8 : 12;
}

template <typename T>
static void launch_blocked(spmv_dev *d, const T *x, T *y)
{
    const BlkSet &S = d->blk;
    const size_t lds = blocked_lds_bytes(S);
#define SPMV_BLK_LAUNCH(UN, DBG)                                                                                                  \
    do {                                                                                                                          \
        ensure_lds<blk_kernel<T, UN, DBG>>(d->device, lds);                                                                       \
        blk_kernel<T, UN, DBG><<<S.B, kWave, lds, d->stream>>>(S.row0, S.R, S.dir, (const T *) S.val, S.meta, S.hdr, S.order, x, y, d->accumulate ? 1 : 0); \
    } while (0)
#define SPMV_BLK_WLAUNCH(UN, W, ORD)                                                                                              \
    do {                                                                                                                          \
        ensure_lds<blk_wide_kernel<T, UN, W, ORD>>(d->device, lds);                                                               \
        blk_wide_kernel<T, UN, W, ORD><<<S.B, kWave * W, lds, d->stream>>>(S.row0, S.R, S.dir, (const T *) S.val, S.meta, S.hdr, S.order, x, y, d->accumulate ? 1 : 0); \
    } while (0)
#define SPMV_BLK_WFORM(UN, W) do { if (S.ordered) SPMV_BLK_WLAUNCH(UN, W, true); else SPMV_BLK_WLAUNCH(UN, W, false); } while (0)
#ifdef SPMV_BLK_DEBUG_FORMS // A/B builds of tools/ only (wrong results): SPMV_HIP_BLK_DEBUG_FORM = 1 / 2 / 3 = no gathers / no LDS adds / neither, 8 groups per step
    static const int dbg_form = getenv("SPMV_HIP_BLK_DEBUG_FORM") ? atoi(getenv("SPMV_HIP_BLK_DEBUG_FORM")) : 0;
    if (dbg_form == 1) { SPMV_BLK_LAUNCH(8, 1); return; }
    if (dbg_form == 2) { SPMV_BLK_LAUNCH(8, 2); return; }
    if (dbg_form == 3) { SPMV_BLK_LAUNCH(8, 3); return; }
#endif
    int un[2];
    blocked_forms(S, un);
    const int form = S.form;
    const int g = d->plan.blk_groups > 0 ? d->plan.blk_groups : un[form];
    if (S.waves == 2) {
        if (g == 12) SPMV_BLK_WFORM(12, 2); else SPMV_BLK_WFORM(8, 2);
    } else if (S.waves == 4) {
        if (g == 12) SPMV_BLK_WFORM(12, 4); else if (g == 6) SPMV_BLK_WFORM(6, 4); else if (g == 4) SPMV_BLK_WFORM(4, 4); else SPMV_BLK_WFORM(8, 4);
    } else if (S.waves == 8) {
        if (g == 8) SPMV_BLK_WFORM(8, 8); else if (g == 4) SPMV_BLK_WFORM(4, 8); else SPMV_BLK_WFORM(6, 8);
    } else {
        if (g == 12) SPMV_BLK_LAUNCH(12, 0);
        else SPMV_BLK_LAUNCH(8, 0);
    }
#undef SPMV_BLK_WFORM
#undef SPMV_BLK_LAUNCH
#undef SPMV_BLK_WLAUNCH
}

// Time the executor forms on the resident streams (x = 1: the gather pattern does not depend on the values) and keep the faster.
template <typename T>
static int autotune_blocked(spmv_dev *d)
{
    d->blk.form = 0;
    d->blk.tune_ms[0] = d->blk.tune_ms[1] = d->blk.tune_ms[2] = 0;
    if (!d->blk_on || !d->plan.autotune || d->plan.blk_groups != 0) return SPMV_HIP_OK;
    float tmin[kBlockedForms];
    const RaceEnd end = race_forms<T>(d, kBlockedForms, kBlockedRounds, tmin, [&](int f) { d->blk.form = f; }, [&](const T *x, T *y) { launch_blocked<T>(d, x, y); return 0; });
    d->blk.form = 0;
    if (end == kRaceNoRoom) return SPMV_HIP_OK; // no room to tune: keep the default
    const int best = blocked_rule(tmin, d->blk.tune_ms);
    if (end == kRaceTimed) d->blk.form = best;
    return SPMV_HIP_OK;
}

// The rows kernel (Balanced's row blocks with `split`, CSR-vector's wide form without): two or four steps in flight?  Timed like the tile forms, on matrices of
// >= 2^24 entries whose blocks mostly stage (27-point stencil under Method_Balanced: 0.55 ms four deep, the fp64 default, 0.47 two deep).
template <typename T>
static int autotune_rows(spmv_dev *d)
{
    d->rows_depth = 0;
    if (d->nnz < (1ll << 24) || d->plan.forced || d->vt_tiles <= 0 || d->vt_staged * 2 < d->vt_tiles) return SPMV_HIP_OK;
    auto depth = [](int k) { return vec_form(kRowsCand[k])->depth; };
    float tmin[kRowsCands];
    const RaceEnd end = race_forms<T>(d, kRowsCands, kRowsRounds, tmin, [&](int k) { d->rows_depth = depth(k); }, [&](const T *x, T *y) { return (int) launch_vector<T>(d, x, y); });
    d->rows_depth = 0;
    if (end == kRaceNoRoom) return SPMV_HIP_OK;
    d->tune_ms[0] = tmin[0];
    d->tune_ms[1] = tmin[1];
    if (end == kRaceTimed) d->rows_depth = depth(rows_rule(tmin));
    return SPMV_HIP_OK;
}

// The staged CSR5 group kernel two tiles deep (csr5_group_pipe_kernel)?  When EVERY group is staged (the pipelined kernel has no
// global-column path) and the values are fp32: in fp64 the second register set costs a wave per SIMD and measured no gain (config 2
// under CSR5: 0.511 vs 0.515 ms).  Option csr5_two_deep 1 / 2: never / also for fp64 (A/B).
static bool csr5_two_deep(const spmv_dev *d, const Csr5Plan &P)
{
    if (P.natural || P.staged <= 0 || P.staged != P.groups || P.group_tiles > kCsr5PipeMaxGroupTiles || d->plan.csr5_two_deep == 1) return false;
    return d->vsize == sizeof(float) || d->plan.csr5_two_deep == 2;
}

// Dynamic LDS of one CSR5 / nnz-split launch: the x windows (when groups are staged) and, behind them, the waves' row maps.
// MAPPED (matrices with empty rows, long-row sub-matrices: P.row_map): every wave stages its tile's row map in LDS, behind the x
// windows in the dynamic segment.  A tile of long rows holds few row starts: kWave ints per wave then (csr5.hpp)
struct Csr5Lds {
    int rm_stride = 0;
    size_t x = 0, rm = 0;
};
static Csr5Lds csr5_lds(const Csr5Plan &P, size_t elem)
{
    Csr5Lds L;
    const int sigma = P.sigma == 4 || P.sigma == 8 ? P.sigma : 16;
    L.rm_stride = P.row_map ? (P.max_tile_rows < kWave ? kWave : (sigma + 1) * kWave) : 0;
    L.rm = (size_t) (kBlock / kWave) * L.rm_stride * sizeof(int);
    L.x = P.staged > 0 ? xwin_lds_bytes(P.maxspan, elem) : 0; // + the zero slot
    return L;
}

// Dynamic LDS of the staged SELL launch: the group's x windows + the zero slot (*xbytes_out), then the group's row sums
static size_t sell_lds_bytes(const spmv_dev *d, size_t *xbytes_out)
{
    const int cpw = d->sell_group * (d->plan.sell_sigma / kSellC);
    const size_t xbytes = xwin_lds_bytes(d->sell_maxspan, d->vsize);
    if (xbytes_out) *xbytes_out = xbytes;
    return xbytes + d->vsize * (size_t) cpw * kSellC;
}

template <typename T, int SIGMA, bool MAPPED>
static void launch_csr5_form(spmv_dev *d, const Csr5Plan &P, const T *x, T *y)
{
    const Csr5Lds L = csr5_lds(P, sizeof(T));
    const int rm_stride = L.rm_stride;
    const size_t rmb = L.rm;
    if (P.staged > 0) { // the inspector staged (at least half of) the groups: their column stream is the 16-bit slot array
        const size_t lds = L.x;
        if (P.natural) {
            // the waves' tile buffers are static LDS next to the x windows: if the full-size buffers would leave
            // one workgroup per CU, hand the tiles over in two halves (half the buffers)
            constexpr size_t full = (size_t) (kBlock / kWave) * NatLds<T, SIGMA, false>::kBytes;
            const bool half = lds + rmb + full > 76 * 1024; // two workgroups no longer fit a CU's 160 KiB
            if (half) {
                ensure_lds<nat_group_kernel<T, SIGMA, MAPPED, true>>(d->device, lds + rmb, (size_t) (kBlock / kWave) * NatLds<T, SIGMA, true>::kBytes);
                nat_group_kernel<T, SIGMA, MAPPED, true><<<P.groups, kBlock, lds + rmb, d->stream>>>(P.group_tiles, P.tiles, (int) P.nnz, P.tile_ptr, P.desc, P.col, P.col16,
                                                                                                    (const T *) P.val, P.row_map, P.wins, x, y, (T *) P.carry, P.n_empty, P.empty_list,
                                                                                                    (int) lds, rm_stride);
            } else {
                ensure_lds<nat_group_kernel<T, SIGMA, MAPPED, false>>(d->device, lds + rmb, full);
                nat_group_kernel<T, SIGMA, MAPPED, false><<<P.groups, kBlock, lds + rmb, d->stream>>>(P.group_tiles, P.tiles, (int) P.nnz, P.tile_ptr, P.desc, P.col, P.col16,
                                                                                                     (const T *) P.val, P.row_map, P.wins, x, y, (T *) P.carry, P.n_empty, P.empty_list,
                                                                                                     (int) lds, rm_stride);
            }
            return;
        }
        if (csr5_two_deep(d, P)) {
            ensure_lds<csr5_group_pipe_kernel<T, SIGMA, MAPPED>>(d->device, lds + rmb);
            csr5_group_pipe_kernel<T, SIGMA, MAPPED><<<P.groups, kBlock, lds + rmb, d->stream>>>(P.group_tiles, P.tiles, P.tile_ptr, P.desc, P.col16, (const T *) P.val, P.row_map, P.wins, P.lane_run,
                                                                                                x, y, (T *) P.carry, P.n_empty, P.empty_list, (int) lds, rm_stride);
            return;
        }
        ensure_lds<csr5_group_kernel<T, SIGMA, MAPPED>>(d->device, lds + rmb);
        csr5_group_kernel<T, SIGMA, MAPPED><<<P.groups, kBlock, lds + rmb, d->stream>>>(P.group_tiles, P.tiles, P.tile_ptr, P.desc, P.col, P.col16, (const T *) P.val, P.row_map, P.wins, P.lane_run,
                                                                                       x, y, (T *) P.carry, P.n_empty, P.empty_list, (int) lds, rm_stride);
        return;
    }
    const int grid = grid_for(P.tiles, kBlock / kWave, INT_MAX);
    const int xcd = d->plan.xcd_order ? 1 : 0; // XCD-aware block order (common.hpp: xcd_block); option xcd_order = 0: dispatch order, for A/B
    if (P.natural && P.forward) {
        const int long_blocks = (P.n_long + 7) & ~7;
        nat_kernel<T, SIGMA, MAPPED, true><<<grid + long_blocks, kBlock, rmb, d->stream>>>(P.tiles, (int) P.nnz, P.tile_ptr, P.desc, P.col, (const T *) P.val, P.row_map, x, y, (T *) P.carry,
                                                                                          P.n_empty, P.empty_list, rm_stride, xcd, P.fwd, P.long_list, P.n_long, long_blocks);
    } else if (P.natural)
        nat_kernel<T, SIGMA, MAPPED><<<grid, kBlock, rmb, d->stream>>>(P.tiles, (int) P.nnz, P.tile_ptr, P.desc, P.col, (const T *) P.val, P.row_map, x, y, (T *) P.carry, P.n_empty,
                                                                      P.empty_list, rm_stride, xcd);
    else
        csr5_kernel<T, SIGMA, MAPPED><<<grid, kBlock, rmb, d->stream>>>(P.tiles, P.tile_ptr, P.desc, P.col, (const T *) P.val, P.row_map, x, y, (T *) P.carry, P.n_empty, P.empty_list,
                                                                       rm_stride, xcd);
}

template <typename T, int SIGMA>
static void launch_csr5_sigma(spmv_dev *d, const Csr5Plan &P, const T *x, T *y)
{
    if (P.row_map) launch_csr5_form<T, SIGMA, true>(d, P, x, y);
    else launch_csr5_form<T, SIGMA, false>(d, P, x, y);
}

// One CSR5 multiply: [y = 0 for the rows outside the plan] + tiles + carry fix-up.
template <typename T>
static int launch_csr5(spmv_dev *d, const Csr5Plan &P, const T *x, T *y)
{
    if (P.nnz == 0) return SPMV_HIP_OK;
    switch (P.sigma) {
    case 4: launch_csr5_sigma<T, 4>(d, P, x, y); break;
    case 8: launch_csr5_sigma<T, 8>(d, P, x, y); break;
    default: launch_csr5_sigma<T, 16>(d, P, x, y); break;
    }
    if (P.fixup && P.tiles > 1 && !P.forward) {
        const int g = grid_for(P.tiles - 1, kBlock, INT_MAX);
        if (P.row_map) csr5_fixup_kernel<T, true><<<g, kBlock, 0, d->stream>>>(P.tiles, P.tile_ptr, P.run_len, P.row_map, (const T *) P.carry, y);
        else csr5_fixup_kernel<T, false><<<g, kBlock, 0, d->stream>>>(P.tiles, P.tile_ptr, P.run_len, nullptr, (const T *) P.carry, y);
    }
    return SPMV_HIP_OK;
}

template <typename T>
static int launch(spmv_dev *d, const T *x, T *y)
{
    if (d->m == 0) return SPMV_HIP_OK;
    if (d->sp_near && d->sp_far) { // A = A_near + A_far (shim/split.hpp): the tile schedule writes every row, the blocked executor adds its part
        d->sp_near->stream = d->sp_far->stream = d->stream;
        const int rc = launch<T>(d->sp_near, x, y);
        return rc ? rc : launch<T>(d->sp_far, x, y);
    }
    if (d->nnz == 0) { // nothing to multiply: y = 0 (the far half of a split: y += 0)
        if (d->accumulate) return SPMV_HIP_OK;
        fill_zero_kernel<T><<<grid_for(d->m, kBlock, d->cus * 8), kBlock, 0, d->stream>>>(d->m, y);
        HIP_TRY(hipGetLastError());
        return SPMV_HIP_OK;
    }
    // y += A x exists in the blocked executor only: a far half that ever ended on another executor would overwrite A_near x
    if (d->accumulate && !d->blk_on) return fail(SPMV_HIP_E_RUNTIME, "internal: the accumulating half of a split matrix has no blocked executor");
    const T *val = (const T *) d->val;
    switch (d->plan.sched) {
    case SPMV_SCHED_CSR_SCALAR:
        csr_scalar_kernel<T><<<grid_for(d->m, kBlock, d->cus * 8), kBlock, 0, d->stream>>>(d->m, d->rowptr, d->colidx, val, x, y);
        break;
    case SPMV_SCHED_CSR_VECTOR:
        if (d->blk_on) { launch_blocked<T>(d, x, y); break; } // no x window could be staged (option "cache_block")
        HIP_TRY(launch_vector<T>(d, x, y)); // the tile or pipe kernel; wide x windows: the rows kernel over uniform 1024-row blocks, slot-index stream
        launch_long_rows<T>(d, x, y);
        break;
    case SPMV_SCHED_NNZ_SPLIT: {
        if (d->blk_on) { launch_blocked<T>(d, x, y); break; }
        const int rc = launch_csr5<T>(d, d->ns, x, y);
        if (rc) return rc;
        break;
    }
    case SPMV_SCHED_ROWBLOCK:
        if (d->blk_on) { launch_blocked<T>(d, x, y); break; }
        HIP_TRY(launch_vector<T>(d, x, y)); // the rows kernel over the equal-nnz row blocks
        launch_long_rows<T>(d, x, y);
        break;
    case SPMV_SCHED_SELL:
        if (d->blk_on) { launch_blocked<T>(d, x, y); break; }
        // staged path when at least half of the windows fit their x span in LDS; the LDS request is
        // sized by the largest staged span actually present (rounded to 16 KiB) to keep occupancy
        if (d->sell_staged > 0) {
            const int cpw = d->sell_group * (d->plan.sell_sigma / kSellC);
            size_t xbytes = 0;
            const size_t lds = sell_lds_bytes(d, &xbytes);
            ensure_lds<sell_window_kernel<T>>(d->device, lds);
            sell_window_kernel<T><<<d->sell_nwin, kSellWinThreads, lds, d->stream>>>(cpw, (long long) d->nchunks, d->m, d->chunk_ptr, d->scol, d->scol16, (const T *) d->sval,
                                                                                     d->perm, d->sell_wins, d->sell_run, d->sell_tmpl, d->scol8, x, y, (int) xbytes);
        }
        else
            sell_kernel<T><<<grid_for(d->nchunks, kBlock / kWave, INT_MAX), kBlock, 0, d->stream>>>(
                d->nchunks, d->chunk_ptr, d->scol, (const T *) d->sval, d->perm, x, y);
        launch_long_rows<T>(d, x, y);
        break;
    case SPMV_SCHED_CSR5: {
        if (d->blk_on) { launch_blocked<T>(d, x, y); break; }
        const int rc = launch_csr5<T>(d, d->c5, x, y);
        if (rc) return rc;
        break;
    }
    default: return fail(SPMV_HIP_E_ARG, "schedule %d has no executor", d->plan.sched);
    }
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

// min over `iters` launches of the schedule as built, on scratch vectors (x = 1), in ms; < 0 if it cannot be timed
template <typename T>
static double time_schedule(spmv_dev *d, int iters)
{
    float best;
    const RaceEnd end = race_forms<T>(d, 1, iters, &best, [](int) {}, [&](const T *x, T *y) { return launch<T>(d, x, y); });
    return end == kRaceTimed ? (double) best : -1.0;
}
