// xwindows_inspect.hpp -- the inspector kernels of the x windows (xwindows.hpp), launched by the shim's inspectors
// (shim/inspect.hpp).  Kept apart from the executors' headers so that the units that only launch executors
// (spmv_vector.hip) do not carry them.
#pragma once
#include "csr_vector_tile.hpp"

namespace spmv {

// Inspector: windows of one row tile + the tile-local 16-bit column stream (written for staged tiles
// only; unstaged tiles and long rows are computed from the original ColIdx).
static __global__ __launch_bounds__(kBlock) void csr_tile_windows_kernel(int m, int n, int rows_per_tile, int long_thr, int max_cols, int slot_bytes,
                                                                  const int *__restrict__ split,
                                                                  const int *__restrict__ rowptr,
                                                                  const int *__restrict__ colidx,
                                                                  TileWindows *__restrict__ wins,
                                                                  unsigned short *__restrict__ col_local,
                                                                  unsigned short *__restrict__ row_slot /* NULL: no run tiles */,
                                                                  unsigned char *__restrict__ col8 /* NULL: no byte tiles */,
                                                                  unsigned short *__restrict__ tmpl /* NULL: no template tiles; else kTmplCount lists of kTmplMax offsets per tile */,
                                                                  unsigned char *__restrict__ row_tid /* template tiles: the list number of every row */,
                                                                  int *__restrict__ staged /* [0] tiles staged, [1] max total, [2] run tiles, [3] their entries, [4] their rows, [5] byte tiles, [6] their entries, [7] their rows,
                                                                                              [8] template tiles, [9] their entries, [10] their rows */)
{
    long long r0, r1;
    tile_rows(blockIdx.x, m, rows_per_tile, split, r0, r1);
    const int sub = threadIdx.x / 16, l = threadIdx.x % 16; // 16 lanes sweep a row
    auto loop = [&](auto body) {
        for (long long r = r0 + sub; r < r1; r += kBlock / 16) {
            const int p0 = rowptr[r], p1 = rowptr[r + 1];
            if (p1 - p0 > long_thr) continue; // long rows are computed elsewhere, from the original ColIdx
            for (int p = p0 + l; p < p1; p += 16) body(colidx[p], (long long) p);
        }
    };
    auto store = [&](long long pos, int slot, int) { col_local[pos] = (unsigned short) (slot * slot_bytes); };
    build_windows(n, max_cols, loop, store, wins[blockIdx.x], staged, true);
    if (!row_slot) return;
    // RUN tile?  every (non-long) row one run of consecutive columns: then row_slot[r] = slot of the row's first column, in the column
    // stream's unit, and the executor never reads col_local for this tile
    __syncthreads(); // wins[blockIdx.x] as written by thread 0
    const TileWindows &tw = wins[blockIdx.x];
    const int nwin = tw.nwin;
    int ok = nwin > 0, entries = 0;
    if (nwin > 0)
        for (long long r = r0 + sub; r < r1; r += kBlock / 16) {
            const int p0 = rowptr[r], p1 = rowptr[r + 1];
            if (p1 - p0 > long_thr || p1 == p0) continue;
            const int c0 = colidx[p0];
            for (int p = p0 + l; p < p1; p += 16) ok &= colidx[p] == c0 + (p - p0);
            if (l == 0) entries += p1 - p0;
        }
    ok = __syncthreads_and(ok);
    if (!ok) {
        // BYTE tile?  Every (non-long) row's slots lie within 255 slots of the row's smallest one -- banded matrices with holes, block rows,
        // anything whose rows span under 256 columns inside one window: the column stream is then ONE byte per entry (the slot's distance from
        // the row's smallest slot, col8) + 16 bits per row (that smallest slot, row_slot) instead of 16 bits per entry.  Every thread re-reads
        // the 16-bit slots it stored itself (build_windows ran the same loop), so no fence is needed in front of this.
        // TEMPLATE tile?  The tile's (non-long, non-empty) rows use at most kTmplCount different lists of slot offsets from their first entry (each of
        // at most kTmplMax entries) -- the interior of any stencil (a 27-point row: three windows, nine runs of three, the same 27 offsets in every
        // row) plus the few other lists of the rows at the grid's edges, block rows, anything assembled from a few element patterns.  Like a RUN tile
        // it reads no column stream at all: 16 bits (row_slot: the slot of the row's first entry) + 8 bits (row_tid: which list) per ROW and the
        // lists once per tile (tmpl); the slot of a row's k-th entry is row_slot + list[k].  RUN = the one list 0, 1, 2, ...
        if (tmpl && nwin > 0 && r1 - r0 <= kTmplRows) {
            __shared__ unsigned s_hash[kTmplCount];
            __shared__ int s_tlen[kTmplCount], s_first[kTmplCount], s_tm[kTmplCount][kTmplMax];
            __shared__ unsigned char s_ids[kTmplRows];
            for (int i = threadIdx.x; i < kTmplCount * kTmplMax; i += kBlock) s_tm[i / kTmplMax][i % kTmplMax] = 0;
            if (threadIdx.x < kTmplCount) { s_hash[threadIdx.x] = 0u; s_tlen[threadIdx.x] = 0; s_first[threadIdx.x] = INT_MAX; }
            __syncthreads();
            int okt = 1, nt = 0;
            auto on_row = [&](int len) { return len > 0 && len <= long_thr; };
            // A: every row hashes its list (length and offsets) and claims or finds one of the kTmplCount list numbers
            for (long long r = r0 + sub; r < r1; r += kBlock / 16) {
                const int p0 = rowptr[r], len = rowptr[r + 1] - p0;
                int id = 0;
                if (on_row(len)) {
                    if (len > kTmplMax) okt = 0;
                    else {
                        const int s0 = col_local[p0];
                        unsigned h = 0x9E3779B9u * (unsigned) len;
                        for (int k = l; k < len; k += 16) {
                            const int dlt = (int) col_local[p0 + k] - s0;
                            okt &= dlt >= 0;
                            h += ((unsigned) dlt + 0x7F4A7C15u) * (2u * (unsigned) k + 1u) * 0x85EBCA6Bu;
                        }
#pragma unroll
                        for (int o = 8; o > 0; o >>= 1) h += __shfl_xor(h, o, 16);
                        h |= 1u; // 0 = a free list number
                        id = -1;
                        if (l == 0)
                            for (int i = 0; i < kTmplCount && id < 0; ++i) {
                                const unsigned old = atomicCAS(&s_hash[i], 0u, h);
                                if (old == 0u || old == h) id = i;
                            }
                        id = __shfl(id, 0, 16);
                        if (id < 0) { okt = 0; id = 0; } // more than kTmplCount different lists in this tile
                    }
                    if (l == 0) nt += len;
                }
                if (l == 0) s_ids[r - r0] = (unsigned char) id;
            }
            __syncthreads();
            // B, C: list i is written by the FIRST row (in row order) that carries it
            for (long long r = r0 + sub; r < r1; r += kBlock / 16) {
                const int len = rowptr[r + 1] - rowptr[r];
                if (l == 0 && on_row(len) && len <= kTmplMax) atomicMin(&s_first[s_ids[r - r0]], (int) (r - r0));
            }
            __syncthreads();
            for (long long r = r0 + sub; r < r1; r += kBlock / 16) {
                const int p0 = rowptr[r], len = rowptr[r + 1] - p0;
                if (!on_row(len) || len > kTmplMax) continue;
                const int id = s_ids[r - r0];
                if (s_first[id] == (int) (r - r0)) {
                    const int s0 = col_local[p0];
                    for (int k = l; k < len; k += 16) s_tm[id][k] = (int) col_local[p0 + k] - s0;
                    if (l == 0) s_tlen[id] = len;
                }
            }
            __syncthreads();
            // D: every row against its list (a hash is not a proof)
            for (long long r = r0 + sub; r < r1; r += kBlock / 16) {
                const int p0 = rowptr[r], len = rowptr[r + 1] - p0;
                if (!on_row(len) || len > kTmplMax) continue;
                const int id = s_ids[r - r0], s0 = col_local[p0];
                okt &= s_tlen[id] == len;
                for (int k = l; k < len; k += 16) okt &= (int) col_local[p0 + k] - s0 == s_tm[id][k];
            }
            okt = __syncthreads_and(okt);
            if (okt) {
                for (long long r = r0 + sub * 16 + l; r < r1; r += kBlock) { // one thread per row
                    const int p0 = rowptr[r], len = rowptr[r + 1] - p0;
                    row_slot[r] = (unsigned short) (on_row(len) ? col_local[p0] : 0);
                    row_tid[r] = on_row(len) ? s_ids[r - r0] : (unsigned char) 0;
                }
                for (int i = threadIdx.x; i < kTmplCount * kTmplMax; i += kBlock)
                    tmpl[(size_t) blockIdx.x * (kTmplCount * kTmplMax) + i] = (unsigned short) s_tm[i / kTmplMax][i % kTmplMax];
#pragma unroll
                for (int o = kWave / 2; o > 0; o >>= 1) nt += __shfl_xor(nt, o, kWave);
                if ((threadIdx.x & (kWave - 1)) == 0 && nt) atomicAdd(staged + 9, nt);
                if (threadIdx.x == 0) {
                    wins[blockIdx.x].runs = 3;
                    atomicAdd(staged + 8, 1);
                    atomicAdd(staged + 10, (int) (r1 - r0));
                }
                return;
            }
        }
        if (!col8 || nwin == 0) return;
        int okb = 1, nb = 0;
        for (long long r = r0 + sub; r < r1; r += kBlock / 16) {
            const int p0 = rowptr[r], p1 = rowptr[r + 1];
            if (p1 - p0 > long_thr || p1 == p0) continue;
            int mn = INT_MAX, mx = 0;
            for (int p = p0 + l; p < p1; p += 16) { const int sl = col_local[p]; mn = sl < mn ? sl : mn; mx = sl > mx ? sl : mx; }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) { mn = min(mn, __shfl_xor(mn, o, 16)); mx = max(mx, __shfl_xor(mx, o, 16)); }
            okb &= mx - mn <= 255 * slot_bytes;
            if (l == 0) nb += p1 - p0;
        }
        okb = __syncthreads_and(okb);
        if (!okb) return;
        for (long long r = r0 + sub; r < r1; r += kBlock / 16) {
            const int p0 = rowptr[r], p1 = rowptr[r + 1];
            int mn = INT_MAX;
            const bool on = p1 - p0 <= long_thr && p1 > p0;
            if (on) for (int p = p0 + l; p < p1; p += 16) { const int sl = col_local[p]; mn = sl < mn ? sl : mn; }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 16));
            if (on) for (int p = p0 + l; p < p1; p += 16) col8[p] = (unsigned char) ((col_local[p] - mn) / slot_bytes);
            if (l == 0) row_slot[r] = (unsigned short) (on ? mn : 0);
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) nb += __shfl_xor(nb, o, kWave);
        if ((threadIdx.x & (kWave - 1)) == 0 && nb) atomicAdd(staged + 6, nb);
        if (threadIdx.x == 0) {
            wins[blockIdx.x].runs = 2;
            atomicAdd(staged + 5, 1);
            atomicAdd(staged + 7, (int) (r1 - r0));
        }
        return;
    }
    for (long long r = r0 + sub * 16 + l; r < r1; r += kBlock) { // one thread per row now
        const int p0 = rowptr[r], p1 = rowptr[r + 1];
        int slot = 0;
        if (p1 > p0 && p1 - p0 <= long_thr) {
            const int c0 = colidx[p0];
            int w = 0;
            for (int k = 1; k < nwin; ++k) w = c0 >= tw.start[k] ? k : w;
            slot = (tw.base[w] + (c0 - tw.start[w])) * slot_bytes; // the whole run lies in window w: windows are maximal runs of touched 64-column segments
        }
        row_slot[r] = (unsigned short) slot;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) entries += __shfl_xor(entries, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && entries) atomicAdd(staged + 3, entries);
    if (threadIdx.x == 0) {
        wins[blockIdx.x].runs = 1;
        atomicAdd(staged + 2, 1);
        atomicAdd(staged + 4, (int) (r1 - r0));
    }
}

// Inspector for tiles that are CONTIGUOUS RANGES of a private column array (CSR5 tile groups,
// nnz-split tile groups, SELL sigma windows): group g covers cols[b, e) with
// b = bounds ? bounds[g * bstride] * scale : g * group_len,  e likewise (clipped to total).
// cols16 == NULL: in place (cols then holds int32 slots for staged groups).  Else cols is left
// alone (unstaged groups keep reading global columns from it) and the staged groups' slots go to the
// 16-bit stream cols16, padding entries to the zero slot; pack16 = 0: same positions, pack16 =
// sigma (CSR5): position t*64*sigma + i*64 + lane -> t*64*sigma + (i/4)*256 + lane*4 + i%4, so a
// lane fetches four slots with one 8-byte load.
static __global__ __launch_bounds__(kBlock) void range_windows_kernel(long long total, long long group_len,
                                                               const long long *__restrict__ bounds, int bstride, int scale,
                                                               long long nbounds /* bounds has nbounds + 1 entries */,
                                                               int n, int max_cols, int *__restrict__ cols,
                                                               unsigned short *__restrict__ cols16, int pack16,
                                                               TileWindows *__restrict__ wins, int *__restrict__ staged, int rewrite)
{
    long long b, e;
    if (bounds) {
        long long i0 = (long long) blockIdx.x * bstride, i1 = i0 + bstride;
        if (i0 > nbounds) i0 = nbounds;
        if (i1 > nbounds) i1 = nbounds;
        b = bounds[i0] * scale;
        e = bounds[i1] * scale;
    }
    else { b = (long long) blockIdx.x * group_len; e = b + group_len; }
    if (e > total) e = total;
    auto loop = [&](auto body) {
        for (long long i = b + threadIdx.x; i < e; i += kBlock) body(cols[i], i);
    };
    auto store = [&](long long pos, int slot, int tile_total) {
        if (!cols16) { if (slot >= 0) cols[pos] = slot; return; }
        long long q = pos;
        if (pack16) {
            const long long tn = (long long) kWave * pack16, t = pos / tn;
            const int o = (int) (pos - t * tn), i = o / kWave, lane = o % kWave;
            q = t * tn + (i / 4) * (4 * kWave) + lane * 4 + (i % 4);
        }
        cols16[q] = (unsigned short) (slot >= 0 ? slot : tile_total);
    };
    build_windows(n, max_cols, loop, store, wins[blockIdx.x], staged, rewrite != 0);
}

// sum of TileWindows::total over `count` tiles: the x elements one launch stages (traffic model, spmv_hip_info.stream_bytes)
static __global__ __launch_bounds__(kBlock) void wins_total_kernel(int count, const TileWindows *__restrict__ wins, unsigned long long *__restrict__ sum,
                                                            unsigned long long *__restrict__ staged_tiles)
{
    unsigned long long t = 0, c = 0;
    for (long long i = (long long) blockIdx.x * kBlock + threadIdx.x; i < count; i += (long long) gridDim.x * kBlock)
        if (wins[i].nwin > 0) { t += (unsigned long long) wins[i].total; c += 1; }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) { t += __shfl_xor(t, o, kWave); c += __shfl_xor(c, o, kWave); }
    if ((threadIdx.x & (kWave - 1)) == 0 && c) { atomicAdd(sum, t); atomicAdd(staged_tiles, c); }
}

} // namespace spmv
