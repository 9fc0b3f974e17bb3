// csr_vector_tile.hpp -- CSR-vector over row tiles with LDS-staged x windows.
//
// Same schedule as csr_vector_pipe_kernel (L lanes per row over plain CSR; reference:
// parallel_spmv.c:12-18 + inner_spmv.h:232-286), organised like the tile kernels that measured
// best on this chip:
//   - a 256-thread workgroup owns a tile of consecutive rows (256 for Method_Parallel, one
//     equal-nnz row block for Method_Balanced), a wave 64 of them at a time (L steps of 64/L rows);
//   - the 65 RowPtr values a wave needs are read by ONE coalesced load and handed to the lane
//     groups through LDS (no per-row dependent RowPtr load in front of the matrix stream);
//   - x WINDOWS (north_star: "LDS staging of x-vector tiles"): the inspector
//     (csr_tile_windows_kernel, xwindows_inspect.hpp) finds, per tile, up to 16 column windows that cover every column
//     its rows reference -- one window when the plain span [min, max] fits the LDS budget (banded
//     matrices), several when the columns sit in a few far-apart bands (3-D stencils: 9 windows of
//     ~260 columns for a 27-point stencil) -- and writes a tile-local copy of ColIdx in which each
//     entry already IS the LDS slot of its column, stored in 16 BITS (a slot is < 48 KiB / sizeof(T)):
//     the staged tiles' column stream is 2 B/nnz instead of ColIdx's 4 B/nnz, i.e. 10 instead of
//     12 B/nnz for fp64.  The executor stages the windows once per tile (coalesced) and every
//     gather is xs[slot], with no index arithmetic at all.  Tiles whose columns do not fit read
//     the original ColIdx and gather from L1/L2;
//   - RUN tiles: a staged tile whose rows each reference ONE run of consecutive columns (banded matrices, 1-D stencils, dense row
//     blocks: col[p] = col[p0] + p - p0) needs no column stream at all: the LDS slot of a row's first column (16 bits per ROW,
//     row_slot) + the entry's position in the row IS the slot.  fp64: 8 B/nnz + 2 B/row instead of 10 B/nnz -- BASELINE config 2's
//     banded matrix streams 2.8 instead of 3.4 GB per multiply.  Same products, same order of additions: the same bits;
//   - matrix stream: 16 B lane loads, DEPTH steps in flight per wave;
//   - the 64 row sums of a wave are collected through LDS and written by ONE coalesced store.
// Rows longer than long_thr are left to the long-row path (a CSR5 plan over their sub-matrix, long_rows.hpp) and
// are excluded from the windows.
// Extra HBM held: col_local uint16[nnz] (read INSTEAD of ColIdx for staged tiles) and 200 B of window
// table per tile.
#pragma once
#include <climits>
#include <type_traits>
#include "common.hpp"
#include "csr_vector4.hpp"
#include "xwindows.hpp"

namespace spmv {

constexpr int kVecTileThreads = 256;           // 4 wavefronts per workgroup (512 measured no better)
constexpr int kVecTileRows = kVecTileThreads;  // rows per workgroup slab (64 per wave)
constexpr int kTmplMax = 64;                   // TEMPLATE tiles: most entries of a row (a power of two: positions are masked with kTmplMax - 1),
constexpr int kTmplCount = 8;                  // ... different offset lists per tile,
constexpr int kTmplRows = 1024;                // ... rows of a tile (the wide form's blocks; Balanced's equal-nnz blocks may hold more: those keep their stream)
// Row range of tile b: fixed 256-row tiles, or the equal-nnz blocks of `split` (Method_Balanced).
__device__ __forceinline__ void tile_rows(int b, int m, int rows_per_tile, const int *__restrict__ split, long long &r0, long long &r1)
{
    if (split) { r0 = split[b]; r1 = split[b + 1]; }
    else { r0 = (long long) b * rows_per_tile; r1 = r0 + rows_per_tile < m ? r0 + rows_per_tile : m; }
}

// Which four entries of a 4L-entry chunk a lane takes.  Every load instruction should cover one
// contiguous run of memory over the wave (a lane stride of 32 B -- four consecutive doubles per
// lane -- makes each 16-byte load touch twice the cache lines it uses).  So a lane takes 16 bytes of
// values per load: fp32 four consecutive entries (one load), fp64 two pairs, entries 2l, 2l+1 and
// 2L+2l, 2L+2l+1 (two loads, each contiguous over the L lanes of the row).
template <typename T, int L>
struct Lane4 {
    static constexpr int EPL = 16 / (int) sizeof(T); // entries per 16-byte load
    static __device__ __forceinline__ int pos(int l, int k) { return (k / EPL) * EPL * L + EPL * l + (k % EPL); }
    // v[0..3] = val[base + pos(l, k)]
    static __device__ __forceinline__ void load_val(const T *__restrict__ val, int base, int l, T (&v)[4])
    {
        if constexpr (EPL == 4) {
            ld_stream4(val + base + 4 * l, v);
        } else {
            const f64x2 a = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(val + base + 2 * l));
            const f64x2 b = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(val + base + 2 * L + 2 * l));
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
        }
    }
    // 16-bit slots, packed two per word in c[0], c[1] (see lds_slot)
    static __device__ __forceinline__ void load_col16(const unsigned short *__restrict__ col, int base, int l, int (&c)[4])
    {
        if constexpr (EPL == 4) {
            ld_stream4(col + base + 4 * l, c);
        } else {
            c[0] = __builtin_nontemporal_load(reinterpret_cast<const int *>(col + base + 2 * l));
            c[1] = __builtin_nontemporal_load(reinterpret_cast<const int *>(col + base + 2 * L + 2 * l));
        }
    }
    // BYTE tiles: one byte per entry (distance from the row's smallest slot); c[0] (fp32: four bytes) or c[0], c[1] (fp64: two bytes each)
    static __device__ __forceinline__ void load_col8(const unsigned char *__restrict__ col, int base, int l, int (&c)[4])
    {
        if constexpr (EPL == 4) {
            c[0] = __builtin_nontemporal_load(reinterpret_cast<const int *>(col + base + 4 * l));
        } else {
            c[0] = (int) __builtin_nontemporal_load(reinterpret_cast<const unsigned short *>(col + base + 2 * l));
            c[1] = (int) __builtin_nontemporal_load(reinterpret_cast<const unsigned short *>(col + base + 2 * L + 2 * l));
        }
    }
    template <int K> static __device__ __forceinline__ unsigned byte_of(const int (&c)[4])
    {
        if constexpr (EPL == 4) return ((unsigned) c[0] >> (8 * K)) & 0xffu;
        else return ((unsigned) c[K / 2] >> (8 * (K % 2))) & 0xffu;
    }
    static __device__ __forceinline__ void load_col32(const int *__restrict__ col, int base, int l, int (&c)[4])
    {
        if constexpr (EPL == 4) {
            ld_stream4(col + base + 4 * l, c);
        } else {
            const i32x2 a = __builtin_nontemporal_load(reinterpret_cast<const i32x2 *>(col + base + 2 * l));
            const i32x2 b = __builtin_nontemporal_load(reinterpret_cast<const i32x2 *>(col + base + 2 * L + 2 * l));
            c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y;
        }
    }
};

// PACKED tiles (fp64): the values of a tile that are all k * 2^e with ONE exponent e and integers |k| < 2^55 are streamed as 7 bytes instead of
// 8 -- the low 32 bits of k in one plane (lo), the high 24 bits, signed, in another (hi) -- from a copy the library keeps beside val.  The copy is
// permuted inside every aligned block of C = 4L entries so that the four entries Lane4 hands lane l (chunk-local q = (k / 2) * 2L + 2l + k % 2)
// sit side by side at slots 4l + k: ONE 16 B load from lo and ONE 12 B load from hi per lane and step, each contiguous over the L lanes of a row
// and over consecutive rows.  Valid where every row's chunks are aligned C-blocks inside the row (the gate, pack_tiles_kernel, checks it).
constexpr int kPackNone = INT_MIN; // per-tile exponent: the tile keeps its 8-byte stream
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((aligned(4))) PackHi3 { unsigned w0, w1, w2; }; // four 24-bit fields; 12 B apart, so only 4 B-aligned
struct PackArgs {
    const unsigned *lo = nullptr;
    const unsigned char *hi = nullptr;
    int e = 0;
};
// slot of absolute position p (C = 4L a power of two)
__host__ __device__ __forceinline__ long long pack_slot(long long p, int L)
{
    const int q = (int) (p & (4 * L - 1)), kh = q / (2 * L), rem = q % (2 * L);
    return p - q + 4 * (rem / 2) + 2 * kh + (rem & 1);
}
// the raw words of one lane's four entries, kept in registers while the loads are in flight; decoded when the step is consumed
struct PackRaw {
    unsigned lo[4] = {0, 0, 0, 0}, hi[3] = {0, 0, 0};
    __device__ __forceinline__ void load(const PackArgs &pk, int base, int l)
    {
        const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(pk.lo + base + 4 * l));
        const PackHi3 *h = reinterpret_cast<const PackHi3 *>(pk.hi + 3 * (size_t) (base + 4 * l));
        lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; lo[3] = a.w;
        hi[0] = __builtin_nontemporal_load(&h->w0); hi[1] = __builtin_nontemporal_load(&h->w1); hi[2] = __builtin_nontemporal_load(&h->w2);
    }
    // v = ldexp(hi * 2^32 + lo, e).  Exact at every step for a value that passed the gate: hi * 2^32 + lo = k is the value scaled by a power of two,
    // so it has at most 53 significant bits and the ONE rounding of the fused multiply-add returns it unchanged ((double) of a 32-bit integer is
    // exact, and so is the product inside the fma); ldexp by e then restores the value itself, which is a double (subnormals included), so nothing is
    // rounded there either.  k = 0 decodes to +0.0: a tile with a -0.0 is not packed.
    __device__ __forceinline__ void decode(int e, double (&v)[4]) const
    {
        const int h0 = (int) (hi[0] << 8) >> 8, h1 = (int) (((hi[0] >> 24) | (hi[1] << 8)) << 8) >> 8,
                  h2 = (int) (((hi[1] >> 16) | (hi[2] << 16)) << 8) >> 8, h3 = (int) hi[2] >> 8;
        v[0] = ldexp(fma((double) h0, 0x1p32, (double) lo[0]), e);
        v[1] = ldexp(fma((double) h1, 0x1p32, (double) lo[1]), e);
        v[2] = ldexp(fma((double) h2, 0x1p32, (double) lo[2]), e);
        v[3] = ldexp(fma((double) h3, 0x1p32, (double) lo[3]), e);
    }
    __device__ __forceinline__ void decode(int, float (&)[4]) const {} // fp32 is never packed
};

// One step of one lane group: lane l of the L lanes of row [p0, p1) multiplies its four entries
// (c, v: already loaded by Lane4 from the chunk starting at the 16 B-aligned position p0 & ~3) and, for
// rows longer than that chunk, walks on in chunks of 4L.  Returns the lane's partial sum (not yet reduced over the group).
// MODE 0: unstaged (global columns), 1: staged (16-bit slots from the column stream), 2: staged RUN tile (slots = rs + position in the row;
// cc0 unused), 3: staged BYTE tile (slots = rs + the entry's byte of the 8-bit column stream, packed in cc0), 4: staged TEMPLATE tile (slots = rs +
// tm[position in the row], tm = the tile's offset list in LDS; cc0 unused)
template <typename T, int L, int MODE, int SHIFT = 0, bool PACK = false>
__device__ __forceinline__ T csr_vector_step(int p0, int p1, int l, const int (&cc0)[4], const T (&vv0)[4],
                                             const int *__restrict__ colidx, const unsigned short *__restrict__ col_local,
                                             const T *__restrict__ val, const T *__restrict__ x,
                                             const unsigned char *__restrict__ xb, unsigned zoff, unsigned rs = 0, const unsigned char *__restrict__ col8 = nullptr,
                                             const unsigned short *__restrict__ tm = nullptr, PackArgs pk = PackArgs() /* PACK: the tile's planes and exponent */)
{
    constexpr bool STAGED = MODE != 0;
    constexpr unsigned INC = SHIFT ? 1u : (unsigned) sizeof(T); // slot unit of the stream: indices (wide form) or bytes
    // slot of entry e (e - p0 < row length) of a RUN tile's row
    auto run_slot = [&](int e) { return rs + (unsigned) (e - p0) * INC; };
    using LMB = Lane4<T, L>;
    // slot of the lane's k-th entry: from the row (RUN), the byte stream (BYTE) or the 16-bit stream
    auto slot_of = [&](auto kc, int e, const int (&cc)[4]) -> unsigned {
        constexpr int K = decltype(kc)::value;
        if constexpr (MODE == 2) return run_slot(e);
        else if constexpr (MODE == 4) return (rs & 0xffffu) + tm[(rs >> 16) + ((unsigned) (e - p0) & (unsigned) (kTmplMax - 1))]; // rs = slot | list number * kTmplMax << 16; out-of-row positions read a slot they never use
        else if constexpr (MODE == 3) return rs + LMB::template byte_of<K>(cc) * INC;
        else return lds_slot<K>(cc);
    };
    using K0 = std::integral_constant<int, 0>; using K1 = std::integral_constant<int, 1>; using K2 = std::integral_constant<int, 2>; using K3 = std::integral_constant<int, 3>;
    // SHIFT = 0: the stream holds LDS byte offsets; SHIFT = log2(sizeof(T)): slot indices (windows above 64 KiB)
    auto xat = [&](unsigned off) { return *reinterpret_cast<const T *>(xb + ((size_t) off << SHIFT)); };
    using LM = Lane4<T, L>;
    const int base = p0 & ~3;
    const int e0 = base + LM::pos(l, 0), e1 = base + LM::pos(l, 1), e2 = base + LM::pos(l, 2), e3 = base + LM::pos(l, 3); // ascending
    T sum = 0;
    if (STAGED) {
        const bool full = (e0 >= p0) & (e3 < p1), none = e0 >= p1;
        if (__all(full | none)) {
            if (full) {
                const T x0 = xat(slot_of(K0{}, e0, cc0)), x1 = xat(slot_of(K1{}, e1, cc0)), x2 = xat(slot_of(K2{}, e2, cc0)), x3 = xat(slot_of(K3{}, e3, cc0));
                sum = fmadd(vv0[0], x0, sum);
                sum = fmadd(vv0[1], x1, sum);
                sum = fmadd(vv0[2], x2, sum);
                sum = fmadd(vv0[3], x3, sum);
            }
        } else {
            const unsigned len = (unsigned) (p1 - p0); // entry e is in the row iff e - p0 < len (unsigned)
            const bool k0 = (unsigned) (e0 - p0) < len, k1 = (unsigned) (e1 - p0) < len, k2 = (unsigned) (e2 - p0) < len,
                       k3 = (unsigned) (e3 - p0) < len;
            const T x0 = xat(k0 ? slot_of(K0{}, e0, cc0) : zoff), x1 = xat(k1 ? slot_of(K1{}, e1, cc0) : zoff),
                    x2 = xat(k2 ? slot_of(K2{}, e2, cc0) : zoff), x3 = xat(k3 ? slot_of(K3{}, e3, cc0) : zoff);
            sum = fmadd(k0 ? vv0[0] : T(0), x0, sum);
            sum = fmadd(k1 ? vv0[1] : T(0), x1, sum);
            sum = fmadd(k2 ? vv0[2] : T(0), x2, sum);
            sum = fmadd(k3 ? vv0[3] : T(0), x3, sum);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = base + LM::pos(l, k);
            const bool ok = (e >= p0) & (e < p1);
            const int ci = ok ? cc0[k] : 0;
            const T xl = x[ci];
            sum = fmadd(ok ? vv0[k] : T(0), ok ? xl : T(0), sum);
        }
    }
    if (__any(base + 4 * L < p1)) { // some row of this step is longer than its first 4L-entry chunk
        for (int bb = base + 4 * L; __any(bb < p1); bb += 4 * L) {
            if (bb < p1) {
                int cc[4] = {0, 0, 0, 0};
                T v2[4];
                if (MODE == 1) LM::load_col16(col_local, bb, l, cc);
                else if (MODE == 0) LM::load_col32(colidx, bb, l, cc);
                else if (MODE == 3) LM::load_col8(col8, bb, l, cc);
                if constexpr (PACK) { PackRaw r2; r2.load(pk, bb, l); r2.decode(pk.e, v2); }
                else LM::load_val(val, bb, l, v2);
                if (MODE == 4) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (bb + LM::pos(l, k) < p1) sum = fmadd(v2[k], xat((rs & 0xffffu) + tm[(rs >> 16) + ((unsigned) (bb + LM::pos(l, k) - p0) & (unsigned) (kTmplMax - 1))]), sum);
                } else if (MODE == 3) {
                    if (bb + LM::pos(l, 0) < p1) sum = fmadd(v2[0], xat(slot_of(K0{}, 0, cc)), sum);
                    if (bb + LM::pos(l, 1) < p1) sum = fmadd(v2[1], xat(slot_of(K1{}, 0, cc)), sum);
                    if (bb + LM::pos(l, 2) < p1) sum = fmadd(v2[2], xat(slot_of(K2{}, 0, cc)), sum);
                    if (bb + LM::pos(l, 3) < p1) sum = fmadd(v2[3], xat(slot_of(K3{}, 0, cc)), sum);
                } else if (MODE == 2) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (bb + LM::pos(l, k) < p1) sum = fmadd(v2[k], xat(run_slot(bb + LM::pos(l, k))), sum);
                } else if (STAGED) {
                    if (bb + LM::pos(l, 0) < p1) sum = fmadd(v2[0], xat(lds_slot<0>(cc)), sum);
                    if (bb + LM::pos(l, 1) < p1) sum = fmadd(v2[1], xat(lds_slot<1>(cc)), sum);
                    if (bb + LM::pos(l, 2) < p1) sum = fmadd(v2[2], xat(lds_slot<2>(cc)), sum);
                    if (bb + LM::pos(l, 3) < p1) sum = fmadd(v2[3], xat(lds_slot<3>(cc)), sum);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (bb + LM::pos(l, k) < p1) sum = fmadd(v2[k], x[cc[k]], sum);
                }
            }
        }
    }
    return sum;
}

// The wave program.  STAGED: c[][0..1] hold four packed 16-bit BYTE offsets into xs (the inspector
// stores slot * sizeof(T)), so a gather is one extract + one ds_read with the LDS base as immediate;
// zoff is the byte offset of a slot that holds 0 (masked entries read it: 0 * 0, never x's NaN/Inf).
// A step whose lanes all hold four entries of their row, or none (regular matrices: every step),
// takes the unmasked path.  The order of the fused multiply-adds is the same on both paths.
// PACK: the tile's values come from the packed planes (pk; r0 = step 0's raw words when PRE); everything after the decode is the same code.
template <typename T, int L, int MODE, int DEPTH, bool PRE = true, int SHIFT = 0, bool PACK = false>
__device__ __forceinline__ void csr_vector_tile_wave(long long row_end, int long_thr, long long rw0, int lane,
                                                     const int *__restrict__ rp_lds, const unsigned *__restrict__ rs_lds /* MODE >= 2: slot of each row's first column (MODE 4: | list number * kTmplMax << 16) */,
                                                     T *__restrict__ y_lds,
                                                     const int *__restrict__ colidx, const unsigned short *__restrict__ col_local,
                                                     const T *__restrict__ val,
                                                     const T *__restrict__ x, const T *__restrict__ xs, unsigned zoff,
                                                     T *__restrict__ y, const int (&c0)[4], const T (&v0)[4], const unsigned char *__restrict__ col8 = nullptr,
                                                     const unsigned short *__restrict__ tm = nullptr, PackArgs pk = PackArgs(), PackRaw r0 = PackRaw())
{
    constexpr int RW = kWave / L; // rows per step
    constexpr int D = DEPTH < L ? DEPTH : L; // steps of matrix stream in flight per wave
    const int l = lane % L, sub = lane / L;
    const unsigned char *xb = reinterpret_cast<const unsigned char *>(xs);
    int c[D][4];
    T v[D][4];
    PackRaw pr[PACK ? D : 1]; // PACK: the raw words instead of v
    pr[0] = r0;
    int pp0[D], pp1[D];
    unsigned rs[D];
#pragma unroll
    for (int k = 0; k < D; ++k) rs[k] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { c[0][k] = c0[k]; v[0][k] = v0[k]; } // PRE: step 0 was issued before the barrier
    auto issue = [&](int s) { // RowPtr pair of step s from LDS, then its stream loads
        const int slot = s % D;
        pp0[slot] = rp_lds[s * RW + sub];
        pp1[slot] = rp_lds[s * RW + sub + 1];
        if (pp1[slot] - pp0[slot] > long_thr) pp1[slot] = pp0[slot];
        if (MODE >= 2) rs[slot] = rs_lds[s * RW + sub];
        if (s > 0 || !PRE) {
            const int an = pp0[slot] & ~3;
            if (MODE == 1) Lane4<T, L>::load_col16(col_local, an, l, c[slot]);
            else if (MODE == 0) Lane4<T, L>::load_col32(colidx, an, l, c[slot]);
            else if (MODE == 3) Lane4<T, L>::load_col8(col8, an, l, c[slot]);
            if constexpr (PACK) pr[slot].load(pk, an, l);
            else Lane4<T, L>::load_val(val, an, l, v[slot]);
        }
    };
#pragma unroll
    for (int s = 0; s < D && s < L; ++s) issue(s);
#pragma unroll
    for (int s = 0; s < L; ++s) {
        const int cur = s % D;
        const int p0 = pp0[cur], p1 = pp1[cur];
        if constexpr (PACK) pr[cur].decode(pk.e, v[cur]);
        T sum = csr_vector_step<T, L, MODE, SHIFT, PACK>(p0, p1, l, c[cur], v[cur], colidx, col_local, val, x, xb, zoff, rs[cur], col8, tm, pk);
        sum = group_sum_dpp<L>(sum);
        if (l == 0) y_lds[s * RW + sub] = sum;
        if (s + D < L) issue(s + D); // refill the slot just consumed
    }
    wave_lds_sync();
    const long long row = rw0 + lane;
    const int len = rp_lds[lane + 1] - rp_lds[lane];
    if (row < row_end && len <= long_thr) y[row] = y_lds[lane]; // one coalesced 64-row store per wave
}

// PACK (fp64): tiles whose entry of tile_e is not kPackNone read their values from the packed planes pk_lo / pk_hi; the others run the 8-byte path.
template <typename T, int L, int DEPTH = 4, bool PRE = true, bool PACK = false>
__global__ __launch_bounds__(kVecTileThreads) void csr_vector_tile_kernel(int m, int long_thr, const int *__restrict__ rowptr,
                                                                          const int *__restrict__ colidx,
                                                                          const unsigned short *__restrict__ col_local,
                                                                          const T *__restrict__ val,
                                                                          const TileWindows *__restrict__ wins,
                                                                          const unsigned short *__restrict__ row_slot,
                                                                          const unsigned char *__restrict__ col8,
                                                                          const unsigned short *__restrict__ tmpl, const unsigned char *__restrict__ row_tid,
                                                                          const T *__restrict__ x, T *__restrict__ y,
                                                                          const unsigned *__restrict__ pk_lo = nullptr, const unsigned char *__restrict__ pk_hi = nullptr,
                                                                          const int *__restrict__ tile_e = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char vec_x_lds[]; // the tile's staged x
    __shared__ unsigned short tm_lds[kTmplCount * kTmplMax];
    T *xs = reinterpret_cast<T *>(vec_x_lds);
    __shared__ int rp_lds[kVecTileThreads / kWave][kWave + 2];
    __shared__ unsigned rs_lds[kVecTileThreads / kWave][kWave];
    __shared__ T y_lds[kVecTileThreads / kWave][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long long rw0 = (long long) blockIdx.x * kVecTileRows + wave * kWave;
    // RowPtr of the wave's 64 rows (+1): one coalesced load, rows past m repeat RowPtr[m]
    long long r = rw0 + lane, re = rw0 + kWave;
    if (r > m) r = m;
    if (re > m) re = m;
    const int rp = rowptr[r];
    const int rpe = rowptr[re]; // wave-uniform
    const TileWindows &tw = wins[blockIdx.x];
    const bool staged = tw.nwin > 0, runs = tw.runs == 1, bytes = tw.runs == 2, templ = tw.runs == 3; // runs / bytes / templ imply staged
    // step 0 of the matrix stream is issued straight from registers (RowPtr handed over by
    // shuffles), BEFORE the x staging and the barrier, so neither sits in front of the first loads
    int c0[4] = {0, 0, 0, 0};
    T v0[4] = {T(0), T(0), T(0), T(0)};
    PackArgs pk;
    PackRaw r0;
    bool packed = false;
    if constexpr (PACK) {
        pk.lo = pk_lo; pk.hi = pk_hi; pk.e = tile_e[blockIdx.x]; // workgroup-uniform
        packed = pk.e != kPackNone;
    }
    if (PRE) {
        const int sub = lane / L, l = lane % L;
        const int q0 = __shfl(rp, sub, kWave);
        const int a = q0 & ~3;
        if (runs | templ) {}
        else if (bytes) Lane4<T, L>::load_col8(col8, a, l, c0);
        else if (staged) Lane4<T, L>::load_col16(col_local, a, l, c0);
        else Lane4<T, L>::load_col32(colidx, a, l, c0);
        if (PACK && packed) r0.load(pk, a, l);
        else Lane4<T, L>::load_val(val, a, l, v0);
    }
    rp_lds[wave][lane] = rp;
    if (lane == 0) rp_lds[wave][kWave] = rpe;
    if (runs | bytes) rs_lds[wave][lane] = row_slot[r]; // r <= m: the array has m + 1 entries
    if (templ) {
        rs_lds[wave][lane] = (unsigned) row_slot[r] | ((unsigned) row_tid[r] * kTmplMax << 16);
        for (int i = threadIdx.x; i < kTmplCount * kTmplMax; i += kVecTileThreads) tm_lds[i] = tmpl[(size_t) blockIdx.x * (kTmplCount * kTmplMax) + i];
    }
    stage_windows<kVecTileThreads, T>(tw, x, xs);
    if (threadIdx.x == 0) xs[tw.total] = T(0); // the zero slot of masked entries
    __syncthreads();
    if (rw0 >= m) return;
    const unsigned zoff = (unsigned) tw.total * (unsigned) sizeof(T);
    // one wave program per tile form, from the 8-byte stream or (PACK, packed tiles) from the packed planes
#define SPMV_TILE_WAVE(MODE, ...)                                                                                                                                   \
    do {                                                                                                                                                            \
        if (PACK && packed) csr_vector_tile_wave<T, L, MODE, DEPTH, PRE, 0, PACK>((long long) m, long_thr, rw0, lane, rp_lds[wave], rs_lds[wave], y_lds[wave], colidx, col_local, val, x, xs, zoff, y, c0, v0, __VA_ARGS__, pk, r0); \
        else csr_vector_tile_wave<T, L, MODE, DEPTH, PRE>((long long) m, long_thr, rw0, lane, rp_lds[wave], rs_lds[wave], y_lds[wave], colidx, col_local, val, x, xs, zoff, y, c0, v0, __VA_ARGS__); \
    } while (0)
    if (runs) SPMV_TILE_WAVE(2, col8, nullptr);
    else if (bytes) SPMV_TILE_WAVE(3, col8, nullptr);
    else if (templ) SPMV_TILE_WAVE(4, col8, tm_lds);
    else if (staged) SPMV_TILE_WAVE(1, col8, nullptr);
    else SPMV_TILE_WAVE(0, col8, nullptr);
#undef SPMV_TILE_WAVE
}

// Balanced form (Method_Balanced): the same wave program over EQUAL-NNZ row blocks.  Block b owns
// rows [split[b], split[b+1]) (init_csrSplitter_balanced2 semantics, parallel_balanced2_spmv.c:41-53,
// built by rowblock_split_kernel) and walks them in 256-row slabs, 64 rows per wave; the x windows
// of the whole block are staged once.
template <typename T, int L, int DEPTH = 4, bool WIDE = false>
__global__ __launch_bounds__(kVecTileThreads) void csr_vector_rows_kernel(int long_thr, const int *__restrict__ split,
                                                                          int rows_per_block, int m,
                                                                          const int *__restrict__ rowptr,
                                                                          const int *__restrict__ colidx,
                                                                          const unsigned short *__restrict__ col_local,
                                                                          const T *__restrict__ val,
                                                                          const TileWindows *__restrict__ wins,
                                                                          const unsigned short *__restrict__ row_slot,
                                                                          const unsigned char *__restrict__ col8,
                                                                          const unsigned short *__restrict__ tmpl, const unsigned char *__restrict__ row_tid,
                                                                          const T *__restrict__ x, T *__restrict__ y)
{
    __shared__ unsigned short tm_lds[kTmplCount * kTmplMax];
    // WIDE: x windows above 64 KiB (fp64 rows whose columns scatter over thousands of columns): the column
    // stream holds slot INDICES instead of byte offsets; blocks are `rows_per_block` consecutive rows
    // (split == NULL) so that one staging serves more rows.
    constexpr int SHIFT = WIDE ? (sizeof(T) == 8 ? 3 : 2) : 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char vec_x_lds[];
    T *xs = reinterpret_cast<T *>(vec_x_lds);
    __shared__ int rp_lds[kVecTileThreads / kWave][kWave + 2];
    __shared__ unsigned rs_lds[kVecTileThreads / kWave][kWave];
    __shared__ T y_lds[kVecTileThreads / kWave][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    long long r_begin, r_end;
    tile_rows(blockIdx.x, m, rows_per_block, split, r_begin, r_end);
    const TileWindows &tw = wins[blockIdx.x];
    const bool staged = tw.nwin > 0, runs = tw.runs == 1, bytes = tw.runs == 2, templ = tw.runs == 3;
    if (templ) for (int i = threadIdx.x; i < kTmplCount * kTmplMax; i += kVecTileThreads) tm_lds[i] = tmpl[(size_t) blockIdx.x * (kTmplCount * kTmplMax) + i];
    stage_windows<kVecTileThreads, T>(tw, x, xs);
    if (threadIdx.x == 0) xs[tw.total] = T(0); // the zero slot of masked entries
    __syncthreads();
    const unsigned zoff = WIDE ? (unsigned) tw.total : (unsigned) tw.total * (unsigned) sizeof(T);
    const int c0[4] = {0, 0, 0, 0};
    const T v0[4] = {T(0), T(0), T(0), T(0)};
    for (long long rw0 = r_begin + (long long) wave * kWave; rw0 < r_end; rw0 += kVecTileRows) {
        long long r = rw0 + lane, re = rw0 + kWave;
        if (r > r_end) r = r_end;
        if (re > r_end) re = r_end;
        rp_lds[wave][lane] = rowptr[r];
        if (lane == 0) rp_lds[wave][kWave] = rowptr[re];
        if (runs | bytes) rs_lds[wave][lane] = row_slot[r];
        if (templ) rs_lds[wave][lane] = (unsigned) row_slot[r] | ((unsigned) row_tid[r] * kTmplMax << 16);
        wave_lds_sync();
        if (runs) csr_vector_tile_wave<T, L, 2, DEPTH, false, SHIFT>(r_end, long_thr, rw0, lane, rp_lds[wave], rs_lds[wave], y_lds[wave], colidx, col_local, val, x, xs, zoff, y, c0, v0);
        else if (bytes) csr_vector_tile_wave<T, L, 3, DEPTH, false, SHIFT>(r_end, long_thr, rw0, lane, rp_lds[wave], rs_lds[wave], y_lds[wave], colidx, col_local, val, x, xs, zoff, y, c0, v0, col8);
        else if (templ) csr_vector_tile_wave<T, L, 4, DEPTH, false, SHIFT>(r_end, long_thr, rw0, lane, rp_lds[wave], rs_lds[wave], y_lds[wave], colidx, col_local, val, x, xs, zoff, y, c0, v0, col8, tm_lds);
        else if (staged) csr_vector_tile_wave<T, L, 1, DEPTH, false, SHIFT>(r_end, long_thr, rw0, lane, rp_lds[wave], rs_lds[wave], y_lds[wave], colidx, col_local, val, x, xs, zoff, y, c0, v0);
        else csr_vector_tile_wave<T, L, 0, DEPTH, false, SHIFT>(r_end, long_thr, rw0, lane, rp_lds[wave], rs_lds[wave], y_lds[wave], colidx, col_local, val, x, xs, zoff, y, c0, v0);
        wave_lds_sync(); // y_lds / rp_lds are reused by the next slab
    }
}

// One CSR-vector launch, resolved by the shim (shim/launch.hpp: vector_args) and made by spmv_vector.hip: which kernel with which
// template arguments, and the device arrays it reads.
enum { kVecPipeKernel, kVecTileKernel, kVecRowsKernel };
struct VecArgs {
    int kernel = kVecPipeKernel;
    int lanes = 64, depth = 4;   // L (lanes per row); steps in flight (tile: 2 / 4 / 8, rows: 2 / 4)
    bool pre = true, wide = false; // tile kernel: step 0 issued before the barrier; rows kernel: slot-index stream over uniform blocks
    int m = 0, long_thr = INT_MAX, tiles = 0, maxspan = 0, rows = 256;
    const int *rowptr = nullptr, *colidx = nullptr, *split = nullptr; // split: Balanced's row blocks (rows kernel; NULL: uniform blocks of `rows`)
    const void *val = nullptr;
    const unsigned short *col = nullptr, *rowslot = nullptr, *tmpl = nullptr;
    const unsigned char *col8 = nullptr, *rowtid = nullptr;
    const TileWindows *wins = nullptr;
    // tile kernel, fp64: the packed value planes and the per-tile exponents (NULL: every tile reads val)
    const unsigned *pk_lo = nullptr;
    const unsigned char *pk_hi = nullptr;
    const int *pk_e = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
};
// spmv_vector.hip: the tile and pipe kernels, the rows kernel
hipError_t vector_launch(const VecArgs &a, const double *x, double *y);
hipError_t vector_launch(const VecArgs &a, const float *x, float *y);
hipError_t vector_launch_packed(const VecArgs &a, const double *x, double *y); // the tile kernel with VecArgs::pk_e set, two or four steps in flight
hipError_t rows_launch(const VecArgs &a, const double *x, double *y);
hipError_t rows_launch(const VecArgs &a, const float *x, float *y);

} // namespace spmv
