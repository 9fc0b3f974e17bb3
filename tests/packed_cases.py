"""Host helpers of the PACKED-tile tests (option pack_values; kernels/csr_vector_tile.hpp, shim/inspect.hpp: pack_tiles_kernel).

Shared by tests/test_gpu_packed_values.py, tests/test_gpu_packed_forms.py (GPU) and tests/test_packed_model_host.py (CPU):
  * matrices: `banded` (wrap-around band), `open_band` (no wrap: every tile a RUN tile), `sparse_rows` (BYTE tiles), `pattern_rows` (TEMPLATE tiles),
    `scattered_rows` (unstaged tiles);
  * values: `edge_values` -- every tile filled with the integers k at the edges of the 24 + 32-bit fields, |k| up to 2^55 - 8;
  * the gate's model `model_packed`, and Python-integer copies of the pack arithmetic: `pack_slot_model`, `encode`, `decode`, `pack_hi_words`,
    `unpack_hi_words`;
  * two references that do not go through the other GPU path: `probe_readback` (exact, order-independent: unit vectors read every stored entry back
    from the packed planes) and `hp_check` (np.longdouble sums with the textbook error bound);
  * `Pair`: one matrix under pack_values = 1 and 0;
  * `fixture(name)`: the structural cases of test_gpu_packed_forms.py, so that the CPU test can check what the GPU test assumes about them.
"""
import math
import struct
from collections import namedtuple

import numpy as np

from spmv_amd import api

TILE = 256
METHOD = int(api.SPMV_METHODS.Method_Parallel)
TILE_KERNEL = "csr_vector_tile_kernel"


# ------------------------------------------------------------------------------------------------ matrices
def _rowptr(lens):
    lens = np.asarray(lens, dtype=np.int64)
    rp = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=rp[1:])
    row = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    return lens, rp, row


def banded(lens, seed=1):
    """m = len(lens) rows, n = m columns; row i holds columns (i - len_i // 2 + j) mod n, j = 0 .. len_i - 1; values uniform in [-1, 1)."""
    lens, rp, row = _rowptr(lens)
    m = lens.size
    j = np.arange(int(rp[-1]), dtype=np.int64) - rp[row]
    ci = ((row - lens[row] // 2 + j) % m).astype(np.int32)
    va = np.random.default_rng(seed).uniform(-1.0, 1.0, size=int(rp[-1]))
    return m, rp.astype(np.int32), ci, va


def open_band(lens, seed=1):
    """-> (m, n, rp, ci, va): row i holds columns i .. i + len_i - 1 of n = m + max(lens): no row wraps, so every tile is a RUN tile."""
    lens, rp, row = _rowptr(lens)
    m = lens.size
    ci = (row + np.arange(int(rp[-1]), dtype=np.int64) - rp[row]).astype(np.int32)
    va = np.random.default_rng(seed).uniform(-1.0, 1.0, size=int(rp[-1]))
    return m, m + int(lens.max()), rp.astype(np.int32), ci, va


def sparse_rows(m, n, lens, window, seed):
    """-> (m, n, rp, ci, va): row i holds lens[i] DISTINCT ascending columns drawn from [start_i, start_i + window), start_i = min(i, n - window):
    a band with holes.  With more than 8 different hole patterns per tile and window <= 256 these are BYTE tiles."""
    lens, rp, row = _rowptr(lens)
    assert lens.max() <= window <= n
    rng = np.random.default_rng(seed)
    order = np.argsort(rng.random((m, window)), axis=1)                      # a random permutation of the window per row
    keep = np.arange(window)[None, :] < lens[:, None]
    picked = np.where(keep, order, window)                                   # the first lens[i] of it; the rest sort behind
    picked.sort(axis=1)
    start = np.minimum(np.arange(m, dtype=np.int64), n - window)
    ci = (start[:, None] + picked)[keep].astype(np.int32)
    va = rng.uniform(-1.0, 1.0, size=int(rp[-1]))
    return m, n, rp.astype(np.int32), ci, va


def pattern_rows(m, n, offsets, seed=1):
    """-> (m, n, rp, ci, va): every row holds base_i + offsets (ascending, within a window of 128), base_i = min(i, n - 128): one offset list for
    the whole matrix, which is a TEMPLATE tile wherever the list is not 0, 1, 2, ..."""
    offsets = np.asarray(offsets, dtype=np.int64)
    assert (np.diff(offsets) > 0).all() and offsets[0] >= 0 and offsets[-1] < 128 <= n
    k = offsets.size
    base = np.minimum(np.arange(m, dtype=np.int64), n - 128)
    ci = (base[:, None] + offsets[None, :]).reshape(-1).astype(np.int32)
    rp = (np.arange(m + 1, dtype=np.int64) * k).astype(np.int32)
    va = np.random.default_rng(seed).uniform(-1.0, 1.0, size=m * k)
    return m, n, rp, ci, va


def scattered_rows(m, k, step, seed=1):
    """-> (m, n, rp, ci, va): row i holds columns i + j * step, j = 0 .. k - 1: a 256-row tile touches k separate bands, more x windows than
    the inspector keeps per tile (16) when k > 16, so no tile stages its x and the tile kernel gathers from global memory."""
    lens, rp, row = _rowptr(np.full(m, k))
    ci = (row + (np.arange(m * k, dtype=np.int64) - rp[row]) * step).astype(np.int32)
    va = np.random.default_rng(seed).uniform(-1.0, 1.0, size=m * k)
    return m, m + (k - 1) * step, rp.astype(np.int32), ci, va


def x_of(n, seed=7):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=n)


def transpose_csr(m, n, rp, ci, va):
    """A^T as (n, m, rp_T, ci_T, va_T), the columns of every row ascending (a stable sort of the entries by column)."""
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp.astype(np.int64)))
    order = np.argsort(ci, kind="stable")
    rpt = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=n), out=rpt[1:])
    return n, m, rpt.astype(np.int32), row[order].astype(np.int32), va[order]


def distinct_mod(rp, ci, stride):
    """every row's columns are distinct modulo stride"""
    row = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp.astype(np.int64)))
    key = row * stride + ci.astype(np.int64) % stride
    return np.unique(key).size == key.size


# ------------------------------------------------------------------------------------------------ the gate's model
def bit_span(v):
    """(top, low) over the non-zero finite values of v: largest leading-bit position, smallest lowest-set-bit position; None if all are zero."""
    b = np.ascontiguousarray(v).view(np.uint64)
    E = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    frac = b & np.uint64((1 << 52) - 1)
    mant = (frac | ((E > 0).astype(np.uint64) << np.uint64(52))).astype(np.int64)
    nz = mant != 0
    if not nz.any():
        return None
    mant, base = mant[nz], np.maximum(E[nz], 1) - 1075
    top = base + np.frexp(mant.astype(np.float64))[1] - 1          # mant < 2^53: exact in a double
    low = base + np.frexp((mant & -mant).astype(np.float64))[1] - 1
    return int(top.max()), int(low.min())


def model_packed(rp, va, L):
    """-> (packed entries, [tile packs?]) by the gate's definition: no row longer than long_thr = max(64 L, 256) (the default rule, which is what
    a handle with lanes_per_row forced -- or with rows of one length -- gets), rows in aligned 4L-blocks, finite values, no -0.0, span <= 54."""
    C, m = 4 * L, rp.size - 1
    long_thr = max(64 * L, 256)
    total, flags = 0, []
    for r0 in range(0, m, TILE):
        r1 = min(m, r0 + TILE)
        starts, lens = rp[r0:r1].astype(np.int64), np.diff(rp[r0:r1 + 1].astype(np.int64))
        v = va[rp[r0]:rp[r1]]
        ok = bool((starts % C == 0).all() and (lens % C == 0).all() and (lens <= long_thr).all())
        ok = ok and bool(np.isfinite(v).all()) and not bool(((v == 0) & np.signbit(v)).any())
        if ok:
            span = bit_span(v)
            ok = span is None or span[0] - span[1] <= 54
        flags.append(ok)
        total += int(rp[r1] - rp[r0]) if ok else 0
    return total, flags


def tile_spans(rp, va):
    """top - low of bit_span per 256-row tile (None: no non-zero value)"""
    out = []
    for r0 in range(0, rp.size - 1, TILE):
        s = bit_span(va[rp[r0]:rp[min(rp.size - 1, r0 + TILE)]])
        out.append(None if s is None else s[0] - s[1])
    return out


# ------------------------------------------------------------------------------------------------ the pack arithmetic in Python integers
def pack_slot_model(p, L):
    """pack_slot (csr_vector_tile.hpp): the slot of absolute position p in the permuted planes"""
    q = p & (4 * L - 1)
    kh, rem = q // (2 * L), q % (2 * L)
    return p - q + 4 * (rem // 2) + 2 * kh + (rem & 1)


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def encode(v, e):
    """pack_tiles_kernel's integer of a value under the tile exponent e -> (lo, hi24): the low 32 bits and the next 24 bits of k = v / 2^e"""
    b = _bits(v)
    E, frac = (b >> 52) & 0x7FF, b & ((1 << 52) - 1)
    mant = frac | (1 << 52) if E else frac
    sh = (E if E else 1) - 1075 - e
    k = mant << sh if sh >= 0 else mant >> -sh
    if b >> 63:
        k = -k
    return k & 0xFFFFFFFF, (k >> 32) & 0xFFFFFF


def pack_hi_words(h):
    """the three 32-bit words pack_tiles_kernel stores for the four 24-bit fields h[0..3]"""
    M = 0xFFFFFFFF
    return (h[0] | h[1] << 24) & M, (h[1] >> 8 | h[2] << 16) & M, (h[2] >> 16 | h[3] << 8) & M


def _sext24(w):
    w &= 0xFFFFFF
    return w - (1 << 24) if w & 0x800000 else w


def unpack_hi_words(w):
    """PackRaw::decode's four signed 24-bit fields from the three words"""
    M = 0xFFFFFFFF
    return (_sext24(w[0]), _sext24((w[0] >> 24) | (w[1] << 8) & M), _sext24((w[1] >> 16) | (w[2] << 16) & M), _sext24(w[2] >> 8))


def decode(lo, hi24, e):
    """PackRaw::decode: ldexp(fma(h, 2^32, lo), e) with h the sign-extended field.  int -> float rounds once, as the fma does."""
    return math.ldexp(float(_sext24(hi24) * (1 << 32) + lo), e)


# ------------------------------------------------------------------------------------------------ values at the edges of the fields
EDGE_E = -40                                  # the tile exponent of edge_values: every tile holds +-2^-40
_A = 2.0 ** 15 - 2.0 ** -37                   # k = 2^55 - 8: hi = 0x7fffff, lo = 0xfffffff8; -k: hi = -2^23 (0x800000), lo = 8
_B = 2.0 ** 14 + 2.0 ** -38                   # k = 2^54 + 4
_C = 2.0 ** -8 - 2.0 ** -40                   # k = 2^32 - 1: hi = 0, lo = 0xffffffff; -k: hi = -1, lo = 1
# None: a random 53-bit multiple of 2^-38 below 2^15, either sign.  13 patterns: coprime with the 4 entries of a lane quad.
EDGE_PATTERNS = [_A, -_A, 2.0 ** -40, -2.0 ** -40, 2.0 ** -8, -2.0 ** -8, _C, -_C, 0.0, _B, -_B, None, None]


def edge_values(nnz, rp, seed=3):
    """va[p] = EDGE_PATTERNS[(p + row of p) % 13]: every pattern in every tile and, as the rows go by, at each of a lane quad's four positions.
    All on the 2^-40 grid below 2^15: the span of every tile of at least 13 entries is exactly 54 (top 14, low -40)."""
    lens = np.diff(rp.astype(np.int64))
    row = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    assert row.size == nnz
    idx = (np.arange(nnz, dtype=np.int64) + row) % len(EDGE_PATTERNS)
    rng = np.random.default_rng(seed)
    rand = np.ldexp(rng.integers(1, 1 << 53, size=nnz).astype(np.float64), -38) * rng.choice([-1.0, 1.0], size=nnz)
    table = np.array([0.0 if p is None else p for p in EDGE_PATTERNS])
    israndom = np.array([p is None for p in EDGE_PATTERNS])
    return np.where(israndom[idx], rand, table[idx])


def dblmax_values(count, seed=11):
    """DBL_MAX = (2^53 - 1) 2^971 at one entry in 32 (one per 32-entry row, at a position that moves with the row) and odd multiples of 2^971 below
    2^992 elsewhere, either sign: e = 971, and no row's sum overflows under |x| < 1."""
    rng = np.random.default_rng(seed)
    v = np.ldexp((2 * rng.integers(0, 1 << 20, size=count) + 1).astype(np.float64), 971) * rng.choice([-1.0, 1.0], size=count)
    p = np.arange(count)
    v[(p % 32) == (p // 32) % 32] = np.finfo(np.float64).max
    return v


def subnormal_values(count, seed=12):
    """the subnormal grid: 5e-324 (k = 1) and 2^-1020 (k = 2^54) at fixed places, a quarter of the entries normal numbers in [2^-1022, 2^-1020)
    (so that every 32-entry row's sum |a x| stays above 2^-1022 and the absolute rounding step 2^-1075 of the subnormal range is inside hp_check's
    relative bound), the rest random subnormals.  e = -1074, span exactly 54."""
    rng = np.random.default_rng(seed)
    v = np.ldexp(rng.integers(1, 1 << 52, size=count).astype(np.float64), -1074)
    p = np.arange(count)
    big = p % 4 == 1
    v[big] = np.ldexp(rng.integers(1 << 52, 1 << 53, size=int(big.sum())).astype(np.float64), -1074 + (p[big] // 4) % 2)
    v *= rng.choice([-1.0, 1.0], size=count)
    v[0::64] = 5e-324
    v[2::64] = 2.0 ** -1020
    return v


# ------------------------------------------------------------------------------------------------ references
def probe_readback(pair, m, n, rp, ci, va, stride, mul=None):
    """Read every stored entry back through the packed handle.  x[c] = 1 where c % stride == r, else 0: as every row's columns are distinct modulo
    stride (asserted), row i of y is the ONE entry of row i in a column = r mod stride, plus zeros -- exact whatever the order of the additions.
    It must equal va's entry bit for bit where that entry exists and is not zero, and be zero elsewhere.  After `stride` multiplies every entry of
    every slot has been compared with the host's array: encode, permutation and decode together.  `mul`: x -> y (default: the packed handle's
    spmv); (m, n, rp, ci, va) describe the operator `mul` applies."""
    assert distinct_mod(rp, ci, stride), "probe_readback needs every row's columns distinct modulo the stride"
    if mul is None:
        mul = lambda x: pair.h[1].spmv(x, np.full(m, np.nan))
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp.astype(np.int64)))
    res = ci.astype(np.int64) % stride
    cols = np.arange(n, dtype=np.int64) % stride
    for r in range(stride):
        y = mul((cols == r).astype(np.float64))
        want = np.zeros(m)
        sel = res == r
        want[row[sel]] = va[sel]
        nz = want != 0
        bad = y.view(np.uint64)[nz] != want.view(np.uint64)[nz]
        assert not bad.any(), f"residue {r}: {int(bad.sum())} entries read back wrong, first in row {int(np.flatnonzero(nz)[bad][0])}"
        assert (y[~nz] == 0).all(), f"residue {r}: {int((y[~nz] != 0).sum())} rows without an entry there are not zero"


def hp_check(y, rp, ci, va, x):
    """|y_i - ref_i| <= 2 len_i 2^-53 sum_j |a_ij x_j| against products and sums in np.longdouble: the bound of len_i fused multiply-adds in any
    order (each rounds once, relative 2^-53, to first order len_i 2^-53 sum |a x|), doubled.  Derived, not measured."""
    ld = np.longdouble
    rp64 = rp.astype(np.int64)
    lens = np.diff(rp64)
    prod = va.astype(ld) * x[ci].astype(ld)
    ref, mag = np.zeros(lens.size, dtype=ld), np.zeros(lens.size, dtype=ld)
    if prod.size:
        full = lens > 0                               # reduceat over the non-empty rows: consecutive starts bound exactly one row each
        ref[full] = np.add.reduceat(prod, rp64[:-1][full])
        mag[full] = np.add.reduceat(np.abs(prod), rp64[:-1][full])
    assert np.isfinite(y).all()
    err = np.abs(y.astype(ld) - ref)
    bound = 2 * lens.astype(ld) * ld(2.0 ** -53) * mag
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), f"row {worst}: |y - ref| = {float(err[worst]):.3e} > {float(bound[worst]):.3e}"


# ------------------------------------------------------------------------------------------------ the two handles
class Pair:
    """The same matrix under pack_values = 1 and pack_values = 0, `options` (and lanes_per_row = lanes, if given) applied to both handles.
    `kernel`: the kernel both must run (None: not checked)."""

    def __init__(self, m, rp, ci, va, lanes=0, options=None, n=None, kernel=TILE_KERNEL):
        self.m, self.n, self.rp, self.ci = m, m if n is None else n, rp, ci
        self.options = dict(options or {})
        if lanes:
            self.options["lanes_per_row"] = lanes
        self.h = {}
        for pack in (1, 0):
            self.h[pack] = self.create(va, pack)
        self.L = self.h[1].info()["lanes_per_row"]
        if kernel is not None:
            assert self.h[1].info()["kernel_name"] == kernel == self.h[0].info()["kernel_name"]
        assert self.h[0].info()["packed_nnz"] == 0

    def create(self, va, pack):
        """a fresh handle over this pattern with the pair's options"""
        api.set_thread_option("pack_values", pack)
        for k, v in self.options.items():
            api.set_thread_option(k, v)
        try:
            return api.Handle(self.m, self.n, self.rp, self.ci, va.copy(), METHOD)
        finally:
            api.clear_thread_options()

    def close(self):
        for h in self.h.values():
            h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def update(self, va):
        for h in self.h.values():
            h.update_values(va.copy())

    def same_bits(self, x):
        y1 = self.h[1].spmv(x, np.full(self.m, np.nan))
        y0 = self.h[0].spmv(x, np.full(self.m, np.nan))
        assert y1.tobytes() == y0.tobytes(), f"{int((y1.view(np.uint64) != y0.view(np.uint64)).sum())} rows differ in their bits"
        return y1

    def check(self, va, x):
        """bits equal, packed_nnz = the model's; -> the model's per-tile flags"""
        want, flags = model_packed(self.rp, va, self.L)
        self.same_bits(x)
        assert self.h[1].info()["packed_nnz"] == want, (self.h[1].info()["packed_nnz"], want, flags)
        return want, flags


# ------------------------------------------------------------------------------------------------ the cases of test_gpu_packed_forms.py
# lanes: lanes_per_row to force; stride: probe_readback's; flags: which 256-row tiles the gate must pack
Case = namedtuple("Case", "m n rp ci va lanes stride flags")


def _case(m, n, rp, ci, va, lanes, stride, flags=None):
    tiles = (m + TILE - 1) // TILE
    return Case(m, n, rp, ci, va, lanes, stride, [True] * tiles if flags is None else flags)


def form_rows(L, chunks):
    """m for the wrap-around band of `chunks` 4L-entry chunks per row: probe_readback needs m % row length == 0 where rows wrap.  The smallest
    such m >= 1088: four whole tiles and a partial one -- except at 4L = 256, where a multiple of the row length is a whole number of tiles."""
    k = 4 * L * chunks
    return -(-1088 // k) * k


def form_case(L, chunks=1):
    """banded rows of `chunks` aligned 4L-entry chunks (tiles 0 and the last hold wrap-around rows: 16-bit slot tiles; the others are RUN tiles)"""
    k = 4 * L * chunks
    m, rp, ci, va = banded(np.full(form_rows(L, chunks), k), seed=L + chunks)
    return _case(m, m, rp, ci, va, L, k)


def _edges():
    m, rp, ci, _ = banded(np.full(1280, 32))
    return m, rp, ci, edge_values(int(rp[-1]), rp)


def _fixture_edges():
    m, rp, ci, va = _edges()
    return _case(m, m, rp, ci, va, 8, 32)


def _fixture_edges_twin():
    """edge_values with ONE 2^15 in tile 2: that tile's span is 55"""
    m, rp, ci, va = _edges()
    va[rp[2 * TILE + 100] + 5] = 2.0 ** 15
    return _case(m, m, rp, ci, va, 8, 32, [True, True, False, True, True])


def _fixture_exotic():
    """tile 0 edge values, tile 1 DBL_MAX and odd multiples of 2^971, tile 2 the subnormal grid, tile 3 all zero, tile 4 uniform"""
    m, rp, ci, va = banded(np.full(1280, 32))
    va[:rp[TILE]] = edge_values(int(rp[-1]), rp)[:rp[TILE]]
    va[rp[TILE]:rp[2 * TILE]] = dblmax_values(TILE * 32)
    va[rp[2 * TILE]:rp[3 * TILE]] = subnormal_values(TILE * 32)
    va[rp[3 * TILE]:rp[4 * TILE]] = 0.0
    return _case(m, m, rp, ci, va, 8, 32)


def _fixture_empty_rows():
    """m = 1056 (the last wave holds 32 rows); empty: tile 1's first and last row, and rows 600 .. 669 (across the wave boundary at 640)"""
    lens = np.full(1056, 32)
    lens[[256, 511]] = 0
    lens[600:670] = 0
    m, rp, ci, va = banded(lens)
    return _case(m, m, rp, ci, va, 8, 32)


def _fixture_empty_tile():
    lens = np.full(1088, 32)
    lens[512:768] = 0
    m, rp, ci, va = banded(lens)
    return _case(m, m, rp, ci, va, 8, 32)


def _fixture_long_row():
    """row 300 (tile 1) holds 16 * 32 + 32 = 544 entries > long_thr = 512 at L = 8: tile 1 alone does not pack"""
    lens = np.full(1280, 32)
    lens[300] = 544
    m, n, rp, ci, va = open_band(lens)
    return _case(m, n, rp, ci, va, 8, 544, [True, False, True, True, True])


def _fixture_run():
    m, n, rp, ci, va = open_band(np.full(1088, 32))
    return _case(m, n, rp, ci, va, 8, 32)


def _fixture_scatter3():
    """96 bands 1024 columns apart, three chunks per row at L = 8; 1024 = 54 mod 97, so i + 1024 j, j < 96, are distinct modulo 97"""
    m, n, rp, ci, va = scattered_rows(1088, 96, 1024)
    return _case(m, n, rp, ci, va, 8, 97)


def _fixture_byte(k, window):
    def make():
        m, n, rp, ci, va = sparse_rows(1088, 1088 + window, np.full(1088, k), window, seed=k)
        return _case(m, n, rp, ci, va, 8, window)
    return make


def _fixture_tmpl(k):
    def make():
        offsets = np.sort(np.random.default_rng(k).permutation(128)[:k])
        m, n, rp, ci, va = pattern_rows(1088, 1088 + 128, offsets, seed=k)
        return _case(m, n, rp, ci, va, 8, 128)
    return make


FIXTURES = {
    "edges": _fixture_edges, "edges_twin": _fixture_edges_twin, "exotic": _fixture_exotic,
    "empty_rows": _fixture_empty_rows, "empty_tile": _fixture_empty_tile, "long_row": _fixture_long_row,
    "run": _fixture_run, "run3": lambda: form_case(8, 3), "scatter3": _fixture_scatter3,
    "byte32": _fixture_byte(32, 48), "byte64": _fixture_byte(64, 96),       # byte64: two chunks per row, the BYTE continuation loop
    "tmpl32": _fixture_tmpl(32), "tmpl64": _fixture_tmpl(64),
}
FORM_LANES = [1, 2, 4, 8, 16, 32, 64]
FORM_CASES = [(L, 1) for L in FORM_LANES] + [(2, 3), (8, 3)]


def fixture(name):
    return FIXTURES[name]()
