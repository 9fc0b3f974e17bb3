"""Cases, budgets and a host model for the LDS capacity boundaries of the staged x-window kernels.

Shared by tests/test_xwindow_model.py (CPU: the generator hits the windows it is meant to hit) and tests/test_gpu_lds_edges.py (GPU: the
kernels are exact there).  A test helper, not a conftest: imported by the tests that use it.

The budgets restate shim/inspect.hpp (kVecXTileBytes, kVecWideXTileBytes, kSellXTileBytes, kCsr5XTileBytes, kNatXTileBytes): a retuned
budget has to be retuned here, and the sweeps then move with it.  A form holds max_cols = budget / sizeof(T) - 1 columns (one slot stays
free for the zero slot) and its launch asks for roundup((total + 1) * sizeof(T), 1 KiB) bytes of dynamic LDS, plus SELL's row sums
(sizeof(T) x group x sigma) and the CSR5 / nnz-split waves' row maps (4 waves x stride x 4 bytes, matrices with empty rows).

expected() and the upper-end cases also restate planner heuristics that have nothing to do with LDS sizing and have to be kept in step
by hand when one of them is retuned: build_vector_tiles' wide-by-cost rule, the fp32 two-deep CSR5 group kernel, the 15 % rule by which
SELL's window groups and CSR5's tile groups grow, the automatic CSR5 tile size (sigma = 4 below 2^19 entries) and the row length from
which CSR-vector hands rows to the long-row path.  No option pins them without also switching the inspector's wide attempts off (a forced
form sets plan.forced), so the cases are shaped to land on one side of each rule and the CPU test checks what it can of that."""
import collections

import numpy as np

from spmv_amd import api, synth

M = api.SPMV_METHODS
KIB = 1024
NARROW, WIDE, SELL, CSR5, NAT = 48 * KIB, 96 * KIB, 96 * KIB, 128 * KIB, 96 * KIB
BUDGETS = (48 * KIB, 96 * KIB, 128 * KIB)
SEG, WIN_MAX, BITMAP_WORDS, SIGMA = 64, 16, 1024, 1024           # xwindows.hpp; SELL's default sigma
METHODS = [M.Method_Parallel, M.Method_Balanced, M.Method_SellCSigma, M.Method_CSR5SPMV, M.Method_Balanced_Yid, M.Method_Balanced2]
DTYPES = {"f64": np.float64, "f32": np.float32}

Case = collections.namedtuple("Case", "name dt m n bands k fill empty_every")


def size_of(dt):
    return np.dtype(DTYPES[dt]).itemsize


def cap(budget, dt):
    """max_cols of a form with this budget."""
    return budget // size_of(dt) - 1


def xbytes(total, dt):
    """The launchers' request for a staged total: the windows + the zero slot, in whole KiB."""
    return ((total + 1) * size_of(dt) + KIB - 1) // KIB * KIB


def matrix(case):
    return synth.span_rows(case.m, case.n, case.bands, case.k, case.fill, case.empty_every, DTYPES[case.dt])


# ----------------------------------------------------------------------------- the window rule, twice
def model_windows(cols, n, max_cols):
    """numpy restatement of build_windows (kernels/xwindows.hpp) for one tile's columns -> (nwin, total); (0, 0) = not staged."""
    cols = np.asarray(cols, dtype=np.int64)
    cols = cols[cols >= 0]
    if cols.size == 0:
        return 0, 0
    mn, mx = int(cols.min()), int(cols.max())
    span = mx - mn + 1
    if span <= max_cols:                                                     # the plain span: one window
        return 1, span
    nseg = (mx >> 6) - (mn >> 6) + 1
    if (nseg + 31) // 32 > BITMAP_WORDS:                                     # spans above 32768 segments are not analysed
        return 0, 0
    segs = np.unique(cols >> 6)
    cut = np.diff(segs) > 1
    first, last = segs[np.r_[True, cut]], segs[np.r_[cut, True]]             # runs of touched 64-column segments
    if first.size > WIN_MAX or segs.size * SEG > max_cols:
        return 0, 0
    return int(first.size), int((np.minimum((last + 1) * SEG, n) - first * SEG).sum())


def intended_windows(case, max_cols):
    """(nwin, total) every tile of the case is meant to have, from the case's DESCRIPTION (bands, n), not from its matrix."""
    lo, hi = case.bands[0][0], case.bands[-1][0] + case.bands[-1][1] - 1
    if hi - lo + 1 <= max_cols:
        return 1, hi - lo + 1
    if ((hi >> 6) - (lo >> 6) + 1 + 31) // 32 > BITMAP_WORDS:
        return 0, 0
    if case.fill != "segments":                                               # a plain span over a budget is used with "segments" only
        raise AssertionError(("over-budget case without the segments fill", case.name))
    segs = [(a >> 6, (a + w - 1) >> 6) for a, w in case.bands]
    assert all(e + 1 < s for (_, e), (s, _) in zip(segs, segs[1:])), ("bands must not share or adjoin segments", case.name)
    bits = sum(e - s + 1 for s, e in segs)
    if len(segs) > WIN_MAX or bits * SEG > max_cols:
        return 0, 0
    return len(segs), sum(min((e + 1) * SEG, case.n) - s * SEG for s, e in segs)


# ----------------------------------------------------------------------------- which form runs
def _c5_kernel(dt):
    return "csr5_group_pipe_kernel" if dt == "f32" else "csr5_group_kernel"   # every group staged: fp32 runs two tiles deep


def expected(method, case, nnz):
    """What create() must settle on for a matrix all of whose tiles hold intended_windows: the first form of the method whose budget
    holds them -> dict(kernel, staged, nwin, span, xbytes); staged = False: the method's global-column kernel."""
    dt, s = case.dt, size_of(case.dt)
    if method == M.Method_Parallel:
        forms = [("csr_vector_tile_kernel", NARROW), ("csr_vector_rows_kernel", WIDE)]
        fallback = "csr_vector_pipe_kernel"
    elif method in (M.Method_Balanced, M.Method_Balanced2):
        forms = [("csr_vector_rows_kernel", NARROW), ("csr_vector_rows_kernel", WIDE)]
        fallback = "csr_vector_rows_kernel"
    elif method == M.Method_SellCSigma:
        forms, fallback = [("sell_window_kernel", SELL)], "sell_kernel"
    elif method == M.Method_CSR5SPMV:
        forms, fallback = [(_c5_kernel(dt), CSR5)], "csr5_kernel"
    else:
        forms, fallback = [("nat_group_kernel", NAT)], "nat_kernel"
    hits = [(kern, b) + intended_windows(case, cap(b, dt)) for kern, b in forms]
    hits = [h for h in hits if h[2] > 0]
    if method == M.Method_Parallel and len(hits) == 2:
        # build_vector_tiles: narrow tiles whose windows cost more than half of the bytes they stream give way to 1024-row blocks of the
        # wide form (a quarter of the window traffic here: every tile has the same windows)
        tiles = (case.m + 255) // 256
        if hits[0][3] * s * tiles > 0.5 * nnz * (s + 2):
            hits = hits[1:]
    if not hits:
        return dict(kernel=fallback, staged=False, nwin=0, span=0, xbytes=0, budget=0)
    kern, b, nwin, total = hits[0]
    return dict(kernel=kern, staged=True, nwin=nwin, span=total, xbytes=xbytes(total, dt), budget=b)


# ----------------------------------------------------------------------------- the cases
# 8 tiles of 256 rows, 2 sigma windows, 8 CSR5 groups of 64 tiles.  64 entries per row: enough for Method_Parallel's narrow tiles to stay narrow at
# their cap (their windows then cost just under half of what they stream), and still one step of a 16-lane group (longer rows would leave for the long-row path)
ROWS, K = 2048, 64
OFF = 5                # first staged column: x[OFF - 1] and x[OFF + S] exist and are the window's neighbours


def _span_case(name, dt, S, k=K, m=ROWS, empty_every=0):
    """One band of S columns.  Up to the smallest budget any fill will do (the plain span stages everywhere): "spread".  Above it some
    form has to turn the span down, and must not be rescued by the several-window path: "segments" (every segment touched)."""
    return Case(name, dt, m, OFF + S + 11, ((OFF, S),), k, "spread" if S <= cap(NARROW, dt) else "segments", empty_every)


def budget_edge_cases():
    """S = max_cols - 1, max_cols (the plain span: staged) and max_cols + 1 (every segment touched: no form of this budget can stage it)."""
    out = []
    for dt in DTYPES:
        for b in BUDGETS:
            c = cap(b, dt)
            out += [_span_case(f"{dt}-{b // KIB}K-below", dt, c - 1), _span_case(f"{dt}-{b // KIB}K-at", dt, c),
                    _span_case(f"{dt}-{b // KIB}K-over", dt, c + 1)]
    return out


LINE_KIB = range(56, 69)


def line_cases():
    """(case, family, lds target): lds_bytes takes every whole KiB from 56 through 68.  family "x": the forms whose request is the
    windows alone (wide rows form, CSR5, nnz-split groups); "sell": the windows + one sigma window's row sums (80 entries per row keep
    the window groups at one sigma window: staging then costs under 15 % of the group's stream)."""
    out = []
    for dt in DTYPES:
        s = size_of(dt)
        for t in LINE_KIB:
            out.append((_span_case(f"{dt}-x-{t}K", dt, t * KIB // s - 1), "x", t * KIB))
            out.append((_span_case(f"{dt}-sell-{t}K", dt, (t * KIB - s * SIGMA) // s - 1, k=80), "sell", t * KIB))
    return out


def multi_window_cases():
    out = []
    gap = 4096
    for dt in DTYPES:
        for w in (15, 16, 17):                                              # W bands of two segments each: staged, staged, not staged
            bands = tuple((SEG + i * gap, 2 * SEG) for i in range(w))
            out.append(Case(f"{dt}-{w}bands", dt, ROWS, w * gap + 100, bands, K, "segments", 0))
        for b in BUDGETS:                                                   # total = max_cols rounded down to whole segments, and 64 more
            segs = cap(b, dt) // SEG
            for extra, tag in ((0, "full"), (1, "plus64")):
                a = segs // 2
                far = 40000 // SEG * SEG + a * SEG                          # the bands' span exceeds every budget
                bands = ((0, a * SEG), (far, (segs - a + extra) * SEG))
                out.append(Case(f"{dt}-{b // KIB}K-{tag}", dt, ROWS, far + (segs + 2) * SEG, bands, K, "segments", 0))
        # the last band ends at n, 37 columns into its last segment
        bands = ((3 * SEG, 4 * SEG), (50000 // SEG * SEG, 3 * SEG), (90000 // SEG * SEG, 2 * SEG + 37))
        out.append(Case(f"{dt}-clipped", dt, ROWS, bands[-1][0] + bands[-1][1], bands, K, "segments", 0))
        for nseg, tag in ((32768, "32768seg"), (32769, "32769seg")):        # the bitmap's limit: analysed, not analysed
            bands = ((0, 8 * SEG), ((nseg - 8) * SEG, 8 * SEG))
            out.append(Case(f"{dt}-{tag}", dt, ROWS, nseg * SEG + 3, bands, 16, "segments", 0))
    return out


# ----------------------------------------------------------------------------- nnz-split groups: full-size or half-size tile buffers
NAT_SIGMA = 4                                                               # build_csr5: the automatic tile size below 2^19 entries (64 x 4 entries)
NAT_SWITCH = 76 * KIB                                                       # launch_csr5_form: above this, two workgroups no longer fit a CU


def nat_tile_buffers(dt, sigma=NAT_SIGMA):
    """Static LDS of nat_group_kernel's full form: per wave 64 lane rows of sigma values + 16 bytes and sigma 16-bit slots + 4 bytes (NatLds)."""
    return 4 * 64 * ((sigma * size_of(dt) + 16) + (sigma * 2 + 4))


def nat_half_from_kib(dt, row_maps=0):
    """The smallest whole-KiB window request that launch_csr5_form hands over in halves: request + row maps + full buffers > 76 KiB."""
    return (NAT_SWITCH - nat_tile_buffers(dt) - row_maps) // KIB + 1


def upper_end_cases():
    """The largest requests: CSR5 at 128 KiB with the waves' row maps at sigma = 16 (16-entry rows: 64 row starts per 1024-entry tile,
    stride 17 x 64 ints, 17 KiB), SELL at its cap with short rows (the window groups grow to what lds_fits allows), the nnz-split groups
    at their cap with row maps (4-entry rows: 64 row starts per 256-entry tile, stride 5 x 64 ints, 5 KiB)."""
    out = []
    for dt in DTYPES:
        out.append(_span_case(f"{dt}-csr5-mapped", dt, cap(CSR5, dt), k=16, m=24576, empty_every=4))
        out.append(_span_case(f"{dt}-sell-groups", dt, cap(SELL, dt), k=8, m=16384))
        out.append(_span_case(f"{dt}-nat-mapped", dt, cap(NAT, dt), k=4, m=16384, empty_every=4))
    return out


def all_cases():
    return budget_edge_cases() + [c for c, _, _ in line_cases()] + multi_window_cases() + upper_end_cases()
