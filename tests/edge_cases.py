"""What the one-hot / tie tests and the second-grid-trip tests share, on top of gqa_cases and lse_cases.

One-hot rows.  One entry per (row, head) is made dominant by a gap of more than GAP = 800 in t_p; exp is exactly 0 below -104 (fp32) and -746
(fp64), so every other weight is an exact 0, Z is exactly 1, and the contract's arithmetic rounds nowhere: every addition of a +-0 term is exact.
Where the dominant entry sits in its row is taken from position_classes(): the places at which the kernels change lane, register, thread stride
or panel segment (kernels/row_blocks.hpp).  Head hd of a row takes the hd-th of the row's positions (cyclically), so a call with NPOS heads
covers every position of every row.

The second grid trip.  grid_pattern(): more rows AND more columns longer than 512 than the 8 * CUs workgroups the long-row kernels are launched
with, so their `for (i = blockIdx.x; i < nlong; i += gridDim.x)` loops run a second iteration."""
import numpy as np

import gqa_cases as gc
from spmv_amd import synth

G0 = 4096.0     # the bias below the dominant entry's; exact in fp16 and bf16
KDROP = -8192.0  # the staircase's extra K column off the dominant entry
GAP = 800.0
SEGS, LONG, STRIDE = 64, 512, 256   # kSpmmSegs, kSpmmLongThr, the threads of a long row's workgroup


# ----------------------------------------------------------------------------- positions
def position_classes(n):
    """{class: 0-based position} of a row of n entries, only the classes that exist in it (position < n)"""
    c = {"first": 0, "second": 1, "last": n - 1, "63": 63, "64": 64, "65": 65, "255": 255, "256": 256, "511": 511, "512": 512}
    c.update({f"64*{u}": 64 * u for u in range(2, 8)})   # a lane's further registers in the wide pass
    if n > STRIDE:
        c["last stride"] = STRIDE * ((n - 1) // STRIDE)   # the first entry of the last (partial) stride of 256
    if n > LONG:
        seg = -(-n // SEGS)                                # the panel's segment edges
        c.update({"seg-1": seg - 1, "seg": seg, "63*seg": 63 * seg})
    return {name: p for name, p in c.items() if 0 <= p < n}


def position_list(n):
    return sorted(set(position_classes(n).values()))


NPOS = max(len(position_list(n)) for n in gc.LENGTHS)


def dominant(csr, heads, shift=0):
    """(heads, m) CSR indices: head hd of row i dominates at the row's position number (hd + shift) mod (its count); -1 on a row without entries"""
    dom = np.full((heads, csr.m), -1, dtype=np.int64)
    for i, n in enumerate(np.diff(csr.rowptr).tolist()):
        pl = position_list(n)
        for hd in range(heads if pl else 0):
            dom[hd, i] = csr.rowptr[i] + pl[(hd + shift) % len(pl)]
    return dom


def tie_pairs(csr, heads):
    """two (heads, m) index tables a < b: head hd of a row with >= 2 entries ties its positions number hd and hd + 1 (cyclically over the adjacent
    pairs of its position list: a and b lie across every class boundary); a row of one entry has a == b; -1 on a row without entries"""
    a, b = np.full((heads, csr.m), -1, dtype=np.int64), np.full((heads, csr.m), -1, dtype=np.int64)
    for i, n in enumerate(np.diff(csr.rowptr).tolist()):
        pl = position_list(n)
        for hd in range(heads if pl else 0):
            q = hd % max(len(pl) - 1, 1)
            a[hd, i], b[hd, i] = csr.rowptr[i] + pl[q], csr.rowptr[i] + pl[min(q + 1, len(pl) - 1)]
    return a, b


def onehot_bias(csr, *doms):
    """(heads, nnz) planes: 0 at the entries of the tables `doms`, -G0 elsewhere"""
    heads = doms[0].shape[0]
    B = np.full((heads, csr.nnz), -G0, dtype=csr.val.dtype)
    for dom in doms:
        for hd in range(heads):
            B[hd, dom[hd][dom[hd] >= 0]] = 0
    return B


def wide_gap(csr, Q, K, B, scale, dom, wide):
    """the smallest gap, over the rows with entries, between head 0's score at dom and the row's largest other score, from scores in `wide`
    precision (Q: m x k, K: n x k, B: a plane or None, dom: (m,)); inf where a row has no other entry"""
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    t = (Q.astype(wide)[rows] * K.astype(wide)[csr.colidx]).sum(1) * wide(scale)
    if B is not None:
        t = t + B.astype(wide)
    has = dom >= 0
    top = t[dom[has]]
    t[dom[has]] = -np.inf
    starts = csr.rowptr[:-1][np.diff(csr.rowptr) > 0]
    return float((top - np.maximum.reduceat(t, starts)).min())


# ----------------------------------------------------------------------------- the staircase: dominance without a bias
_STAIR = {}


def staircase(dtype):
    """the rows gqa_cases.LENGTHS with disjoint consecutive column ranges: n = nnz, every column in exactly one row"""
    key = np.dtype(dtype)
    if key not in _STAIR:
        rp = np.zeros(len(gc.LENGTHS) + 1, dtype=np.int32)
        np.cumsum(gc.LENGTHS, out=rp[1:])
        nnz = int(rp[-1])
        _STAIR[key] = synth.CSR(len(gc.LENGTHS), nnz, rp, np.arange(nnz, dtype=np.int32), np.ones(nnz, dtype=dtype))
    return _STAIR[key]


def staircase_operands(csr, heads, k, dv, dom):
    """gqa_cases.operands with one extra column per head of Q (1) and K (0 at the head's dominant column of the row that owns the column, KDROP
    elsewhere): Q (m x heads*(k+1)), K (n x heads*(k+1)), V (n x heads*dv), G (m x heads*dv)"""
    Q0, K0, V, G = gc.operands(csr, heads, heads, k, dv)
    dt = csr.val.dtype
    Q, K = np.ones((csr.m, heads * (k + 1)), dtype=dt), np.full((csr.n, heads * (k + 1)), KDROP, dtype=dt)
    for hd in range(heads):
        Q[:, hd * (k + 1):hd * (k + 1) + k] = Q0[:, hd * k:(hd + 1) * k]
        K[:, hd * (k + 1):hd * (k + 1) + k] = K0[:, hd * k:(hd + 1) * k]
        K[csr.colidx[dom[hd][dom[hd] >= 0]], hd * (k + 1) + k] = 0
    return Q, K, V, G


# ----------------------------------------------------------------------------- the exact results
def onehot_o(csr, V, dom, kv, dv):
    """O of one-hot rows: V's row at the dominant column, its K / V block's columns; +0 on a row without entries"""
    heads = dom.shape[0]
    gs = heads // kv
    O = np.zeros((csr.m, heads * dv), dtype=V.dtype)
    for hd in range(heads):
        has = dom[hd] >= 0
        O[has, hd * dv:(hd + 1) * dv] = V[csr.colidx[dom[hd][has]], (hd // gs) * dv:(hd // gs + 1) * dv]
    return O


def onehot_dv(csr, rp_t, perm, dom, G, kv, dv):
    """dV of one-hot rows, plain additions in G's dtype in the contract's order (kernels/row_blocks.hpp, kernels/attention_backward.hpp): per head,
    column j's chain runs over its entries in A^T's order (rp_t, perm: api.transpose_map) from +0 -- a column of more than 512 entries in 64
    equal segments, each a chain from +0, added left to right --; every weight is exactly 1 or 0, so the chain is the sum of G's rows at the
    dominant entries.  The heads of a K / V group are then added in ascending head (gqa_cases.group_sums)."""
    heads = dom.shape[0]
    row_of = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    len_t = np.diff(rp_t)
    col_of = np.repeat(np.arange(csr.n), len_t)
    terms = []
    for hd in range(heads):
        isdom = np.zeros(csr.nnz, dtype=bool)
        isdom[dom[hd][dom[hd] >= 0]] = True
        part = {}   # (column, segment) -> its chain; filled in A^T's order, so a column's segments come out left to right
        for q in np.flatnonzero(isdom[perm]).tolist():
            j = int(col_of[q])
            seg = (q - int(rp_t[j])) // -(-int(len_t[j]) // SEGS) if len_t[j] > LONG else 0
            x = G[row_of[perm[q]], hd * dv:(hd + 1) * dv]
            part[j, seg] = x.copy() if (j, seg) not in part else part[j, seg] + x
        term = np.zeros((csr.n, dv), dtype=G.dtype)
        for (j, _), x in part.items():
            term[j] = term[j] + x
        terms.append(term)
    return gc.group_sums(terms, heads, kv)


# ----------------------------------------------------------------------------- the second grid trip
IRREGULAR = [0, 1, 64, 511, 512, 1025, 2049]
GRID_LEN, GRID_EVERY = 600, 97
_GRID = {}


def grid_lengths(cus):
    n = 8 * cus + 67
    lens = np.full(n, GRID_LEN, dtype=np.int64)
    odd = np.arange(GRID_EVERY - 1, n, GRID_EVERY)
    lens[odd] = [min(IRREGULAR[q % len(IRREGULAR)], n) for q in range(odd.size)]
    return lens


def grid_pattern(dtype, cus):
    """m = n = 8 * cus + 67; row i holds the columns (i + j) mod n, j < len_i; len_i = 600 except every 97th row, which takes the next length of
    IRREGULAR.  Built once per dtype and CU count, shared, never changed."""
    key = (np.dtype(dtype), cus)
    if key not in _GRID:
        lens = grid_lengths(cus)
        n = lens.size
        rp = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(lens, out=rp[1:])
        rows = np.repeat(np.arange(n, dtype=np.int64), lens)
        ci = ((rows + np.arange(int(rp[-1]), dtype=np.int64) - rp[rows]) % n).astype(np.int32)
        _GRID[key] = synth.CSR(n, n, rp, ci, np.random.default_rng(23).uniform(-1, 1, ci.size).astype(dtype))
    return _GRID[key]


def long_counts(csr):
    """(rows, columns) with more than 512 entries"""
    return int((np.diff(csr.rowptr) > LONG).sum()), int((np.bincount(csr.colidx, minlength=csr.n) > LONG).sum())


def cuts(total, most=1024):
    """ascending bounds that cut range(total) into the fewest equal parts of at most `most`; the last one is total"""
    parts = -(-total // most)
    return [total * (q + 1) // parts for q in range(parts)]


def row_slices(csr, most=1024):
    """csr cut by row: -> [(slice as a CSR of its own over the same columns, r0, r1, e0, e1)], rows [r0, r1) and entries [e0, e1) of csr"""
    out, r0 = [], 0
    for r1 in cuts(csr.m, most):
        e0, e1 = int(csr.rowptr[r0]), int(csr.rowptr[r1])
        out.append((synth.CSR(r1 - r0, csr.n, (csr.rowptr[r0:r1 + 1] - e0).astype(np.int32), csr.colidx[e0:e1].copy(), csr.val[e0:e1].copy()), r0, r1, e0, e1))
        r0 = r1
    return out


def keep_rows(csr, rows):
    """csr with every row outside `rows` emptied: -> (the CSR, same m and n; idx, the kept entries' positions in csr's CSR order)"""
    keep = np.zeros(csr.m, dtype=bool)
    keep[rows] = True
    lens = np.where(keep, np.diff(csr.rowptr), 0)
    rp = np.zeros(csr.m + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    idx = np.flatnonzero(np.repeat(keep, np.diff(csr.rowptr)))
    return synth.CSR(csr.m, csr.n, rp, csr.colidx[idx].copy(), csr.val[idx].copy()), idx


def grid_sample(csr, cus):
    """what the second-trip tests hold against the wide reference: two blocks of 32 columns, one of them beyond column 8 * cus, with EVERY row that
    reaches them (so those columns' gradients are complete), and every row of another length than 600 with its two neighbours.
    -> (the columns; the rows to keep, ascending; of those, 32 long rows, half of them with an index in the long-row list >= 8 * cus)"""
    cols = np.r_[100:132, 8 * cus + 12:8 * cus + 44]
    lens = np.diff(csr.rowptr)
    reach = np.zeros(csr.m, dtype=bool)
    reach[np.repeat(np.arange(csr.m), lens)[np.isin(csr.colidx, cols)]] = True
    longs = np.flatnonzero(lens > LONG)   # the long-row list is in ascending row order
    late, early = longs[8 * cus:], longs[:8 * cus]
    picked = np.r_[early[reach[early]][::41][:16], late[reach[late]][:16]]
    odd = np.flatnonzero(lens != GRID_LEN)
    reach[np.clip(np.r_[odd - 1, odd, odd + 1], 0, csr.m - 1)] = True
    return cols, np.flatnonzero(reach), picked
