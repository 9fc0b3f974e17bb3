"""What the three grouped-query attention GPU test files share: the patterns and shapes of test_gpu_attention_heads_backward.py restated, the
operands at the grouped widths, and the oracles -- the single-head bias calls on column slices, K and V expanded by numpy indexing for the
existing multi-head calls, and the left-to-right sum of the per-head dK / dV terms in the handle's dtype (include/spmv_hip.h)."""
import numpy as np

from spmv_amd import api, synth

M = api.SPMV_METHODS
METHODS = [M.Method_Parallel, M.Method_Balanced, M.Method_Balanced_Yid, M.Method_CSR5SPMV, M.Method_SellCSigma]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
E_ARG, E_NOSTATE = 3, 5
DEV = "cuda:0"
CANARY = -7.25
N = 300
LENGTHS = [0, 1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64, 65, 511, 512, 513, 575, 576, 577, 1025, 2047, 2048, 2049, 4097, 5000]
GOLDENS = ["rowlen_sweep", "single_long", "powerlaw", "empty_mix", "nnz0", "tiny"]
COMBOS = [(1, 1), (2, 1), (3, 3), (4, 2), (6, 2), (4, 1)]   # (heads, kv_heads): groups of 1, 2, 1, 2, 3 and 4
COMBO_IDS = [f"{h}over{g}" for h, g in COMBOS]
BIASES = ["none", "planes", "shared"]
OPTION = "attention_backward_heads"


def shapes(dtype):
    """(k, dv) of one head: width 1, an odd width that forces element access, a head wider than a panel in each role"""
    W, KP = (2, 16) if np.dtype(dtype) == np.float64 else (4, 32)
    return [(1, 1), (W + 1, 16 // np.dtype(dtype).itemsize), (8 * W + 1, KP + 1), (KP, 2)]


_PAT = {}


def pattern_a(dtype):
    """the rows LENGTHS in a shuffled order, with runs of empty rows at the start, in the middle and at the end; columns in [0, N).  Built
    once per dtype, shared, never changed."""
    key = ("a", np.dtype(dtype))
    if key not in _PAT:
        rng = np.random.default_rng(11)
        order = rng.permutation(len(LENGTHS))
        lens = [0] * 5
        for pos, i in enumerate(order):
            if pos == len(order) // 2:
                lens += [0] * 70   # more empty rows than a wave looks at in one step
            lens.append(LENGTHS[i])
        lens += [0] * 6
        rp = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(lens, out=rp[1:])
        nnz = int(rp[-1])
        ci = rng.integers(0, N, nnz).astype(np.int32)
        _PAT[key] = synth.CSR(len(lens), N, rp, ci, rng.uniform(-1, 1, nnz).astype(dtype))
        assert set(np.diff(rp).tolist()) == set(LENGTHS)
    return _PAT[key]


def pattern_b(dtype):
    """pattern A transposed on the host (a stable sort by column): the COLUMNS have the lengths LENGTHS, with the runs of empty columns"""
    key = ("b", np.dtype(dtype))
    if key not in _PAT:
        a = pattern_a(dtype)
        rows = np.repeat(np.arange(a.m, dtype=np.int32), np.diff(a.rowptr))
        order = np.argsort(a.colidx, kind="stable")
        rp = np.zeros(a.n + 1, dtype=np.int32)
        np.cumsum(np.bincount(a.colidx, minlength=a.n), out=rp[1:])
        _PAT[key] = synth.CSR(a.n, a.m, rp, rows[order].copy(), a.val[order].copy())
        assert set(np.bincount(_PAT[key].colidx, minlength=a.m).tolist()) == set(LENGTHS)
    return _PAT[key]


PATTERNS = {"rows": pattern_a, "cols": pattern_b}


def operands(csr, heads, kv, k, dv, seed=0):
    """Q (m x heads*k), K (n x kv*k), V (n x kv*dv), G (m x heads*dv), uniform in [-1, 1]"""
    rng = np.random.default_rng(10000 * heads + 1000 * kv + 100 * k + dv + seed)
    dt = csr.val.dtype
    return tuple(rng.uniform(-1, 1, shape).astype(dt) for shape in ((csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv), (csr.m, heads * dv)))


def bias_of(csr, heads, kind, seed=7):
    """None, (heads, nnz) planes or one shared (nnz,) plane, uniform in [-2, 2]"""
    rng = np.random.default_rng(seed + heads)
    if kind == "none":
        return None
    shape = (heads, csr.nnz) if kind == "planes" else (csr.nnz,)
    return rng.uniform(-2, 2, shape).astype(csr.val.dtype)


def plane(B, hd):
    """head hd's bias plane for a single-head call"""
    return None if B is None else (B if B.ndim == 1 else B[hd])


def expand(X, heads, kv):
    """K or V as the heads calls want it: block h // (heads // kv) of X at block h -- repeat_interleave by numpy indexing"""
    n, w = X.shape[0], X.shape[1] // kv
    return np.ascontiguousarray(X.reshape(n, kv, w)[:, np.arange(heads) // (heads // kv), :].reshape(n, heads * w))


def handle(csr, method=M.Method_Parallel, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method)
    finally:
        api.clear_thread_options()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def all_same(got, want):
    return all((g is None and w is None) or (g is not None and w is not None and same_bits(g, w)) for g, w in zip(got, want))


def device_ops(arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


# ----------------------------------------------------------------------------- forward
def gqa_host(h, csr, heads, kv, Q, K, V, B, scale, pad=3):
    """the GQA call through host pointers into a canary-filled O with `pad` elements behind every row and a row behind the last"""
    w = heads * (V.shape[1] // kv)
    buf = np.full((csr.m + 1, w + pad), CANARY, dtype=csr.val.dtype)
    api.attention_gqa(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, B, buf[:csr.m, :w], scale=scale)
    assert (buf[:, w:] == CANARY).all() and (buf[csr.m] == CANARY).all(), "written outside O's elements"
    return buf[:csr.m, :w].copy()


def forward_head_by_head(h, csr, heads, kv, Q, K, V, B, scale):
    """the oracle: api.attention_bias with ONE head per query head on Q + h*k, K + (h/gs)*k, V + (h/gs)*dv, O + h*dv and plane h of B"""
    gs, k, dv = heads // kv, Q.shape[1] // heads, V.shape[1] // kv
    O = np.full((csr.m, heads * dv), CANARY, dtype=csr.val.dtype)
    for hd in range(heads):
        g = hd // gs
        api.attention_bias(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, 1, Q[:, hd * k:(hd + 1) * k], K[:, g * k:(g + 1) * k], V[:, g * dv:(g + 1) * dv],
                           plane(B, hd), O[:, hd * dv:(hd + 1) * dv], scale=scale)
    return O


# ----------------------------------------------------------------------------- backward
def out_shapes(csr, heads, Q, K, V):
    return (csr.m, Q.shape[1]), (csr.n, K.shape[1]), (csr.n, V.shape[1]), (heads, csr.nnz)


def gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, scale, need=(True, True, True, True), pad=3):
    """the GQA backward through host pointers, into canary-filled outputs with `pad` extra elements behind every row / plane and a row behind the
    last; -> (dQ, dK, dV, dB)"""
    shp = out_shapes(csr, heads, Q, K, V)
    bufs = [np.full((rows + 1, w + pad), CANARY, dtype=csr.val.dtype) if want else None for want, (rows, w) in zip(need, shp)]
    views = [None if b is None else b[:rows, :w] for b, (rows, w) in zip(bufs, shp)]
    api.attention_gqa_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, B, G, *views, scale=scale)
    for b, v in zip(bufs, views):
        if b is not None:
            assert (b[:, v.shape[1]:] == CANARY).all() and (b[v.shape[0]] == CANARY).all(), "written outside an output's elements"
    return tuple(None if v is None else v.copy() for v in views)


def per_head_terms(h, csr, heads, kv, Q, K, V, B, G, scale):
    """the single-head backward (api.attention_bias_backward, heads = 1) per query head on its slices -> dQ (full), dB (full), and the LISTS of
    the heads' dK and dV terms, each (n, k) / (n, dv)"""
    gs, k, dv = heads // kv, Q.shape[1] // heads, V.shape[1] // kv
    dt = csr.val.dtype
    dQ, dB = np.full((csr.m, heads * k), CANARY, dtype=dt), np.full((heads, csr.nnz), CANARY, dtype=dt)
    tK, tV = [], []
    for hd in range(heads):
        g = hd // gs
        tK.append(np.full((csr.n, k), CANARY, dtype=dt))
        tV.append(np.full((csr.n, dv), CANARY, dtype=dt))
        api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, 1, Q[:, hd * k:(hd + 1) * k], K[:, g * k:(g + 1) * k], V[:, g * dv:(g + 1) * dv],
                                    plane(B, hd), G[:, hd * dv:(hd + 1) * dv], dQ[:, hd * k:(hd + 1) * k], tK[-1], tV[-1], dB[hd:hd + 1], scale=scale)
    return dQ, dB, tK, tV


def chain(terms, order=None):
    """(((t0 + t1) + t2) + ..) in the terms' dtype: the first taken as it is, every other one one plain addition -- an explicit loop"""
    order = range(len(terms)) if order is None else order
    acc = None
    for i in order:
        acc = terms[i].copy() if acc is None else acc + terms[i]
    assert acc.dtype == terms[0].dtype
    return acc


def group_sums(terms, heads, kv, order=None):
    """the groups' chains side by side: (n, kv * w); order: a permutation of range(gs) applied inside every group (None: ascending)"""
    gs = heads // kv
    return np.concatenate([chain(terms[g * gs:(g + 1) * gs], order) for g in range(kv)], axis=1)


def backward_oracle(h, csr, heads, kv, Q, K, V, B, G, scale, need=(True, True, True, True)):
    """-> (dQ, dK, dV, dB) as the contract states them"""
    dQ, dB, tK, tV = per_head_terms(h, csr, heads, kv, Q, K, V, B, G, scale)
    full = (dQ, group_sums(tK, heads, kv), group_sums(tV, heads, kv), dB)
    return tuple(f if n else None for f, n in zip(full, need))
