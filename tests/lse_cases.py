"""What the log-sum-exp attention test files share, on top of gqa_cases: pattern A cut into parts by column, the calls through canary-filled
host buffers, the high-precision row-by-row reference of attention and its gradients over a pattern, and the error measure of the value tests."""
import numpy as np

import gqa_cases as gc
from spmv_amd import api, synth

CANARY = gc.CANARY
_PARTS = {}


def split(csr, bounds):
    """csr cut by column at `bounds` (ascending, the last one n): -> [(part, idx)], part r the entries with bounds[r-1] <= column < bounds[r],
    columns renumbered from 0, rows and the order inside a row kept; idx: the entries' positions in csr's CSR order"""
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    out, lo = [], 0
    for hi in bounds:
        idx = np.flatnonzero((csr.colidx >= lo) & (csr.colidx < hi))
        rp = np.zeros(csr.m + 1, dtype=np.int32)
        np.cumsum(np.bincount(rows[idx], minlength=csr.m), out=rp[1:])
        out.append((synth.CSR(csr.m, hi - lo, rp, (csr.colidx[idx] - lo).astype(np.int32), csr.val[idx].copy()), idx))
        lo = hi
    assert sum(p.nnz for p, _ in out) == csr.nnz
    return out


def parts_a(dtype, nparts):
    """pattern A in two parts (columns < 150 and the rest: rows of length 1 are empty in one part, the 5000-row is long in both) or three
    (100 / 100 / 100); built once per dtype, shared, never changed.  -> (csr, [(part, idx)], bounds)"""
    key = (np.dtype(dtype), nparts)
    if key not in _PARTS:
        a = gc.pattern_a(dtype)
        bounds = [150, gc.N] if nparts == 2 else [100, 200, gc.N]
        _PARTS[key] = (a, split(a, bounds), bounds)
    return _PARTS[key]


def part_bias(B, idx):
    """the part's bias: B's entries at the part's positions"""
    return None if B is None else np.ascontiguousarray(B[..., idx])


def rows_of(X, bounds, r):
    lo = 0 if r == 0 else bounds[r - 1]
    return np.ascontiguousarray(X[lo:bounds[r]])


# ----------------------------------------------------------------------------- the calls, through canary-filled host buffers
def lse_host(h, csr, heads, kv, Q, K, V, B, scale, pad=3, want_l=True):
    """spmv_hip_attention_gqa_lse through host pointers: O with `pad` elements behind every row and a row behind the last, L with `pad` elements
    behind every plane and a plane behind the last; -> (O, L)"""
    dt = csr.val.dtype
    w = heads * (V.shape[1] // kv)
    ob = np.full((csr.m + 1, w + pad), CANARY, dtype=dt)
    lb = np.full((heads + 1, csr.m + pad), CANARY, dtype=dt)
    api.attention_gqa_lse(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, B, ob[:csr.m, :w], lb[:heads, :csr.m] if want_l else None, scale=scale)
    assert (ob[:, w:] == CANARY).all() and (ob[csr.m] == CANARY).all(), "written outside O's elements"
    assert (lb[:, csr.m:] == CANARY).all() and (lb[heads] == CANARY).all(), "written outside L's elements"
    if not want_l:
        assert (lb == CANARY).all()
    return ob[:csr.m, :w].copy(), (lb[:heads, :csr.m].copy() if want_l else None)


def merge_host(h, m, heads, O1, L1, O2, L2, pad=3, want_l=True):
    """spmv_hip_attention_merge through host pointers into canary-filled outputs; -> (O, L)"""
    dt = next(a.dtype for a in (O1, L1, O2, L2) if isinstance(a, np.ndarray))   # the others may be device tensors
    w = O1.shape[1]
    ob = np.full((m + 1, w + pad), CANARY, dtype=dt)
    lb = np.full((heads + 1, m + pad), CANARY, dtype=dt)
    api.attention_merge(h.h, heads, O1, L1, O2, L2, ob[:m, :w], lb[:heads, :m] if want_l else None)
    assert (ob[:, w:] == CANARY).all() and (ob[m] == CANARY).all(), "written outside O's elements"
    assert (lb[:, m:] == CANARY).all() and (lb[heads] == CANARY).all(), "written outside L's elements"
    if not want_l:
        assert (lb == CANARY).all()
    return ob[:m, :w].copy(), (lb[:heads, :m].copy() if want_l else None)


def bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, scale, need=(True, True, True, True), pad=3):
    """spmv_hip_attention_gqa_backward_lse through host pointers into canary-filled outputs (gqa_cases.gqa_bwd_host's layout); -> (dQ, dK, dV, dB)"""
    shp = gc.out_shapes(csr, heads, Q, K, V)
    bufs = [np.full((rows + 1, w + pad), CANARY, dtype=csr.val.dtype) if want else None for want, (rows, w) in zip(need, shp)]
    views = [None if b is None else b[:rows, :w] for b, (rows, w) in zip(bufs, shp)]
    api.attention_gqa_backward_lse(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, B, G, O, L, *views, scale=scale)
    for b, v in zip(bufs, views):
        if b is not None:
            assert (b[:, v.shape[1]:] == CANARY).all() and (b[v.shape[0]] == CANARY).all(), "written outside an output's elements"
    return tuple(None if v is None else v.copy() for v in views)


def fold(hs, parts, bounds, heads, kv, Q, K, V, B, scale):
    """one attention_gqa_lse per part, folded left to right with attention_merge (host pointers); -> (O, L)"""
    O = L = None
    for r, ((p, idx), h) in enumerate(zip(parts, hs)):
        Or, Lr = lse_host(h, p, heads, kv, Q, rows_of(K, bounds, r), rows_of(V, bounds, r), part_bias(B, idx), scale)
        O, L = (Or, Lr) if r == 0 else merge_host(hs[0], p.m, heads, O, L, Or, Lr)
    return O, L


# ----------------------------------------------------------------------------- the high-precision reference
def hp(dtype):
    """float64 for fp32 handles, np.longdouble for fp64"""
    return np.float64 if np.dtype(dtype) == np.float32 else np.longdouble


def reference(csr, heads, kv, Q, K, V, B, scale, G=None):
    """row by row in hp(): -> (O, L) or, with G, (O, L, dQ, dK, dV, dB).  Rows without entries: O = 0, L = -inf, no gradient."""
    T = hp(csr.val.dtype)
    gs, k, dv = heads // kv, Q.shape[1] // heads, V.shape[1] // kv
    Qh, Kh, Vh = Q.astype(T), K.astype(T), V.astype(T)
    O, L = np.zeros((csr.m, heads * dv), dtype=T), np.full((heads, csr.m), -np.inf, dtype=T)
    if G is not None:
        Gh = G.astype(T)
        dQ, dK, dV, dB = np.zeros(Q.shape, dtype=T), np.zeros(K.shape, dtype=T), np.zeros(V.shape, dtype=T), np.zeros((heads, csr.nnz), dtype=T)
    sc = T(scale)
    for i in range(csr.m):
        s, e = int(csr.rowptr[i]), int(csr.rowptr[i + 1])
        if s == e:
            continue
        cols = csr.colidx[s:e]
        for hd in range(heads):
            g = hd // gs
            Kr, Vr = Kh[cols, g * k:(g + 1) * k], Vh[cols, g * dv:(g + 1) * dv]
            t = (Kr @ Qh[i, hd * k:(hd + 1) * k]) * sc
            if B is not None:
                t = t + (B[s:e] if B.ndim == 1 else B[hd, s:e]).astype(T)
            mx = t.max()
            ex = np.exp(t - mx)
            z = ex.sum()
            P = ex / z
            L[hd, i] = mx + np.log(z)
            O[i, hd * dv:(hd + 1) * dv] = P @ Vr
            if G is not None:
                gi = Gh[i, hd * dv:(hd + 1) * dv]
                dP = Vr @ gi
                db = P * (dP - (P * dP).sum())
                dB[hd, s:e] = db
                ds = db * sc
                dQ[i, hd * k:(hd + 1) * k] = ds @ Kr
                np.add.at(dK[:, g * k:(g + 1) * k], cols, np.outer(ds, Qh[i, hd * k:(hd + 1) * k]))
                np.add.at(dV[:, g * dv:(g + 1) * dv], cols, np.outer(P, gi))
    return (O, L) if G is None else (O, L, dQ, dK, dV, dB)


def err(got, ref):
    """max |got - ref| over the finite elements of ref, in ref's precision (the infinite ones must agree exactly)"""
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin].astype(ref.dtype), ref[~fin])
    return float(np.max(np.abs(got[fin].astype(ref.dtype) - ref[fin]))) if fin.any() else 0.0


# ----------------------------------------------------------------------------- the value of L: reference, derived bound, the order restated
# The bound of test_gpu_attention_lse.py, |L - L_ref| <= (a(len) + c(len)) * eps * max(1, |L_ref|), L_ref the log-sum-exp in np.longdouble of the
# SAME t_p the kernel holds (api.sddmm, * scale, + B in the handle's dtype: the kernel's bits by contract).  Derivation, first order in eps, with
# M = max t exact in any order, e_p = exp(t_p - M), Z = sum e_p >= 1, w_p = e_p / Z:
#   sums         a(len) additions lie on the longest path of the documented order (kernels/row_blocks.hpp): for len <= 512, W = row_width(len)
#                chains of ceil(len / W) terms and a tree of log2 W levels: ceil(len / W) - 1 + log2 W; for longer rows 256 chains, a tree of 6
#                levels per wave and 2 levels over the four waves: ceil(len / 256) - 1 + 6 + 2.  Each is charged a full eps of Z (the rounding is
#                eps / 2; the slack pays the second-order terms).
#   subtraction  t_p - M is rounded by eps / 2 * |t_p - M|, which changes e_p by that relative amount: in Z, eps / 2 * sum w_p |t_p - M|, and
#                sum w_p (M - t_p) = H(w) - log Z <= ln(len) (H the entropy of w): ln(len) / 2.
#   exp, log     the installed ROCm ships no accuracy table for its device math library (no document under its share/doc names an ulp bound);
#                the library (OCML) is built to the OpenCL C specification's table "Relative error as ULPs", which gives exp and log <= 3 ulp
#                in single and double precision, and HIP's published table (HIP programming guide, "HIP math API") is not above it.  exp: 3 of Z.
#                log: 3 ulp of log Z, and 0 <= log Z <= ln(len): 3 * max(1, ln(len)), against max(1, |L_ref|) >= 1.
#   addition     M + log Z: 1 / 2, relative to |L|.
# A relative error d of Z moves log Z by d, absolutely: every term above is an absolute error of L in units of eps * max(1, |L_ref|).
EXP_ULP = LOG_ULP = 3


def a_len(n):
    """additions on the longest path of the row softmax's sum over n terms"""
    if n <= 512:
        W = 1 if n <= 1 else min(64, 1 << int(n - 1).bit_length())
        return max(0, -(-n // W) - 1) + W.bit_length() - 1
    return -(-n // 256) - 1 + 6 + 2


def c_len(n):
    ln = float(np.log(max(n, 1)))
    return ln / 2 + EXP_ULP + LOG_ULP * max(1.0, ln) + 0.5


def l_bound(n, l_ref, dtype):
    return (a_len(n) + c_len(n)) * float(np.finfo(dtype).eps) * max(1.0, abs(float(l_ref)))


def scores(h, csr, Q, K, B, scale):
    """t_p of one head in the handle's dtype, from the existing calls: api.sddmm, then * scale and + B in numpy (two roundings)"""
    dt = csr.val.dtype
    s = np.empty(csr.nnz, dtype=dt)
    api.sddmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, np.ascontiguousarray(Q), np.ascontiguousarray(K), s)
    t = s * dt.type(scale)
    return t if B is None else t + B


def l_reference(csr, t):
    """log-sum-exp of every row of t in np.longdouble (-inf for a row without entries)"""
    out = np.full(csr.m, -np.inf, dtype=np.longdouble)
    for i in range(csr.m):
        r = t[csr.rowptr[i]:csr.rowptr[i + 1]].astype(np.longdouble)
        if r.size:
            mx = r.max()
            out[i] = mx + np.log(np.exp(r - mx).sum())
    return out


def _tree(v):
    """row_group_reduce's sum over a power-of-two number of chains: neighbours first"""
    while v.size > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def lse_restated(r):
    """M + log(Z) of one row r (>= 1 terms) in r's dtype, in the documented order of the row softmax, numpy's exp and log in place of the device's"""
    dt = r.dtype.type
    n, M = r.size, r.max()
    e = np.exp(r - M)
    assert e.dtype == r.dtype
    W = 256 if n > 512 else (1 if n <= 1 else min(64, 1 << int(n - 1).bit_length()))
    chains = np.full(W, dt(-0.0))
    for c in range(W):
        terms = e[c::W]
        if terms.size:
            acc = terms[0]
            for x in terms[1:]:
                acc = dt(acc + x)
            chains[c] = acc
    if n > 512:
        w = [_tree(chains[i * 64:(i + 1) * 64]) for i in range(4)]
        Z = dt(dt(w[0] + w[1]) + dt(w[2] + w[3]))
    else:
        Z = _tree(chains)
    return dt(M + np.log(Z))
