"""The host model of spmv_hip_cg and the matrices its tests share (tests/test_cg_host.py, tests/test_gpu_cg.py).

`dot` and `cg` restate the arithmetic contract of include/spmv_hip.h in numpy -- the order of a dot, the roundings of alpha and beta, the order
of the vector updates -- so that a solve can be compared BIT FOR BIT.  The multiply is a callback: on the GPU it is Handle.spmv (the model
then has spmv()'s bits), on the CPU a plain CSR product (`matvec`)."""
import numpy as np

from spmv_amd import synth

CONVERGED, MAX_ITERATIONS, BREAKDOWN, NONFINITE = 0, 1, 2, 3


# ----------------------------------------------------------------------------- the dot
def geometry(m):
    """-> (P workgroups, L elements per workgroup) of a dot over m >= 1 elements"""
    P = min(1024, -(-m // 1024))
    return P, 1024 * -(-m // (1024 * P))


def _pairs(v):
    """the adjacent-pair binary tree over the last axis (a power of two)"""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _workgroup(t):
    """256 thread sums (last axis) -> the workgroup's sum: the wave tree, then (w0 + w1) + (w2 + w3)"""
    w = _pairs(t.reshape(t.shape[:-1] + (4, 64)))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _slots(a):
    """four slots (last axis) -> (a0 + a1) + (a2 + a3)"""
    return (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])


def dot(a, b):
    """<a, b> in the order of the contract, as a Python float (fp64)"""
    m = a.size
    if m == 0:
        return 0.0
    P, L = geometry(m)
    prod = np.zeros(P * L, dtype=np.float64)          # absent elements add +0.0
    with np.errstate(all="ignore"):
        prod[:m] = a.astype(np.float64) * b.astype(np.float64)
        prod = prod.reshape(P, L // 1024, 256, 4)     # workgroup, step, thread, slot
        acc = np.zeros((P, 256, 4), dtype=np.float64)
        for s in range(L // 1024):                    # ascending step
            acc = acc + prod[:, s]
        part = np.zeros(1024, dtype=np.float64)       # the P partials padded with +0.0
        part[:P] = _workgroup(_slots(acc))
        return float(_workgroup(_slots(part.reshape(256, 4))))


# ----------------------------------------------------------------------------- the loop
def cg(multiply, b, x0=None, dinv=None, rtol=0.0, atol=0.0, max_iterations=0, watch=None):
    """Preconditioned CG as spmv_hip_cg runs it.  multiply(p) -> A p in b's dtype.  -> dict: x, status, iterations, rr, bb, history (rr after
    iteration 0 .. iterations), iterates (x after iteration 0 .. iterations: what a run with a smaller max_iterations returns) and end: the
    kernel and the test that ended the loop ("direction:converged", ...; "budget" when none did).  watch(*values), when given, sees every
    vector and every scalar of type T as it is formed."""
    T = b.dtype.type
    m = b.size
    if m == 0:
        return dict(x=b.copy(), status=CONVERGED, iterations=0, rr=0.0, bb=0.0, history=np.zeros(0), iterates=[], end="begin:empty")
    fin = np.isfinite
    see = watch if watch is not None else (lambda *values: None)
    with np.errstate(all="ignore"):
        if x0 is None:
            x, r = np.zeros_like(b), b.copy()
        else:
            x = x0.copy()
            r = b - multiply(x)
        z = dinv * r if dinv is not None else r.copy()
        p = z.copy()
        see(b, x, r, z) if dinv is None else see(b, x, r, z, dinv)
        rz, rr, bb = dot(r, z), dot(r, r), dot(b, b)
        thresh = max(rtol * rtol * bb, atol * atol)
        status, end = None, "budget"
        if not (fin(bb) and fin(rr) and fin(rz)):
            status, end = NONFINITE, "begin:nonfinite"
        elif bb == 0:
            status, rr, x, end = CONVERGED, 0.0, np.zeros_like(b), "begin:bb_zero"
        elif rr <= thresh:
            status, end = CONVERGED, "begin:converged"
        elif rz <= 0:
            status, end = BREAKDOWN, "begin:rz_breakdown"
        history, iterates, k = [rr], [x.copy()], 0
        while status is None and k < max_iterations:
            q = multiply(p)
            pq = dot(p, q)
            if not (fin(pq) and fin(rz)):
                status, end = NONFINITE, "update:dot_nonfinite"
                break
            if pq <= 0:
                status, end = BREAKDOWN, "update:pq_breakdown"
                break
            see(q)
            alpha = T(np.float64(rz) / np.float64(pq))     # fp64 quotient, rounded to T once
            if not fin(alpha):
                status, end = NONFINITE, "update:alpha_nonfinite"
                break
            ap, aq = alpha * p, alpha * q
            x = x + ap                                      # a multiply, then an add, in T
            r = r - aq
            z = dinv * r if dinv is not None else r
            see(alpha, ap, aq, x, r, z)
            rz_new, rr = dot(r, z), dot(r, r)
            k += 1
            history.append(rr)
            iterates.append(x.copy())
            beta = T(np.float64(rz_new) / np.float64(rz))
            if not (fin(rr) and fin(rz_new)):
                status, end = NONFINITE, "direction:nonfinite"
            elif rr <= thresh:
                status, end = CONVERGED, "direction:converged"
            elif rz_new <= 0:
                status, end = BREAKDOWN, "direction:rz_breakdown"
            elif not fin(beta):
                status, end = NONFINITE, "direction:beta_nonfinite"
            else:
                bp = beta * p
                p = z + bp
                see(beta, bp, p)
                rz = rz_new
    return dict(x=x, status=MAX_ITERATIONS if status is None else status, iterations=k, rr=rr, bb=bb, history=np.array(history), iterates=iterates,
                end=end)


# ----------------------------------------------------------------------------- matrices
def _from_coo(m, rows, cols, vals, dtype):
    """CSR of the (row, col) entries, duplicates summed, columns ascending in every row"""
    key = rows.astype(np.int64) * m + cols.astype(np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    v = np.zeros(uniq.size, dtype=np.float64)
    np.add.at(v, inv, vals)
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(uniq // m, minlength=m), out=rp[1:])
    return synth.CSR(m, m, rp, (uniq % m).astype(np.int32), v.astype(dtype))


def lap2d(g, dtype=np.float64):
    """the 5-point Laplacian on a g x g grid (4 on the diagonal, -1 to the neighbours)"""
    idx = np.arange(g * g).reshape(g, g)
    rows = [idx.ravel(), idx[:, :-1].ravel(), idx[:, 1:].ravel(), idx[:-1, :].ravel(), idx[1:, :].ravel()]
    cols = [idx.ravel(), idx[:, 1:].ravel(), idx[:, :-1].ravel(), idx[1:, :].ravel(), idx[:-1, :].ravel()]
    vals = [np.full(g * g, 4.0)] + [np.full(r.size, -1.0) for r in rows[1:]]
    return _from_coo(g * g, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), dtype)


def tri(m, dtype=np.float64):
    """tridiagonal (-1, 2 + 1/8, -1): exactly representable entries, strictly diagonally dominant"""
    i = np.arange(m)
    rows = np.concatenate([i, i[:-1], i[1:]])
    cols = np.concatenate([i, i[1:], i[:-1]])
    vals = np.concatenate([np.full(m, 2.125), np.full(2 * (m - 1), -1.0)])
    return _from_coo(m, rows, cols, vals, dtype)


def scaled(g, dtype=np.float64):
    """D^(1/2) lap2d(g) D^(1/2) with D spread over 1e0 .. 1e6: what a Jacobi preconditioner undoes"""
    a = lap2d(g, np.float64)
    s = np.sqrt(10.0 ** (6.0 * np.arange(a.m) / (a.m - 1)))
    rows = np.repeat(np.arange(a.m), np.diff(a.rowptr))
    return synth.CSR(a.m, a.n, a.rowptr, a.colidx, (s[rows] * a.val * s[a.colidx]).astype(dtype))


def dominant(m, dtype=np.float64, per_row=4, seed=5):
    """a symmetric random pattern (about 2 * per_row off-diagonal entries per row) with diagonal = 2 * sum |off-diagonal|"""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(m), per_row)
    j = rng.integers(0, m, i.size)
    keep = i != j
    i, j = i[keep], j[keep]
    v = rng.uniform(-1, 1, i.size)
    off = _from_coo(m, np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([v, v]), np.float64)
    rows = np.repeat(np.arange(m), np.diff(off.rowptr))
    diag = 2.0 * np.bincount(rows, weights=np.abs(off.val), minlength=m) + (np.diff(off.rowptr) == 0)   # an isolated row: 1
    return _from_coo(m, np.concatenate([rows, np.arange(m)]), np.concatenate([off.colidx, np.arange(m)]), np.concatenate([off.val, diag]), dtype)


def signs(m, dtype=np.float64):
    """diag(1, -1, 1, ...): symmetric, indefinite -- the breakdown case"""
    i = np.arange(m)
    return _from_coo(m, i, i, np.where(i % 2 == 0, 1.0, -1.0), dtype)


def diagonal(csr):
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    d = np.zeros(csr.m, dtype=csr.val.dtype)
    on = rows == csr.colidx
    d[rows[on]] = csr.val[on]
    return d


def matvec(csr, dtype=None):
    """a plain CSR product as a multiply callback (every row has an entry), in `dtype` (default: the matrix's)"""
    val = csr.val if dtype is None else csr.val.astype(dtype)
    starts = csr.rowptr[:-1].astype(np.int64)
    assert (np.diff(csr.rowptr) > 0).all()

    def multiply(x):
        with np.errstate(all="ignore"):
            return np.add.reduceat(val * x.astype(val.dtype)[csr.colidx], starts)
    return multiply


def true_residual(csr, b, x):
    """||b - A x|| / ||b|| in fp64"""
    r = b.astype(np.float64) - matvec(csr, np.float64)(x.astype(np.float64))
    return float(np.linalg.norm(r) / np.linalg.norm(b.astype(np.float64)))


def rhs(m, dtype, seed=0):
    return np.random.default_rng(100 + seed).uniform(-1, 1, m).astype(dtype)
