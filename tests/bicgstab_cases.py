"""The host model of spmv_hip_bicgstab and the matrices its tests share (tests/test_bicgstab_host.py, tests/test_gpu_bicgstab.py).

`bicgstab` restates the arithmetic contract of include/spmv_hip.h in numpy on top of cg_cases.dot -- the order of every dot, the roundings of
alpha, omega and beta, the order of the vector updates and of the tests that end the loop -- so that a solve can be compared BIT FOR BIT.  The
multiply is a callback: on the GPU it is Handle.spmv (the model then has spmv()'s bits), on the CPU a plain CSR product (cg_cases.matvec)."""
import numpy as np

from cg_cases import CONVERGED, MAX_ITERATIONS, BREAKDOWN, NONFINITE  # noqa: F401 -- the tests read them from here
from cg_cases import dot, geometry, _from_coo, matvec, true_residual, rhs, diagonal  # noqa: F401
from spmv_amd import synth


# ----------------------------------------------------------------------------- the loop
def bicgstab(multiply, b, x0=None, dinv=None, rtol=0.0, atol=0.0, max_iterations=0, watch=None):
    """Right-preconditioned BiCGStab as spmv_hip_bicgstab runs it.  multiply(p) -> A p in b's dtype.  -> dict: x, status, iterations, rr, bb,
    history (rr after iteration 0 .. iterations), iterates (x after iteration 0 .. iterations: what a run with a smaller max_iterations
    returns), halves (<s,s> of the half step of iteration 1 .. iterations, behind rr of iteration 0) and end: the kernel and the test that ended
    the loop ("update:tt_zero", ...; "budget" when none did).  watch(*values), when given, sees every vector and every scalar of type T as it
    is formed."""
    T = b.dtype.type
    f64 = np.float64
    m = b.size
    if m == 0:
        return dict(x=b.copy(), status=CONVERGED, iterations=0, rr=0.0, bb=0.0, history=np.zeros(0), iterates=[], end="begin:empty", halves=np.zeros(0))
    fin = np.isfinite
    see = watch if watch is not None else (lambda *values: None)
    with np.errstate(all="ignore"):
        if x0 is None:
            x, r = np.zeros_like(b), b.copy()
        else:
            x = x0.copy()
            r = b - multiply(x)
        rhat, p = r.copy(), r.copy()
        see(b, x, r) if dinv is None else see(b, x, r, dinv)
        rho, rr, bb = dot(rhat, r), dot(r, r), dot(b, b)
        thresh = max(rtol * rtol * bb, atol * atol)
        status, end = None, "budget"
        if not (fin(bb) and fin(rr) and fin(rho)):
            status, end = NONFINITE, "begin:nonfinite"
        elif bb == 0:
            status, rr, x, end = CONVERGED, 0.0, np.zeros_like(b), "begin:bb_zero"
        elif rr <= thresh:
            status, end = CONVERGED, "begin:converged"
        history, iterates, halves, k = [rr], [x.copy()], [rr], 0
        while status is None and k < max_iterations:
            ph = dinv * p if dinv is not None else p
            v = multiply(ph)
            rv = dot(rhat, v)
            if not (fin(rv) and fin(rho)):
                status, end = NONFINITE, "half:dot_nonfinite"
                break
            if rv == 0 or rho == 0:
                status, end = BREAKDOWN, "half:rv_zero" if rv == 0 else "half:rho_zero"
                break
            see(ph, v)
            alpha = T(f64(rho) / f64(rv))                  # fp64 quotient, rounded to T once
            if not fin(alpha):
                status, end = NONFINITE, "half:alpha_nonfinite"
                break
            ap, av = alpha * ph, alpha * v
            x = x + ap                                      # a multiply, then an add, in T
            s = r - av
            see(alpha, ap, av, x, s)
            ss = dot(s, s)
            k += 1
            halves.append(ss)
            if not fin(ss) or ss <= thresh:                 # the half step ends the loop
                status, end = (CONVERGED, "update:ss_converged") if fin(ss) else (NONFINITE, "update:ss_nonfinite")
                rr = ss
                history.append(rr)
                iterates.append(x.copy())
                break
            sh = dinv * s if dinv is not None else s
            t = multiply(sh)
            see(sh, t)
            ts, tt = dot(t, s), dot(t, t)
            omega = T(f64(ts) / f64(tt))
            half = None
            if not (fin(ts) and fin(tt)):
                half, end = NONFINITE, "update:ts_tt_nonfinite"
            elif tt == 0 or ts == 0:
                half, end = BREAKDOWN, "update:tt_zero" if tt == 0 else "update:ts_zero"
            elif not fin(omega):
                half, end = NONFINITE, "update:omega_nonfinite"
            elif omega == 0:
                half, end = BREAKDOWN, "update:omega_zero"
            if half is not None:                            # x keeps the half step
                status, rr = half, ss
                history.append(rr)
                iterates.append(x.copy())
                break
            osh, ot = omega * sh, omega * t
            x = x + osh
            r = s - ot
            see(omega, osh, ot, x, r)
            rho_new, rr = dot(rhat, r), dot(r, r)
            history.append(rr)
            iterates.append(x.copy())
            if not (fin(rr) and fin(rho_new)):
                status, end = NONFINITE, "direction:nonfinite"
                break
            if rr <= thresh:
                status, end = CONVERGED, "direction:converged"
                break
            beta = T((f64(rho_new) / f64(rho)) * (f64(alpha) / f64(omega)))
            if not fin(beta):
                status, end = NONFINITE, "direction:beta_nonfinite"
                break
            ov = omega * v                                  # four separate operations in T
            d = p - ov
            bd = beta * d
            p = r + bd
            see(beta, ov, d, bd, p)
            rho = rho_new
    return dict(x=x, status=MAX_ITERATIONS if status is None else status, iterations=k, rr=rr, bb=bb, history=np.array(history), iterates=iterates,
                end=end, halves=np.array(halves))


# ----------------------------------------------------------------------------- matrices
def tri_ns(m, dtype=np.float64):
    """tridiagonal (-1.5, 2.125, -0.5): exactly representable entries, strictly diagonally dominant, not symmetric"""
    i = np.arange(m)
    rows = np.concatenate([i, i[1:], i[:-1]])
    cols = np.concatenate([i, i[:-1], i[1:]])
    vals = np.concatenate([np.full(m, 2.125), np.full(m - 1, -1.5), np.full(m - 1, -0.5)])
    return _from_coo(m, rows, cols, vals, dtype)


def upwind(g, dtype=np.float64):
    """the 5-point stencil on a g x g grid with 4.5 on the diagonal, -1.5 to the west and -1 to the other three neighbours"""
    idx = np.arange(g * g).reshape(g, g)
    rows = [idx.ravel(), idx[:, 1:].ravel(), idx[:, :-1].ravel(), idx[:-1, :].ravel(), idx[1:, :].ravel()]
    cols = [idx.ravel(), idx[:, :-1].ravel(), idx[:, 1:].ravel(), idx[1:, :].ravel(), idx[:-1, :].ravel()]
    vals = [np.full(g * g, 4.5), np.full(rows[1].size, -1.5)] + [np.full(r.size, -1.0) for r in rows[2:]]
    return _from_coo(g * g, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), dtype)


def nonsym_dominant(m, dtype=np.float64, per_row=8, seed=5):
    """an unsymmetrised random pattern (about per_row off-diagonal entries in (-1, 1) per row) with diagonal = 1.25 * sum |off-diagonal| (1 on
    an empty row)"""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(m), per_row)
    j = rng.integers(0, m, i.size)
    keep = i != j
    i, j = i[keep], j[keep]
    off = _from_coo(m, i, j, rng.uniform(-1, 1, i.size), np.float64)
    rows = np.repeat(np.arange(m), np.diff(off.rowptr))
    diag = 1.25 * np.bincount(rows, weights=np.abs(off.val), minlength=m) + (np.diff(off.rowptr) == 0)
    return _from_coo(m, np.concatenate([rows, np.arange(m)]), np.concatenate([off.colidx, np.arange(m)]), np.concatenate([off.val, diag]), dtype)


def scaled_upwind(g, e, dtype=np.float64):
    """S^(1/2) upwind(g) S^(1/2) with S spread over 1e0 .. 10^e: what a Jacobi preconditioner undoes"""
    a = upwind(g, np.float64)
    s = np.sqrt(10.0 ** (float(e) * np.arange(a.m) / (a.m - 1)))
    rows = np.repeat(np.arange(a.m), np.diff(a.rowptr))
    return synth.CSR(a.m, a.n, a.rowptr, a.colidx, (s[rows] * a.val * s[a.colidx]).astype(dtype))


def skew(m, dtype=np.float64):
    """+1 above the diagonal, -1 below, no diagonal: with B = ones <rhat, A rhat> is exactly 1 + (-1) -- the breakdown case"""
    i = np.arange(m)
    rows = np.concatenate([i[:-1], i[1:]])
    cols = np.concatenate([i[1:], i[:-1]])
    vals = np.concatenate([np.full(m - 1, 1.0), np.full(m - 1, -1.0)])
    return _from_coo(m, rows, cols, vals, dtype)


def twice_identity(m, dtype=np.float64):
    """2 I: alpha = 1/2 and s = r - r/2 * 2 = 0 exactly -- the loop ends through the half step"""
    i = np.arange(m)
    return _from_coo(m, i, i, np.full(m, 2.0), dtype)
