"""The host model of spmv_hip_gmres and the matrices its tests share (tests/test_gmres_host.py, tests/test_gpu_gmres.py).

`gmres` restates the arithmetic contract of include/spmv_hip.h in numpy on top of cg_cases.dot -- the order of every dot, the two passes of
classical Gram-Schmidt, the fp64 scalars one operation at a time, the roundings to T, the order of the tests that end the loop, the cycle's
end and the restart -- so that a solve can be compared BIT FOR BIT.  np.sqrt on a float64 is the correctly rounded square root.  The multiply
is a callback: on the GPU it is Handle.spmv (the model then has spmv()'s bits), on the CPU a plain CSR product (cg_cases.matvec)."""
import numpy as np

from cg_cases import CONVERGED, MAX_ITERATIONS, BREAKDOWN, NONFINITE  # noqa: F401 -- the tests read them from here
from cg_cases import dot, geometry, _from_coo, matvec, true_residual, rhs, diagonal  # noqa: F401
from bicgstab_cases import tri_ns, upwind, nonsym_dominant, scaled_upwind  # noqa: F401
from spmv_amd import synth  # noqa: F401

RESTART_MAX = 32
GROUP = 8                       # kGmresGroup: basis vectors per trip of gmres_dots
PARTIAL_ARRAYS = RESTART_MAX + 3
STATE_ROOM = 10240


# true <b - A x, b - A x> / rr on the well-conditioned systems of tests/test_gmres_host.py, which measures it on the model alone: the largest
# value over those systems x restart {10, 30} was 1.0000048 (upwind32, fp64, restart 10; fp32: 1.0000040); with a factor of two:
RATIO_BOUND = 2.00001


def true_rr(csr, b, x):
    """<b - A x, b - A x> in longdouble"""
    r = b.astype(np.longdouble) - matvec(csr, np.longdouble)(x.astype(np.longdouble))
    return float(r @ r)


def workspace_bytes(m, itemsize, restart):
    """what the header documents: (restart + 3) vectors, 35 partial arrays, the state"""
    return (restart + 3) * ((m * itemsize + 255) // 256 * 256) + PARTIAL_ARRAYS * 8192 + STATE_ROOM


def _apply(T, V, R, g, n, x, dinv, see=lambda *values: None):
    """the cycle's end over the n steps applied: R y = g by back substitution in fp64, u = sum T(y_i) v_i, x + Dinv u"""
    f64 = np.float64
    y = [f64(0)] * n
    for i in range(n - 1, -1, -1):
        s = f64(0)
        for c in range(i + 1, n):
            ry = R[c][i] * y[c]
            s = s + ry
            see(ry)
        y[i] = (g[i] - s) / R[i][i]
        see(s, g[i] - s, y[i], T(y[i]))
    u = None
    for i in range(n):
        yv = T(y[i]) * V[i]
        u = yv if u is None else u + yv
        see(yv, u)
    xn = x + (dinv * u if dinv is not None else u)
    see(xn) if dinv is None else see(xn, dinv * u)
    return xn


def gmres(multiply, b, restart, x0=None, dinv=None, rtol=0.0, atol=0.0, max_iterations=0, watch=None):
    """Right-preconditioned GMRES(restart) as spmv_hip_gmres runs it.  multiply(p) -> A p in b's dtype.  -> dict: x, status, iterations, rr, bb,
    history (the estimate after iteration 0 .. iterations), iterates (x after iteration 0 .. iterations: what a run with a smaller
    max_iterations returns) and end: the test that ended the loop ("rotate:converged", ...; "budget" when none did).  watch(*values), when given, sees every vector and
    every scalar, of type T or fp64, as it is formed."""
    T = b.dtype.type
    f64 = np.float64
    m = b.size
    assert 1 <= restart <= RESTART_MAX
    if m == 0:
        return dict(x=b.copy(), status=CONVERGED, iterations=0, rr=0.0, bb=0.0, history=np.zeros(0), iterates=[], end="begin:empty")
    fin = np.isfinite
    see = watch if watch is not None else (lambda *values: None)
    with np.errstate(all="ignore"):
        if x0 is None:
            x, r = np.zeros_like(b), b.copy()
        else:
            x = x0.copy()
            ax = multiply(x)
            r = b - ax
            see(ax)
        rr, bb = dot(r, r), dot(b, b)
        see(b, x, r, f64(rr), f64(bb)) if dinv is None else see(b, x, r, f64(rr), f64(bb), dinv)
        thresh = max(rtol * rtol * bb, atol * atol)
        see(f64(rtol * rtol), f64(rtol * rtol * bb), f64(atol * atol))
        status, end = None, "budget"
        if not (fin(bb) and fin(rr)):
            status, end = NONFINITE, "begin:nonfinite"
        elif bb == 0:
            status, rr, x, end = CONVERGED, 0.0, np.zeros_like(b), "begin:bb_zero"
        elif rr <= thresh:
            status, end = CONVERGED, "begin:converged"
        history, iterates, k = [rr], [x.copy()], 0
        rr_cycle = f64(rr)
        while status is None and k < max_iterations:
            # ---- a cycle
            beta = np.sqrt(rr_cycle)
            g = [beta]
            V = [r * T(f64(1) / beta)]
            see(beta, f64(1) / beta, T(f64(1) / beta), V[0])
            R, cs, sn = [], [], []
            n = 0                                             # steps of this cycle that were applied
            while status is None and k < max_iterations and n < restart:
                j = n + 1
                z = dinv * V[n] if dinv is not None else V[n]
                w = multiply(z)
                see(z, w)
                a = [T(dot(V[i], w)) for i in range(j)]      # pass 1: all dots of the same w
                see(*(f64(dot(V[i], w)) for i in range(j)), *a)
                for i in range(j):
                    av = a[i] * V[i]
                    w = w - av
                    see(av, w)
                e = [T(dot(V[i], w)) for i in range(j)]      # pass 2
                see(*(f64(dot(V[i], w)) for i in range(j)), *e)
                for i in range(j):
                    ev = e[i] * V[i]
                    w = w - ev
                    see(ev, w)
                ww = f64(dot(w, w))
                hn = np.sqrt(ww)
                h = [f64(a[i]) + f64(e[i]) for i in range(j)]
                see(ww, hn, *h)
                finite = bool(fin(ww)) and all(fin(v) for v in h)
                for i in range(j - 1):
                    hi, hk = h[i], h[i + 1]
                    t1, t2, t3, t4 = cs[i] * hi, sn[i] * hk, sn[i] * hi, cs[i] * hk
                    h[i], h[i + 1] = t1 + t2, t4 - t3
                    see(t1, t2, t3, t4, h[i], h[i + 1])
                    finite = finite and bool(fin(h[i])) and bool(fin(h[i + 1]))
                hj = h[j - 1]
                d = np.sqrt(hj * hj + hn * hn)
                see(hj * hj, hn * hn, hj * hj + hn * hn, d)
                finite = finite and bool(fin(d))
                if not finite:
                    status, end = NONFINITE, "rotate:nonfinite"
                    break
                if d == 0:
                    status, end = BREAKDOWN, "rotate:d_zero"
                    break
                c, s = hj / d, hn / d
                gn, gc = -(s * g[j - 1]), c * g[j - 1]
                est = gn * gn
                see(c, s, s * g[j - 1], gc, est)
                if not (fin(c) and fin(s) and fin(gc) and fin(est)):
                    status, end = NONFINITE, "rotate:rotation_nonfinite"
                    break
                h[j - 1] = d                                  # the step is applied
                R.append(h)
                cs.append(c)
                sn.append(s)
                g[j - 1] = gc
                g.append(gn)
                n, k = j, k + 1
                history.append(float(est))
                iterates.append(_apply(T, V, R, g, n, x, dinv, see))
                if est <= thresh:
                    status, end = CONVERGED, "rotate:converged"
                elif hn == 0:
                    status, end = BREAKDOWN, "rotate:exhausted"
                else:
                    V.append(w * T(f64(1) / hn))
                    see(f64(1) / hn, T(f64(1) / hn), V[-1])
            if n > 0:
                x = iterates[-1].copy()
            if status is None and n == restart:              # the restart behind every full cycle, also when the budget ends on it
                ax = multiply(x)
                r = b - ax
                rr_cycle = f64(dot(r, r))
                see(ax, r, rr_cycle)
                if not fin(rr_cycle):
                    status, end = NONFINITE, "restart:nonfinite"
                elif rr_cycle == 0:
                    status, end = CONVERGED, "restart:zero"
    return dict(x=x, status=MAX_ITERATIONS if status is None else status, iterations=k, rr=history[-1], bb=bb, history=np.array(history), iterates=iterates,
                end=end)


# ----------------------------------------------------------------------------- matrices
def diag_of(values, dtype=np.float64):
    """diag(values), explicit zeros kept as entries"""
    v = np.asarray(values, dtype=np.float64)
    i = np.arange(v.size)
    return _from_coo(v.size, i, i, v, dtype)


def two_values(m, dtype=np.float64):
    """diag(2, 2, -2, -2, ...) (m a multiple of 4): with B = ones and m a power of 4 every Krylov vector is exact and step 2 leaves w = 0"""
    return diag_of(np.where(np.arange(m) % 4 < 2, 2.0, -2.0), dtype)


def half_singular(m, dtype=np.float64):
    """diag(2, 2, 0, 0, ...): with B = ones the space is exhausted at step 2 while half of the residual is out of reach"""
    return diag_of(np.where(np.arange(m) % 4 < 2, 2.0, 0.0), dtype)


def shift(m, dtype=np.float64):
    """A e_i = e_(i+1) for i < 1, everything else 0 (explicit zeros on the diagonal): B = e_0 gives w = 0 at step 2 and d = 0 there"""
    i = np.arange(m)
    return _from_coo(m, np.concatenate([i, [1]]), np.concatenate([i, [0]]), np.concatenate([np.zeros(m), [1.0]]), dtype)


def zero_matrix(m, dtype=np.float64):
    return diag_of(np.zeros(m), dtype)


def overflowing(m, dtype=np.float64):
    """2 I with A[1,0] = A[2,0] = -1 and A[5,1] = A[5,2] = 0.9 * the largest finite value of dtype: with B = e_0, v_2 = -(e_1 + e_2) / sqrt(2) and
    row 5 of A v_2 overflows to -infinity -- an infinity that A's values bring in at step 2.  (An infinity written into A's values would meet
    a zero of v_1 at step 1 already, as a NaN.)"""
    big = 0.9 * float(np.finfo(dtype).max)
    i = np.arange(m)
    return _from_coo(m, np.concatenate([i, [1, 2, 5, 5]]), np.concatenate([i, [0, 0, 1, 2]]), np.concatenate([np.full(m, 2.0), [-1.0, -1.0, big, big]]), dtype)
