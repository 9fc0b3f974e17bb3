"""The host model of spmv_hip_lsqr and the matrices its tests share (tests/test_lsqr_host.py, tests/test_gpu_lsqr.py).

`lsqr` restates the arithmetic contract of include/spmv_hip.h in numpy -- the two dots with their own geometries, the square roots, the scalar
chain with every operation separate, the factors rounded to T once, the order of the vector updates and of the tests -- so that a solve can
be compared BIT FOR BIT.  The two multiplies are callbacks: on the GPU they are Handle.spmv and Handle.spmv_transpose (the model then has their
bits), on the CPU plain CSR products (`products`).  The dot is spmv_hip_cg's: cg_cases.dot."""
import numpy as np

from cg_cases import dot
from spmv_amd import synth

CONVERGED, MAX_ITERATIONS, NONFINITE, LEAST_SQUARES = 0, 1, 3, 5


# ----------------------------------------------------------------------------- the loop
def lsqr(multiply, multiply_t, b, n, x0=None, damp=0.0, rtol=0.0, atol=0.0, ls_tol=0.0, max_iterations=0):
    """LSQR as spmv_hip_lsqr runs it.  multiply(v) -> A v (m elements), multiply_t(u) -> A^T u (n elements), both in b's dtype.  -> dict: x,
    status, iterations, rr, bb, ar, anorm, history (rr after iteration 0 .. iterations), iterates (x after iteration 0 .. iterations: what a run
    with a smaller max_iterations returns), estimates ((ar, anorm) after iteration 0 .. iterations) and end: the place and the test that ended
    the loop ("begin:...": the tests on bb and uu; "first:...": those on the first alpha; "step:...": iteration k; "budget" when none did)."""
    T, f = b.dtype.type, np.float64
    m = b.size
    if m == 0:
        return dict(x=np.zeros(n, dtype=b.dtype), status=CONVERGED, iterations=0, rr=0.0, bb=0.0, ar=0.0, anorm=0.0, history=np.zeros(0), iterates=[], estimates=[],
                    end="begin:empty")
    fin = np.isfinite
    with np.errstate(all="ignore"):
        if x0 is None:
            x, u = np.zeros(n, dtype=b.dtype), b.copy()
        else:
            x = x0.copy()
            u = b - multiply(x)
        bb, uu = f(dot(b, b)), f(dot(u, u))
        thr = max(f(rtol) * f(rtol) * bb, f(atol) * f(atol))
        rr, ar, anorm = uu, f(0), f(0)
        status, end = None, "budget"
        if not (fin(bb) and fin(uu)):
            status, end = NONFINITE, "begin:nonfinite"
        elif bb == 0:
            status, rr, x, end = CONVERGED, f(0), np.zeros(n, dtype=b.dtype), "begin:bb_zero"
        elif rr <= thr:
            status, end = CONVERGED, "begin:converged"
        if status is None:
            beta = np.sqrt(uu)
            u = u / T(beta)
            v = multiply_t(u)
            vv = f(dot(v, v))
            if not fin(vv):
                status, end = NONFINITE, "first:nonfinite"
            else:
                alpha = np.sqrt(vv)
                if alpha == 0:
                    status, end = LEAST_SQUARES, "first:alpha_zero"
                else:
                    v = v / T(alpha)
                    w = v.copy()
                    phibar, rhobar, a2, psi2 = beta, alpha, alpha * alpha, f(0)
                    ar, anorm = alpha * beta, np.sqrt(a2)
        history, iterates, estimates, k = [rr], [x.copy()], [(ar, anorm)], 0
        dsq = f(damp) * f(damp)
        while status is None and k < max_iterations:
            q = multiply(v)                                   # 1
            au = T(alpha) * u
            u = q - au                                        # 2: a multiply, then a subtraction, in T
            uu = f(dot(u, u))
            if not fin(uu):
                status, end = NONFINITE, "step:uu_nonfinite"
                break
            beta = np.sqrt(uu)                                # 3
            if beta > 0:
                u = u / T(beta)
            qt = multiply_t(u)                                # 4
            bv = T(beta) * v
            v = qt - bv                                       # 5
            vv = f(dot(v, v))
            if not fin(vv):
                status, end = NONFINITE, "step:vv_nonfinite"
                break
            alpha = np.sqrt(vv)                               # 6
            if alpha > 0:
                v = v / T(alpha)
            a2n = ((a2 + beta * beta) + alpha * alpha) + dsq  # 7
            rhobar1 = np.sqrt(rhobar * rhobar + dsq)          # 8
            c1, s1 = rhobar / rhobar1, f(damp) / rhobar1
            psi = s1 * phibar                                 # 9
            phibar1 = c1 * phibar
            psi2n = psi2 + psi * psi
            rho = np.sqrt(rhobar1 * rhobar1 + beta * beta)    # 10
            c, s = rhobar1 / rho, beta / rho
            theta = s * alpha                                 # 11
            rhobarn = -(c * alpha)
            phi = c * phibar1
            phibarn = s * phibar1
            tau = s * phi
            tx, tw = T(phi / rho), T(theta / rho)             # 12: rounded to T once
            if not (fin(tx) and fin(tw)):
                status, end = NONFINITE, "step:factor_nonfinite"
                break
            xw = tx * w
            x = x + xw                                        # 13
            k += 1
            a2, rhobar, phibar, psi2 = a2n, rhobarn, phibarn, psi2n
            rr = phibar * phibar + psi2                       # 14
            ar, anorm = alpha * np.abs(tau), np.sqrt(a2)
            history.append(rr)
            iterates.append(x.copy())
            estimates.append((ar, anorm))
            if not (fin(rr) and fin(ar) and fin(a2)):         # 15
                status, end = NONFINITE, "step:nonfinite"
            elif rr <= thr:
                status, end = CONVERGED, "step:converged"
            elif ar <= f(ls_tol) * (np.sqrt(a2) * np.sqrt(rr)):
                status, end = LEAST_SQUARES, "step:least_squares"
            else:
                ww = tw * w
                w = v - ww                                    # 16
    return dict(x=x, status=MAX_ITERATIONS if status is None else status, iterations=k, rr=float(rr), bb=float(bb), ar=float(ar), anorm=float(anorm),
                history=np.array(history, dtype=np.float64), iterates=iterates, estimates=estimates, end=end)


def workspace_bytes(m, n, item):
    """the bytes of spmv_hip_lsqr's workspace block (include/spmv_hip.h)"""
    up = lambda v: (v + 255) // 256 * 256
    return 2 * up(m * item) + 3 * up(n * item) + 3 * 8192 + 256


# ----------------------------------------------------------------------------- matrices
def from_dense(d, dtype=None):
    """CSR of a dense array's non-zero entries"""
    d = np.asarray(d)
    m, n = d.shape
    rows, cols = np.nonzero(d)
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=m), out=rp[1:])
    return synth.CSR(m, n, rp, cols.astype(np.int32), d[rows, cols].astype(dtype or d.dtype))


def dense(csr, dtype=None):
    d = np.zeros((csr.m, csr.n), dtype=dtype or csr.val.dtype)
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    d[rows, csr.colidx] = csr.val
    return d


def products(csr):
    """-> (multiply, multiply_t): the two CSR products as the model's callbacks on the CPU, in the matrix's dtype, by np.add.at in CSR order"""
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    cols, val, T = csr.colidx, csr.val, csr.val.dtype

    def multiply(v):
        y = np.zeros(csr.m, dtype=T)
        with np.errstate(all="ignore"):
            np.add.at(y, rows, val * v.astype(T)[cols])
        return y

    def multiply_t(u):
        y = np.zeros(csr.n, dtype=T)
        with np.errstate(all="ignore"):
            np.add.at(y, cols, val * u.astype(T)[rows])
        return y
    return multiply, multiply_t


def sparse_rect(m, n, dtype=np.float64, per_row=3, seed=0, holes=True):
    """m x n with up to per_row entries in a row, uniform in (-1, 1).  holes: row 1 and the last row are empty where m >= 5, and column
    n - 2 is empty where n >= 3 -- the x of that column stays exactly 0"""
    rng = np.random.default_rng(1000 * seed + 7 * m + n)
    live = np.array([j for j in range(n) if not (holes and n >= 3 and j == n - 2)])
    lens = np.minimum(per_row, live.size) * np.ones(m, dtype=np.int64)
    if holes and m >= 5:
        lens[[1, m - 1]] = 0
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    if live.size <= 64:
        ci = np.concatenate([np.sort(rng.choice(live, size=k, replace=False)) for k in lens] + [np.zeros(0, dtype=np.int64)])
    else:                                                      # distinct columns without a choice per row: a random start and odd strides
        start = rng.integers(0, live.size, m)
        step = 1 + rng.integers(0, max(1, live.size // per_row - 1), m)
        ci = np.concatenate([np.sort(live[(start[i] + step[i] * np.arange(lens[i])) % live.size]) for i in range(m)])
    val = rng.uniform(-1, 1, ci.size)
    val[np.abs(val) < 0.05] = 0.5
    return synth.CSR(m, n, rp, ci.astype(np.int32), val.astype(dtype))


def two_per_row(m, n, dtype=np.float64):
    """m x n with the entries (i, i mod n) = 1 + (i mod 5) / 8 and (i, (i + 3) mod n) = -1/2: exactly representable, built without a loop"""
    i = np.arange(m, dtype=np.int64)
    a, c = i % n, (i + 3) % n
    lo, hi = np.minimum(a, c), np.maximum(a, c)
    va, vc = 1.0 + (i % 5) / 8.0, np.full(m, -0.5)
    first = np.where(a < c, va, vc)
    second = np.where(a < c, vc, va)
    rp = (2 * np.arange(m + 1)).astype(np.int32)
    ci = np.stack([lo, hi], axis=1).reshape(-1).astype(np.int32)
    val = np.stack([first, second], axis=1).reshape(-1).astype(dtype)
    return synth.CSR(m, n, rp, ci, val)


def well_conditioned(m, n, dtype=np.float64, seed=0):
    """tall, dense enough that the singular values lie close together: 2 on the (i, i mod n) entries plus small random ones"""
    rng = np.random.default_rng(50 + seed)
    d = np.where(rng.uniform(0, 1, (m, n)) < 0.3, rng.uniform(-0.3, 0.3, (m, n)), 0.0)
    d[np.arange(m), np.arange(m) % n] = 2.0
    return from_dense(d, dtype)


def identity_over_zero(n, dtype=np.float64):
    """[I; 0], 2n x n: the rows n .. 2n - 1 are empty"""
    rp = np.concatenate([np.arange(n + 1), np.full(n, n)]).astype(np.int32)
    return synth.CSR(2 * n, n, rp, np.arange(n, dtype=np.int32), np.ones(n, dtype=dtype))


def rhs(m, dtype, seed=0):
    return np.random.default_rng(300 + seed).uniform(-1, 1, m).astype(dtype)


def end_cases(dtype):
    """name -> (csr, b, keywords of lsqr(), the model's expected end): every end of the loop that `dtype` can reach.  The dots are fp64, so the
    ends that need an overflowing dot exist in fp64 alone"""
    T = np.dtype(dtype).type
    tall = sparse_rect(40, 6, dtype, seed=1)
    mul, _ = products(tall)
    xs = rhs(6, dtype, 1)
    xs[4] = 0                                                  # the empty column
    tol = 1e-9 if dtype == np.float64 else 1e-4
    nan_b = rhs(40, dtype, 2)
    nan_b[17] = np.nan
    one = lambda *v: np.array(v, dtype=dtype)
    cases = {
        "consistent": (tall, mul(xs), dict(rtol=tol, ls_tol=0.0, max_iterations=50), "step:converged"),
        "inconsistent": (tall, rhs(40, dtype, 3), dict(rtol=0.0, ls_tol=tol, max_iterations=50), "step:least_squares"),
        "damped": (tall, rhs(40, dtype, 3), dict(rtol=0.0, ls_tol=tol, damp=0.5, max_iterations=50), "step:least_squares"),
        "orthogonal_b": (from_dense([[1.0], [1.0]], dtype), one(1, -1), dict(max_iterations=5), "first:alpha_zero"),
        "beta_zero": (identity_over_zero(4, dtype), one(3, 0, 0, 0, 0, 0, 0, 0), dict(max_iterations=5), "step:converged"),
        "beta_zero_damped": (identity_over_zero(4, dtype), one(3, 0, 0, 0, 0, 0, 0, 0), dict(damp=0.5, max_iterations=5), "step:least_squares"),
        "zero_b": (tall, np.zeros(40, dtype=dtype), dict(rtol=1e-6, max_iterations=5), "begin:bb_zero"),
        "good_guess": (tall, mul(xs), dict(x0=xs, rtol=1e-3, max_iterations=5), "begin:converged"),
        "budget": (tall, rhs(40, dtype, 3), dict(max_iterations=3), "budget"),
        "no_budget": (tall, rhs(40, dtype, 3), dict(max_iterations=0), "budget"),
        "nan_in_b": (tall, nan_b, dict(rtol=1e-6, max_iterations=5), "begin:nonfinite"),
        # phi / rho = |b| / |a| overflows T while bb = b^2 and vv = a^2 stay finite and above zero (fp64: vv is subnormal)
        "factor_overflow": (from_dense([[1e-160 if dtype == np.float64 else 1e-10]], dtype), one(1e150 if dtype == np.float64 else 1e30), dict(max_iterations=5),
                            "step:factor_nonfinite"),
    }
    if dtype == np.float64:
        cases.update({
            "first_overflow": (from_dense([[1e200]]), one(1), dict(max_iterations=5), "first:nonfinite"),
            "uu_overflow": (from_dense([[1.0], [1e200]]), one(1, 0), dict(max_iterations=5), "step:uu_nonfinite"),
            "vv_overflow": (from_dense([[1.0, 0.0], [1.0, 1e200]]), one(1, 0), dict(max_iterations=5), "step:vv_nonfinite"),
            "a2_overflow": (from_dense([[1e154, 0.0], [0.5e154, 0.7e154]]), one(1, 1), dict(max_iterations=5), "step:nonfinite"),
        })
    assert all(case[1].dtype == T for case in cases.values())
    return cases
