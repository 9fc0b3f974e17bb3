"""Exact reference for the dyadic operands of spmv_amd.synth (dyadic_values / dyadic_x): y = A x evaluated in integers.

val = vi * 2**ev and x = xi * 2**ex, so row i of A x is (sum of vi * xi over the row) * 2**(ev + ex).  The integer sums are taken in int64
(prefix sums differenced at RowPtr on the host, index_add_ on the device): the bit budget keeps every row sum below 2^53, so the int64
prefix sums are exact modulo 2^64 and their differences exact.  A float64 cumsum over the whole matrix would round here.  The sum is
scaled with ldexp and cast to the value type, both exactly.

Non-finite entries (in x or in the values) are classified per row from the products:
    NaN   if any product is NaN (Inf * 0 included) or both +Inf and -Inf products are present;
    +-Inf if otherwise an infinite product is present;
    the exact finite value otherwise (a row with no non-finite product must not see one: the leak check).
The finite magnitudes stay far from overflow, so the classification does not depend on the summation order.

A test helper, not a conftest: imported by the tests that use it."""
import numpy as np


def _ints(a64, e, what):
    """Integer mantissas of the finite entries of a float64 array on the 2**e grid (non-finite -> 0)."""
    fin = np.isfinite(a64)
    m = np.ldexp(np.where(fin, a64, 0.0), -e)
    assert np.array_equal(m, np.round(m)) and (np.abs(m) < 2.0**53).all(), f"{what} is not on the 2**{e} grid"
    return m.astype(np.int64)


def spmv(rowptr, colidx, val, x, ev, ex):
    """-> y in val's dtype (numpy)."""
    rp = np.asarray(rowptr, dtype=np.int64)
    ci = np.asarray(colidx, dtype=np.int64)
    v64, x64 = np.asarray(val).astype(np.float64), np.asarray(x).astype(np.float64)
    m = rp.shape[0] - 1
    vi, xi = _ints(v64, ev, "val"), _ints(x64, ex, "x")
    cs = np.zeros(ci.shape[0] + 1, dtype=np.int64)
    with np.errstate(over="ignore"):
        np.cumsum(vi * xi[ci], out=cs[1:])                       # wraps modulo 2^64 on long matrices; the differences are exact
    s = cs[rp[1:]] - cs[rp[:-1]]
    y = np.ldexp(s.astype(np.float64), ev + ex)
    with np.errstate(invalid="ignore"):
        prod = v64 * x64[ci]
    row_of = np.repeat(np.arange(m), np.diff(rp))
    nan = np.bincount(row_of, np.isnan(prod), minlength=m) > 0
    pinf = np.bincount(row_of, prod == np.inf, minlength=m) > 0
    ninf = np.bincount(row_of, prod == -np.inf, minlength=m) > 0
    y = np.where(pinf, np.inf, np.where(ninf, -np.inf, y))
    y[nan | (pinf & ninf)] = np.nan
    return y.astype(np.asarray(val).dtype)


def spmv_csr(csr, x, plan):
    return spmv(csr.rowptr, csr.colidx, csr.val, x, plan.ev, plan.ex)


def transpose(rowptr, colidx, val, n):
    """-> (rowptr, colidx, val) of A^T (numpy; entries of a column in row order)."""
    rp = np.asarray(rowptr, dtype=np.int64)
    ci = np.asarray(colidx, dtype=np.int64)
    order = np.argsort(ci, kind="stable")
    rt = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=n), out=rt[1:])
    rows = np.repeat(np.arange(rp.shape[0] - 1), np.diff(rp))
    return rt, rows[order], np.asarray(val)[order]


def mismatches(y, want):
    """Rows where y differs from the exact reference: finite and infinite rows bit for bit (so +0.0 is not -0.0), NaN rows by isnan."""
    y, want = np.asarray(y), np.asarray(want)
    assert y.dtype == want.dtype and y.shape == want.shape, (y.dtype, want.dtype, y.shape, want.shape)
    u = np.uint64 if y.dtype == np.float64 else np.uint32
    nw = np.isnan(want)
    ok = np.where(nw, np.isnan(y), y.view(u) == want.view(u))
    return np.nonzero(~ok)[0]


# ----------------------------------------------------------------------------- device (torch) twins, for matrices that exist only in HBM
def spmv_device(rp, ci, va, x, ev, ex):
    """Device twin of spmv: torch tensors in, y in va's dtype on va's device."""
    import torch
    dev = va.device
    r = rp.to(torch.int64)
    lens = r[1:] - r[:-1]
    m = lens.shape[0]
    row_of = torch.repeat_interleave(torch.arange(m, device=dev), lens)
    c = ci.to(torch.int64)
    v64, x64 = va.to(torch.float64), x.to(torch.float64)

    def ints(a64, e, what):
        fin = torch.isfinite(a64)
        mm = torch.where(fin, a64, 0.0) * 2.0**-e                 # power-of-two scalars: exact (torch.ldexp goes through pow)
        assert bool(torch.equal(mm, torch.round(mm))) and bool((mm.abs() < 2.0**53).all()), f"{what} is not on the 2**{e} grid"
        return mm.to(torch.int64)

    s = torch.zeros(m, dtype=torch.int64, device=dev)
    s.index_add_(0, row_of, ints(v64, ev, "val") * ints(x64, ex, "x")[c])
    y = s.to(torch.float64) * 2.0**(ev + ex)
    prod = v64 * x64[c]
    flags = torch.zeros((m, 3), dtype=torch.int32, device=dev)
    for k, f in enumerate((torch.isnan(prod), prod == float("inf"), prod == float("-inf"))):
        flags[:, k].index_add_(0, row_of, f.to(torch.int32))
    nan, pinf, ninf = (flags[:, k] > 0 for k in range(3))
    y = torch.where(pinf, float("inf"), torch.where(ninf, float("-inf"), y))
    y = torch.where(nan | (pinf & ninf), float("nan"), y)
    return y.to(va.dtype)


def mismatches_device(y, want):
    """Device twin of mismatches: -> int64 tensor of the differing rows."""
    import torch
    it = torch.int64 if y.dtype == torch.float64 else torch.int32
    nw = torch.isnan(want)
    ok = torch.where(nw, torch.isnan(y), y.view(it) == want.view(it))
    return torch.nonzero(~ok).flatten()


def sprinkle_nonfinite(colidx, val, x, seed, x_share=0.003, n_values=6):
    """Copies of val and x with non-finite entries: about x_share of the columns of x set to NaN / +Inf / -Inf (always the first and
    the last), and n_values entries of val set to +Inf / -Inf / NaN, half of them at columns where x is zero (Inf * 0 = NaN).  numpy."""
    rng = np.random.default_rng(seed)
    val, x = np.array(val, copy=True), np.array(x, copy=True)
    n, nnz = x.shape[0], val.shape[0]
    special = np.array([np.nan, np.inf, -np.inf], dtype=x.dtype)
    if n:
        cols = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, max(1, int(n * x_share)))]))
        x[cols] = special[rng.integers(0, 3, cols.size)]
    if nnz:
        ci = np.asarray(colidx, dtype=np.int64)
        at_zero = np.nonzero(x[ci] == 0)[0]
        k = min(n_values // 2, at_zero.size)
        pick = np.concatenate([rng.choice(at_zero, k, replace=False) if k else np.zeros(0, np.int64),
                               rng.integers(0, nnz, n_values - k)])
        val[pick] = special[rng.integers(0, 3, pick.size)].astype(val.dtype)
    return val, x


def signed_zero_rows(csr, x, seed):
    """About a third of the non-empty rows (at least one) get negative values and x = +0.0 at all their columns: every product of such
    a row is -0.0, and the reference's accumulators start at +0.0, so its result is +0.0.  The other rows keep their draw where x is
    not zeroed.  -> (val, x, the rows of -0.0 products)."""
    rng = np.random.default_rng(seed)
    lens = np.diff(csr.rowptr.astype(np.int64))
    z = (rng.random(csr.m) < 0.3) & (lens > 0)
    if lens.any() and not z.any():
        z[rng.choice(np.nonzero(lens)[0])] = True
    neg = np.repeat(z, lens)
    x = x.copy()
    x[csr.colidx[neg]] = 0.0
    return np.where(neg, -np.abs(csr.val), csr.val), x, np.nonzero(z)[0]
