"""A catalogue of the ways spmv_hip_lsqr can end (tests/test_lsqr_ends_host.py, tests/test_gpu_lsqr_ends.py), in the style of
tests/solve_end_cases.py and tests/gmres_end_cases.py.

A case is a LADDER: a lower-bidiagonal matrix of n + 1 rows and n columns with A[k, k] = a[k] and A[k + 1, k] = b[k], and a right-hand side
whose leading entries are `rhs` (beta_1 e_0 where `rhs` has one entry).  Golub-Kahan bidiagonalisation of a ladder from beta_1 e_0 reproduces the
ladder: u_k and v_k are unit vectors, alpha_(k+1) = a[k] and beta_(k+2) = b[k], and with power-of-two entries every vector operation is exact.
A case therefore chooses every alpha and beta of its run, and so the iteration at which the run ends and the test that ends it.  `system` embeds
the ladder's rows and columns into an otherwise empty m x n matrix at spread positions -- first, last, both sides of the workgroup boundary
(1023 and 1024) -- so that the live entries land in different workgroups' partials of the two dots, whose geometries P(m) and P(n) differ.
Adding zeros is exact: a case ends at every shape where its own ladder ends.

A line says the status, the iteration count and the `end` in the words of the model (lsqr_cases.lsqr: result["end"]).  Every ladder runs a
second time from a non-zero guess of small integers with B moved by A x0, which is exact: u = B - A x0 is the ladder's own B and the run ends
where the ladder's does.  Where B has two entries, or a guess is there to make A x0 or A^T u overflow, u is no unit vector and the end's
place is what the model said on the CPU.  tests/test_lsqr_ends_host.py proves every line with the model alone; tests/test_gpu_lsqr_ends.py then asks the device for the same bits."""
from collections import namedtuple

import numpy as np

import lsqr_cases as lc
from spmv_amd import synth

F32, F64 = np.float32, np.float64
BOTH = (F64, F32)
C, M, N, L = lc.CONVERGED, lc.MAX_ITERATIONS, lc.NONFINITE, lc.LEAST_SQUARES

# a, b: the ladder's n diagonal and n sub-diagonal entries (a zero is no entry); rhs: the leading entries of B (the rest is 0); x0: the n
# elements of a guess, or None; damp, rtol, atol, ls_tol, budget: of the run; dtypes: where the line holds; status, iterations, end: what it reports
Case = namedtuple("Case", "name a b rhs x0 damp rtol atol ls_tol budget dtypes status iterations end")

BUDGET = 12                             # more than the iterations + 1 of every case that does not say otherwise

# the shapes of the GPU test: the ladder's own; P(m) = 2, P(n) = 2; P(m) = 5, P(n) = 2; P(m) = 2, P(n) = 5; none but the first a multiple of 4
SHAPES = ("own", (1025, 1030), (4099, 1025), (1030, 4099))
BIG = (2 ** 20 + 5, 1030)               # P(m) = 1024, two steps per thread; P(n) = 2: 1022 entries of <v,v>'s partial array stay +0.0

# the ends found while MAKING iteration `iterations` + 1, which is then not applied: lsqr_unit_u and lsqr_v change nothing, lsqr_step applies nothing
MAKING = ("step:uu_nonfinite", "step:vv_nonfinite", "step:factor_nonfinite")

BASE_A = (1, 2, 1, .5, 1, 2, 1, 1)
BASE_B = (1, 1, 2, 1, .5, 1, 1, 1)
GUESS = (1, 0, -1, 0, 2, 0, 1, 0)       # the guess of the B = 0 line: X is zeroed whatever it held


def _c(name, a, b, rhs, status, iterations, end, x0=None, damp=0.0, rtol=0.0, atol=0.0, ls_tol=0.0, budget=None, dtypes=BOTH):
    row = lambda v: None if v is None else tuple(float(e) for e in v)
    assert len(a) == len(b) and 1 <= len(rhs) <= len(a) + 1 and (x0 is None or len(x0) == len(a))
    return Case(name, row(a), row(b), row(rhs), row(x0), float(damp), float(rtol), float(atol), float(ls_tol), max(BUDGET, iterations + 2) if budget is None else budget,
                tuple(dtypes), status, iterations, end)


def swap(base, j, value):
    return tuple(value if i == j else e for i, e in enumerate(base))


def ladder(a, b):
    """the ladder (a, b) as a dense fp64 array of n + 1 rows and n columns"""
    n = len(a)
    d = np.zeros((n + 1, n))
    d[np.arange(n), np.arange(n)] = a
    d[np.arange(1, n + 1), np.arange(n)] = b
    return d


def times(a, b, xs, plus=()):
    """the leading entries of B = A xs (+ the leading entries `plus`) for the ladder (a, b): exact for small integers"""
    out = ladder(a, b) @ np.asarray(xs, dtype=np.float64)
    out[:len(plus)] += plus
    return tuple(float(v) for v in out)


def spread(count, size):
    """`count` ascending positions in range(size): the first, the last, 1023 and 1024 where they exist, the others spread evenly between them"""
    if size == count:
        return np.arange(count)
    assert size >= 2 * count
    picked = sorted({0, size - 1} | {p for p in (1023, 1024) if p < size})[:count]
    for p in np.linspace(0, size - 1, 3 * count + 2).astype(np.int64)[1:-1]:
        if len(picked) < count and int(p) not in picked:
            picked.append(int(p))
    assert len(picked) == count
    return np.array(sorted(picked), dtype=np.int64)


def shape_of(case, shape):
    return (len(case.a) + 1, len(case.a)) if shape == "own" else shape


def system(case, shape, dtype):
    """-> (CSR of the ladder embedded into an empty m x n matrix, B, x0 or None) in `dtype`; shape: (m, n), or "own" for the ladder's"""
    m, n = shape_of(case, shape)
    d = ladder(case.a, case.b)
    rows, cols = spread(d.shape[0], m), spread(d.shape[1], n)
    i, j = np.nonzero(d)
    order = np.lexsort((cols[j], rows[i]))
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[i], minlength=m), out=rp[1:])
    with np.errstate(over="ignore"):
        val = d[i, j][order].astype(dtype)
        b = np.zeros(m, dtype=dtype)
        b[rows[:len(case.rhs)]] = np.asarray(case.rhs, dtype=np.float64).astype(dtype)
    assert np.isfinite(val).all() and (val != 0).all(), "an entry is not representable"
    x0 = None
    if case.x0 is not None:
        x0 = np.zeros(n, dtype=dtype)
        x0[cols] = np.asarray(case.x0, dtype=np.float64).astype(dtype)
    return synth.CSR(m, n, rp, cols[j][order].astype(np.int32), val), b, x0


def keywords(case, **kw):
    """the keywords of lsqr_cases.lsqr (and, but for x0, of Handle.lsqr) for a run of the case"""
    out = dict(damp=case.damp, rtol=case.rtol, atol=case.atol, ls_tol=case.ls_tol, max_iterations=case.budget)
    out.update(kw)
    return out


def run(case, shape, dtype, **kw):
    """the model on the case at `shape`, over lsqr_cases.products -> its result dict"""
    csr, b, x0 = system(case, shape, dtype)
    return lc.lsqr(*lc.products(csr), b, csr.n, x0=x0, **keywords(case, **kw))


def products_wide(csr):
    """lsqr_cases.products for an fp32 matrix with every row (of A and of A^T) accumulated in fp64 and rounded to fp32 once: what a multiply
    with fused multiply-adds can return where `products` rounds every product"""
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    cols, val = csr.colidx, csr.val.astype(np.float64)
    assert csr.val.dtype == F32

    def multiply(v):
        y = np.zeros(csr.m)
        with np.errstate(all="ignore"):
            np.add.at(y, rows, val * v.astype(np.float64)[cols])
            return y.astype(F32)

    def multiply_t(u):
        y = np.zeros(csr.n)
        with np.errstate(all="ignore"):
            np.add.at(y, cols, val * u.astype(np.float64)[rows])
            return y.astype(F32)
    return multiply, multiply_t


def found_at(case):
    """the iteration whose kernels find the end: `iterations` + 1 for an end found while making it, `iterations` for one found behind it"""
    return case.iterations + (1 if case.end in MAKING else 0)


def batch_places(case):
    """-> the set of "first", "middle" and "last": where in a batch of check_every = 2, 3 or 8 iterations the case's end is found"""
    out, k = set(), found_at(case)
    if not case.end.startswith("step:"):
        return out
    for every in (2, 3, 8):
        pos = (k - 1) % every + 1
        out.add("first" if pos == 1 else "last" if pos == every else "middle")
    return out


# ----------------------------------------------------------------------------- the ladders: one entry replaced at j = 1, 3 or 5
# name -> (a, b, rhs, keywords, dtypes, status, iterations, end) without a guess.  The fp64 overflow lines need fp64 dots that overflow, as in
# lsqr_cases.end_cases.  step:factor_nonfinite is T(theta / rho) = T(beta alpha / rho^2) rounding to infinity behind finite dots:
# alpha_j = beta_(j+1) = 2^-70 make rho^2 = 2^-139 and alpha_(j+1) = 2^60 makes the factor 2^129 in fp32; in fp64 2^-520 and 2^511 make it 2^1030
# (the squares 2^-1040 are subnormal doubles and still exact; a smaller alpha's square would be 0, a larger alpha_(j+1)'s infinite)
HUGE, ROOT_HUGE = 1e200, 1e154
BIG32 = 1.5 * 2.0 ** 127
E0 = (1,)
LADDERS = {}
for _j in (1, 3, 5):
    LADDERS.update({
        f"l_uu_{_j}": (BASE_A, swap(BASE_B, _j, HUGE), E0, {}, (F64,), N, _j, "step:uu_nonfinite"),
        f"l_vv_{_j}": (swap(BASE_A, _j, HUGE), BASE_B, E0, {}, (F64,), N, _j - 1, "step:vv_nonfinite"),
        f"l_beta_zero_{_j}": (BASE_A, swap(BASE_B, _j, 0), E0, {}, BOTH, C, _j + 1, "step:converged"),                        # rr = 0
        f"l_beta_zero_damped_{_j}": (BASE_A, swap(BASE_B, _j, 0), E0, dict(damp=0.5), BOTH, L, _j + 1, "step:least_squares"),  # ar = 0
        f"l_alpha_zero_{_j}": (swap(BASE_A, _j, 0), BASE_B, E0, {}, BOTH, L, _j, "step:least_squares"),                      # ar = 0, beta > 0
        f"l_a2_{_j}": (swap(BASE_A, _j, ROOT_HUGE), swap(BASE_B, _j, ROOT_HUGE), E0, {}, (F64,), N, _j + 1, "step:nonfinite"),
        f"l_factor_32_{_j}": (swap(swap(BASE_A, _j, 2.0 ** -70), _j + 1, 2.0 ** 60), swap(BASE_B, _j, 2.0 ** -70), E0, {}, (F32,), N, _j, "step:factor_nonfinite"),
        f"l_factor_64_{_j}": (swap(swap(BASE_A, _j, 2.0 ** -520), _j + 1, 2.0 ** 511), swap(BASE_B, _j, 2.0 ** -520), E0, {}, (F64,), N, _j, "step:factor_nonfinite"),
    })
LADDERS["l_exhausted"] = (BASE_A, BASE_B, E0, {}, BOTH, L, 8, "step:least_squares")   # n = 8: the Krylov space is exhausted, ar = 0
# fp32: the dots are fp64 sums of squares of floats and cannot overflow, so <u,u> and <v,v> turn non-finite only through an infinite ELEMENT:
# two finite products of one row of A (b[j] v_j + a[j+1] v_(j+1)) or of A^T (a[j] u_j + b[j] u_(j+1)) whose sum is not, with both entries
# 1.5 * 2^127.  From beta_1 e_0 the vectors are unit vectors and a row holds one product, so these lines start from a B of two entries; where
# the run then ends is what the model said on the CPU (the sign of a[j+1] does not move it)
for _name, _j, _rhs, _k in (("a", 1, (3, 4), 2), ("b", 3, (3, 4), 3), ("c", 1, (1, -1), 4), ("d", 1, (1, 1), 5), ("e", 5, (3, 4), 6)):
    LADDERS[f"l_uu_32_{_name}"] = (swap(BASE_A, _j + 1, BIG32), swap(BASE_B, _j, BIG32), _rhs, {}, (F32,), N, _k, "step:uu_nonfinite")
# (not a[5] = b[5] under B = (1, 1): its sum passes 2^128 in iteration 6 by a rounding error, and in iteration 7 where a row is accumulated
# wider and rounded once, as a fused multiply-add does: every line here ends alike under lsqr_cases.products and under products_wide)
for _name, _j, _rhs, _k in (("a", 1, (2, 1), 0), ("b", 1, (3, 4), 1), ("c", 1, (1, -1), 2), ("d", 3, (3, 4), 3), ("e", 5, (3, 4), 4)):
    LADDERS[f"l_vv_32_{_name}"] = (swap(BASE_A, _j, BIG32), swap(BASE_B, _j, BIG32), _rhs, {}, (F32,), N, _k, "step:vv_nonfinite")

XS = (1, -2, 3, 0, 1, 2, -1, 1)                          # B = A xs: a consistent ladder
ODD = (1, 2, -1, 3, 1, 1, 2, -2, 1)                      # a B outside A's range: an inconsistent ladder
# the guess of every ladder's second line: zero in the odd columns, so every row of A x0 holds ONE product, which is exact whatever the entry
# (and the replaced entries of the columns 1, 3 and 5 meet a zero).  B is the ladder's B plus A x0, so u = B - A x0 is the ladder's own B bit for
# bit and the run from the guess ends where the ladder's does -- through lsqr_init's other form, and with x = x0 + what the ladder adds
LADDER_GUESS = (1, 0, -1, 0, 1, 0, 1, 0)


def _cases():
    out = [_c(name, a, b, rhs, status, k, end, dtypes=dtypes, **kw) for name, (a, b, rhs, kw, dtypes, status, k, end) in LADDERS.items()]
    out += [
        # ---- carried over from lsqr_cases.end_cases as ladders, so that they run at the larger shapes too
        _c("l_orthogonal_b", (1,), (1,), (1, -1), L, 0, "first:alpha_zero"),
        _c("l_identity_over_zero", (1, 1, 1, 1), (0, 0, 0, 0), (3,), C, 1, "step:converged"),
        _c("l_identity_over_zero_damped", (1, 1, 1, 1), (0, 0, 0, 0), (3,), L, 1, "step:least_squares", damp=0.5),
        _c("l_factor_overflow_64", (1e-160,), (0,), (1e150,), N, 0, "step:factor_nonfinite", dtypes=(F64,)),
        _c("l_factor_overflow_32", (1e-10,), (0,), (1e30,), N, 0, "step:factor_nonfinite", dtypes=(F32,)),
        _c("l_first_overflow", (HUGE,), (0,), (1,), N, 0, "first:nonfinite", dtypes=(F64,)),
        _c("l_uu_overflow", (1,), (HUGE,), (1,), N, 0, "step:uu_nonfinite", dtypes=(F64,)),
        _c("l_vv_overflow", (1, HUGE), (1, 0), (1,), N, 0, "step:vv_nonfinite", dtypes=(F64,)),
        _c("l_a2_overflow", (1e154, .7e154), (.5e154, 0), (1, 1), N, 2, "step:nonfinite", dtypes=(F64,)),
        _c("l_zero_b", BASE_A, BASE_B, (0,), C, 0, "begin:bb_zero", rtol=1e-6),
        _c("l_zero_b_guess", BASE_A, BASE_B, (0,), C, 0, "begin:bb_zero", x0=GUESS),
        _c("l_nan_in_b", BASE_A, BASE_B, (1, float("nan")), N, 0, "begin:nonfinite", rtol=1e-6),
        _c("l_good_guess", BASE_A, BASE_B, times(BASE_A, BASE_B, XS), C, 0, "begin:converged", x0=XS),      # rr = 0, bb != 0: X keeps the guess
        _c("l_begin_rtol", BASE_A, BASE_B, (1,), C, 0, "begin:converged", rtol=1.0),                        # rr = bb <= rtol^2 bb
        # a guess whose product overflows, and in fp32 the one way a ladder reaches first:nonfinite: two entries of one column of A^T u
        # that are finite and whose sum is not
        _c("l_begin_inf_32", swap(BASE_A, 0, 2.0 ** 100), BASE_B, (1,), N, 0, "begin:nonfinite", x0=(2.0 ** 100,) + (0,) * 7, dtypes=(F32,)),
        _c("l_begin_inf_64", swap(BASE_A, 0, 2.0 ** 900), BASE_B, (1,), N, 0, "begin:nonfinite", x0=(2.0 ** 900,) + (0,) * 7, dtypes=(F64,)),
        _c("l_first_sum_32", swap(BASE_A, 0, BIG32), swap(BASE_B, 0, BIG32), (1,), N, 0, "first:nonfinite", x0=(-2.0 ** -124,) + (0,) * 7, dtypes=(F32,)),
        # phi / rho overflows in the first iteration: alpha_1 = beta_2 = 2^-70 under beta_1 = 2^60
        _c("l_factor_first_32", swap(BASE_A, 0, 2.0 ** -70), swap(BASE_B, 0, 2.0 ** -70), (2.0 ** 60,), N, 0, "step:factor_nonfinite", dtypes=(F32,)),
        # ---- the tolerances decide, and a run that is still going at its budget
        _c("l_consistent", BASE_A, BASE_B, times(BASE_A, BASE_B, XS), C, 3, "step:converged", rtol=2.0 ** -4),
        _c("l_inconsistent", BASE_A, BASE_B, ODD, L, 3, "step:least_squares", ls_tol=2.0 ** -3),
        _c("l_budget", BASE_A, BASE_B, ODD, M, 5, "budget", budget=5),
    ]
    # ---- every ladder once more from a guess, per type (LADDER_GUESS): the same end at the same iteration
    for name, (a, b, rhs, kw, dtypes, status, k, end) in LADDERS.items():
        for dtype in dtypes:
            out.append(_c(guessed_name(name, dtype), a, b, times(a, b, LADDER_GUESS, plus=rhs), status, k, end, x0=LADDER_GUESS, dtypes=(dtype,), **kw))
    return out


def guessed_name(name, dtype):
    return f"{name}_g{8 * np.dtype(dtype).itemsize}"


CASES = _cases()


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ----------------------------------------------------------------------------- what the model can return
# every `end` of the model but "begin:empty" (m = 0) is a key of test_lsqr_host.STATUS_OF_END.  Not reached, by type: step:nonfinite in fp32.
# It needs rr, ar or a2 to overflow behind finite dots; the dots are fp64 sums of squares of floats, so alpha and beta stay below
# 2^128 sqrt(m + n) and every scalar of the chain far inside fp64's range
ALLOWED_GAPS = {F64: (), F32: ("step:nonfinite",)}

# the runs at BIG: a NONFINITE found in the middle of a default batch (iteration 4 of 8) in fp64; a zero beta and such a NONFINITE in fp32
BIG_CASES = ((F64, "l_uu_3"), (F32, "l_beta_zero_3"), (F32, "l_uu_32_b"))

NAMES = {np.float32: "f32", np.float64: "f64"}


def run_id(run):
    return f"{run[0].name}-{NAMES[run[1]]}"


def ended(r):
    return r["status"], r["iterations"], r["end"]


def declared(case):
    return case.status, case.iterations, case.end


# ----------------------------------------------------------------------------- atol
# With damp = 0, rr = phibar^2 is the square of a double at every iteration k >= 1, and B = (3, 4, 0, ...) makes rr = 25 at iteration 0: the run
# of this line is the ladder on which solve_end_cases.atol_probes finds a place at every k.  Its budget stays below n = 8
ATOL_CASE = "l_three_four"
CASES.append(_c(ATOL_CASE, BASE_A, BASE_B, (3, 4), M, 7, "budget", budget=7))
RUNS = [(c, d) for c in CASES for d in c.dtypes]


def probe_picks(probes, budget):
    """of solve_end_cases.atol_probes' places in front of the budget (the next double below then runs one iteration further) the first two,
    one in the middle and the last two"""
    probes = [p for p in probes if p[1] < budget]
    return list(dict.fromkeys(probes[:2] + probes[len(probes) // 2:len(probes) // 2 + 1] + probes[-2:]))


# ----------------------------------------------------------------------------- one matrix for the test of state between solves
def state_system(dtype, shape=(1030, 1025), rect=(1000, 40)):
    """A ladder beside a lsqr_cases.sparse_rect part in one matrix: the part fills the rows and columns below `rect`, the ladder's rows and
    columns lie spread behind them (the last, 1023 and 1024 among them), and one row behind `rect` is empty.  The right-hand side chooses whose
    recurrence runs.  -> (CSR, runs): runs is a list of (name, B, x0 or None, keywords, (status, iterations, end)) -- what the model says on the
    CPU -- whose first is the solve from a guess of finfo.max, whose second is the ordinary solve and whose last is B = 0"""
    (m, n), (mr, nr) = shape, rect
    case, rtol, ls_tol = (by_name("l_uu_3"), 0.5, 0.5) if dtype == F64 else (by_name("l_uu_32_b"), 0.375, 0.41)
    part = lc.sparse_rect(mr, nr, dtype, per_row=4, seed=11)
    d = ladder(case.a, case.b)
    rows, cols = mr + spread(d.shape[0], m - mr), nr + spread(d.shape[1], n - nr)
    empty = next(r for r in range(mr, m) if r not in rows)
    i, j = np.nonzero(d)
    r = np.concatenate([np.repeat(np.arange(mr), np.diff(part.rowptr)), rows[i]])
    c = np.concatenate([part.colidx, cols[j]])
    v = np.concatenate([part.val.astype(np.float64), d[i, j]])
    order = np.lexsort((c, r))
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=m), out=rp[1:])
    csr = synth.CSR(m, n, rp, c[order].astype(np.int32), v[order].astype(dtype))
    assert np.isfinite(csr.val).all()

    def on_ladder(values):
        b = np.zeros(m, dtype=dtype)
        b[rows[:len(values)]] = np.asarray(values, dtype=np.float64).astype(dtype)
        return b

    def guess(values):
        x = np.zeros(n, dtype=dtype)
        x[cols[:len(values)]] = np.asarray(values, dtype=np.float64).astype(dtype)
        return x
    ordinary = np.zeros(m, dtype=dtype)
    ordinary[:mr] = lc.rhs(mr, dtype, 12)
    alone = np.zeros(m, dtype=dtype)
    alone[empty] = 1
    xs = (1, -2, 3)                                           # the columns in front of the replaced entries
    consistent = on_ladder(times(case.a, case.b, xs + (0,) * (len(case.a) - 3)))
    budget = dict(max_iterations=6)
    runs = [
        # the largest budget of all: the first solve's history block is as long as any later one's
        ("huge_guess", ordinary, np.full(n, np.finfo(dtype).max, dtype=dtype), dict(max_iterations=BUDGET), (N, 0, "begin:nonfinite")),
        ("ordinary", ordinary, None, dict(damp=0.25, max_iterations=6), (M, 6, "budget")),
        # before the ladder's run meets the replaced entries in iteration 4 it has rr / bb = 1, 1/2, 1/6 and ar / (anorm sqrt(rr)) = 1, 0.577,
        # 0.289 in fp64 (l_uu_3) and rr / bb = 1, 0.204, 0.0918 and ar / (anorm sqrt(rr)) = 1, 0.435, 0.400 in fp32 (l_uu_32_b)
        ("converged", on_ladder(case.rhs), None, dict(rtol=rtol, max_iterations=BUDGET), (C, 2, "step:converged")),
        ("least_squares", on_ladder(case.rhs), None, dict(ls_tol=ls_tol, max_iterations=BUDGET), (L, 2, "step:least_squares")),
        ("good_guess", consistent, guess(xs), budget, (C, 0, "begin:converged")),
        ("empty_row", alone, None, budget, (L, 0, "first:alpha_zero")),
        ("ladder", on_ladder(case.rhs), None, dict(max_iterations=BUDGET, check_every=3), (case.status, case.iterations, case.end)),
        ("ordinary_again", ordinary, None, dict(damp=0.25, max_iterations=6), (M, 6, "budget")),
        ("zero_b", np.zeros(m, dtype=dtype), guess(xs), budget, (C, 0, "begin:bb_zero")),
    ]
    return csr, runs


# ----------------------------------------------------------------------------- a matrix for LSQR on every executor
def arrow_rect(m, n, dtype, per_row=4, seed=3):
    """solve_end_cases.arrow for a rectangular matrix: m x n with a dense first row (n entries: longer than any long-row threshold) and a
    dense first column (m entries: the longest row of A^T) around a random pattern of about per_row entries per row; every entry is a
    multiple of 1/8 in [-1, 1] without 0, (0, 0) is 2: exact in fp32"""
    rng = np.random.default_rng(seed)

    def eighths(k):
        return rng.integers(1, 9, k) * rng.choice((-1.0, 1.0), k) / 8.0
    i = np.repeat(np.arange(1, m), per_row)
    j = rng.integers(1, n, i.size)
    key = np.unique(i * n + j)                                # a duplicate would be merged: dropped instead
    i, j = key // n, key % n
    rows = np.concatenate([i, np.zeros(n, dtype=np.int64), np.arange(1, m)])
    cols = np.concatenate([j, np.arange(n), np.zeros(m - 1, dtype=np.int64)])
    vals = np.concatenate([eighths(i.size), eighths(n), eighths(m - 1)])
    vals[i.size] = 2.0
    order = np.lexsort((cols, rows))
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=m), out=rp[1:])
    return synth.CSR(m, n, rp, cols[order].astype(np.int32), vals[order].astype(dtype))
