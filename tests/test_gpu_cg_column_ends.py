"""GPU: every way a column of spmv_hip_cg_columns can end, in mixed company -- beside columns that end elsewhere, earlier or later, and one that
runs on -- anywhere in an enqueued batch, at every budget edge, at every k, through the element-access kernels, behind calls that left NaN and
infinity in the workspace, under atol, under the timer and on a matrix with a long row (include/spmv_hip.h, "the arithmetic contract").

The yardstick is cg_columns_cases.solve -- cg_cases.cg per column -- around column 0 of the SAME handle's spmm (cg_columns_cases.spmm_column),
run with the x0, the Dinv, the tolerances and the budget of the call it is compared with; X, status, iterations, rr, bb and the history of every
column are compared bit for bit and no tolerance appears anywhere.  The one freedom: a NaN equals a NaN whatever its sign and payload.  The
columns come from tests/solve_end_cases.py (columns_system: the CG catalogue as the columns of one call), whose every group
tests/test_cg_column_ends_host.py proves on the CPU first; here every column must also reach the (status, iterations, end) it declares under the
handle's own multiply -- bits that match a model which ends elsewhere would mean the INPUT is wrong, not the kernel.  The helpers that the
solvers share are in tests/solve_harness.py."""
import numpy as np
import pytest

import cg_cases as cgc
import cg_columns_cases as ccc
import solve_end_cases as sec
import solve_harness as sh
from solve_harness import CANARY, DEV, EVERY, NAMES, ended, handle, run_bits, same

pytestmark = pytest.mark.gpu

ROW = sh.ROWS["cg_columns"]
NOT_REACHED = "the case does not reach its end on this multiply"
# (shift of B, shift of X in elements, padding of B, padding of X in columns): all but the first run the element-access kernels
LAYOUTS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, 3, 1), (1, 1, 3, 1))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = sh.library()
    assert hasattr(lib, "spmv_hip_cg_columns")
    return lib


def figures(res):
    """the result dicts of a call as arrays that `same` compares"""
    return np.array([(r["status"], r["iterations"]) for r in res]), np.array([(r["rr"], r["bb"]) for r in res], dtype=np.float64)


def same_call(a, b, cols=None):
    """two (X, res, hist); cols: column j of a is column cols[j] of b"""
    (Xa, ra, ha), (Xb, rb, hb) = a, b
    if cols is not None:
        Xb, rb, hb = Xb[:, cols], [rb[j] for j in cols], hb[:, cols]
    return same(np.ascontiguousarray(Xa), np.ascontiguousarray(Xb)) and all(same(p, q) for p, q in zip(figures(ra), figures(rb))) and same(np.ascontiguousarray(ha), np.ascontiguousarray(hb))


def solve(h, B, X0=None, **kw):
    """through host pointers, with a canary in X when there is no guess and rtol = 0 unless set -> (X, list of result dicts, history)"""
    return sh.solve_columns(h, B, X0, **dict(ROW.zero_tols, **kw))


def models_of(mul, B, X0=None, dinv=None, **kw):
    return ccc.solve(mul, np.ascontiguousarray(B), None if X0 is None else np.ascontiguousarray(X0), dinv=dinv, **kw)


def check_call(models, got, what=None):
    """a call against model runs with the same arguments, column by column, however each ended"""
    X, res, hist = got
    assert len(res) == X.shape[1] == len(models) and hist.shape == (1 + max(mo["iterations"] for mo in models), len(models)), (what, hist.shape)
    for j, mo in enumerate(models):
        its, at = mo["iterations"], (what, j, mo["end"])
        assert (res[j]["status"], res[j]["iterations"]) == (mo["status"], its), (at, res[j])
        assert same(np.ascontiguousarray(X[:, j]), mo["x"]), (at, "x")
        assert same(np.float64(res[j]["rr"]), np.float64(mo["rr"])) and same(np.float64(res[j]["bb"]), np.float64(mo["bb"])), (at, res[j], mo["rr"], mo["bb"])
        assert same(np.ascontiguousarray(hist[:its + 1, j]), mo["history"]), (at, hist[:, j], mo["history"])
        assert np.isnan(hist[its + 1:, j]).all(), (at, "history behind the column's end")       # api.cg_columns fills with NaN; nothing was written there


def declared(cases, models, budget=sec.BUDGET):
    assert [ended(mo) for mo in models] == sec.declared_columns(cases, budget), (NOT_REACHED, budget, [(c.name, ended(mo)) for c, mo in zip(cases, models)])
    assert np.isfinite(models[-1]["x"]).all()


# ----------------------------------------------------------------------------- a. every end, anywhere in a batch, at every budget edge
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("m", sec.SIZES)
@pytest.mark.parametrize("group", sec.GROUPS)
def test_every_end_in_mixed_company_at_every_place_in_a_batch(group, m, dtype):
    """k is 11 .. 15: a column's element position inside the 16-byte groups changes from row to row.  Every call also with the columns in
    the reverse order, which puts every case next to other neighbours: column j has the same bits"""
    csr, B, X0, Dinv, cases = sec.columns_system(group, m, dtype)
    k = B.shape[1]
    rev = list(range(k))[::-1]
    assert 11 <= k <= 15 and {c.iterations for c in cases} == {0, 1, 2}
    reached = set()
    with handle(csr) as h:
        mul = ccc.spmm_column(h)
        for run, G, ones in sec.column_runs(group, B, X0):
            dinv = np.ones(csr.m, dtype=dtype) if ones else Dinv
            Gr = None if G is None else G[:, rev]
            models = {}
            for budget, every in [(sec.BUDGET, e) for e in EVERY] + [(b, e) for b in range(4) for e in (0, 1)]:
                if budget not in models:
                    models[budget] = models_of(mul, B, G, dinv, max_iterations=budget)
                    declared(cases, models[budget], budget)
                what = (run, budget, every)
                got = solve(h, B, G, dinv=dinv, max_iterations=budget, check_every=every)
                check_call(models[budget], got, what)
                back = solve(h, B[:, rev], Gr, dinv=dinv, max_iterations=budget, check_every=every)
                check_call(models[budget][::-1], back, what + ("reversed",))
                assert same_call(got, back, rev), what
            reached |= {mo["end"] for mo in models[sec.BUDGET]}
    assert reached == {c.end for c in cases} | {"budget"}


# ----------------------------------------------------------------------------- b. every k from 1 to 16
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("m", [5, 1025, 2049])
def test_bits_against_the_model_at_every_k(m, dtype):
    """CcgMap's f / k and f % k, have(i) (one slot to k = 4, two to 8, three to 12, four to 16) and spmm's lane-group width all move with k.
    k = 1 with ldb = ldx = 1 is spmv_hip_cg around the handle's spmv(), which tests/test_gpu_cg_columns.py compares with cg(): here k = 1 runs with
    leading dimensions of 2, the k-column kernels' own k = 1"""
    csr = cgc.tri(m, dtype)
    run_bits(csr, dtype, list(range(2, 17)), 20)
    rng = np.random.default_rng(m)
    b, guess, jac = ccc.columns(m, 1, dtype, 21), rng.uniform(-1, 1, (m, 1)).astype(dtype), rng.uniform(0.5, 1.5, m).astype(dtype)
    with handle(csr) as h:
        mul = ccc.spmm_column(h)
        for X0 in (None, guess):
            for dinv in (None, jac):
                for budget in (0, 1, 2, 5):
                    Bw, Xw = np.full((m, 2), np.nan, dtype=dtype), np.full((m, 2), CANARY, dtype=dtype)
                    Bw[:, 0] = b[:, 0]
                    if X0 is not None:
                        Xw[:, 0] = X0[:, 0]
                    got = h.cg_columns(Bw[:, :1], Xw[:, :1], x0=X0 is not None, rtol=0.0, max_iterations=budget, dinv=dinv, history=True)
                    check_call(models_of(mul, b, X0, dinv, max_iterations=budget), got, (X0 is not None, dinv is not None, budget))
                    assert (Xw[:, 1] == CANARY).all()


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_frozen_columns_at_every_k(dtype):
    """the first k columns of the group without guesses, and the first k - 1 with the column that runs on: frozen columns at every k"""
    csr, B, _, _, cases = sec.columns_system("plain_nox0", 1026, dtype)
    n = len(cases)
    with handle(csr) as h:
        models = models_of(ccc.spmm_column(h), B, max_iterations=sec.BUDGET)           # a column's model does not depend on k
        declared(cases, models)
        for k in range(1, 12):
            for cols in ([list(range(k))] if k <= n else []) + ([list(range(k - 1)) + [n]] if k >= 2 else []):
                for every in (0, 1):
                    got = solve(h, B[:, cols], max_iterations=sec.BUDGET, check_every=every)
                    check_call([models[j] for j in cols], got, (k, cols, every))


# ----------------------------------------------------------------------------- c. frozen columns in the element-access kernels
def device_call(h, B, X0, dinv, layout, **kw):
    """the call on device operands in a layout of LAYOUTS: B's padding holds NaN, X's padding and one 16-byte unit on each side canaries.
    -> (X, res, hist) after the canaries have been found intact"""
    import torch
    m, k = B.shape
    shift_b, shift_x, pad_b, pad_x = layout
    tdt = torch.from_numpy(B).dtype
    ldb, ldx = k + pad_b, k + pad_x
    bbuf = torch.full((m * ldb + 1,), float("nan"), dtype=tdt, device=DEV)
    Bd = bbuf[shift_b:shift_b + m * ldb].view(m, ldb)[:, :k]
    Bd.copy_(torch.from_numpy(np.ascontiguousarray(B)))
    edge = 16 // B.dtype.itemsize
    xbuf = torch.full((m * ldx + 2 * edge + 1,), CANARY, dtype=tdt, device=DEV)
    Xd = xbuf[edge + shift_x:edge + shift_x + m * ldx].view(m, ldx)[:, :k]
    assert (Bd.data_ptr() % 16 != 0) == bool(shift_b) and (Xd.data_ptr() % 16 != 0) == bool(shift_x)
    if X0 is not None:
        Xd.copy_(torch.from_numpy(np.ascontiguousarray(X0)))
    kw.setdefault("rtol", 0.0)
    got, res, hist = h.cg_columns(Bd, Xd, x0=X0 is not None, dinv=None if dinv is None else torch.from_numpy(dinv).to(DEV), history=True, **kw)
    torch.cuda.synchronize()
    assert got is Xd
    out = xbuf.cpu().numpy()
    body = out[edge + shift_x:edge + shift_x + m * ldx].reshape(m, ldx)
    assert (out[:edge + shift_x] == CANARY).all() and (out[edge + shift_x + m * ldx:] == CANARY).all() and (body[:, k:] == CANARY).all(), (layout, "a canary beside X")
    return body[:, :k].copy(), res, hist


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("group", ["plain", "pre"])
def test_frozen_columns_in_the_element_access_kernels(group, dtype):
    """padded or unaligned device operands: ccg_store4's `keep` mask is what leaves an ended column of X alone, the B = 0 column is zeroed by a
    pitched memset and the column whose guess overflows keeps its guess: the bits of the host-pointer call, every canary intact"""
    csr, B, X0, Dinv, cases = sec.columns_system(group, 1026, dtype)
    names = [c.name for c in cases]
    assert group != "plain" or ("c_begin_zero" in names and any(n.startswith("c_begin_inf") for n in names))
    with handle(csr) as h:
        mul = ccc.spmm_column(h)
        for budget in (sec.BUDGET, 1):
            models = models_of(mul, B, X0, Dinv, max_iterations=budget)
            declared(cases, models, budget)
            want = solve(h, B, X0, dinv=Dinv, max_iterations=budget)
            check_call(models, want, (budget, "host"))
            for layout in LAYOUTS:
                for every in (0, 1):
                    got = device_call(h, B, X0, Dinv, layout, max_iterations=budget, check_every=every)
                    check_call(models, got, (budget, layout, every))
                    assert same_call(got, want), (budget, layout, every)


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_one_zero_column_in_a_wider_x(dtype):
    """k = 1 with ldx = 2: a column like any other; B = 0 zeroes that column of X and not its neighbour"""
    import torch
    case = sec.by_name("c_begin_zero")
    csr, B, X0, _, _ = sec.columns_system([case], 1026, dtype)
    with handle(csr) as h:
        models = models_of(ccc.spmm_column(h), B[:, :1], X0[:, :1], max_iterations=sec.BUDGET)
        assert ended(models[0]) == (case.status, case.iterations, case.end) and X0[:, 0].any(), NOT_REACHED
        wide = np.full((csr.m, 2), CANARY, dtype=dtype)
        wide[:, 0] = X0[:, 0]
        X, res, hist = h.cg_columns(B[:, :1], wide[:, :1], x0=True, rtol=0.0, max_iterations=sec.BUDGET, history=True)
        check_call(models, (X, res, hist), "host")
        assert not wide[:, 0].any() and (wide[:, 1] == CANARY).all()
        for shift in (0, 1):
            edge = 16 // np.dtype(dtype).itemsize
            xbuf = torch.full((2 * csr.m + 2 * edge + 1,), CANARY, dtype=torch.from_numpy(B).dtype, device=DEV)
            Xd = xbuf[edge + shift:edge + shift + 2 * csr.m].view(csr.m, 2)
            Xd[:, 0] = torch.from_numpy(X0[:, 0].copy())
            Bd = torch.from_numpy(B).to(DEV)
            X, res, hist = h.cg_columns(Bd[:, :1], Xd[:, :1], x0=True, rtol=0.0, max_iterations=sec.BUDGET, history=True)
            torch.cuda.synchronize()
            check_call(models, (X.cpu().numpy(), res, hist), ("device", shift))
            out = xbuf.cpu().numpy()
            body = out[edge + shift:edge + shift + 2 * csr.m].reshape(csr.m, 2)
            assert not body[:, 0].any() and (body[:, 1] == CANARY).all() and (out[:edge + shift] == CANARY).all() and (out[edge + shift + 2 * csr.m:] == CANARY).all(), shift


# ----------------------------------------------------------------------------- d. state between calls
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_a_call_is_unaffected_by_what_earlier_calls_left(dtype):
    """One handle on a matrix that holds every CG case's blocks and a tridiagonal tail.  The workspace is carved by the columns it HOLDS and
    partial array (a, c) sits at a * k + c of the CALL's k: a call that leaves NaN and infinity in r, p, q and the partials, then ordinary calls
    with fewer and more columns, the groups of ends, a call that turns non-finite inside the loop -- and the ordinary calls again, with the bits
    of their first time.  Device operands, so that device_bytes moves with the workspace alone (the history block is sized by the first call)"""
    import torch
    csr, groups, tail_columns = sec.columns_state_system(dtype)
    m, item = csr.m, np.dtype(dtype).itemsize
    jac = (2.0 ** np.random.default_rng(11).integers(-1, 2, m)).astype(dtype)
    firsts = {}
    with handle(csr) as h:
        mul = ccc.spmm_column(h)
        mul(np.zeros(m, dtype=dtype))                                   # spmm's tables and stage buffers appear here, before device_bytes is watched

        def call(B, X0=None, dinv=None, budget=sec.BUDGET, every=0):
            models = models_of(mul, B, X0, dinv, max_iterations=budget)
            got = device_call(h, B, X0, dinv, LAYOUTS[0], max_iterations=budget, check_every=every)
            check_call(models, got, (B.shape[1], every))
            return models, got

        def the_ordinary_calls(ks):
            for k in ks:
                for dinv in (None, jac):
                    models, got = call(tail_columns(k, 3), dinv=dinv, budget=6)
                    assert all(ended(mo) == (cgc.MAX_ITERATIONS, 6, "budget") and np.isfinite(mo["x"]).all() for mo in models)
                    key = (k, dinv is not None)
                    assert same_call(got, firsts.setdefault(key, got)), key
                    yield k

        def the_group(name, every=0):
            B, X0, Dinv, cases = groups[name]
            models, _ = call(B, X0, Dinv, every=every)
            declared(cases, models)
            return models

        before = h.info()["device_bytes"]
        B, _, Dinv, cases = groups["pre"]
        assert B.shape[1] == 11
        huge = np.full(B.shape, np.finfo(dtype).max, dtype=dtype)       # r = b - A x0 overflows: NaN and infinity from the init kernel on
        models, _ = call(B, huge, Dinv, budget=16)                      # the first solve of the handle: it allocates the workspace
        assert all(ended(mo) == (cgc.NONFINITE, 0, "begin:nonfinite") for mo in models) and (~np.isfinite(mul(huge[:, 0].copy()))).any()
        held = h.info()["device_bytes"]
        assert held - before >= ROW.workspace(m, 11, item)        # ... and the history block
        for k in the_ordinary_calls((3, 15, 2)):
            assert h.info()["device_bytes"] - held == (0 if k == 3 else ROW.workspace(m, 15, item) - ROW.workspace(m, 11, item)), k
        grown = h.info()["device_bytes"]
        the_group("plain")
        the_group("pre")
        list(the_ordinary_calls((3,)))
        later = the_group("pre", every=3)                               # overflows INSIDE the loop, in the middle of an enqueued batch
        assert any(mo["end"] == "direction:nonfinite" and mo["iterations"] >= 1 for mo in later)
        list(the_ordinary_calls((3, 2, 15)))
        assert h.info()["device_bytes"] == grown


# ----------------------------------------------------------------------------- e. atol
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_atol_decides_with_less_or_equal_column_by_column(dtype):
    """On a column's own model some rr on the way is the square of a double a: a call with atol = a ends THAT column there (the test is <=), the
    next double below does not, and every other column matches its own model under the same atol"""
    exact = [c for c in sec.column_groups(dtype)["plain_nox0"] if c.exact and c.status != cgc.NONFINITE]
    places = set()
    for m in sec.ATOL_SIZES:
        csr, B, _, _, cases = sec.columns_system(exact, m, dtype)
        with handle(csr) as h:
            mul = ccc.spmm_column(h)
            declared(cases, models_of(mul, B, max_iterations=sec.BUDGET))
            seen = {}
            for j in range(B.shape[1]):
                b = np.ascontiguousarray(B[:, j])
                for a, its, end in sec.atol_probes(lambda atol: cgc.cg(mul, b, atol=atol, max_iterations=sec.BUDGET)):
                    places.add(end)
                    for atol, there in ((a, True), (float(np.nextafter(a, 0.0)), False)):
                        if atol not in seen:
                            seen[atol] = models_of(mul, B, atol=atol, max_iterations=sec.BUDGET)
                            for every in (1, 0):
                                check_call(seen[atol], solve(h, B, atol=atol, max_iterations=sec.BUDGET, check_every=every), (m, j, atol, every))
                        mine = seen[atol][j]
                        assert ((mine["iterations"], mine["end"]) == (its, end)) == there and (not there or mine["status"] == cgc.CONVERGED), (m, j, atol)
    assert places == {"begin:converged", "direction:converged"}, places


# ----------------------------------------------------------------------------- f. the timer runs the solve's arithmetic
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("k", [3, 16])
def test_the_timed_launches_do_the_arithmetic_of_the_solve(k, dtype):
    import torch
    csr = cgc.tri(1026, dtype)
    m = csr.m
    rng = np.random.default_rng(5)
    B, guess, jac = ccc.columns(m, k, dtype, 7), rng.uniform(-1, 1, (m, k)).astype(dtype), rng.uniform(0.5, 1.5, m).astype(dtype)
    tdt = torch.from_numpy(B).dtype

    def timed(X0, dinv, pad, budget, warmup, iters):
        """time_cg_columns_iterations on device operands (pad: ldb = k + 3 and ldx = k + 1, B's padding NaN, X's canaries) -> X afterwards"""
        ldb, ldx = (k + 3, k + 1) if pad else (k, k)
        Bw = torch.full((m, ldb), float("nan"), dtype=tdt, device=DEV)
        Bw[:, :k] = torch.from_numpy(B)
        Xw = torch.full((m, ldx), CANARY, dtype=tdt, device=DEV)
        if X0 is not None:
            Xw[:, :k] = torch.from_numpy(X0)
        mean, runs = ROW.timer(h.h, Bw[:, :k], Xw[:, :k], budget, x0=X0 is not None, dinv=None if dinv is None else torch.from_numpy(dinv).to(DEV),
                                                    warmup=warmup, iters=iters)
        torch.cuda.synchronize()
        out = Xw.cpu().numpy()
        assert mean > 0 and runs.shape == (iters,) and (runs > 0).all() and (out[:, k:] == CANARY).all(), (pad, "a canary beside X")
        return np.ascontiguousarray(out[:, :k])

    with handle(csr) as h:
        mul = ccc.spmm_column(h)
        for dinv in (None, jac):
            assert all(ended(mo) == (cgc.MAX_ITERATIONS, 8, "budget") for mo in models_of(mul, B, None, dinv, max_iterations=8))   # still running at 6
            models = models_of(mul, B, None, dinv, max_iterations=6)
            want = solve(h, B, dinv=dinv, max_iterations=6)
            check_call(models, want, "from zero")
            from_guess = solve(h, B, guess, dinv=dinv, max_iterations=6)
            check_call(models_of(mul, B, guess, dinv, max_iterations=6), from_guess, "from the guess")
            half = solve(h, B, guess, dinv=dinv, max_iterations=3)[0]
            again = solve(h, B, half, dinv=dinv, max_iterations=3)[0]       # the solve restarted from its own result: not one run of 6
            assert not same(from_guess[0], want[0]) and not same(again, from_guess[0])
            for pad in (False, True):
                what = (pad, dinv is not None)
                assert same(timed(None, dinv, pad, 6, 1, 2), want[0]), ("timer", what)             # every run starts from x = 0
                assert same(timed(guess, dinv, pad, 6, 0, 1), from_guess[0]), ("timer, x0", what)  # one run: from the guess in X
                assert same(timed(guess, dinv, pad, 3, 1, 1), again), ("timer, x0 twice", what)    # the second run starts from what the first left in X


# ----------------------------------------------------------------------------- g. a long row, and two steps per workgroup
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_a_long_row_under_the_column_solver(dtype):
    """a dense first row and column: the first solve through spmm's long-row list"""
    csr = sec.arrow(2049, dtype, symmetric=True)
    rng = np.random.default_rng(6)
    B, guess = ccc.columns(csr.m, 5, dtype, 13), rng.uniform(-1, 1, (csr.m, 5)).astype(dtype)
    jac = (1.0 / cgc.diagonal(csr).astype(np.float64)).astype(dtype)
    with handle(csr) as h:
        assert h.info()["max_row_len"] == 2049
        mul = ccc.spmm_column(h)
        for X0, dinv in ((None, None), (guess, jac)):
            models = models_of(mul, B, X0, dinv, max_iterations=12)
            assert all(mo["iterations"] == 12 and np.isfinite(mo["x"]).all() for mo in models), [ended(mo) for mo in models]
            check_call(models, solve(h, B, X0, dinv=dinv, max_iterations=12), X0 is not None)


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_three_ends_and_a_running_column_at_two_steps_per_workgroup(dtype):
    cases = [sec.by_name(n) for n in sec.BIG_GROUP]
    csr, B, X0, _, _ = sec.columns_system(cases, sec.BIG, dtype)
    assert csr.m == sec.BIG
    longest = max(c.iterations for c in cases)
    with handle(csr) as h:
        mul = ccc.spmm_column(h)
        models = models_of(mul, B, X0, max_iterations=sec.BUDGET)
        declared(cases, models)
        for every in (1, 0):
            check_call(models, solve(h, B, X0, max_iterations=sec.BUDGET, check_every=every), every)
        short = models_of(mul, B, X0, max_iterations=longest - 1)
        declared(cases, short, longest - 1)
        check_call(short, solve(h, B, X0, max_iterations=longest - 1), "short")
