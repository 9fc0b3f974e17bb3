"""GPU: every way spmv_hip_cg_mixed can end, behind every kind of segment end, anywhere in an enqueued batch and on every executor
(include/spmv_hip.h, "mixed-precision conjugate gradients"); the sections are those of tests/test_gpu_solve_ends.py.

The yardstick is the host model of tests/cg_mixed_cases.py driven by the SAME pair's two spmv(); x, status, iterations, updates, rr, bb and the
history are compared bit for bit and no tolerance appears anywhere.  The one freedom: a NaN equals a NaN whatever its sign and payload.  The
cases come from tests/cg_mixed_end_cases.py, whose every line tests/test_cg_mixed_ends_host.py proves on the CPU first; here each case must also
reach the (status, iterations, updates, end, segments) it declares under the pair's own multiplies -- bits that match a model which ends
elsewhere would mean the INPUT is wrong, not the kernel.  The bodies that the solvers share are in tests/solve_harness.py."""
import functools

import numpy as np
import pytest

import cg_cases as cgc
import cg_mixed_cases as mix
import cg_mixed_end_cases as me
import solve_end_cases as sec
import solve_harness as sh
from solve_harness import CANARY, DEV, EVERY, EXECUTORS, M, METHODS, multiplies_of, pair, same

pytestmark = pytest.mark.gpu

ROW = sh.ROWS["cg_mixed"]
# the runs of the atol test (tests/test_cg_mixed_ends_host.py looks first): a segment that ends by the estimate test and a committed rr that converges
ATOL_CASES = ("m_resume_converged_after_estimate", "m_resume_converged_after_every", "m_resume_converged_after_drop",
              "m_resume_budget_after_estimate")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return sh.library()


check = functools.partial(sh.check, ROW)


def solve(hi, lo, b, x0=None, **kw):
    return sh.solve(ROW, (hi, lo), b, x0, **kw)


def signature(r):
    return r["status"], r["iterations"], r["updates"], r["end"], tuple(r["segments"])


def declared(case):
    return case.status, case.iterations, case.updates, case.end, case.segments


# ----------------------------------------------------------------------------- 1. every end, anywhere in a batch, at every budget edge
@pytest.mark.parametrize("case", me.CASES, ids=lambda c: c.name)
def test_every_end_at_every_place_in_a_batch(case):
    for m in me.SIZES:
        high, low, b, dinv, x0 = me.system(case, m // 2)
        what = (case.name, m)
        with pair(high, low) as (hi, lo):
            mh, ml = multiplies_of(hi, lo)

            def run(watch=None, **kw):
                return mix.cg_mixed(mh, ml, b, x0=x0, dinv=dinv, watch=watch, **me.options(case, **kw))
            model, trace = me.traced(run)
            assert signature(model) == declared(case), (what, signature(model), "the case does not reach its end on these multiplies")
            if case.name.startswith("m_rise_"):                  # committed although the true residual rose: x moved, the update counts
                assert set(me.rises(trace)) & {"every", "budget"} and model["status"] != mix.STAGNATED and model["updates"] >= 1, (what, trace)
            e = case.every
            for every in sorted(set(EVERY) | ({e - 1, e, e + 1} - {0, -1} if e > 0 else set())):
                x, res = solve(hi, lo, b, x0, dinv=dinv, check_every=every, **me.options(case))
                check(model, x, res, what + (every,))
            # budgets on, one before and one behind the end and every segment's end: `resume` comes before the budget test
            around = sorted({case.iterations} | {at for at, *_ in trace})
            for budget in sorted({k + d for k in around for d in (-1, 0, 1) if 0 <= k + d <= case.budget}):
                short = run(max_iterations=budget)
                assert short["iterations"] <= budget
                for every in (0, 1):
                    x, res = solve(hi, lo, b, x0, dinv=dinv, check_every=every, **me.options(case, max_iterations=budget))
                    check(short, x, res, what + ("budget", budget, every))


def test_a_case_at_two_steps_per_workgroup():
    case = me.by_name(me.BIG_CASE)
    high, low, b, dinv, x0 = me.system(case, me.BIG // 2)
    with pair(high, low) as (hi, lo):
        mh, ml = multiplies_of(hi, lo)
        model = mix.cg_mixed(mh, ml, b, x0=x0, dinv=dinv, **me.options(case))
        assert signature(model) == declared(case) and case.iterations >= 1 and case.updates >= 1
        for every in (1, 0):
            x, res = solve(hi, lo, b, x0, dinv=dinv, check_every=every, **me.options(case))
            check(model, x, res, every)
        short = mix.cg_mixed(mh, ml, b, x0=x0, dinv=dinv, **me.options(case, max_iterations=case.iterations - 1))
        x, res = solve(hi, lo, b, x0, dinv=dinv, **me.options(case, max_iterations=case.iterations - 1))
        check(short, x, res, "short")


# ----------------------------------------------------------------------------- 2. atol
def test_atol_decides_with_less_or_equal():
    """The estimate test (rs <= thr ends a segment) and the committed rr after an update (resume:converged): where the value compared is the
    square of a double a, atol = a must decide there and the next double below must not; a small rtol beside atol changes nothing, and a large
    rtol beside a small atol decides instead."""
    places = set()
    for case in (me.by_name(n) for n in ATOL_CASES):
        for m in me.SIZES[:3]:
            high, low, b, dinv, x0 = me.system(case, m // 2)
            with pair(high, low) as (hi, lo):
                mh, ml = multiplies_of(hi, lo)

                def model(atol, watch=None, rtol=0.0):
                    return mix.cg_mixed(mh, ml, b, x0=x0, dinv=dinv, watch=watch, **me.options(case, rtol=rtol, atol=atol))

                def run(atol, rtol=0.0, **kw):
                    return solve(hi, lo, b, x0, dinv=dinv, **me.options(case, rtol=rtol, atol=atol), **kw)
                for a, k, where in me.atol_probes(model):
                    what = (case.name, m, a, k, where)
                    places.add(where)

                    def before(at, under):
                        assert signature(at) != signature(under) or not same(at["x"], under["x"]) or at["rr"] != under["rr"], what
                    sh.atol_ladder(model, run, check, a, k, what, before, same_end=lambda p, q: signature(p) == signature(q) and same(p["x"], q["x"]),
                                   target=lambda at, a: a * a, converges=False)
    assert places == {"estimate", "resume:converged"}, places


# ----------------------------------------------------------------------------- 3. state between solves
def test_a_solve_is_unaffected_by_what_earlier_solves_left():
    """One pair, one pair of matrices that hold the blocks of several cases side by side and a tridiagonal tail (the right-hand side chooses
    whose recurrence runs): solves that leave NaN and infinity in xn, q64, r, p, q, y and the partial arrays; an ordinary solve without and
    with Dinv; one of each end; the ordinary solves again; Handle.cg on either handle in between, each against its own model."""
    cases, high, low, select = me.state_system()
    jac = (2.0 ** np.random.default_rng(11).integers(-1, 2, high.m)).astype(np.float32)
    huge = np.full(high.m, np.finfo(np.float64).max)
    ordinary, _, _ = select(None, 1)
    with pair(high, low) as (hi, lo):
        mh, ml = multiplies_of(hi, lo)

        def both(b, x0=None, dinv=None, every=0, **kw):
            model = mix.cg_mixed(mh, ml, b, x0=x0, dinv=dinv, **kw)
            x, res = solve(hi, lo, b, x0, dinv=dinv, check_every=every, **kw)
            check(model, x, res, (model["end"], every))
            return model

        def the_ordinary_solves():
            for dinv in (None, jac):
                model = both(ordinary, dinv=dinv, rtol=0.0, max_iterations=7, update_every=3)
                assert (model["status"], model["iterations"], model["end"]) == (mix.MAX_ITERATIONS, 7, "resume:budget") and model["updates"] == 3
                assert np.isfinite(model["x"]).all()

        def the_single_solves():
            """Handle.cg on `high` and on `low`: their own workspaces, between mixed solves that share the handles"""
            for h, mul, b in ((hi, mh, ordinary), (lo, ml, ordinary.astype(np.float32))):
                model = cgc.cg(mul, b, max_iterations=6)
                x, res, hist = h.cg(b, np.full(b.size, CANARY, dtype=b.dtype), rtol=0.0, max_iterations=6, history=True)
                assert (res["status"], res["iterations"]) == (model["status"], model["iterations"]) == (cgc.MAX_ITERATIONS, 6)
                assert same(x, model["x"]) and same(hist, model["history"]) and res["rr"] == model["rr"]

        def the_nonfinite_solves():
            first = both(ordinary, x0=huge, dinv=jac, rtol=0.0, max_iterations=5)      # r64 = b - A x0 overflows in every row
            assert (first["status"], first["iterations"], first["end"]) == (mix.NONFINITE, 0, "start:nonfinite") and (~np.isfinite(mh(huge))).sum() > high.m // 2
            last = cases[-1]
            b, dinv, x0 = select(len(cases) - 1)                                       # ... and one that overflows inside the loop
            later = both(b, x0, dinv, every=3, **me.options(last))
            assert signature(later) == declared(last) and last.status == mix.NONFINITE and last.iterations >= 1

        def one_of_each_end():
            for j, case in enumerate(cases):
                b, dinv, x0 = select(j)
                for every in (0, 1):
                    model = both(b, x0, dinv, every=every, **me.options(case))
                    assert signature(model) == declared(case), (case.name, signature(model))

        the_nonfinite_solves()                                    # the first use of the pair: they allocate the workspace
        the_ordinary_solves()
        the_single_solves()
        one_of_each_end()
        the_ordinary_solves()
        the_nonfinite_solves()
        j = next(i for i, c in enumerate(cases) if c.status == mix.BREAKDOWN)
        b, dinv, x0 = select(j)
        model = both(b, x0, dinv, **me.options(cases[j]))         # a BREAKDOWN directly behind a NONFINITE solve
        assert signature(model) == declared(cases[j])
        the_single_solves()
        the_ordinary_solves()


# ----------------------------------------------------------------------------- 4. the timer runs the solve's arithmetic
def test_the_timed_launches_do_the_arithmetic_of_the_solve():
    import torch
    high = cgc.tri(1026)
    low = mix.narrowed(high)
    rng = np.random.default_rng(5)
    b, guess, jac = cgc.rhs(high.m, np.float64, 7), rng.uniform(-1, 1, high.m), rng.uniform(0.5, 1.5, high.m).astype(np.float32)
    e = 3
    with pair(high, low) as (hi, lo):
        mh, ml = multiplies_of(hi, lo)
        for dinv in (None, jac):
            for x0 in (None, guess):
                # update_drop next to 0 and no tolerance: every segment ends by "every", and every update lowers rr, so the timer's "every update is
                # committed" and the solve agree
                kw = dict(rtol=0.0, atol=0.0, max_iterations=3 * e, update_every=e, update_drop=1e-30)
                model, trace = me.traced(lambda watch: mix.cg_mixed(mh, ml, b, x0=x0, dinv=dinv, watch=watch, **kw))
                assert model["segments"] == ["every"] * 3 and model["updates"] == 3 and all(t[3] < t[2] and t[4] for t in trace), trace
                want, res = solve(hi, lo, b, x0, dinv=dinv, **kw)
                check(model, want, res, ("solve", dinv is not None, x0 is not None))
                bd, jd = torch.from_numpy(b).to(DEV), None if dinv is None else torch.from_numpy(dinv).to(DEV)
                xd = torch.full((high.m,), CANARY, dtype=torch.float64, device=DEV) if x0 is None else torch.from_numpy(x0).to(DEV)
                # one run when it starts from X (a second would start from what the first left), two from x = 0
                mean, runs = ROW.timer(hi.h, lo.h, bd, xd, 3 * e, update_every=e, x0=x0 is not None, dinv=jd, warmup=0 if x0 is not None else 1,
                                                          iters=1 if x0 is not None else 2)
                torch.cuda.synchronize()
                assert mean > 0 and (runs > 0).all() and same(xd.cpu().numpy(), want), ("timer", dinv is not None, x0 is not None)
            # a second run with use_x0 starts from what the first left in X: two runs of e are a solve of e from the solve of e's x
            first, _ = solve(hi, lo, b, guess, dinv=dinv, rtol=0.0, max_iterations=e, update_every=e, update_drop=1e-30)
            again, res = solve(hi, lo, b, first, dinv=dinv, rtol=0.0, max_iterations=e, update_every=e, update_drop=1e-30)
            assert res["updates"] == 1 and not same(again, first)
            xd = torch.from_numpy(guess).to(DEV)
            ROW.timer(hi.h, lo.h, bd, xd, e, update_every=e, x0=True, dinv=jd, warmup=1, iters=1)
            torch.cuda.synchronize()
            assert same(xd.cpu().numpy(), again), ("timer, x0 twice", dinv is not None)


# ----------------------------------------------------------------------------- 5. cg_mixed on every executor
def twelve_iterations(hi, lo, high, seed):
    """rtol = 0 and update_every = 5 for 12 iterations, without and with a guess and Jacobi, against the model on this pair's own multiplies"""
    rng = np.random.default_rng(seed)
    b, guess = cgc.rhs(high.m, np.float64, seed), rng.uniform(-1, 1, high.m)
    jac = (1.0 / cgc.diagonal(high)).astype(np.float32)
    mh, ml = multiplies_of(hi, lo)
    for x0, dinv in ((None, None), (guess, jac)):
        kw = dict(rtol=0.0, max_iterations=12, update_every=5)
        model = mix.cg_mixed(mh, ml, b, x0=x0, dinv=dinv, **kw)
        assert model["iterations"] == 12 and model["updates"] >= 2 and np.isfinite(model["x"]).all(), signature(model)
        x, res = solve(hi, lo, b, x0, dinv=dinv, **kw)
        check(model, x, res, (x0 is not None,))


def arrow_pair():
    high = sec.arrow(2049, np.float64, symmetric=True)
    return high, mix.narrowed(high)                               # every entry is exact in fp32


def check_arrow_executor(h, method):
    sh.check_executor_layout(h.info(), method)


@pytest.mark.parametrize("method", METHODS, ids=lambda mth: mth.name)
def test_every_executor_under_cg_mixed(method):
    """both sides on the same method: the arrow matrix of tests/test_gpu_solve_ends.py as built, and on the row-block x column-slab executor
    (cache_block = 2; CSR-scalar schedules never take it)"""
    high, low = arrow_pair()
    with pair(high, low, method) as (hi, lo):
        check_arrow_executor(hi, method), check_arrow_executor(lo, method)
        twelve_iterations(hi, lo, high, 1)
    if EXECUTORS[method][0] == "csr_scalar_kernel":
        return
    with pair(high, low, method, high_opts=dict(cache_block=2), low_opts=dict(cache_block=2)) as (hi, lo):
        sh.check_blocked_layout(hi.info()), sh.check_blocked_layout(lo.info())
        twelve_iterations(hi, lo, high, 2)


def check_band_executor(h, csr, pack):
    sh.check_tile_layout(h.info(), csr, pack)


@pytest.mark.parametrize("pack", [0, 1])
def test_the_long_row_launch_beside_the_tile_kernel_and_packed_tiles(pack):
    """rows of 32 aligned entries at 8 lanes per row run on the CSR-vector TILE kernel; row 300 (544 entries > long_thr = 512) goes to the
    long-row launch behind it.  pack = 1: every tile of `high` but row 300's streams 7-byte values"""
    high = sec.band32(1280, np.float64, long_row=300)
    low = mix.narrowed(high)
    with pair(high, low, M.Method_Parallel, high_opts=dict(lanes_per_row=8, pack_values=pack), low_opts=dict(lanes_per_row=8)) as (hi, lo):
        check_band_executor(hi, high, pack), check_band_executor(lo, low, 0)
        twelve_iterations(hi, lo, high, 3 + pack)


def test_a_packed_parallel_high_beside_a_sell_low():
    high = sec.band32(1280, np.float64, long_row=300)
    low = mix.narrowed(high)
    with pair(high, low, M.Method_Parallel, M.Method_SellCSigma, high_opts=dict(lanes_per_row=8, pack_values=1)) as (hi, lo):
        check_band_executor(hi, high, 1)
        assert lo.info()["launch_kernels"][0] == EXECUTORS[M.Method_SellCSigma][0], lo.info()
        twelve_iterations(hi, lo, high, 5)


def test_a_csr5_high_beside_a_parallel_low():
    high, low = arrow_pair()
    with pair(high, low, M.Method_CSR5SPMV, M.Method_Parallel) as (hi, lo):
        check_arrow_executor(hi, M.Method_CSR5SPMV), check_arrow_executor(lo, M.Method_Parallel)
        twelve_iterations(hi, lo, high, 6)
