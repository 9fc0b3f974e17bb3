"""GPU: every way spmv_hip_gmres can end, at every step of a cycle, anywhere in an enqueued batch and on every executor (include/spmv_hip.h, "the
arithmetic contract"); the sections are those of tests/test_gpu_solve_ends.py.

The yardstick is the host model of tests/gmres_cases.py driven by the SAME handle's spmv(); x, rr, bb, history, status and iterations are
compared bit for bit and no tolerance appears anywhere.  The one freedom: a NaN equals a NaN whatever its sign and payload; and, as in
tests/test_gpu_gmres.py, rr, bb and the history are not compared where the solve ends in begin:nonfinite.  The cases come from
tests/gmres_end_cases.py, whose every line tests/test_gmres_ends_host.py proves on the CPU first; here each case must also reach the (status,
iterations, end) it declares under the handle's own multiply -- bits that match a model which ends elsewhere would mean the INPUT is wrong,
not the kernel.  The bodies that the solvers share are in tests/solve_harness.py."""
import functools

import numpy as np
import pytest

import gmres_cases as gc
import gmres_end_cases as ge
import solve_end_cases as sec
import solve_harness as sh
from solve_harness import CANARY, DEV, EVERY, METHODS, NAMES, ended, handle, multiply_of, run_id, same

pytestmark = pytest.mark.gpu

ROW = sh.ROWS["gmres"]
G = gc.GROUP
RUNS = [(c, d) for c in ge.CASES for d in c.dtypes]
HISTORY_RUNS = [(c, d) for c in ge.HISTORY_CASES for d in ge.BOTH]
# the runs of the atol test: exact or not, some estimate on their way is the square of a double (tests/test_gmres_ends_host.py looks first)
ATOL_CASES = ("g_begin_conv", "g_cyclic_2", "g_restart_zero_64_c2s3", "g_restart_zero_32_c5s2", "g_rotate_converged_32_c2s1", "g_restart_zero_64_c1s2")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return sh.library()


check = functools.partial(sh.check, ROW)


def solve(h, b, restart, x0=None, **kw):
    return sh.solve0(ROW, h, b, x0, restart=restart, **kw)


def model_of(h, case, b, dinv, x0, **kw):
    kw.setdefault("atol", case.atol)
    kw.setdefault("max_iterations", case.budget)
    return ROW.model(h, b, case.restart, x0=x0, dinv=dinv, **kw)


# ----------------------------------------------------------------------------- 1. every end, anywhere in a batch, at every budget edge
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_every_end_at_every_place_in_a_batch(run):
    case, dtype = run
    k, s, R = case.iterations, len(case.block), case.restart
    for m in ge.sizes(case):
        csr, b, dinv, x0 = ge.system(case, m // s, dtype)
        what = (case.name, m)
        with handle(csr) as h:
            model = model_of(h, case, b, dinv, x0)
            assert ended(model) == (case.status, k, case.end), (what, ended(model), "the case does not reach its end on this multiply")
            for every in EVERY + (R,):
                x, res = solve(h, b, R, x0, dinv=dinv, atol=case.atol, max_iterations=case.budget, check_every=every)
                check(model, x, res, what + (every,))

            def expect(budget, short):
                if budget < k or (budget == k and ge.found_making_a_step(case)) or case.end == "budget":
                    assert ended(short) == (gc.MAX_ITERATIONS, budget, "budget"), (what, budget)       # found while making step k + 1: not with a budget of k
                else:
                    assert ended(short) == ended(model), (what, budget)
            sh.budget_edges(k, lambda budget: model_of(h, case, b, dinv, x0, max_iterations=budget),
                            lambda budget, every: solve(h, b, R, x0, dinv=dinv, atol=case.atol, max_iterations=budget, check_every=every), expect, what, check)


@pytest.mark.parametrize("run", HISTORY_RUNS, ids=run_id)
def test_an_atol_from_the_history_ends_a_later_cycle(run):
    """rotate:converged at step 1 and in the middle of a later cycle: x holds the finished cycles and, in the middle, the pending columns that
    gmres_finish adds.  atol is the smallest double whose square reaches the model's own estimate at iteration k; the next double below runs on"""
    case, dtype = run
    R, k = case.restart, case.iterations
    for m in ge.HISTORY_SIZES:
        csr, b = gc.tri_ns(m, dtype), gc.rhs(m, dtype)
        with handle(csr) as h:
            mul = multiply_of(h)
            a, at, below = ge.history_probe(lambda atol: gc.gmres(mul, b, R, atol=atol, max_iterations=k + 3), k)
            assert ge.place(R, at["iterations"], at["end"]) == (case.cycle, case.step)
            for every in EVERY + (R,):
                x, res = solve(h, b, R, atol=a, max_iterations=k + 3, check_every=every)
                check(at, x, res, (case.name, m, every))
            for every in (1, 0):
                x, res = solve(h, b, R, atol=float(np.nextafter(a, 0.0)), max_iterations=k + 3, check_every=every)
                check(below, x, res, (case.name, m, every, "below"))


@pytest.mark.parametrize("dtype", ge.BOTH, ids=NAMES.get)
def test_a_case_at_two_steps_per_workgroup(dtype):
    case = ge.by_name(ge.BIG_CASE)
    s, R = len(case.block), case.restart
    csr, b, dinv, x0 = ge.system(case, ge.BIG // s, dtype)
    with handle(csr) as h:
        model = model_of(h, case, b, dinv, x0)
        assert ended(model) == (case.status, case.iterations, case.end)
        for every in (1, 0):
            x, res = solve(h, b, R, x0, dinv=dinv, atol=case.atol, max_iterations=case.budget, check_every=every)
            check(model, x, res, every)
        short = model_of(h, case, b, dinv, x0, max_iterations=case.iterations - 1)
        assert ended(short) == (gc.MAX_ITERATIONS, case.iterations - 1, "budget") and same(short["x"], model["iterates"][case.iterations - 1])
        x, res = solve(h, b, R, x0, dinv=dinv, atol=case.atol, max_iterations=case.iterations - 1)
        check(short, x, res, "short")


# ----------------------------------------------------------------------------- 2. atol
@pytest.mark.parametrize("dtype", ge.BOTH, ids=NAMES.get)
def test_atol_decides_with_less_or_equal(dtype):
    """Some estimate on the way is the square of a double a.  atol = a must end the run there (the test is <=) and the next double below must
    not; with a small rtol beside it atol still decides, and with a small atol beside a large rtol, rtol does."""
    places = set()
    for case in (ge.by_name(n) for n in ATOL_CASES if dtype in ge.by_name(n).dtypes):
        s, R = len(case.block), case.restart
        for m in ge.sizes(case)[:3]:
            csr, b, dinv, x0 = ge.system(case, m // s, dtype)
            with handle(csr) as h:
                mul = multiply_of(h)

                def model(atol, rtol=0.0):
                    return gc.gmres(mul, b, R, x0=x0, dinv=dinv, rtol=rtol, atol=atol, max_iterations=case.budget)

                def run(**kw):
                    return solve(h, b, R, x0, dinv=dinv, max_iterations=case.budget, **kw)
                probes = sec.atol_probes(model)
                for a, k, end in dict.fromkeys(probes[:2] + probes[-2:]):       # the first two and the last two places
                    what = (case.name, m, a, k, end)
                    places.add((end, "later" if k > R else "first"))

                    def before(at, under):
                        assert (at["iterations"], at["end"], at["status"]) == (k, end, gc.CONVERGED) and (under["iterations"], under["end"]) != (k, end), what
                    sh.atol_ladder(model, run, check, a, k, what, before)
    assert {p[0] for p in places} == {"begin:converged", "rotate:converged"} and ("rotate:converged", "later") in places, places


# ----------------------------------------------------------------------------- 3. state between solves
@pytest.mark.parametrize("dtype", ge.BOTH, ids=NAMES.get)
def test_a_solve_is_unaffected_by_what_earlier_solves_left(dtype):
    """One handle, one matrix that holds the blocks of several cases side by side and a tridiagonal tail (the right-hand side chooses whose
    recurrence runs): solves that leave NaN and infinity in the basis, in w and in the partial arrays; an ordinary solve without and with
    Dinv; one of each end; a larger restart, which allocates the workspace anew, and the NONFINITE solves in it; then smaller restarts, which
    run in the larger workspace over what those left."""
    cases, csr, select = ge.state_system(dtype)
    jac = (2.0 ** np.random.default_rng(11).integers(-1, 2, csr.m)).astype(dtype)
    huge = np.full(csr.m, np.finfo(dtype).max, dtype=dtype)
    ordinary, _, _ = select(None, 1)
    item = np.dtype(dtype).itemsize
    grown = gc.workspace_bytes(csr.m, item, G + 1) - gc.workspace_bytes(csr.m, item, 3)
    with handle(csr) as h:
        mul = multiply_of(h)

        def both(b, restart, x0=None, dinv=None, atol=0.0, budget=ge.BUDGET, every=0):
            model = gc.gmres(mul, b, restart, x0=x0, dinv=dinv, atol=atol, max_iterations=budget)
            x, res = solve(h, b, restart, x0, dinv=dinv, atol=atol, max_iterations=budget, check_every=every)
            check(model, x, res, (model["end"], restart, every))
            return model

        def the_ordinary_solves(restart):
            for dinv in (None, jac):
                for budget in (2 * restart, 2 * restart + 1):      # on a restart, and one step behind it
                    model = both(ordinary, restart, dinv=dinv, budget=budget)
                    assert ended(model) == (gc.MAX_ITERATIONS, budget, "budget") and np.isfinite(model["x"]).all()

        def the_nonfinite_solves(restart):
            first = both(ordinary, restart, x0=huge, dinv=jac)    # r = b - A x0 overflows in every row: NaN and infinity from the init kernel on
            assert ended(first) == (gc.NONFINITE, 0, "begin:nonfinite") and (~np.isfinite(mul(huge))).sum() > csr.m // 2
            b, dinv, x0 = select(len(cases) - 1)                  # ... and one that overflows inside the loop: w, the dots' partials
            last = cases[-1]
            later = both(b, last.restart, x0, dinv, every=3)
            assert ended(later) == (gc.NONFINITE, last.iterations, last.end) and later["iterations"] >= 1

        def one_of_each_end():
            for j, case in enumerate(cases):
                b, dinv, x0 = select(j)
                for every in (0, 1):
                    model = both(b, case.restart, x0, dinv, atol=case.atol, budget=case.budget, every=every)
                    assert ended(model) == (case.status, case.iterations, case.end), (case.name, ended(model))

        small, large = 3, G + 1
        assert max(c.restart for c in cases) <= small
        the_nonfinite_solves(small)                               # the first use of the handle: they allocate the workspace
        the_ordinary_solves(small)
        one_of_each_end()
        the_ordinary_solves(small)
        held = h.info()["device_bytes"]
        the_ordinary_solves(large)                                # a larger restart: the workspace is allocated anew (a longer history may grow too)
        assert h.info()["device_bytes"] - held >= grown > 0
        held = h.info()["device_bytes"]
        the_nonfinite_solves(large)                               # NaN and infinity in the larger workspace's vectors
        j = next(i for i, c in enumerate(cases) if c.status == gc.BREAKDOWN)
        b, dinv, x0 = select(j)
        model = both(b, cases[j].restart, x0, dinv)               # a BREAKDOWN directly behind a NONFINITE solve, a smaller restart in the larger workspace
        assert ended(model) == (gc.BREAKDOWN, cases[j].iterations, cases[j].end)
        the_ordinary_solves(small)
        one_of_each_end()
        the_ordinary_solves(large)
        assert h.info()["device_bytes"] == held                   # the smaller restarts ran in the larger workspace


# ----------------------------------------------------------------------------- 4. the timer runs the solve's arithmetic
@pytest.mark.parametrize("dtype", ge.BOTH, ids=NAMES.get)
def test_the_timed_launches_do_the_arithmetic_of_the_solve(dtype):
    import torch
    csr = gc.tri_ns(1026, dtype)
    rng = np.random.default_rng(5)
    b, guess, jac = gc.rhs(csr.m, dtype, 7), rng.uniform(-1, 1, csr.m).astype(dtype), rng.uniform(0.5, 1.5, csr.m).astype(dtype)
    R = 4
    with handle(csr) as h:
        for dinv in (None, jac):
            model = gc.gmres(multiply_of(h), b, R, dinv=dinv, max_iterations=3 * R)
            assert ended(model) == (gc.MAX_ITERATIONS, 3 * R, "budget")           # still running at 2 R + 2
            want, res = solve(h, b, R, dinv=dinv, max_iterations=2 * R)
            assert (res["status"], res["iterations"]) == (gc.MAX_ITERATIONS, 2 * R) and same(want, model["iterates"][2 * R])
            bd, jd = torch.from_numpy(b).to(DEV), None if dinv is None else torch.from_numpy(dinv).to(DEV)
            xd = torch.full((csr.m,), CANARY, dtype=bd.dtype, device=DEV)
            mean, runs = ROW.timer(h.h, bd, xd, 2 * R, restart=R, dinv=jd, warmup=1, iters=2)   # every run starts from x = 0
            torch.cuda.synchronize()
            assert mean > 0 and runs.shape == (2,) and same(xd.cpu().numpy(), want), ("timer", dinv is not None)
            # a budget that is no multiple of R leaves the last finished cycle's x: gmres_finish is not part of the timer
            for budget in (2 * R + 2, 2 * R + 1, R - 1):
                xd.fill_(CANARY)
                ROW.timer(h.h, bd, xd, budget, restart=R, dinv=jd, warmup=0, iters=1)
                torch.cuda.synchronize()
                assert same(xd.cpu().numpy(), model["iterates"][budget // R * R]) and not same(model["iterates"][budget], model["iterates"][budget // R * R]), ("timer", budget)
            from_guess, res = solve(h, b, R, guess, dinv=dinv, max_iterations=2 * R)
            assert res["iterations"] == 2 * R and not same(from_guess, want)
            xd.copy_(torch.from_numpy(guess))
            ROW.timer(h.h, bd, xd, 2 * R, restart=R, x0=True, dinv=jd, warmup=0, iters=1)       # one run: from the guess in X
            torch.cuda.synchronize()
            assert same(xd.cpu().numpy(), from_guess), ("timer, x0", dinv is not None)
            # a second run with use_x0 starts from what the first left in X; for GMRES(R) two runs of R ARE one run of 2 R: the restart forgets
            # everything but x, so the solve from the first run's x is the second cycle
            again, _ = solve(h, b, R, solve(h, b, R, guess, dinv=dinv, max_iterations=R)[0], dinv=dinv, max_iterations=R)
            xd.copy_(torch.from_numpy(guess))
            ROW.timer(h.h, bd, xd, R, restart=R, x0=True, dinv=jd, warmup=1, iters=1)
            torch.cuda.synchronize()
            assert same(xd.cpu().numpy(), again) and same(again, from_guess), ("timer, x0 twice", dinv is not None)


# ----------------------------------------------------------------------------- 5. gmres on every executor
def cycles_and_three(h, csr, dtype, seed):
    """R = G + 1, so that gmres_dots and gmres_sub_dots take their second trip, for 2 R + 3 iterations without and with a guess and Jacobi,
    against the model on this handle's spmv()"""
    sh.guess_and_jacobi_iterations(ROW, h, csr, dtype, seed, 2 * (G + 1) + 3, restart=G + 1)


@pytest.mark.parametrize("dtype", ge.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("method", METHODS, ids=lambda mth: mth.name)
def test_every_executor_under_gmres(method, dtype):
    csr = sec.arrow(2049, dtype, symmetric=False)
    sh.every_executor(csr, method, lambda h, seed: cycles_and_three(h, csr, dtype, seed))


@pytest.mark.parametrize("dtype", ge.BOTH, ids=NAMES.get)
def test_the_long_row_launch_beside_the_tile_kernel_and_packed_tiles(dtype):
    sh.the_long_row_launch_beside_the_tile_kernel(dtype, lambda h, csr, seed: cycles_and_three(h, csr, dtype, seed))
