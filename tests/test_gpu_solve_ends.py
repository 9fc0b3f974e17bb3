"""GPU: every way spmv_hip_cg and spmv_hip_bicgstab can end, anywhere in an enqueued batch and on every executor (include/spmv_hip.h, "the
arithmetic contract").

The yardstick is the host model of tests/cg_cases.py / tests/bicgstab_cases.py driven by the SAME handle's spmv(); x, rr, bb, history, status
and iterations are compared bit for bit and no tolerance appears anywhere.  The one freedom: a NaN equals a NaN whatever its sign and payload
(the contract gives a NaN neither; numpy's and the device's differ in the sign).  The cases come from tests/solve_end_cases.py, whose every line
tests/test_solve_ends_host.py proves on the CPU first; here each case must also reach the (status, iterations, end) it declares under the
handle's own multiply -- bits that match a model which ends elsewhere would mean the INPUT is wrong, not the kernel.  The bodies that the
solvers share are in tests/solve_harness.py."""
import functools

import numpy as np
import pytest

import bicgstab_cases as bc
import cg_cases as cgc
import solve_end_cases as sec
import solve_harness as sh
from solve_harness import CANARY, DEV, EVERY, M, METHODS, NAMES, ended, handle, multiply_of, run_id, same

pytestmark = pytest.mark.gpu

SOLVERS = ("cg", "bicgstab")
BIG_CASES = {"bicgstab": "b_half_2", "cg": "c_rr_2"}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return sh.library()


def of(solver):
    """-> the solver's row, its model, its solve with rtol = 0 unless set, its check"""
    row = sh.ROWS[solver]
    return row, row.model, functools.partial(sh.solve0, row), functools.partial(sh.check, row)


def runs_of(solver):
    return [(c, d) for c in sec.CASES if c.solver == solver for d in c.dtypes]


# ----------------------------------------------------------------------------- 1. every end, anywhere in a batch, at every budget edge
@pytest.mark.parametrize("run", runs_of("bicgstab") + runs_of("cg"), ids=run_id)
def test_every_end_at_every_place_in_a_batch(run):
    case, dtype = run
    k = case.iterations
    _, model_of, solve, check = of(case.solver)
    for m in sec.SIZES:
        for pre in (False, True) if case.solver == "bicgstab" and case.dinv is None else (False,):
            csr, b, dinv, x0 = sec.system(case, m // 2, dtype, pre)
            what = (case.name, m, pre)
            with handle(csr) as h:
                model = model_of(h, b, x0=x0, dinv=dinv, max_iterations=sec.BUDGET)
                assert ended(model) == (case.status, k, case.end), (what, ended(model), "the case does not reach its end on this multiply")
                for every in EVERY:
                    x, res = solve(h, b, x0, dinv=dinv, max_iterations=sec.BUDGET, check_every=every)
                    check(model, x, res, what + (every,))

                def expect(budget, short):
                    if budget < k or (budget == k and sec.first_kernel(case)):      # found while starting iteration k + 1: not with a budget of k
                        assert ended(short) == (cgc.MAX_ITERATIONS, budget, "budget"), (what, budget)
                    else:
                        assert ended(short) == ended(model), (what, budget)
                sh.budget_edges(k, lambda budget: model_of(h, b, x0=x0, dinv=dinv, max_iterations=budget),
                                lambda budget, every: solve(h, b, x0, dinv=dinv, max_iterations=budget, check_every=every), expect, what, check)


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", SOLVERS)
def test_an_exact_case_at_two_steps_per_workgroup(solver, dtype):
    case = sec.by_name(BIG_CASES[solver])
    assert case.exact
    _, model_of, solve, check = of(solver)
    csr, b, dinv, x0 = sec.system(case, sec.BIG // 2, dtype)
    with handle(csr) as h:
        model = model_of(h, b, x0=x0, dinv=dinv, max_iterations=sec.BUDGET)
        assert ended(model) == (case.status, case.iterations, case.end)
        for every in (1, 0):
            x, res = solve(h, b, x0, dinv=dinv, max_iterations=sec.BUDGET, check_every=every)
            check(model, x, res, every)
        x, res = solve(h, b, x0, dinv=dinv, max_iterations=case.iterations - 1)
        assert (res["status"], res["iterations"]) == (cgc.MAX_ITERATIONS, case.iterations - 1) and same(x, model["iterates"][case.iterations - 1])


# ----------------------------------------------------------------------------- 2. atol
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", SOLVERS)
def test_atol_decides_with_less_or_equal(solver, dtype):
    """On exact cases some rr on the way is the square of a double a.  atol = a must end the run there (the test is <=) and the next double
    below must not; with a small rtol beside it atol still decides, and with a small atol beside a large rtol, rtol does."""
    _, model_of, solve, check = of(solver)
    places = set()
    for case in (c for c in sec.CASES if c.solver == solver and c.exact and c.status != cgc.NONFINITE):
        for m in sec.ATOL_SIZES:
            csr, b, dinv, x0 = sec.system(case, m // 2, dtype)
            with handle(csr) as h:
                def model(atol, rtol=0.0):
                    return model_of(h, b, x0=x0, dinv=dinv, rtol=rtol, atol=atol, max_iterations=sec.BUDGET)

                def run(**kw):
                    return solve(h, b, x0, dinv=dinv, max_iterations=sec.BUDGET, **kw)
                for a, k, end in sec.atol_probes(model):
                    what = (case.name, m, a, k, end)
                    places.add(end)

                    def before(at, under):
                        assert (at["iterations"], at["end"], at["status"]) == (k, end, cgc.CONVERGED) and (under["iterations"], under["end"]) != (k, end), what
                    sh.atol_ladder(model, run, check, a, k, what, before)
    assert places == ({"begin:converged", "direction:converged"} | ({"update:ss_converged"} if solver == "bicgstab" else set())), places


# ----------------------------------------------------------------------------- 3. state between solves
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", SOLVERS)
def test_a_solve_is_unaffected_by_what_earlier_solves_left(solver, dtype):
    """One handle, one matrix that holds the blocks of several cases side by side and a tridiagonal tail (the right-hand side chooses whose
    recurrence runs): solves that leave NaN and infinity in r, p, the scratch vectors, y and the partial arrays; an ordinary solve without and
    with Dinv; one of each breakdown; the ordinary solve again."""
    _, model_of, solve, check = of(solver)
    cases, csr, select = sec.state_system(solver, dtype)
    jac = (2.0 ** np.random.default_rng(11).integers(-1, 2, csr.m)).astype(dtype)
    huge = np.full(csr.m, np.finfo(dtype).max, dtype=dtype)
    ordinary, _, _ = select(None, 1)
    with handle(csr) as h:
        mul = multiply_of(h)

        def both(b, x0=None, dinv=None, budget=sec.BUDGET, every=0):
            model = model_of(h, b, x0=x0, dinv=dinv, max_iterations=budget)
            x, res = solve(h, b, x0, dinv=dinv, max_iterations=budget, check_every=every)
            check(model, x, res, (model["end"], every))
            return model

        def the_ordinary_solves():
            for dinv in (None, jac):
                model = both(ordinary, dinv=dinv, budget=6)
                assert ended(model) == (cgc.MAX_ITERATIONS, 6, "budget") and np.isfinite(model["x"]).all()

        def the_nonfinite_solves():
            first = both(ordinary, x0=huge, dinv=jac)             # r = b - A x0 overflows in every row: NaN and infinity from the init kernel on
            assert ended(first) == (cgc.NONFINITE, 0, "begin:nonfinite") and (~np.isfinite(mul(huge))).sum() > csr.m // 2
            b, dinv, x0 = select(len(cases) - 1)                  # ... and one that overflows inside the loop: the scratch vectors, their partials
            later = both(b, x0, dinv, every=3)
            assert ended(later) == (cgc.NONFINITE, cases[-1].iterations, cases[-1].end) and later["iterations"] >= 1

        the_nonfinite_solves()                                    # the first use of the handle: they allocate the workspace
        the_ordinary_solves()
        for j, case in enumerate(cases):
            b, dinv, x0 = select(j)
            for every in (0, 1):
                model = both(b, x0, dinv, every=every)
                assert ended(model) == (case.status, case.iterations, case.end), (case.name, ended(model))
        the_ordinary_solves()
        the_nonfinite_solves()
        both(*[select(1)[i] for i in (0, 2, 1)])                  # a breakdown directly behind a NONFINITE solve
        the_ordinary_solves()


# ----------------------------------------------------------------------------- 4. the timer runs the solve's arithmetic
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", SOLVERS)
def test_the_timed_launches_do_the_arithmetic_of_the_solve(solver, dtype):
    import torch
    row, model_of, solve, _ = of(solver)
    csr = row.tri(1026, dtype)
    rng = np.random.default_rng(5)
    b, guess, jac = cgc.rhs(csr.m, dtype, 7), rng.uniform(-1, 1, csr.m).astype(dtype), rng.uniform(0.5, 1.5, csr.m).astype(dtype)
    with handle(csr) as h:
        for dinv in (None, jac):
            model = model_of(h, b, dinv=dinv, max_iterations=8)
            assert ended(model) == (cgc.MAX_ITERATIONS, 8, "budget")              # still running at k = 6
            want, res = solve(h, b, dinv=dinv, max_iterations=6)
            assert (res["status"], res["iterations"]) == (cgc.MAX_ITERATIONS, 6) and same(want, model["iterates"][6])
            bd, jd = torch.from_numpy(b).to(DEV), None if dinv is None else torch.from_numpy(dinv).to(DEV)
            xd = torch.full((csr.m,), CANARY, dtype=bd.dtype, device=DEV)
            mean, runs = row.timer(h.h, bd, xd, 6, dinv=jd, warmup=1, iters=2)       # every run starts from x = 0
            torch.cuda.synchronize()
            assert mean > 0 and runs.shape == (2,) and same(xd.cpu().numpy(), want), ("timer", dinv is not None)
            from_guess, res = solve(h, b, guess, dinv=dinv, max_iterations=6)
            assert res["iterations"] == 6 and not same(from_guess, want)
            xd.copy_(torch.from_numpy(guess))
            row.timer(h.h, bd, xd, 6, x0=True, dinv=jd, warmup=0, iters=1)           # one run: from the guess in X
            torch.cuda.synchronize()
            assert same(xd.cpu().numpy(), from_guess), ("timer, x0", dinv is not None)
            # a second run with use_x0 starts from what the first left in X (include/spmv_hip_tools.h): two runs of 3 are not one run of 6 ...
            again, _ = solve(h, b, solve(h, b, guess, dinv=dinv, max_iterations=3)[0], dinv=dinv, max_iterations=3)
            xd.copy_(torch.from_numpy(guess))
            row.timer(h.h, bd, xd, 3, x0=True, dinv=jd, warmup=1, iters=1)
            torch.cuda.synchronize()
            assert same(xd.cpu().numpy(), again) and not same(again, from_guess), ("timer, x0 twice", dinv is not None)


# ----------------------------------------------------------------------------- 5. the solvers on every executor
def twelve_iterations(h, solver, csr, dtype, seed, jac=None):
    """12 iterations without and with a guess and Dinv (1 / diagonal unless one is given), against the model on this handle's spmv()"""
    sh.guess_and_jacobi_iterations(sh.ROWS[solver], h, csr, dtype, seed, 12, jac)


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("method", METHODS, ids=lambda mth: mth.name)
@pytest.mark.parametrize("solver", SOLVERS)
def test_every_executor_under_the_solvers(solver, method, dtype):
    csr = sec.arrow(2049, dtype, symmetric=solver == "cg")
    sh.every_executor(csr, method, lambda h, seed: twelve_iterations(h, solver, csr, dtype, seed))


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", SOLVERS)
def test_the_long_row_launch_beside_the_tile_kernel_and_packed_tiles(solver, dtype):
    sh.the_long_row_launch_beside_the_tile_kernel(dtype, lambda h, csr, seed: twelve_iterations(h, solver, csr, dtype, seed))


@functools.lru_cache(maxsize=None)
def partly_local(kind):
    """2^20 rows of 32 entries around the diagonal with every tenth row, or the last tenth of the rows, on random columns: the partly local
    matrices of tests/test_gpu_routing.py at the size from which create() builds the pair A_near + A_far and times it against the schedule as
    built (kernels/split.hpp).  In fp64: every value is exact in fp32 too"""
    m = 1 << 20
    return sec.band32(m, np.float64, every=10) if kind == "every10" else sec.band32(m, np.float64, tail=m // 10)


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("method", [M.Method_Parallel, M.Method_CSR5SPMV], ids=lambda mth: mth.name)
@pytest.mark.parametrize("kind", ["every10", "tail10"])
def test_a_split_handle_under_the_solvers(kind, method, dtype):
    """create() keeps a split only where it measures the pair faster.  Where it did (far_nnz > 0) the near part writes y and the far part adds
    into it under both solvers; where it did not, the pair was built and timed and lost on the clock, and the handle that is left is one of
    the executors of test_every_executor_under_the_solvers"""
    wide = partly_local(kind)
    csr = wide if dtype == np.float64 else bc.synth.CSR(wide.m, wide.n, wide.rowptr, wide.colidx, wide.val.astype(dtype))
    with handle(csr, method) as h:
        info = h.info()
        assert info["split_ms"][0] > 0 and info["split_ms"][1] > 0, info                    # create() built and timed the pair
        print(f"{kind} {method.name} {NAMES[dtype]}: far_nnz {info['far_nnz']}, split_ms {info['split_ms']}, {info['launch_kernels']}")
        if info["far_nnz"] > 0:
            assert 0.08 * info["nnz"] <= info["far_nnz"] <= 0.13 * info["nnz"], info         # about a tenth of the entries is far
            jac = np.random.default_rng(9).uniform(1 / 32, 1 / 16, csr.m).astype(dtype)
            for solver in SOLVERS:
                twelve_iterations(h, solver, csr, dtype, 5, jac)
        else:
            assert info["split_ms"][1] >= 0.9 * info["split_ms"][0], info                   # rejected only because it was not faster
