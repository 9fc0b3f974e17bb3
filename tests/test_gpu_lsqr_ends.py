"""GPU: every way spmv_hip_lsqr can end, at every step, anywhere in an enqueued batch, at shapes whose two dots have different geometries and on
every executor (include/spmv_hip.h, "the arithmetic contract"); the sections are those of tests/test_gpu_solve_ends.py.

The yardstick is the host model of tests/lsqr_cases.py driven by the SAME handle's spmv() and spmv_transpose(); x, status, iterations, rr, bb,
ar, anorm and the history are compared bit for bit and no tolerance appears anywhere.  The one freedom: a NaN equals a NaN whatever its sign and
payload; and, as in tests/test_gpu_lsqr.py, rr, bb and the history are not compared where the solve ends in begin:nonfinite.  The cases come from
tests/lsqr_end_cases.py, whose every line tests/test_lsqr_ends_host.py proves on the CPU first; here each case must also reach the (status,
iterations, end) it declares under the handle's own multiplies -- bits that match a model which ends elsewhere would mean the INPUT is wrong,
not the kernel.  The bodies that the solvers share are in tests/solve_harness.py."""
import functools

import numpy as np
import pytest

import lsqr_cases as lc
import lsqr_end_cases as le
import solve_end_cases as sec
import solve_harness as sh
from solve_harness import CANARY, DEV, EVERY, METHODS, handle, multiplies_with_transpose, same
from spmv_amd import api

pytestmark = pytest.mark.gpu

ROW = sh.ROWS["lsqr"]
NAMES, RUNS, run_id, ended, declared = le.NAMES, le.RUNS, le.run_id, le.ended, le.declared


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return sh.library()


check = functools.partial(sh.check, ROW)
solve = functools.partial(sh.solve0, ROW)


def model_of(h, b, x0=None, **kw):
    kw.pop("check_every", None)
    return ROW.model(h, b, x0=x0, **kw)


def budget_edges(h, case, b, x0, model, what, everys=(0, 1), budgets=None):
    """budgets of iterations - 1, iterations and iterations + 1, each against a model run with that budget.  What a budget equal to the end's
    iteration reports (tests/test_gpu_lsqr.py: check_against): the end itself where lsqr_step finds it BEHIND the iteration it applied; where
    it is found while making iteration `iterations` + 1, a budget of `iterations` never sees it"""
    k = case.iterations

    def expect(budget, short):
        if budget < k or (budget == k and case.end in le.MAKING) or (budget == k and case.end == "budget"):
            assert ended(short) == (lc.MAX_ITERATIONS, budget, "budget"), (what, budget, ended(short))
            assert same(short["x"], model["iterates"][budget]) and same(short["history"], model["history"][:budget + 1]), (what, budget)
        elif case.end != "budget":
            assert ended(short) == ended(model), (what, budget)
    sh.budget_edges(k, lambda budget: model_of(h, b, x0, **le.keywords(case, max_iterations=budget)),
                    lambda budget, every: solve(h, b, x0, check_every=every, **le.keywords(case, max_iterations=budget)), expect, what, check, everys, budgets)


# ----------------------------------------------------------------------------- 1. every end, anywhere in a batch, at every budget edge
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_every_end_at_every_place_in_a_batch(run):
    case, dtype = run
    for shape in le.SHAPES:
        csr, b, x0 = le.system(case, shape, dtype)
        what = (case.name, shape)
        with handle(csr) as h:
            model = model_of(h, b, x0, **le.keywords(case))
            assert ended(model) == declared(case), (what, ended(model), "the case does not reach its end on these multiplies")
            for every in EVERY:
                x, res = solve(h, b, x0, check_every=every, **le.keywords(case))
                check(model, x, res, what + (every,))
            budget_edges(h, case, b, x0, model, what)


@pytest.mark.parametrize("run", le.BIG_CASES, ids=lambda run: f"{run[1]}-{NAMES[run[0]]}")
def test_a_case_at_two_steps_per_thread(run):
    """P(m) = 1024 and two steps per thread over m; P(n) = 2, so 1022 entries of <v,v>'s partial array are the +0.0 of the allocation"""
    dtype, name = run
    case = le.by_name(name)
    csr, b, x0 = le.system(case, le.BIG, dtype)
    assert case.iterations >= 2 and "middle" in le.batch_places(case)
    with handle(csr) as h:
        model = model_of(h, b, x0, **le.keywords(case))
        assert ended(model) == declared(case), ended(model)
        for every in (1, 0):
            x, res = solve(h, b, x0, check_every=every, **le.keywords(case))
            check(model, x, res, every)
        budget_edges(h, case, b, x0, model, (case.name,), everys=(0,), budgets=(case.iterations - 1,))


# ----------------------------------------------------------------------------- 2. atol
def atol_systems(dtype):
    """-> [(name, CSR, B, damp, budget)]: a tall and a wide sparse_rect without and with damp, and the catalogue's ladder with B = (3, 4, 0, ...)"""
    out = []
    for m, n in ((1025, 40), (40, 1025)):
        csr = lc.sparse_rect(m, n, dtype, per_row=4, seed=13)
        out += [((m, n, damp), csr, lc.rhs(m, dtype, 13), damp, 10) for damp in (0.0, 0.5)]
    case = le.by_name(le.ATOL_CASE)
    csr, b, _ = le.system(case, le.SHAPES[1], dtype)
    return out + [(case.name, csr, b, case.damp, case.budget)]


@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
def test_atol_decides_with_less_or_equal(dtype):
    """Some rr on the way is the square of a double a (with damp = 0 every one behind iteration 0: rr = phibar^2).  atol = a must end the run
    there (the test is <=) and the next double below must run one iteration further; with a small rtol beside it atol still decides, and with a
    small atol beside a large rtol, rtol does."""
    places = set()
    for name, csr, b, damp, budget in atol_systems(dtype):
        with handle(csr) as h:
            def model(atol, rtol=0.0):
                return model_of(h, b, damp=damp, rtol=rtol, atol=atol, max_iterations=budget)

            def run(**kw):
                return solve(h, b, damp=damp, max_iterations=budget, **kw)
            probes = sec.atol_probes(model)
            picks = le.probe_picks(probes, budget)
            print(f"{name} {NAMES[dtype]}: {len(probes)} places where rr is a square: {[k for _, k, _ in probes]}; taken {[k for _, k, _ in picks]}")
            assert len(picks) >= 3, (name, probes)
            for a, k, end in picks:
                what = (name, a, k, end)
                places.add((end, k))

                def before(at, under):
                    assert ended(at) == (lc.CONVERGED, k, end) and at["rr"] == a * a and under["iterations"] > k, (what, ended(at), ended(under))
                sh.atol_ladder(model, run, check, a, k, what, before)
    assert ("begin:converged", 0) in places and any(end == "step:converged" and k > 1 for end, k in places), places


# ----------------------------------------------------------------------------- 3. B = 0 and the ends of iteration 0 through device pointers
@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
def test_bb_zero_and_begin_ends_with_device_pointers(dtype):
    """x has n elements and B has m: on a tall and on a wide matrix, X a slice of a device tensor with a canary of one 16-byte unit on each side,
    aligned and shifted by one element.  B = 0 zeroes exactly X whatever the guess, a guess that solves the system stays bit for bit, a NaN in B
    without a guess leaves x = 0"""
    import torch
    pad = 16 // np.dtype(dtype).itemsize
    for m, n in ((1030, 40), (40, 1030)):
        csr = lc.sparse_rect(m, n, dtype, per_row=4, seed=14)
        guess = lc.rhs(n, dtype, 15)
        nan_b = lc.rhs(m, dtype, 16)
        nan_b[m // 2] = np.nan
        with handle(csr) as h:
            mul, _ = multiplies_with_transpose(h)
            solved = mul(guess)                                                  # B = A x0 in the handle's own bits: u = B - A x0 is exactly 0
            assert solved.any() and guess.all()
            runs = (("zero_b", np.zeros(m, dtype=dtype), None, "begin:bb_zero"), ("zero_b_guess", np.zeros(m, dtype=dtype), guess, "begin:bb_zero"),
                    ("good_guess", solved, guess, "begin:converged"), ("nan_in_b", nan_b, None, "begin:nonfinite"))
            for name, b, x0, end in runs:
                model = model_of(h, b, x0, max_iterations=5)
                assert ended(model) == (lc.NONFINITE if end == "begin:nonfinite" else lc.CONVERGED, 0, end), (name, ended(model))
                want = guess if name == "good_guess" else np.zeros(n, dtype=dtype)
                assert same(model["x"], want)
                for shift in (0, 1):
                    what = (name, (m, n), shift)
                    bd = torch.from_numpy(b).to(DEV)
                    buf = torch.full((n + 2 * pad + 1,), CANARY, dtype=bd.dtype, device=DEV)
                    xd = buf[pad + shift:pad + shift + n]
                    assert (xd.data_ptr() % 16 != 0) == bool(shift)
                    if x0 is not None:
                        xd.copy_(torch.from_numpy(x0))
                    for every in (0, 1):
                        got, res, hist = h.lsqr(bd, xd, x0=x0 is not None, rtol=0.0, ls_tol=0.0, max_iterations=5, check_every=every, history=True)
                        torch.cuda.synchronize()
                        res["history"] = hist
                        out = buf.cpu().numpy()
                        assert got is xd
                        check(model, out[pad + shift:pad + shift + n], res, what)
                        assert out[pad + shift:pad + shift + n].tobytes() == want.tobytes(), what     # +0.0 everywhere, or the guess bit for bit
                        assert (out[:pad + shift] == CANARY).all() and (out[pad + shift + n:] == CANARY).all(), (what, "written outside X")
                        if end == "begin:bb_zero":
                            assert (res["rr"], res["bb"], res["status_name"]) == (0.0, 0.0, "converged"), what


# ----------------------------------------------------------------------------- 4. state between solves
@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
def test_a_solve_is_unaffected_by_what_earlier_solves_left(dtype):
    """One handle, one matrix that holds a ladder beside a sparse_rect part (the right-hand side chooses whose recurrence runs).  The first
    solve starts from a guess of finfo.max: the workspace is born with infinity and NaN in q, u, v and the partial arrays.  Then an ordinary
    solve, one of each end, a NONFINITE inside the loop with iterations enqueued behind it, the ordinary solve again and B = 0 -- each against
    the model, twice over, in a workspace that never grows"""
    csr, runs = le.state_system(dtype)
    with handle(csr) as h:
        mul, mul_t = multiplies_with_transpose(h)
        assert runs[0][0] == "huge_guess" and (~np.isfinite(mul(runs[0][2]))).sum() > 100           # A x0 overflows
        mul_t(np.zeros(csr.m, dtype=dtype))                     # both of the model's multiplies now own their staging buffers (and the transpose is
                                                                # built): device_bytes moves no more on their account.  The solver has nothing yet
        held = None
        for trip in range(2):
            for name, b, x0, kw, want in runs:
                model = model_of(h, b, x0, **kw)
                assert ended(model) == want, (name, ended(model))
                x, res = solve(h, b, x0, **kw)
                check(model, x, res, (trip, name))
                if held is None:
                    held = h.info()["device_bytes"]                             # behind the first solve: the workspace and the history block
                assert h.info()["device_bytes"] == held, (trip, name)


# ----------------------------------------------------------------------------- 5. the timer runs the solve's arithmetic
@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
def test_the_timed_launches_do_the_arithmetic_of_the_solve(dtype):
    import torch
    csr = lc.sparse_rect(4099, 1030, dtype, per_row=4, seed=17)
    b, guess = lc.rhs(csr.m, dtype, 17), lc.rhs(csr.n, dtype, 18)
    with handle(csr) as h:
        bd = torch.from_numpy(b).to(DEV)
        for k in (5, 1):
            for damp in (0.0, 0.25):
                what = (k, damp)
                model = model_of(h, b, damp=damp, max_iterations=k + 1)
                assert ended(model) == (lc.MAX_ITERATIONS, k + 1, "budget"), what             # still going behind iteration k
                xd = torch.full((csr.n,), CANARY, dtype=bd.dtype, device=DEV)
                mean, runs = ROW.timer(h.h, bd, xd, k, damp=damp, warmup=1, iters=2)   # every run starts from x = 0
                torch.cuda.synchronize()
                assert mean > 0 and runs.shape == (2,) and same(xd.cpu().numpy(), model["iterates"][k]), ("timer",) + what
                from_guess, res = solve(h, b, guess, damp=damp, max_iterations=k)
                assert (res["status"], res["iterations"]) == (lc.MAX_ITERATIONS, k) and not same(from_guess, model["iterates"][k])
                check(model_of(h, b, guess, damp=damp, max_iterations=k), from_guess, res, ("guess",) + what)
                xd.copy_(torch.from_numpy(guess))
                ROW.timer(h.h, bd, xd, k, damp=damp, x0=True, warmup=0, iters=1)        # one run: from the guess in X
                torch.cuda.synchronize()
                assert same(xd.cpu().numpy(), from_guess), ("timer, x0",) + what
                # a second run with use_x0 starts from what the first left in X: two chained solves of k iterations, not one of 2 k
                again, res = solve(h, b, from_guess, damp=damp, max_iterations=k)
                assert res["iterations"] == k and not same(again, from_guess)
                xd.copy_(torch.from_numpy(guess))
                ROW.timer(h.h, bd, xd, k, damp=damp, x0=True, warmup=1, iters=1)
                torch.cuda.synchronize()
                assert same(xd.cpu().numpy(), again), ("timer, x0 twice",) + what


# ----------------------------------------------------------------------------- 6. lsqr on every executor
def nine_iterations(h, csr, dtype, seed):
    """9 iterations without and with (a guess and damp = 0.25), against the model on this handle's spmv() and spmv_transpose()"""
    b, guess = lc.rhs(csr.m, dtype, seed), lc.rhs(csr.n, dtype, seed + 50)
    for x0, damp in ((None, 0.0), (guess, 0.25)):
        model = model_of(h, b, x0, damp=damp, max_iterations=9)
        assert model["iterations"] == 9 and np.isfinite(model["x"]).all() and model["x"].any(), ended(model)
        x, res = solve(h, b, x0, damp=damp, max_iterations=9)
        check(model, x, res, (x0 is not None,))


def transpose_of(h, want_longest):
    """the schedule of A^T behind the first solve: printed; what it must be is its size and that something is launched"""
    info = api.get_transpose_info(h.h)
    print(f"A^T: {info['schedule_name']} {info['launch_kernels']}, max_row_len {info['max_row_len']}, lanes_per_row {info['lanes_per_row']}, packed_nnz {info['packed_nnz']}")
    assert info["max_row_len"] == want_longest and info["launch_kernels"] and info["nnz"] == h.info()["nnz"], info
    return info


@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("method", METHODS, ids=lambda mth: mth.name)
def test_every_executor_under_lsqr(method, dtype):
    """a rectangular arrow: the first row of A (1030 entries) is longer than any long-row threshold and so is the first row of A^T (2049), a
    carry crosses every CSR5 / nnz-split tile boundary.  As built, and on the row-block x column-slab executor (cache_block = 2; CSR-scalar
    schedules never take it)"""
    csr = le.arrow_rect(2049, 1030, dtype)

    def iterate(h, seed):
        nine_iterations(h, csr, dtype, seed)
        transpose_of(h, 2049)
    sh.every_executor(csr, method, iterate, longest=1030)


@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
def test_the_long_row_launch_beside_the_tile_kernel_and_packed_tiles(dtype):
    """rows of 32 aligned entries at 8 lanes per row run on the CSR-vector TILE kernel; row 300 (544 entries > long_thr = 512) goes to the
    long-row launch behind it.  fp64 also with pack_values = 1: every tile but row 300's streams 7-byte values"""
    def iterate(h, csr, seed):
        nine_iterations(h, csr, dtype, seed)
        transpose_of(h, int(np.bincount(csr.colidx, minlength=csr.n).max()))
    sh.the_long_row_launch_beside_the_tile_kernel(dtype, iterate)
