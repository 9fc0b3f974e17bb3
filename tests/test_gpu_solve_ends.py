"""GPU: every way spmv_hip_cg and spmv_hip_bicgstab can end, anywhere in an enqueued batch and on every executor (include/spmv_hip.h, "the
arithmetic contract").

The yardstick is the host model of tests/cg_cases.py / tests/bicgstab_cases.py driven by the SAME handle's spmv(); x, rr, bb, history, status
and iterations are compared bit for bit and no tolerance appears anywhere.  The one freedom: a NaN equals a NaN whatever its sign and payload
(the contract gives a NaN neither; numpy's and the device's differ in the sign).  The cases come from tests/solve_end_cases.py, whose every line
tests/test_solve_ends_host.py proves on the CPU first; here each case must also reach the (status, iterations, end) it declares under the
handle's own multiply -- bits that match a model which ends elsewhere would mean the INPUT is wrong, not the kernel."""
import functools

import numpy as np
import pytest

import bicgstab_cases as bc
import cg_cases as cgc
import packed_cases as pc
import solve_end_cases as sec
from spmv_amd import api, build

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
DEV = "cuda:0"
CANARY = -7.25
NAMES = {np.float32: "f32", np.float64: "f64"}
SOLVERS = ("cg", "bicgstab")
EVERY = (1, 2, 3, 0, 64)           # check_every: the end falls first, in the middle and last in an enqueued batch
BIG_CASES = {"bicgstab": "b_half_2", "cg": "c_rr_2"}
MODEL = {"cg": cgc.cg, "bicgstab": bc.bicgstab}
TIMER = {"cg": api.time_cg_iterations, "bicgstab": api.time_bicgstab_iterations}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def handle(csr, method=M.Method_Parallel, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method)
    finally:
        api.clear_thread_options()


def multiply_of(h):
    """the model's multiply: this handle's spmv() on host vectors"""
    def multiply(x):
        return h.spmv(np.ascontiguousarray(x), np.empty_like(x))
    return multiply


def solve(h, solver, b, x0=None, **kw):
    """through host pointers, with a canary in X when there is no guess -> (x, result dict with history)"""
    x = np.full(b.size, CANARY, dtype=b.dtype) if x0 is None else x0.copy()
    kw.setdefault("rtol", 0.0)
    x, res, hist = getattr(h, solver)(b, x, x0=x0 is not None, history=True, **kw)
    res["history"] = hist
    return x, res


def same(a, b):
    """the same type, shape and bits; a NaN equals a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    both = np.isnan(a) & np.isnan(b)
    return np.where(both, 0, a).tobytes() == np.where(both, 0, b).tobytes()


def check(model, x, res, what=None):
    """a run against a model run with the same arguments, however either ended"""
    assert (res["status"], res["iterations"]) == (model["status"], model["iterations"]), (what, res, model["end"])
    assert same(x, model["x"]), (what, "x")
    assert same(np.float64(res["rr"]), np.float64(model["rr"])) and same(np.float64(res["bb"]), np.float64(model["bb"])), (what, res, model["rr"], model["bb"])
    assert same(res["history"], model["history"]), (what, res["history"], model["history"])


def ended(r):
    return r["status"], r["iterations"], r["end"]


def runs_of(solver):
    return [(c, d) for c in sec.CASES if c.solver == solver for d in c.dtypes]


def run_id(run):
    return f"{run[0].name}-{NAMES[run[1]]}"


# ----------------------------------------------------------------------------- 1. every end, anywhere in a batch, at every budget edge
@pytest.mark.parametrize("run", runs_of("bicgstab") + runs_of("cg"), ids=run_id)
def test_every_end_at_every_place_in_a_batch(run):
    case, dtype = run
    k = case.iterations
    for m in sec.SIZES:
        for pre in (False, True) if case.solver == "bicgstab" and case.dinv is None else (False,):
            csr, b, dinv, x0 = sec.system(case, m // 2, dtype, pre)
            what = (case.name, m, pre)
            with handle(csr) as h:
                mul = multiply_of(h)
                model = MODEL[case.solver](mul, b, x0=x0, dinv=dinv, max_iterations=sec.BUDGET)
                assert ended(model) == (case.status, k, case.end), (what, ended(model), "the case does not reach its end on this multiply")
                for every in EVERY:
                    x, res = solve(h, case.solver, b, x0, dinv=dinv, max_iterations=sec.BUDGET, check_every=every)
                    check(model, x, res, what + (every,))
                for budget in (k - 1, k, k + 1):
                    if budget < 0:
                        continue
                    short = MODEL[case.solver](mul, b, x0=x0, dinv=dinv, max_iterations=budget)
                    if budget < k or (budget == k and sec.first_kernel(case)):      # found while starting iteration k + 1: not with a budget of k
                        assert ended(short) == (cgc.MAX_ITERATIONS, budget, "budget"), (what, budget)
                    else:
                        assert ended(short) == ended(model), (what, budget)
                    for every in (0, 1):
                        x, res = solve(h, case.solver, b, x0, dinv=dinv, max_iterations=budget, check_every=every)
                        check(short, x, res, what + (budget, every))


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", SOLVERS)
def test_an_exact_case_at_two_steps_per_workgroup(solver, dtype):
    case = sec.by_name(BIG_CASES[solver])
    assert case.exact
    csr, b, dinv, x0 = sec.system(case, sec.BIG // 2, dtype)
    with handle(csr) as h:
        mul = multiply_of(h)
        model = MODEL[solver](mul, b, x0=x0, dinv=dinv, max_iterations=sec.BUDGET)
        assert ended(model) == (case.status, case.iterations, case.end)
        for every in (1, 0):
            x, res = solve(h, solver, b, x0, dinv=dinv, max_iterations=sec.BUDGET, check_every=every)
            check(model, x, res, every)
        x, res = solve(h, solver, b, x0, dinv=dinv, max_iterations=case.iterations - 1)
        assert (res["status"], res["iterations"]) == (cgc.MAX_ITERATIONS, case.iterations - 1) and same(x, model["iterates"][case.iterations - 1])


# ----------------------------------------------------------------------------- 2. atol
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", SOLVERS)
def test_atol_decides_with_less_or_equal(solver, dtype):
    """On exact cases some rr on the way is the square of a double a.  atol = a must end the run there (the test is <=) and the next double
    below must not; with a small rtol beside it atol still decides, and with a small atol beside a large rtol, rtol does."""
    places = set()
    for case in (c for c in sec.CASES if c.solver == solver and c.exact and c.status != cgc.NONFINITE):
        for m in sec.ATOL_SIZES:
            csr, b, dinv, x0 = sec.system(case, m // 2, dtype)
            with handle(csr) as h:
                mul = multiply_of(h)

                def model(atol, rtol=0.0):
                    return MODEL[solver](mul, b, x0=x0, dinv=dinv, rtol=rtol, atol=atol, max_iterations=sec.BUDGET)
                for a, k, end in sec.atol_probes(model):
                    what = (case.name, m, a, k, end)
                    places.add(end)
                    below = float(np.nextafter(a, 0.0))
                    at, under = model(a), model(below)
                    assert (at["iterations"], at["end"], at["status"]) == (k, end, cgc.CONVERGED) and (under["iterations"], under["end"]) != (k, end), what
                    for every in (1, 0):
                        x, res = solve(h, solver, b, x0, dinv=dinv, atol=a, max_iterations=sec.BUDGET, check_every=every)
                        check(at, x, res, what)
                        x, res = solve(h, solver, b, x0, dinv=dinv, atol=below, max_iterations=sec.BUDGET, check_every=every)
                        check(under, x, res, what + ("below",))
                    # rtol^2 bb is the smaller: atol still decides, at the same place
                    small = 2.0 ** -30
                    assert small * small * at["bb"] < a * a
                    both = model(a, small)
                    assert ended(both) == ended(at)
                    x, res = solve(h, solver, b, x0, dinv=dinv, rtol=small, atol=a, max_iterations=sec.BUDGET)
                    check(both, x, res, what + ("rtol below",))
                    # ... and the reverse: atol^2 is the smaller, rtol decides: the run ends where atol alone does not end it
                    rtol = 2.0 ** 20
                    while rtol * rtol * at["bb"] / 4 >= at["rr"]:
                        rtol /= 2                                                      # the smallest power of two with rtol^2 bb >= rr
                    low = a * 2.0 ** -10
                    by_rtol, alone = model(low, rtol), model(low)
                    assert rtol * rtol * at["bb"] >= at["rr"] > low * low and by_rtol["status"] == cgc.CONVERGED and by_rtol["iterations"] <= k
                    assert ended(alone) != ended(by_rtol), what
                    x, res = solve(h, solver, b, x0, dinv=dinv, rtol=rtol, atol=low, max_iterations=sec.BUDGET)
                    check(by_rtol, x, res, what + ("rtol above",))
    assert places == ({"begin:converged", "direction:converged"} | ({"update:ss_converged"} if solver == "bicgstab" else set())), places


# ----------------------------------------------------------------------------- 3. state between solves
@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", SOLVERS)
def test_a_solve_is_unaffected_by_what_earlier_solves_left(solver, dtype):
    """One handle, one matrix that holds the blocks of several cases side by side and a tridiagonal tail (the right-hand side chooses whose
    recurrence runs): solves that leave NaN and infinity in r, p, the scratch vectors, y and the partial arrays; an ordinary solve without and
    with Dinv; one of each breakdown; the ordinary solve again."""
    cases, csr, select = sec.state_system(solver, dtype)
    jac = (2.0 ** np.random.default_rng(11).integers(-1, 2, csr.m)).astype(dtype)
    huge = np.full(csr.m, np.finfo(dtype).max, dtype=dtype)
    ordinary, _, _ = select(None, 1)
    with handle(csr) as h:
        mul = multiply_of(h)

        def both(b, x0=None, dinv=None, budget=sec.BUDGET, every=0):
            model = MODEL[solver](mul, b, x0=x0, dinv=dinv, max_iterations=budget)
            x, res = solve(h, solver, b, x0, dinv=dinv, max_iterations=budget, check_every=every)
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
    csr = cgc.tri(1026, dtype) if solver == "cg" else bc.tri_ns(1026, dtype)
    rng = np.random.default_rng(5)
    b, guess, jac = cgc.rhs(csr.m, dtype, 7), rng.uniform(-1, 1, csr.m).astype(dtype), rng.uniform(0.5, 1.5, csr.m).astype(dtype)
    with handle(csr) as h:
        for dinv in (None, jac):
            model = MODEL[solver](multiply_of(h), b, dinv=dinv, max_iterations=8)
            assert ended(model) == (cgc.MAX_ITERATIONS, 8, "budget")              # still running at k = 6
            want, res = solve(h, solver, b, dinv=dinv, max_iterations=6)
            assert (res["status"], res["iterations"]) == (cgc.MAX_ITERATIONS, 6) and same(want, model["iterates"][6])
            bd, jd = torch.from_numpy(b).to(DEV), None if dinv is None else torch.from_numpy(dinv).to(DEV)
            xd = torch.full((csr.m,), CANARY, dtype=bd.dtype, device=DEV)
            mean, runs = TIMER[solver](h.h, bd, xd, 6, dinv=jd, warmup=1, iters=2)  # every run starts from x = 0
            torch.cuda.synchronize()
            assert mean > 0 and runs.shape == (2,) and same(xd.cpu().numpy(), want), ("timer", dinv is not None)
            from_guess, res = solve(h, solver, b, guess, dinv=dinv, max_iterations=6)
            assert res["iterations"] == 6 and not same(from_guess, want)
            xd.copy_(torch.from_numpy(guess))
            TIMER[solver](h.h, bd, xd, 6, x0=True, dinv=jd, warmup=0, iters=1)      # one run: from the guess in X
            torch.cuda.synchronize()
            assert same(xd.cpu().numpy(), from_guess), ("timer, x0", dinv is not None)
            # a second run with use_x0 starts from what the first left in X (include/spmv_hip_tools.h): two runs of 3 are not one run of 6 ...
            again, _ = solve(h, solver, b, solve(h, solver, b, guess, dinv=dinv, max_iterations=3)[0], dinv=dinv, max_iterations=3)
            xd.copy_(torch.from_numpy(guess))
            TIMER[solver](h.h, bd, xd, 3, x0=True, dinv=jd, warmup=1, iters=1)
            torch.cuda.synchronize()
            assert same(xd.cpu().numpy(), again) and not same(again, from_guess), ("timer, x0 twice", dinv is not None)


# ----------------------------------------------------------------------------- 5. the solvers on every executor
METHODS = [mth for mth in M if mth != M.Method_Total_Size]
LONG_ROW_KERNELS = ("csr5_group_kernel", "csr5_group_pipe_kernel", "csr5_kernel")   # the long rows' CSR5 sub-matrix, behind the row-granular kernel
# launch_kernels of a multiply on the 2049-row arrow matrices, as spmv_hip_info reports them: the first kernel; is a long-row launch beside it
EXECUTORS = {
    M.Method_Serial: ("csr_scalar_kernel", False), M.Method_Numa: ("csr_scalar_kernel", False),
    M.Method_Parallel: ("csr_vector_rows_kernel", True), M.Method_SellCSigma: ("sell_window_kernel", True),
    M.Method_Balanced: ("nat_group_kernel", False), M.Method_Balanced2: ("nat_group_kernel", False), M.Method_Balanced_Yid: ("nat_group_kernel", False),
    M.Method_CSR5SPMV: (None, False),                                                  # csr5_group_kernel or, in fp32, its two-deep form
}


def twelve_iterations(h, solver, csr, dtype, seed, jac=None):
    """12 iterations without and with a guess and Dinv (1 / diagonal unless one is given), against the model on this handle's spmv()"""
    rng = np.random.default_rng(seed)
    b, guess = cgc.rhs(csr.m, dtype, seed), rng.uniform(-1, 1, csr.m).astype(dtype)
    if jac is None:
        jac = (1.0 / cgc.diagonal(csr).astype(np.float64)).astype(dtype)
    mul = multiply_of(h)
    for x0, dinv in ((None, None), (guess, jac)):
        model = MODEL[solver](mul, b, x0=x0, dinv=dinv, max_iterations=12)
        assert model["iterations"] == 12 and np.isfinite(model["x"]).all(), ended(model)
        x, res = solve(h, solver, b, x0, dinv=dinv, max_iterations=12)
        check(model, x, res, (x0 is not None,))


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("method", METHODS, ids=lambda mth: mth.name)
@pytest.mark.parametrize("solver", SOLVERS)
def test_every_executor_under_the_solvers(solver, method, dtype):
    """a dense first row and column: a row longer than any long-row threshold, a carry across every CSR5 / nnz-split tile boundary.  As built,
    and on the row-block x column-slab executor (cache_block = 2; CSR-scalar schedules never take it)"""
    csr = sec.arrow(2049, dtype, symmetric=solver == "cg")
    first, long_rows = EXECUTORS[method]
    with handle(csr, method) as h:
        info = h.info()
        names = info["launch_kernels"]
        assert info["max_row_len"] == 2049 and info["cache_blocked"] == 0 and info["far_nnz"] == 0, info
        assert first is None or names[0] == first, names
        if long_rows:
            assert len(names) == 3 and names[1] in LONG_ROW_KERNELS and names[2] == "csr5_fixup_kernel", names
        elif first != "csr_scalar_kernel":
            assert names[-1] == "csr5_fixup_kernel" and names[0] in ("nat_group_kernel",) + LONG_ROW_KERNELS, names   # carries and their fix-up
        twelve_iterations(h, solver, csr, dtype, 1)
    if first == "csr_scalar_kernel":
        return
    with handle(csr, method, cache_block=2) as h:
        info = h.info()
        assert info["cache_blocked"] == 1 and info["launch_kernels"] in (["blk_kernel"], ["blk_wide_kernel"]), info
        twelve_iterations(h, solver, csr, dtype, 2)


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", SOLVERS)
def test_the_long_row_launch_beside_the_tile_kernel_and_packed_tiles(solver, dtype):
    """rows of 32 aligned entries at 8 lanes per row run on the CSR-vector TILE kernel; row 300 (544 entries > long_thr = 512) goes to the
    long-row launch behind it.  fp64 also with pack_values = 1: every tile but row 300's streams 7-byte values"""
    csr = sec.band32(1280, dtype, long_row=300)
    for pack in (0, 1) if dtype == np.float64 else (0,):
        with handle(csr, M.Method_Parallel, lanes_per_row=8, pack_values=pack) as h:
            info = h.info()
            names = info["launch_kernels"]
            assert info["lanes_per_row"] == 8 and info["max_row_len"] == 544, info
            assert len(names) == 3 and names[0] == pc.TILE_KERNEL and names[1] in LONG_ROW_KERNELS and names[2] == "csr5_fixup_kernel", names
            if pack:
                want, flags = pc.model_packed(csr.rowptr, csr.val, 8)
                assert flags == [True, False, True, True, True] and info["packed_nnz"] == want == info["nnz"] - (255 * 32 + 544) > 0, info
            else:
                assert info["packed_nnz"] == 0
            twelve_iterations(h, solver, csr, dtype, 3 + pack)


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
