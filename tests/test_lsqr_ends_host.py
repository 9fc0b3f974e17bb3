"""CPU: the catalogue of tests/lsqr_end_cases.py, proven with the host model alone (lsqr_cases.lsqr over lsqr_cases.products) before
tests/test_gpu_lsqr_ends.py asks the device for the same ends.  No tolerance appears: every comparison is of statuses, counts or bits."""
import inspect
import re

import numpy as np
import pytest

import cg_cases as cgc
import lsqr_cases as lc
import lsqr_end_cases as le
import solve_end_cases as sec
from test_lsqr_host import STATUS_OF_END

NAMES, RUNS, run_id, ended, declared = le.NAMES, le.RUNS, le.run_id, le.ended, le.declared
STEP_ENDS = sorted(e for e in STATUS_OF_END if e.startswith("step:"))


def mine(dtype):
    return [c for c in le.CASES if dtype in c.dtypes]


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_each_case_ends_as_declared_at_every_shape(run):
    case, dtype = run
    assert case.status == STATUS_OF_END[case.end] and case.budget <= le.BUDGET
    own = le.run(case, "own", dtype)
    for shape in le.SHAPES:
        csr, b, x0 = le.system(case, shape, dtype)
        m, n = le.shape_of(case, shape)
        assert (csr.m, csr.n, b.size) == (m, n, m) and csr.val.size == np.count_nonzero(le.ladder(case.a, case.b)) and (x0 is None) == (case.x0 is None)
        r = le.run(case, shape, dtype)
        assert ended(r) == declared(case), (shape, ended(r))
        assert len(r["history"]) == len(r["iterates"]) == case.iterations + 1
        cols = le.spread(len(case.a), n)
        assert not np.delete(r["x"], cols).any(), shape
        if len(case.rhs) == 1 and case.x0 is None:
            # unit vectors: a dot has one non-zero product, so the scalars of the run are the ladder's own, bit for bit, and so is x
            assert np.array_equal(r["history"], own["history"], equal_nan=True) and np.array_equal(r["estimates"], own["estimates"], equal_nan=True), shape
            assert np.array_equal(r["x"][cols], own["x"], equal_nan=True), shape


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_budget_edges(run):
    """budgets of iterations - 1, iterations and iterations + 1: a non-finite <u,u>, <v,v> or factor is found while MAKING iteration
    iterations + 1, so a budget of `iterations` never sees it; every other end is found behind the iteration that spent the budget"""
    case, dtype = run
    k = case.iterations
    free = le.run(case, le.SHAPES[1], dtype)
    for budget in (k - 1, k, k + 1):
        if budget < 0 or (budget > k and case.end == "budget"):                    # where a run goes behind its line's budget is not declared
            continue
        r = le.run(case, le.SHAPES[1], dtype, max_iterations=budget)
        if budget < k or (budget == k and case.end in le.MAKING) or case.end == "budget":
            assert ended(r) == (lc.MAX_ITERATIONS, budget, "budget"), (budget, ended(r))
        else:
            assert ended(r) == declared(case), (budget, ended(r))
        assert np.array_equal(r["x"], free["iterates"][min(budget, k)], equal_nan=True)


@pytest.mark.parametrize("run", [r for r in RUNS if r[1] == np.float32], ids=run_id)
def test_an_fp32_case_ends_alike_where_a_row_is_rounded_once(run):
    """the lines whose vectors are no unit vectors -- the sums of two products that pass 2^128 among them -- must not hinge on a rounding error
    that a fused multiply-add does not make"""
    case, dtype = run
    for shape in le.SHAPES[::3]:
        csr, b, x0 = le.system(case, shape, dtype)
        r = lc.lsqr(*le.products_wide(csr), b, csr.n, x0=x0, **le.keywords(case))
        assert ended(r) == declared(case), (shape, ended(r))


def test_the_shapes_have_two_different_geometries():
    P = lambda shape: (cgc.geometry(shape[0])[0], cgc.geometry(shape[1])[0])
    assert [P(s) for s in le.SHAPES[1:]] == [(2, 2), (5, 2), (2, 5)] and all(v % 4 for s in le.SHAPES[1:] for v in s)
    assert cgc.geometry(le.BIG[0]) == (1024, 2048) and cgc.geometry(le.BIG[1]) == (2, 1024)
    for size in (1025, 1030, 4099, le.BIG[0]):
        for count in (8, 9):
            at = le.spread(count, size)
            assert at.size == count == np.unique(at).size and {0, 1023, 1024, size - 1} <= set(at.tolist()), (count, size)


def test_the_list_of_ends_is_the_models():
    named = set(re.findall(r'"((?:begin|first|step):\w+|budget)"', inspect.getsource(lc.lsqr))) - {"begin:empty"}
    assert named == set(STATUS_OF_END)
    assert set(le.MAKING) <= named and all(set(gaps) <= named for gaps in le.ALLOWED_GAPS.values())
    assert len({c.name for c in le.CASES}) == len(le.CASES)


@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
def test_every_end_and_every_place_in_a_batch_is_reached(dtype):
    cases = mine(dtype)
    reached = {c.end for c in cases}
    print(f"lsqr {NAMES[dtype]}: not reached {sorted(set(STATUS_OF_END) - reached)}")
    assert reached == set(STATUS_OF_END) - set(le.ALLOWED_GAPS[dtype])
    for end in STEP_ENDS:
        if end in le.ALLOWED_GAPS[dtype]:
            continue
        counts = sorted({c.iterations for c in cases if c.end == end})
        places = set().union(*(le.batch_places(c) for c in cases if c.end == end))
        print(f"lsqr {NAMES[dtype]}: {end} at iterations {counts}")
        assert len(counts) >= 3, (end, counts)
        assert places == {"first", "middle", "last"}, (end, places)
        # ... and by a line WITHOUT a guess at each of the three places of one batch length
        exact = [c for c in cases if c.end == end and c.x0 is None]
        assert any({(le.found_at(c) - 1) % every + 1 for c in exact} >= {1, 2, every} for every in (3, 8)), end
    # the ends before the loop run with and without a guess
    for end in ("begin:bb_zero", "begin:converged", "begin:nonfinite"):
        assert {c.x0 is None for c in cases if c.end == end} == {True, False}, end
    assert any(c.end == "step:converged" and c.rtol > 0 for c in cases) and any(c.end == "step:least_squares" and c.ls_tol > 0 for c in cases)
    assert any(c.end == "budget" and c.x0 is None for c in cases) and any(c.x0 is not None and c.iterations >= 1 for c in cases)


def test_every_ladder_runs_once_more_from_a_guess():
    """... with B moved by A x0, which is exact, so that u = B - A x0 is the ladder's own B bit for bit: the same end at the same iteration,
    the same scalars, through lsqr_init's form with a guess"""
    for name, (_, _, _, _, dtypes, _, _, _) in le.LADDERS.items():
        plain = le.by_name(name)
        for dtype in dtypes:
            guessed = le.by_name(le.guessed_name(name, dtype))
            assert guessed.x0 == tuple(float(v) for v in le.LADDER_GUESS) and any(guessed.x0) and not any(guessed.x0[1::2]) and guessed.dtypes == (dtype,)
            assert (guessed.a, guessed.b, guessed.damp, declared(guessed)) == (plain.a, plain.b, plain.damp, declared(plain))
            for shape in le.SHAPES[:2]:
                csr, b, x0 = le.system(guessed, shape, dtype)
                _, b_plain, _ = le.system(plain, shape, dtype)
                with np.errstate(over="ignore"):
                    u = b - lc.products(csr)[0](x0)
                assert u.tobytes() == b_plain.tobytes() and np.isfinite(b).all() and b.tobytes() != b_plain.tobytes(), (name, shape)
                with_guess, without = le.run(guessed, shape, dtype), le.run(plain, shape, dtype)
                assert ended(with_guess) == ended(without) and np.array_equal(with_guess["history"], without["history"], equal_nan=True), (name, shape)
                assert with_guess["estimates"] == without["estimates"] or not np.isfinite(without["estimates"]).all(), (name, shape)


@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
def test_the_atol_probes_exist(dtype):
    """rr is the square of a double at iteration 0 (B = (3, 4, 0, ...): 25) and, with damp = 0, at every later one: atol = sqrt(rr) ends the run
    there and the next double below does not"""
    case = le.by_name(le.ATOL_CASE)
    for shape in le.SHAPES:
        free = le.run(case, shape, dtype)
        assert free["history"][0] == 25.0 and all(np.sqrt(h) ** 2 == h for h in free["history"][1:])
        probes = sec.atol_probes(lambda atol, rtol=0.0: le.run(case, shape, dtype, atol=atol, rtol=rtol))
        picks = le.probe_picks(probes, case.budget)
        ends = [(k, end) for _, k, end in picks]
        assert (0, "begin:converged") in ends and sum(end == "step:converged" for _, end in ends) >= 2 and any(k > 1 for k, _ in ends), ends
        for a, k, end in picks:
            at, below = le.run(case, shape, dtype, atol=a), le.run(case, shape, dtype, atol=float(np.nextafter(a, 0.0)))
            assert ended(at) == (lc.CONVERGED, k, end) and at["rr"] == a * a and below["iterations"] > k


@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
def test_one_matrix_reaches_each_end_by_its_right_hand_side(dtype):
    """the matrix of the GPU test of state between solves: a ladder beside a sparse_rect part"""
    csr, runs = le.state_system(dtype)
    assert (csr.m, csr.n) == (1030, 1025)
    mul, mul_t = lc.products(csr)
    seen = set()
    for name, b, x0, kw, want in runs:
        r = lc.lsqr(mul, mul_t, b, csr.n, x0=x0, **{key: v for key, v in kw.items() if key != "check_every"})
        assert ended(r) == want, (name, ended(r))
        seen.add(r["end"])
    assert seen == {"begin:nonfinite", "budget", "step:converged", "step:least_squares", "begin:converged", "first:alpha_zero", "begin:bb_zero",
                    "step:uu_nonfinite"}
    first, last = runs[0], runs[-1]
    assert first[4] == (lc.NONFINITE, 0, "begin:nonfinite") and (~np.isfinite(mul(first[2]))).sum() > 100              # A x0 overflows
    assert last[4][2] == "begin:bb_zero" and not last[1].any() and last[2].any()
    in_loop = runs[6]
    assert in_loop[4][0] == lc.NONFINITE and in_loop[4][1] == 3 and in_loop[3]["check_every"] == 3     # found in iteration 4: first of the second batch of 3


@pytest.mark.parametrize("dtype", le.BOTH, ids=NAMES.get)
def test_the_rectangular_arrow(dtype):
    csr = le.arrow_rect(2049, 1030, dtype)
    lens = np.diff(csr.rowptr)
    assert lens[0] == lens.max() == 1030 and np.bincount(csr.colidx, minlength=csr.n)[0] == 2049 and 4 <= csr.val.size / csr.m <= 6
    assert all((np.diff(csr.colidx[csr.rowptr[i]:csr.rowptr[i + 1]]) > 0).all() for i in range(0, csr.m, 97))
    assert np.array_equal(csr.val.astype(np.float64) * 8, np.round(csr.val.astype(np.float64) * 8)) and (csr.val != 0).all()
