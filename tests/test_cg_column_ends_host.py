"""CPU: the CG catalogue of tests/solve_end_cases.py as the columns of ONE call of spmv_hip_cg_columns, proven with the host models alone
(cg_columns_cases.solve, which is cg_cases.cg per column) before tests/test_gpu_cg_column_ends.py asks the device for the same ends.

sec.columns_system puts every CG case of a type into one matrix -- block j of every group of blocks is case j's -- with a tridiagonal tail, and
makes case j's right-hand side column j of B: column j then runs case j's recurrence, ends where the catalogue says, and the last column, an
ordinary right-hand side on the tail, is still running at the budget.  Under both multiplies (cg_cases.matvec, and sec.matvec_wide, which
rounds a row once).  No tolerance appears: every comparison is of statuses, counts or bits."""
import functools

import numpy as np
import pytest

import cg_cases as cgc
import cg_columns_cases as ccc
import solve_end_cases as sec

NAMES = {np.float32: "f32", np.float64: "f64"}
MULTIPLIES = {"plain": cgc.matvec, "wide": sec.matvec_wide}
EXPECTED = {np.float64: {"plain": 13, "plain_nox0": 10, "pre": 10}, np.float32: {"plain": 14, "plain_nox0": 11, "pre": 10}}


def ended(r):
    return r["status"], r["iterations"], r["end"]


def same(a, b):
    """the same type, shape and bits; a NaN equals a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    both = np.isnan(a) & np.isnan(b)
    return np.where(both, 0, a).tobytes() == np.where(both, 0, b).tobytes()


@functools.lru_cache(maxsize=None)
def system(group, m, dtype):
    return sec.columns_system(group, m, dtype)


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_the_groups_hold_every_cg_case_once_and_every_end(dtype):
    groups = sec.column_groups(dtype)
    assert {g: len(cases) for g, cases in groups.items()} == EXPECTED[dtype] and tuple(groups) == sec.GROUPS
    mine = [c for c in sec.CASES if c.solver == "cg" and dtype in c.dtypes]
    assert sorted(c.name for c in groups["plain"] + groups["pre"]) == sorted(c.name for c in mine)
    assert all(c.x0 is None for c in groups["plain_nox0"] + groups["pre"]) and all(c.dinv is not None for c in groups["pre"])
    assert max(len(cases) for cases in groups.values()) + 1 <= 15
    reached = {c.end for cases in groups.values() for c in cases}
    assert reached == set(sec.ENDS["cg"]) and len(sec.ENDS["cg"]) == 11, set(sec.ENDS["cg"]) - reached
    # in every group one column ends in ccg_alpha and another in ccg_beta of the SAME iteration: ccg_alpha of iteration it ends a column
    # that reports it - 1 iterations, ccg_beta one that reports it
    for cases in groups.values():
        assert any(sec.first_kernel(a) and not sec.first_kernel(b) and a.iterations + 1 == b.iterations for a in cases for b in cases)
    assert [c.name for c in (sec.by_name(n) for n in sec.BIG_GROUP)] == list(sec.BIG_GROUP) and all(sec.by_name(n).exact for n in sec.BIG_GROUP)


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("m", sec.SIZES)
@pytest.mark.parametrize("group", sec.GROUPS)
def test_the_system_is_what_the_issue_says(group, m, dtype):
    csr, B, X0, Dinv, cases = system(group, m, dtype)
    n = len(cases)
    reps, tail = sec.columns_shape(n, m)
    assert (reps, tail) == ((1, 4) if m == 2 else ((m - 4) // (2 * n), m - 2 * n * ((m - 4) // (2 * n)))) and tail >= 4
    assert csr.m == 2 * n * reps + tail == B.shape[0] and (csr.m == m or m == 2) and B.shape[1] == n + 1 <= 15
    assert (X0 is None) == (group != "plain") and (Dinv is None) == (group != "pre")
    head = 2 * n * reps
    for j, case in enumerate(cases):
        own = (2 * (j + n * np.arange(reps))[:, None] + np.arange(2)).ravel()
        rest = np.setdiff1d(np.arange(csr.m), own)
        assert not B[rest, j].any() and np.array_equal(B[own, j], np.tile(np.array(case.b, dtype=dtype), reps))
        if X0 is not None:
            assert not X0[rest, j].any() and np.array_equal(X0[own, j], np.tile(np.array(case.x0 or (0, 0), dtype=dtype), reps))
        if Dinv is not None:
            assert np.array_equal(Dinv[own], np.tile(np.array(case.dinv, dtype=dtype), reps))
    assert not B[:head, n].any() and B[head:, n].all() and (X0 is None or not X0[:, n].any()) and (Dinv is None or (Dinv[head:] == 1).all())
    assert not sec.subnormal(csr.val, B, *(v for v in (X0, Dinv) if v is not None))


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("m", sec.SIZES)
@pytest.mark.parametrize("group", sec.GROUPS)
def test_every_column_ends_as_declared_and_the_tail_runs_on(group, m, dtype):
    csr, B, X0, Dinv, cases = system(group, m, dtype)
    want = sec.declared_columns(cases)
    assert want[-1] == (cgc.MAX_ITERATIONS, sec.BUDGET, "budget")
    for name, multiply in MULTIPLIES.items():
        mul = multiply(csr)
        for run, G, ones in sec.column_runs(group, B, X0):
            dinv = np.ones(csr.m, dtype=dtype) if ones else Dinv
            models = ccc.solve(mul, B, G, dinv=dinv, max_iterations=sec.BUDGET)
            assert [ended(r) for r in models] == want, (name, run, [(c.name, ended(r)) for c, r in zip(cases, models) if ended(r) != (c.status, c.iterations, c.end)])
            assert np.isfinite(models[-1]["x"]).all() and models[-1]["rr"] > 0
            # a column of the mixed system is its own solve
            for j, r in enumerate(models):
                own = cgc.cg(mul, np.ascontiguousarray(B[:, j]), x0=None if G is None else np.ascontiguousarray(G[:, j]), dinv=dinv, max_iterations=sec.BUDGET)
                assert ended(own) == ended(r) and same(own["x"], r["x"]) and same(own["history"], r["history"]) and same(np.float64(own["rr"]), np.float64(r["rr"]))
                assert same(np.float64(own["bb"]), np.float64(r["bb"]))
            # an exact case among other blocks is the case alone: the same values, iteration for iteration
            for case, r in zip(cases, models):
                if case.exact and name == "plain" and not ones and (G is not None or case.x0 is None):
                    alone = sec.run(case, sec.columns_shape(len(cases), m)[0], dtype)
                    assert np.array_equal(alone["history"], r["history"]) and alone["bb"] == r["bb"], case.name


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("m", sec.SIZES)
@pytest.mark.parametrize("group", sec.GROUPS)
def test_the_budget_edges_of_every_column(group, m, dtype):
    """budgets 0 .. 3 around iteration counts of 0 .. 2: every column at iterations - 1, iterations and iterations + 1, each model run WITH that
    budget.  An end that ccg_alpha finds reports MAX_ITERATIONS at budget == iterations while its neighbours report their own ends"""
    csr, B, X0, Dinv, cases = system(group, m, dtype)
    assert {c.iterations for c in cases} == {0, 1, 2}
    for name, multiply in MULTIPLIES.items():
        mul = multiply(csr)
        for run, G, ones in sec.column_runs(group, B, X0):
            dinv = np.ones(csr.m, dtype=dtype) if ones else Dinv
            free = ccc.solve(mul, B, G, dinv=dinv, max_iterations=sec.BUDGET)
            for budget in range(4):
                models = ccc.solve(mul, B, G, dinv=dinv, max_iterations=budget)
                assert [ended(r) for r in models] == sec.declared_columns(cases, budget), (name, run, budget)
                for r, f in zip(models, free):
                    assert same(r["x"], f["iterates"][r["iterations"]]) and same(r["history"], f["history"][:r["iterations"] + 1])
                edge = [c.name for c, r in zip(cases, models) if sec.first_kernel(c) and c.iterations == budget]
                assert all(r["status"] == cgc.MAX_ITERATIONS for c, r in zip(cases, models) if c.name in edge)
            assert any(sec.first_kernel(c) for c in cases) and any(not sec.first_kernel(c) for c in cases)


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_the_three_cases_and_the_tail_at_two_steps_per_workgroup(dtype):
    cases = [sec.by_name(n) for n in sec.BIG_GROUP]
    csr, B, X0, Dinv, _ = sec.columns_system(cases, sec.BIG, dtype)
    assert csr.m == sec.BIG and sec.columns_shape(3, sec.BIG) == (174762, 6) and Dinv is None and X0 is not None
    for multiply in MULTIPLIES.values():
        models = ccc.solve(multiply(csr), B, X0, max_iterations=sec.BUDGET)
        assert [ended(r) for r in models] == sec.declared_columns(cases) and np.isfinite(models[-1]["x"]).all()


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_atol_decides_in_a_column_at_begin_and_at_the_direction_test(dtype):
    """what the GPU test of atol relies on: among the columns of the exact cases without a guess there are residuals that are the square of a
    double a at both places that compare with the threshold; atol = a ends THAT column there, the next double below does not"""
    exact = [c for c in sec.column_groups(dtype)["plain_nox0"] if c.exact and c.status != cgc.NONFINITE]
    assert len(exact) >= 5
    places = set()
    for m in sec.ATOL_SIZES:
        csr, B, _, _, cases = sec.columns_system(exact, m, dtype)
        mul = cgc.matvec(csr)
        for j in range(B.shape[1]):
            b = np.ascontiguousarray(B[:, j])
            for a, k, end in sec.atol_probes(lambda atol: cgc.cg(mul, b, atol=atol, max_iterations=sec.BUDGET)):
                places.add(end)
                below = cgc.cg(mul, b, atol=float(np.nextafter(a, 0.0)), max_iterations=sec.BUDGET)
                assert (below["iterations"], below["end"]) != (k, end) and a > 0
    assert places == {"begin:converged", "direction:converged"}, places
