"""CPU: the catalogue of tests/gmres_end_cases.py, proven with the host model alone (gmres_cases.gmres on cg_cases.matvec) before
tests/test_gpu_gmres_ends.py asks the device for the same ends.  No tolerance appears: every comparison is of statuses, counts or bits."""
import inspect
import re

import numpy as np
import pytest

import cg_cases as cgc
import gmres_cases as gc
import gmres_end_cases as ge
import solve_end_cases as sec

NAMES = {np.float32: "f32", np.float64: "f64"}
RUNS = [(c, d) for c in ge.CASES for d in c.dtypes]
HISTORY_RUNS = [(c, d) for c in ge.HISTORY_CASES for d in ge.BOTH]


def run_id(run):
    return f"{run[0].name}-{NAMES[run[1]]}"


def ended(r):
    return r["status"], r["iterations"], r["end"]


def declared(case):
    return case.status, case.iterations, case.end


def sizes_of(case):
    return ge.sizes(case) + ((ge.BIG,) if case.name == ge.BIG_CASE else ())


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_each_case_ends_as_declared_without_a_subnormal(run):
    case, dtype = run
    s = len(case.block)
    assert ge.place(case.restart, case.iterations, case.end) == (case.cycle, case.step)
    for m in sizes_of(case):
        csr, b, dinv, x0 = ge.system(case, m // s, dtype)
        assert csr.m == m == b.size and not sec.subnormal(csr.val, b, *(v for v in (dinv, x0) if v is not None)), m
        seen = []
        r = ge.run(case, m // s, dtype, watch=lambda *values: seen.append(sec.subnormal(*values)))
        assert ended(r) == declared(case), (m, ended(r))
        assert seen and not any(seen), (m, "a vector or a scalar of the run is a non-zero subnormal")
        assert r["history"].size == case.iterations + 1 and len(r["iterates"]) == case.iterations + 1
        # the same end when every row is accumulated in the next wider type and rounded once
        w = ge.run(case, m // s, dtype, multiply=sec.matvec_wide)
        assert ended(w) == declared(case), (m, ended(w))


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_budget_edges(run):
    """budgets of iterations - 1, iterations and iterations + 1: d = 0 and a non-finite h or d are found while MAKING step iterations + 1, so a
    budget of `iterations` never sees them; a restart's end is found behind the step that spent the budget, so it does"""
    case, dtype = run
    s, k = len(case.block), case.iterations
    for m in ge.sizes(case)[:3:2]:
        free = ge.run(case, m // s, dtype, max_iterations=k + 1)
        for budget in (k - 1, k, k + 1):
            if budget < 0:
                continue
            r = ge.run(case, m // s, dtype, max_iterations=budget)
            if budget < k or (budget == k and ge.found_making_a_step(case)) or case.end == "budget":
                assert ended(r) == (gc.MAX_ITERATIONS, budget, "budget"), (m, budget, ended(r))
            else:
                assert ended(r) == declared(case), (m, budget, ended(r))
            assert np.array_equal(r["x"], free["iterates"][min(budget, len(free["iterates"]) - 1)], equal_nan=True)


@pytest.mark.parametrize("run", HISTORY_RUNS, ids=run_id)
def test_an_atol_from_the_models_history_ends_a_later_cycle(run):
    case, dtype = run
    assert ge.place(case.restart, case.iterations, case.end) == (case.cycle, case.step) and case.cycle > 1
    for m in ge.HISTORY_SIZES:
        csr, b = gc.tri_ns(m, dtype), gc.rhs(m, dtype)
        for multiply in (cgc.matvec(csr), sec.matvec_wide(csr)):
            a, at, below = ge.history_probe(lambda atol: gc.gmres(multiply, b, case.restart, atol=atol, max_iterations=case.iterations + 3), case.iterations)
            assert a > 0 and at["rr"] <= a * a and not at["rr"] <= float(np.nextafter(a, 0.0)) ** 2


def test_the_list_of_ends_is_the_models():
    text = inspect.getsource(gc.gmres)
    named = set(re.findall(r'"((?:begin|rotate|restart):\w+)"', text)) - {"begin:empty"}
    assert named == set(ge.ENDS) and len(set(ge.ENDS)) == len(ge.ENDS)
    assert {c.end for c in ge.CASES} <= named | {"budget"}
    assert set(ge.ALLOWED_GAPS) <= {"rotate:exhausted", "rotate:rotation_nonfinite"}


def test_every_end_and_every_place_is_reached():
    reached = {c.end for c in ge.CASES} - {"budget"}
    places = ge.places_reached()
    print(f"gmres: ends reached {sorted(reached)}; not reached {sorted(set(ge.ENDS) - reached)}")
    print("gmres: (cycle, step) reached per end: " + "; ".join(f"{end}: {sorted((c.cycle, c.step) for c in ge.CASES + ge.HISTORY_CASES if c.end == end)}" for end in ge.REQUIRED_PLACES))
    assert reached == set(ge.ENDS) - set(ge.ALLOWED_GAPS)
    assert places == ge.REQUIRED_PLACES, {end: ge.REQUIRED_PLACES[end] - places[end] for end in places}
    for dtype in ge.BOTH:                    # ... in both types, and rotate:nonfinite in both at step 2 or later of the first cycle and in a later cycle
        assert {c.end for c in ge.CASES if dtype in c.dtypes} >= reached
        mine = [c for c in ge.CASES if dtype in c.dtypes and c.end == "rotate:nonfinite"]
        assert any(c.cycle == 1 and c.step >= 2 for c in mine) and any(c.cycle > 1 for c in mine), NAMES[dtype]


def test_a_seeded_search_never_reaches_the_allowed_gaps():
    """what ALLOWED_GAPS rests on beside its reasons: 4000 random blocks with and without a Dinv and a guess end in every other way and never in
    rotate:exhausted or rotate:rotation_nonfinite"""
    ends = {}
    for case, dtype in ge.random_systems(20, 4000):
        end = ge.run(case, 1, dtype)["end"]
        ends[end] = ends.get(end, 0) + 1
    print(f"gmres: 4000 random systems ended {sorted(ends.items())}")
    assert not set(ends) & set(ge.ALLOWED_GAPS) and {"rotate:nonfinite", "restart:nonfinite", "restart:zero", "rotate:d_zero", "rotate:converged"} <= set(ends)


@pytest.mark.parametrize("dtype", ge.BOTH, ids=NAMES.get)
def test_one_matrix_reaches_each_end_by_its_right_hand_side(dtype):
    """the matrix of the GPU test of state between solves: the blocks of several cases side by side and a tridiagonal tail"""
    cases, csr, select = ge.state_system(dtype)
    assert csr.m == 1026 and {c.end for c in cases} >= {"rotate:converged", "rotate:d_zero", "restart:zero", "begin:converged", "begin:bb_zero"}
    assert cases[-1].status == gc.NONFINITE and cases[-1].iterations >= 1 and max(c.restart for c in cases) <= 3
    for multiply in (cgc.matvec(csr), sec.matvec_wide(csr)):
        for j, case in enumerate(cases):
            b, dinv, x0 = select(j)
            r = gc.gmres(multiply, b, case.restart, x0=x0, dinv=dinv, atol=case.atol, max_iterations=case.budget)
            assert ended(r) == declared(case), (case.name, ended(r))
        b, _, _ = select(None, 1)
        for restart in (3, ge.G + 1):
            for dinv in (None, (2.0 ** np.random.default_rng(11).integers(-1, 2, csr.m)).astype(dtype)):
                r = gc.gmres(multiply, b, restart, dinv=dinv, max_iterations=2 * restart + 1)
                assert ended(r) == (gc.MAX_ITERATIONS, 2 * restart + 1, "budget") and np.isfinite(r["x"]).all() and r["rr"] > 1e-6 * r["bb"]
