"""CPU: the catalogue of tests/solve_end_cases.py, proven with the host models alone (cg_cases.cg, bicgstab_cases.bicgstab on cg_cases.matvec) before
tests/test_gpu_solve_ends.py asks the device for the same ends.  No tolerance appears: every comparison is of statuses, counts or bits."""
import inspect
import re

import numpy as np
import pytest

import bicgstab_cases as bc
import cg_cases as cgc
import solve_end_cases as sec

NAMES = {np.float32: "f32", np.float64: "f64"}
# (case, dtype, with PRE folded in): every line of the catalogue in every type it lists, the BiCGStab ones that carry no Dinv of their own also
# behind the power-of-two right preconditioner
RUNS = [(c, d, pre) for c in sec.CASES for d in c.dtypes for pre in ((False, True) if c.solver == "bicgstab" and c.dinv is None else (False,))]
# the exact cases that the GPU test also runs at 2^20 + 2
BIG_CASES = ("b_half_2", "c_rr_2")


def run_id(run):
    return f"{run[0].name}-{NAMES[run[1]]}" + ("-pre" if run[2] else "")


def ended(r):
    return r["status"], r["iterations"], r["end"]


def declared(case):
    return case.status, case.iterations, case.end


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_each_case_ends_as_declared_without_a_subnormal(run):
    case, dtype, pre = run
    for m in sec.SIZES + ((sec.BIG,) if case.name in BIG_CASES else ()):
        csr, b, dinv, x0 = sec.system(case, m // 2, dtype, pre)
        assert csr.m == m == b.size and not sec.subnormal(csr.val, b, *(v for v in (dinv, x0) if v is not None)), m
        seen = []
        r = sec.run(case, m // 2, dtype, pre, watch=lambda *values: seen.append(sec.subnormal(*values)))
        assert ended(r) == declared(case), (m, ended(r))
        assert seen and not any(seen), (m, "a vector or a scalar of the run is a non-zero subnormal")
        assert r["history"].size == case.iterations + 1 and len(r["iterates"]) == case.iterations + 1
        if not case.exact:      # the same end when every row is accumulated in the next wider type and rounded once
            w = sec.run(case, m // 2, dtype, pre, multiply=sec.matvec_wide)
            assert ended(w) == declared(case), (m, ended(w))


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_budget_edges(run):
    """budgets of iterations - 1, iterations and iterations + 1: an end that the first kernel behind a multiply finds belongs to the iteration
    that was being started, so a budget of `iterations` never sees it"""
    case, dtype, pre = run
    k = case.iterations
    for m in (2, 1026):
        free = sec.run(case, m // 2, dtype, pre)
        for budget in (k - 1, k, k + 1):
            if budget < 0:
                continue
            r = sec.run(case, m // 2, dtype, pre, max_iterations=budget)
            if budget < k or (budget == k and sec.first_kernel(case)):
                assert ended(r) == (cgc.MAX_ITERATIONS, budget, "budget"), (m, budget, ended(r))
            else:
                assert ended(r) == declared(case), (m, budget, ended(r))
            assert np.array_equal(r["x"], free["iterates"][min(budget, k)], equal_nan=True)


@pytest.mark.parametrize("case", [c for c in sec.CASES if c.exact], ids=lambda c: c.name)
def test_exact_cases_have_the_same_values_in_both_types(case):
    assert case.dtypes == sec.BOTH
    for m in sec.SIZES + ((sec.BIG,) if case.name in BIG_CASES else ()):
        for pre in (False, True) if case.solver == "bicgstab" and case.dinv is None else (False,):
            lo, hi = sec.run(case, m // 2, np.float32, pre), sec.run(case, m // 2, np.float64, pre)
            assert ended(lo) == ended(hi) == declared(case)
            assert np.array_equal(lo["history"], hi["history"]) and lo["bb"] == hi["bb"] and lo["rr"] == hi["rr"]
            assert np.array_equal(lo.get("halves", 0), hi.get("halves", 0))
            assert len(lo["iterates"]) == len(hi["iterates"])
            for a, b in zip(lo["iterates"], hi["iterates"]):
                assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), b)


def test_the_rows_of_the_issue_that_are_exact_stay_exact():
    for name in ("b_rv0_1", "b_half_1", "b_half_2", "b_tt0_1", "b_ts0_1"):
        assert sec.by_name(name).exact, name
    assert all(sec.by_name(name).exact for name in BIG_CASES)


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_the_list_of_ends_is_the_models(solver):
    text = inspect.getsource(cgc.cg if solver == "cg" else bc.bicgstab)
    named = set(re.findall(r'"((?:begin|half|update|direction):\w+)"', text)) - {"begin:empty"}
    assert named == set(sec.ENDS[solver]) and len(set(sec.ENDS[solver])) == len(sec.ENDS[solver])
    assert {c.end for c in sec.CASES if c.solver == solver} <= named


def reached(solver, dtype, later=False):
    return {c.end for c in sec.CASES if c.solver == solver and dtype in c.dtypes and (c.iterations >= 1 or not later)}


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_every_end_is_reached_in_both_types(solver, dtype):
    missing = set(sec.ENDS[solver]) - reached(solver, dtype)
    print(f"{solver} {NAMES[dtype]}: reached {sorted(reached(solver, dtype))}; not reached {sorted(missing)}")
    assert missing <= set(sec.ALLOWED_GAPS[solver]), missing
    # ... and, in one type at least, at an iteration count >= 1 (an end of iteration 0 has none)
    loop = {e for e in sec.ENDS[solver] if not e.startswith("begin:")} - set(sec.ALLOWED_GAPS[solver])
    assert loop <= reached(solver, np.float32, True) | reached(solver, np.float64, True)
    # an end with an exact case among the integer blocks uses it
    for end in ("half:rv_zero", "update:ss_converged", "update:tt_zero", "update:ts_zero", "direction:converged") if solver == "bicgstab" else \
               ("begin:rz_breakdown", "update:pq_breakdown", "direction:rz_breakdown", "direction:converged"):
        assert any(c.exact for c in sec.CASES if c.solver == solver and c.end == end), end


def test_the_ends_no_case_reaches():
    gaps = {NAMES[d]: sorted(set(sec.ENDS["bicgstab"]) - reached("bicgstab", d)) for d in sec.BOTH}
    assert all(set(g) <= set(sec.ALLOWED_GAPS["bicgstab"]) for g in gaps.values())
    assert not set(sec.ENDS["cg"]) - (reached("cg", np.float32) & reached("cg", np.float64))
    if any(gaps.values()):
        pytest.skip("no catalogue case reaches these ends of the BiCGStab model: " + "; ".join(f"{t}: {', '.join(g)}" for t, g in gaps.items() if g) +
                    " (direction:nonfinite: a non-finite <r,r> or rho in bicg_direction; update:omega_nonfinite: omega non-finite behind finite <t,s> and <t,t>)")


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
def test_atol_decides_at_begin_at_the_half_step_and_at_the_direction_test(dtype):
    """what tests/test_gpu_solve_ends.py relies on: among the exact cases there are runs whose rr is the square of a double a at each of the
    three places that compare with the threshold, and there atol = a ends the run while the next double below does not"""
    places = {"cg": set(), "bicgstab": set()}
    for case in (c for c in sec.CASES if c.exact and c.status != cgc.NONFINITE):
        for m in sec.ATOL_SIZES:
            for a, k, end in sec.atol_probes(lambda atol: sec.run(case, m // 2, dtype, atol=atol)):
                places[case.solver].add(end)
                below = sec.run(case, m // 2, dtype, atol=float(np.nextafter(a, 0.0)))
                assert (below["iterations"], below["end"]) != (k, end) and a > 0
    assert places["bicgstab"] == {"begin:converged", "update:ss_converged", "direction:converged"}, places
    assert places["cg"] == {"begin:converged", "direction:converged"}, places


@pytest.mark.parametrize("dtype", sec.BOTH, ids=NAMES.get)
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_one_matrix_reaches_each_end_by_its_right_hand_side(solver, dtype):
    """the matrix of the GPU test of state between solves: the blocks of several cases side by side and a tridiagonal tail"""
    cases, csr, select = sec.state_system(solver, dtype)
    mul, solve = cgc.matvec(csr), sec.solver(cases[0])
    assert csr.m == 1026 and {c.end for c in cases} >= {e for e in sec.ENDS[solver] if e.endswith(("_zero", "_breakdown"))} - {"begin:bb_zero"}
    for j, case in enumerate(cases):
        b, dinv, x0 = select(j)
        r = solve(mul, b, x0=x0, dinv=dinv, max_iterations=sec.BUDGET)
        assert ended(r) == declared(case), (case.name, ended(r))
    assert cases[-1].status == cgc.NONFINITE and cases[-1].iterations >= 1
    b, _, _ = select(None, 1)
    for dinv in (None, (2.0 ** np.random.default_rng(11).integers(-1, 2, csr.m)).astype(dtype)):
        r = solve(mul, b, dinv=dinv, max_iterations=8)
        assert ended(r) == (cgc.MAX_ITERATIONS, 8, "budget") and np.isfinite(r["x"]).all() and r["rr"] > 1e-6 * r["bb"]
