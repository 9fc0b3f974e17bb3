"""CPU: the catalogue of tests/cg_mixed_end_cases.py, proven with the host model alone (cg_mixed_cases.cg_mixed on cg_cases.matvec) before
tests/test_gpu_cg_mixed_ends.py asks the device for the same ends.  No tolerance appears: every comparison is of statuses, counts or bits."""
import inspect
import re

import numpy as np
import pytest

import cg_cases as cgc
import cg_mixed_cases as mix
import cg_mixed_end_cases as me
import solve_end_cases as sec


def signature(r):
    return r["status"], r["iterations"], r["updates"], r["end"], tuple(r["segments"])


def declared(case):
    return case.status, case.iterations, case.updates, case.end, case.segments


def trace_of(case, reps=1, **kw):
    return me.traced(lambda watch: me.run(case, reps, watch=watch, **kw))


@pytest.mark.parametrize("case", me.CASES, ids=lambda c: c.name)
def test_each_case_ends_as_declared_without_a_subnormal(case):
    for m in me.SIZES + ((me.BIG,) if case.name == me.BIG_CASE else ()):
        hi, lo, b, dinv, x0 = me.system(case, m // 2)
        assert hi.m == lo.m == m == b.size and not sec.subnormal(hi.val, lo.val, b, *(v for v in (dinv, x0) if v is not None)), m
        seen = []
        r = me.run(case, m // 2, watch=lambda *values, what=None: seen.append(sec.subnormal(*values)))
        assert signature(r) == declared(case), (m, signature(r))
        assert seen and not any(seen), (m, "a vector or a scalar of the run is a non-zero subnormal")
        assert r["history"].size == case.iterations + 1 and len(r["iterates"]) == case.iterations + 1
        # the same end through the same segments when every row is accumulated in the next wider type and rounded once, on both sides
        w = me.run(case, m // 2, multiply=sec.matvec_wide)
        assert signature(w) == declared(case), (m, signature(w))


def first_kernel(case):
    """is the end found while STARTING iteration `iterations` + 1 (a segment's start, cg_update)?  A budget of `iterations` then never sees it"""
    return case.end.startswith(("segment:", "update:"))


@pytest.mark.parametrize("case", me.CASES, ids=lambda c: c.name)
def test_the_budget_edges_of_the_end_and_of_every_segment(case):
    """budgets of k - 1, k and k + 1 around the end and around every segment's end.  A budget the free run never spends changes nothing.  A
    budget it would overrun ends the solve AT the budget, in the update behind it -- `resume` comes before the budget test: the segments in
    front are the free run's, the last one ends as the free run's does when that ends there too and by "budget" otherwise, and what is tried is
    the free run's iterate."""
    for m in (2, 1026):
        free, trace = trace_of(case, m // 2)
        assert signature(free) == declared(case)
        for budget in sorted({k + d for k in {case.iterations} | {t[0] for t in trace} for d in (-1, 0, 1) if 0 <= k + d <= case.budget}):
            r, cut = trace_of(case, m // 2, max_iterations=budget)
            what = (m, budget, signature(r))
            if budget > case.iterations or (budget == case.iterations and not first_kernel(case)):
                assert signature(r) == declared(case) and np.array_equal(r["x"], free["x"], equal_nan=True), what
                continue
            assert r["iterations"] == budget, what
            if budget == 0:
                assert signature(r) == (mix.MAX_ITERATIONS, 0, 0, "start:budget", ()), what
                continue
            before = [t for t in trace if t[0] < budget]
            here = [t for t in trace if t[0] == budget]
            assert cut[:-1] == before and cut[-1][0] == budget and cut[-1][1] == (here[0][1] if here else "budget"), what
            assert cut[-1][3] == me.true_rr(case, m // 2, free["iterates"][budget]), what
            tried, committed = cut[-1][3], cut[-1][4]
            if not np.isfinite(tried):
                assert r["end"] == "resume:nonfinite" and not committed, what
            elif cut[-1][1] in ("exact", "estimate", "drop") and tried >= cut[-1][2]:
                assert r["end"] == "resume:stagnated" and not committed, what
            else:
                thr = max(case.rtol * case.rtol * r["bb"], case.atol * case.atol)
                assert committed and r["end"] == ("resume:converged" if tried <= thr else "resume:budget"), what
                assert r["rr"] == tried and np.array_equal(r["x"], free["iterates"][budget]) and r["updates"] == len(cut), what


@pytest.mark.parametrize("case", [c for c in me.CASES if c.name.startswith("m_rise_")], ids=lambda c: c.name)
def test_a_rise_behind_every_or_budget_is_committed(case):
    for m in me.SIZES:
        r, trace = trace_of(case, m // 2)
        risen = [(n, t) for n, t in enumerate(trace) if t[4] and t[3] >= t[2]]
        assert risen and {t[1] for _, t in risen} <= {"every", "budget"}, trace
        n, (at, reason, before, after, _) = risen[0]
        assert r["updates"] > n and r["history"][at] == after >= before          # committed: counted, and the history holds the risen rr
        assert not np.array_equal(r["iterates"][at], r["iterates"][0]) and not (r["status"] == mix.STAGNATED and r["updates"] == n)
        if n == len(trace) - 1:                                                  # the last thing the run did: x is x + y, rr the risen one
            assert np.array_equal(r["x"], r["iterates"][at]) and r["rr"] == after


def test_the_list_of_ends_is_the_models():
    text = inspect.getsource(mix.cg_mixed)
    named = set(re.findall(r'"((?:start|segment|update|direction|resume):\w+)"', text)) - {"start:empty"}
    assert named == set(me.ENDS) and len(set(me.ENDS)) == len(me.ENDS) == 17 and me.ALLOWED_GAPS == ()
    assert set(re.findall(r'reason = "(\w+)"', text)) == set(me.SEGMENT_ENDS)
    assert {c.end for c in me.CASES} <= named and len({c.name for c in me.CASES}) == len(me.CASES)


def test_every_end_and_every_place_is_reached():
    reached = {c.end for c in me.CASES}
    traces = {c.name: trace_of(c)[1] for c in me.CASES}
    places = me.places_reached(traces)
    print(f"cg_mixed: ends reached {sorted(reached)}; not reached {sorted(set(me.ENDS) - reached)}")
    print(f"cg_mixed: (end, segment in front) reached: {sorted({(c.end, len(c.segments), c.segments[-1] if c.segments else None) for c in me.CASES})}")
    print(f"cg_mixed: required places reached: {sorted(places)}")
    assert reached == set(me.ENDS) - set(me.ALLOWED_GAPS)
    assert places == me.REQUIRED_PLACES, me.REQUIRED_PLACES - places
    # every non-start end at one iteration or more
    assert {c.end for c in me.CASES if c.iterations >= 1} >= {e for e in me.ENDS if not e.startswith("start:")}
    # the rise lines: one ends its segment by "every", one by "budget"
    assert {reason for c in me.CASES if c.name.startswith("m_rise_") for reason in me.rises(traces[c.name])} == {"every", "budget"}


def test_atol_decides_at_the_estimate_and_at_the_committed_residual():
    """what tests/test_gpu_cg_mixed_ends.py relies on: runs whose rs at an "estimate" end, and whose committed rr at a resume:converged, is the
    square of a double a: atol = a ends the run there while the next double below does not"""
    places = set()
    for case in me.CASES:
        for m in (2, 1024, 1026):
            for a, k, where in me.atol_probes(lambda atol, watch=None: me.run(case, m // 2, watch=watch, rtol=0.0, atol=atol)):
                places.add(where)
    assert places == {"estimate", "resume:converged"}, places


def test_one_pair_of_matrices_reaches_each_end_by_its_right_hand_side():
    """the pair of the GPU test of state between solves: the blocks of several cases side by side and a tridiagonal tail"""
    cases, high, low, select = me.state_system()
    assert high.m == low.m == 1026 and {c.status for c in cases} == {mix.CONVERGED, mix.MAX_ITERATIONS, mix.BREAKDOWN, mix.NONFINITE, mix.STAGNATED}
    assert {c.end.split(":")[0] for c in cases} == {"start", "segment", "update", "direction", "resume"}
    assert cases[-1].status == mix.NONFINITE and cases[-1].iterations >= 1
    for multiply in (cgc.matvec, sec.matvec_wide):
        mh, ml = multiply(high), multiply(low)
        for j, case in enumerate(cases):
            b, dinv, x0 = select(j)
            r = mix.cg_mixed(mh, ml, b, x0=x0, dinv=dinv, **me.options(case))
            assert signature(r) == declared(case), (case.name, signature(r))
        b, _, _ = select(None, 1)
        for dinv in (None, (2.0 ** np.random.default_rng(11).integers(-1, 2, high.m)).astype(np.float32)):
            r = mix.cg_mixed(mh, ml, b, dinv=dinv, rtol=0.0, max_iterations=7, update_every=3)
            assert signature(r)[:4] == (mix.MAX_ITERATIONS, 7, 3, "resume:budget") and np.isfinite(r["x"]).all() and r["rr"] > 1e-6 * r["bb"]
