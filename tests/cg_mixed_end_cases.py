"""A catalogue of the ways spmv_hip_cg_mixed can end (tests/test_cg_mixed_ends_host.py, tests/test_gpu_cg_mixed_ends.py), in the style of
tests/solve_end_cases.py.

A case is a symmetric 2 x 2 fp64 block `high`, a float block `low` of the same pattern (which need NOT be the narrowed `high`: a `low` of
high / 4 is how a recurrence claims a drop that the truth does not show), a right-hand side of two elements and, where it needs them, a Dinv, a
guess, rtol, atol, update_every, update_drop and the budget it runs with.  `system` repeats them `reps` times along the diagonal, so every row,
every workgroup and every size runs the same small recurrence.  A line says the status, the iterations, the committed updates, the `end` in the
words of the model (cg_mixed_cases.cg_mixed: result["end"]) and the reasons that ended its segments, in order (result["segments"]).
tests/test_cg_mixed_ends_host.py proves every line with the model alone; tests/test_gpu_cg_mixed_ends.py then asks the device for the same bits.

Entries are a mantissa of {0, +-1, 1.25, -1.5, +-2} times a power of two, so that a dot, alpha or beta overflows without any operand being a
subnormal number: denormal handling is not part of the contract.  Every line but the first comes from a random search over such blocks; a line
was kept only where it ends the same way, through the same segments, at every size of SIZES, under cg_cases.matvec and under
solve_end_cases.matvec_wide on both sides, without a subnormal.  The m_rise_* lines are the ones in which an update behind "every" or "budget"
is COMMITTED although the true residual rose (`low` is a fraction of `high`)."""
from collections import namedtuple

import numpy as np

import cg_cases as cgc
import cg_mixed_cases as mix

C, M, B, N, S = mix.CONVERGED, mix.MAX_ITERATIONS, mix.BREAKDOWN, mix.NONFINITE, mix.STAGNATED

Case = namedtuple("Case", "name high low b dinv x0 rtol atol every drop budget status iterations updates end segments")

SIZES = (2, 1024, 1026, 4100)           # one workgroup, one full workgroup, two elements in a second workgroup, five workgroups
BIG = 2 ** 20 + 2                       # P = 1024, two steps per workgroup
BIG_CASE = "m_resume_converged_after_exact"


def _m(name, high, b, budget, status, iterations, updates, end, segments, low=None, dinv=None, x0=None, rtol=0.0, atol=0.0, every=0, drop=0.0):
    pair = lambda v: None if v is None else tuple(float(e) for e in v)
    high = tuple(pair(row) for row in high)
    low = high if low is None else tuple(pair(row) for row in low)
    assert high[0][1] == high[1][0] and low[0][1] == low[1][0]
    return Case(name, high, low, pair(b), pair(dinv), pair(x0), float(rtol), float(atol), every, float(drop), budget, status, iterations, updates, end,
                tuple(segments))


CASES = [
    _m("m_start_budget", [[2, -1], [-1, 2]], [1, 2], 0, M, 0, 0, "start:budget", []),
    _m("m_rise_resume_budget_after_every", [[1, -1], [-1, -2]], [1.25, -1], 1, M, 1, 1, "resume:budget", ('every',), low=[[2.0 ** -2, -2.0 ** -2], [-2.0 ** -2, -2.0 ** -1]], every=1, drop=0.5),
    _m("m_rise_resume_budget_after_every_b", [[1, -1.5], [-1.5, 2]], [0, -1], 1, M, 1, 1, "resume:budget", ('every',), low=[[2.0 ** -2, -1.5 * 2.0 ** -2], [-1.5 * 2.0 ** -2, 2.0 ** -1]], every=1, drop=0.5),
    _m("m_rise_update_pq_breakdown_after_every", [[1, -1.5], [-1.5, 2]], [-1, 2], 3, B, 1, 1, "update:pq_breakdown", ('every',), low=[[2.0 ** -2, -1.5 * 2.0 ** -2], [-1.5 * 2.0 ** -2, 2.0 ** -1]], every=1, drop=0.001),
    _m("m_rise_update_pq_breakdown_after_every_b", [[2, 2], [2, -1.5]], [-1, -2], 4, B, 1, 1, "update:pq_breakdown", ('every',), low=[[2.0 ** -1, 2.0 ** -1], [2.0 ** -1, -1.5 * 2.0 ** -2]], every=1),
    _m("m_rise_resume_budget_after_budget", [[2, -2], [-2, 1]], [2, -1], 1, M, 1, 1, "resume:budget", ('budget',), low=[[2.0 ** -2, -2.0 ** -2], [-2.0 ** -2, 2.0 ** -3]], every=2, drop=0.001),
    _m("m_rise_resume_budget_after_budget_b", [[1.25, 1], [1, 1]], [2, -1], 1, M, 1, 1, "resume:budget", ('budget',), low=[[1.25 * 2.0 ** -2, 2.0 ** -2], [2.0 ** -2, 2.0 ** -2]], every=2, drop=0.001),
    _m("m_rise_resume_budget_after_drop_every_budget", [[2, -1], [-1, 1.25]], [2, 1], 5, M, 5, 3, "resume:budget", ('drop', 'every', 'budget'), low=[[1, -2.0 ** -1], [-2.0 ** -1, 1.25 * 2.0 ** -1]], every=2),
    _m("m_rise_resume_budget_after_every_budget", [[1, -1], [-1, 1]], [1.25, -1], 3, M, 3, 2, "resume:budget", ('every', 'budget'), low=[[2.0 ** -2, -2.0 ** -2], [-2.0 ** -2, 2.0 ** -2]], every=2, drop=0.001),
    _m("m_resume_converged_after_every_estimate", [[1.25, 1.25], [1.25, 2]], [0, 1], 2, C, 2, 2, "resume:converged", ('every', 'estimate'), rtol=2.0 ** -4, every=1),
    _m("m_update_pq_breakdown_after_drop", [[2, 1], [1, -1]], [1.25, 0], 5, B, 1, 1, "update:pq_breakdown", ('drop',), dinv=[2, 2], every=1, drop=0.5),
    _m("m_update_pq_breakdown", [[-1.5, 1.25], [1.25, 2]], [-1.5, 2], 1, B, 0, 0, "update:pq_breakdown", (), low=[[-1.5 * 2.0 ** 1, 1.25 * 2.0 ** 1], [1.25 * 2.0 ** 1, 4]], every=2, drop=0.25),
    _m("m_resume_stagnated_after_drop", [[-1, 1], [1, 1.25]], [1, 2], 6, S, 1, 0, "resume:stagnated", ('drop',), low=[[-2.0 ** -2, 2.0 ** -2], [2.0 ** -2, 1.25 * 2.0 ** -2]], rtol=2.0 ** -7, every=3, drop=0.5),
    _m("m_resume_converged_after_estimate", [[1, -2], [-2, 0]], [-1.5, 1], 6, C, 1, 1, "resume:converged", ('estimate',), rtol=2.0 ** -3, every=3, drop=0.5),
    _m("m_update_pq_breakdown_after_every", [[-1, 1.25], [1.25, -1.5]], [1.25, 2], 4, B, 1, 1, "update:pq_breakdown", ('every',), low=[[1.25, 1], [1, -1.5]], rtol=2.0 ** -7, every=1, drop=0.5),
    _m("m_resume_stagnated_after_estimate", [[1.25, 1], [1, 2]], [-1.5, 1.25], 6, S, 2, 0, "resume:stagnated", ('estimate',), low=[[1.25 * 2.0 ** -2, 2.0 ** -2], [2.0 ** -2, 2.0 ** -1]], dinv=[1, 2], rtol=2.0 ** -8),
    _m("m_segment_rz_breakdown", [[0, 1.25], [1.25, 2]], [1, 1], 1, B, 0, 0, "segment:rz_breakdown", (), dinv=[-1, 2.0 ** -1], rtol=2.0 ** -5),
    _m("m_resume_budget_after_exact", [[1, 0], [0, -2]], [-2, 0], 1, M, 1, 1, "resume:budget", ('exact',), low=[[2, 0], [0, -4]], rtol=2.0 ** -6, drop=0.5),
    _m("m_resume_budget_after_exact_exact_budget", [[2, -1], [-1, 2]], [0, 2], 5, M, 5, 3, "resume:budget", ('exact', 'exact', 'budget'), every=3),
    _m("m_direction_rz_breakdown", [[2, -2], [-2, -1.5]], [-1, -2], 2, B, 1, 0, "direction:rz_breakdown", (), dinv=[-2.0 ** -1, 2.0 ** -1], rtol=2.0 ** -11),
    _m("m_resume_budget_after_every_every_every", [[-2, 1.25], [1.25, 2]], [1, -1], 3, M, 3, 3, "resume:budget", ('every', 'every', 'every'), low=[[1, 1.25], [1.25, 2]], every=1),
    _m("m_resume_budget_after_budget", [[1.25, -2], [-2, 1.25]], [0, -2], 1, M, 1, 1, "resume:budget", ('budget',), atol=2.0 ** 0, every=2, drop=0.25),
    _m("m_resume_converged_after_drop_drop_drop_drop", [[1, 0], [0, 1]], [1, 1], 5, C, 4, 4, "resume:converged", ('drop', 'drop', 'drop', 'drop'), dinv=[2, 1], drop=0.5),
    _m("m_resume_budget_after_every", [[-2, 2], [2, 1.25]], [-2, -2], 1, M, 1, 1, "resume:budget", ('every',), every=1),
    _m("m_resume_budget_after_drop_drop", [[1.25, -1], [-1, 1.25]], [1, -1], 2, M, 2, 2, "resume:budget", ('drop', 'drop'), dinv=[2.0 ** -1, 1], every=1, drop=0.25),
    _m("m_start_bb_zero", [[1.25, 1.25], [1.25, 0]], [0, 0], 4, C, 0, 0, "start:bb_zero", (), dinv=[2, 2], atol=2.0 ** -7, every=1),
    _m("m_resume_stagnated_after_exact", [[2, 1], [1, 2]], [-2, -1.5], 3, S, 2, 0, "resume:stagnated", ('exact',), low=[[1, 1.25], [1.25, 2]], rtol=2.0 ** -4, drop=0.25),
    _m("m_resume_converged_after_every_exact", [[1.25, 1], [1, 1]], [1, -1], 2, C, 2, 2, "resume:converged", ('every', 'exact'), atol=2.0 ** -9, every=1, drop=0.25),
    _m("m_resume_budget_after_drop", [[-2, 1.25], [1.25, 2]], [1, 0], 1, M, 1, 1, "resume:budget", ('drop',), low=[[-4, 1.25 * 2.0 ** 1], [1.25 * 2.0 ** 1, 4]], x0=[-1, -2]),
    _m("m_resume_converged_after_exact", [[2, 0], [0, 1]], [0, 1], 3, C, 1, 1, "resume:converged", ('exact',), dinv=[2, 1], rtol=2.0 ** -2, every=2),
    _m("m_update_pq_breakdown_after_estimate", [[-1.5, -2], [-2, 1]], [-1.5, 2], 5, B, 1, 1, "update:pq_breakdown", ('estimate',), low=[[-1.5 * 2.0 ** 1, -4], [-4, 2]], dinv=[2.0 ** -1, 1], rtol=2.0 ** -4),
    _m("m_resume_budget_after_exact_exact_exact_exact", [[-1, 0], [0, 2]], [0, -2], 4, M, 4, 4, "resume:budget", ('exact', 'exact', 'exact', 'exact'), low=[[-2, 0], [0, 4]], every=1, drop=0.25),
    _m("m_resume_converged_after_drop", [[2, 0], [0, 1]], [-1.5, 1.25], 2, C, 2, 1, "resume:converged", ('drop',), every=3, drop=0.25),
    _m("m_resume_stagnated_after_drop_drop", [[-1, 1], [1, 1]], [0, -1.5], 4, S, 3, 1, "resume:stagnated", ('drop', 'drop'), low=[[1, 1], [1, 2]], dinv=[2, 2], rtol=2.0 ** -4, every=2, drop=0.5),
    _m("m_start_converged", [[0, 2], [2, 2]], [0, 2], 4, C, 0, 0, "start:converged", (), low=[[0, 4], [4, 4]], x0=[1, 0], every=1),
    _m("m_update_pq_breakdown_after_every_every", [[1.25, 1], [1, -2]], [1, -1], 6, B, 2, 2, "update:pq_breakdown", ('every', 'every'), low=[[2, -2], [-2, 2]], dinv=[1, 1], x0=[-1.5, 1.25], every=1),
    _m("m_resume_budget_after_estimate", [[1.25, -1], [-1, 1.25]], [0, -2], 2, M, 2, 1, "resume:budget", ('estimate',), low=[[1.25 * 2.0 ** 1, -2], [-2, 1.25 * 2.0 ** 1]], dinv=[2, 1], rtol=2.0 ** -1, every=3, drop=0.25),
    _m("m_resume_stagnated_after_exact_estimate", [[-1, 0], [0, 1.25]], [1, -1.5], 2, S, 2, 1, "resume:stagnated", ('exact', 'estimate'), low=[[1.25, 0], [0, 1.25]], atol=2.0 ** -6),
    _m("m_resume_budget_after_exact_exact_exact_exact_exact_estimate", [[1.25, 0], [0, 1]], [-1, 0], 6, M, 6, 6, "resume:budget", ('exact', 'exact', 'exact', 'exact', 'exact', 'estimate'), low=[[1.25 * 2.0 ** 1, 0], [0, 2]], rtol=2.0 ** -10, every=2),
    _m("m_resume_converged_after_estimate_every_every_every_every", [[2, -1], [-1, 2]], [1.25, 0], 6, C, 5, 5, "resume:converged", ('estimate', 'every', 'every', 'every', 'every'), low=[[4, -2], [-2, 4]], dinv=[2.0 ** -1, 1], x0=[2, 1.25], rtol=2.0 ** -1, every=1),
    _m("m_update_pq_breakdown_after_exact", [[-1, -2], [-2, 2]], [-1, 1], 3, B, 2, 1, "update:pq_breakdown", ('exact',), low=[[2, -2], [-2, 2]], dinv=[1, 2.0 ** -1]),
    _m("m_segment_rz_breakdown_after_estimate", [[-1.5, 1.25], [1.25, 1]], [-1.5, -1.5], 2, B, 1, 1, "segment:rz_breakdown", ('estimate',), low=[[1.25, 1.25], [1.25, 1.25]], dinv=[-2.0 ** -1, 2], rtol=2.0 ** -3),
    _m("m_resume_converged_after_drop_budget", [[1, 1], [1, 1]], [-1, -1], 2, C, 2, 2, "resume:converged", ('drop', 'budget'), low=[[2, 1], [1, 1]], x0=[1.25, 2], atol=2.0 ** -8, every=3, drop=0.25),
    _m("m_resume_converged_after_every", [[1.25, 0], [0, 1]], [2, 2], 1, C, 1, 1, "resume:converged", ('every',), low=[[1, 0], [0, 1.25]], dinv=[2.0 ** -1, 2], rtol=2.0 ** -1, every=1),
    _m("m_direction_nonfinite_after_every_every", [[2, 1], [1, -1.5]], [-1.5, 1.25], 5, N, 5, 2, "direction:nonfinite", ('every', 'every'), low=[[1, -1], [-1, 1]], x0=[-1, 2], every=2, drop=0.5),
    _m("m_resume_nonfinite_after_every", [[2.0 ** -100, 0], [0, 2.0 ** 30]], [-2.0 ** 60, 2.0 ** 30], 5, N, 2, 0, "resume:nonfinite", ('every',), rtol=2.0 ** -3, every=2),
    _m("m_update_dot_nonfinite", [[2.0 ** 101, -1], [-1, 2.0 ** 60]], [-2.0 ** 101, 2], 4, N, 1, 0, "update:dot_nonfinite", (), low=[[1.25 * 2.0 ** -60, -1.5 * 2.0 ** -60], [-1.5 * 2.0 ** -60, 1.25 * 2.0 ** 60]], atol=2.0 ** -11, drop=0.25),
    _m("m_direction_nonfinite", [[1.25 * 2.0 ** -60, 2.0 ** -99], [2.0 ** -99, 2.0 ** 101]], [-2.0 ** -60, 0], 4, N, 1, 0, "direction:nonfinite", (), low=[[-1.5 * 2.0 ** 100, 1.25 * 2.0 ** -30], [1.25 * 2.0 ** -30, 2.0 ** -99]], x0=[-1, -2], atol=2.0 ** -6, every=2),
    _m("m_update_alpha_nonfinite", [[-1.5 * 2.0 ** -60, 2.0 ** -100], [2.0 ** -100, 0]], [0, -2.0 ** 31], 3, N, 0, 0, "update:alpha_nonfinite", (), dinv=[2, 2], x0=[0, 2], atol=2.0 ** 2, every=1),
    _m("m_direction_beta_nonfinite", [[-2.0 ** -100, 1.25 * 2.0 ** 60], [1.25 * 2.0 ** 60, 2.0 ** 100]], [1.25, 1.25 * 2.0 ** -100], 2, N, 1, 0, "direction:beta_nonfinite", (), atol=2.0 ** -4, every=3),
    _m("m_update_alpha_nonfinite_after_drop", [[2.0 ** 61, -1.5], [-1.5, 0]], [-2.0 ** 31, 2.0 ** -29], 4, N, 1, 1, "update:alpha_nonfinite", ('drop',), low=[[2.0 ** 62, -1.5 * 2.0 ** 1], [-1.5 * 2.0 ** 1, 0]], every=2),
    _m("m_update_dot_nonfinite_after_every", [[2.0 ** -59, 1], [1, 1]], [-1.5 * 2.0 ** 30, 1.25 * 2.0 ** -100], 2, N, 1, 1, "update:dot_nonfinite", ('every',), low=[[2.0 ** -58, 2], [2, 2]], x0=[1, -1], atol=2.0 ** -10, every=1, drop=0.5),
    _m("m_resume_nonfinite_after_drop", [[2.0 ** -60, -2.0 ** -100], [-2.0 ** -100, 0]], [-2.0 ** 101, -2.0 ** 61], 4, N, 1, 0, "resume:nonfinite", ('drop',), every=3),
    _m("m_resume_nonfinite_after_budget", [[2.0 ** -30, -2.0 ** -59], [-2.0 ** -59, 2.0 ** -60]], [-1.5 * 2.0 ** 30, -2.0 ** 100], 1, N, 1, 0, "resume:nonfinite", ('budget',), low=[[2.0 ** -29, -2.0 ** -58], [-2.0 ** -58, 2.0 ** -59]], dinv=[2.0 ** -1, 1]),
    _m("m_resume_nonfinite_after_exact", [[2.0 ** -60, 1.25 * 2.0 ** -100], [1.25 * 2.0 ** -100, 1.25 * 2.0 ** -100]], [1.25 * 2.0 ** -60, -2.0 ** 60], 6, N, 2, 0, "resume:nonfinite", ('exact',), rtol=2.0 ** -11, every=3, drop=0.25),
    _m("m_update_dot_nonfinite_after_every_every", [[2.0 ** 100, -1.5 * 2.0 ** 30], [-1.5 * 2.0 ** 30, 1.25 * 2.0 ** -30]], [-1.5 * 2.0 ** -30, 1.25], 3, N, 2, 2, "update:dot_nonfinite", ('every', 'every'), low=[[2.0 ** 98, -1.5 * 2.0 ** 28], [-1.5 * 2.0 ** 28, 1.25 * 2.0 ** -32]], atol=2.0 ** -3, every=1),
    _m("m_direction_nonfinite_after_drop", [[2.0 ** 31, 1.25 * 2.0 ** -30], [1.25 * 2.0 ** -30, 2]], [2.0 ** -29, -2.0 ** 100], 5, N, 2, 1, "direction:nonfinite", ('drop',), low=[[2.0 ** 32, 1.25 * 2.0 ** -29], [1.25 * 2.0 ** -29, 4]], every=3, drop=0.5),
    _m("m_update_alpha_nonfinite_after_estimate", [[1.25 * 2.0 ** -60, 0], [0, 2.0 ** -60]], [-1.5 * 2.0 ** 60, -2.0 ** -60], 5, N, 1, 1, "update:alpha_nonfinite", ('estimate',), low=[[1.25 * 2.0 ** -59, 0], [0, 2.0 ** -59]], atol=2.0 ** -1, every=1, drop=0.5),
    _m("m_direction_nonfinite_after_every", [[2.0 ** -100, 1.25], [1.25, 1.25 * 2.0 ** 30]], [-1.5 * 2.0 ** 60, 2.0 ** 61], 6, N, 2, 1, "direction:nonfinite", ('every',), x0=[-1, 0], atol=2.0 ** -10, every=1, drop=0.25),
    _m("m_resume_nonfinite_after_estimate", [[1.25 * 2.0 ** -60, -1.5 * 2.0 ** -100], [-1.5 * 2.0 ** -100, -1.5]], [-1.5 * 2.0 ** 100, 0], 3, N, 1, 0, "resume:nonfinite", ('estimate',), low=[[1.25 * 2.0 ** -59, -1.5 * 2.0 ** -99], [-1.5 * 2.0 ** -99, -1.5 * 2.0 ** 1]], rtol=2.0 ** -8, every=2),
    _m("m_update_dot_nonfinite_after_estimate", [[0, 2.0 ** -99], [2.0 ** -99, 2.0 ** 30]], [-2.0 ** 30, 2.0 ** 61], 3, N, 2, 1, "update:dot_nonfinite", ('estimate',), low=[[0, 2.0 ** -98], [2.0 ** -98, 2.0 ** 31]], rtol=2.0 ** -3),
    _m("m_direction_beta_nonfinite_after_estimate", [[2.0 ** 101, -2.0 ** -99], [-2.0 ** -99, 1.25 * 2.0 ** 30]], [0, 2.0 ** 30], 6, N, 2, 1, "direction:beta_nonfinite", ('estimate',), atol=2.0 ** -8, drop=0.5),
    _m("m_update_dot_nonfinite_after_drop", [[-2.0 ** 100, -2.0 ** -99], [-2.0 ** -99, 2.0 ** -29]], [-2.0 ** -99, 1.25 * 2.0 ** 60], 4, N, 1, 1, "update:dot_nonfinite", ('drop',), low=[[-2.0 ** 101, -2.0 ** -98], [-2.0 ** -98, 2.0 ** -28]], atol=2.0 ** -11),
    _m("m_update_dot_nonfinite_after_drop_drop", [[2.0 ** 61, 1], [1, 2.0 ** 101]], [-2.0 ** 30, -2.0 ** -59], 6, N, 4, 2, "update:dot_nonfinite", ('drop', 'drop'), dinv=[2.0 ** -1, 1], every=3, drop=0.25),
    _m("m_segment_zero_after_exact", [[2.0 ** 101, 1.25 * 2.0 ** -100], [1.25 * 2.0 ** -100, 2]], [-2, 0], 3, S, 1, 1, "segment:zero", ('exact',), dinv=[1, 1], every=3),
    _m("m_segment_nonfinite_after_every", [[-1.5 * 2.0 ** 60, -2.0 ** 101], [-2.0 ** 101, 2.0 ** 31]], [-1, 2.0 ** 61], 4, N, 1, 1, "segment:nonfinite", ('every',), low=[[2.0 ** -100, 2.0 ** -30], [2.0 ** -30, 2.0 ** -30]], every=1),
    _m("m_update_alpha_nonfinite_after_drop_every", [[2.0 ** 60, -1.5 * 2.0 ** -100], [-1.5 * 2.0 ** -100, 2.0 ** -59]], [-2.0 ** -100, 1.25 * 2.0 ** 60], 5, N, 2, 2, "update:alpha_nonfinite", ('drop', 'every'), low=[[2.0 ** 61, -1.5 * 2.0 ** -99], [-1.5 * 2.0 ** -99, 2.0 ** -58]], dinv=[2, 1], every=1),
    _m("m_resume_nonfinite_after_every_estimate", [[2.0 ** -99, 0], [0, 1]], [2.0 ** 30, -1.5 * 2.0 ** 30], 6, N, 4, 1, "resume:nonfinite", ('every', 'estimate'), x0=[-2, -1], rtol=2.0 ** -11, every=2, drop=0.25),
    _m("m_direction_beta_nonfinite_after_exact", [[0, 2.0 ** 61], [2.0 ** 61, 2.0 ** -29]], [-2.0 ** -100, -2], 6, N, 2, 1, "direction:beta_nonfinite", ('exact',), x0=[-1, -1], every=3, drop=0.5),
    _m("m_update_pq_breakdown_after_exact_drop", [[1.25 * 2.0 ** 30, -1], [-1, 0]], [-2.0 ** -60, -1.5 * 2.0 ** -60], 4, B, 2, 2, "update:pq_breakdown", ('exact', 'drop'), x0=[1, -2], rtol=2.0 ** -8),
    _m("m_direction_beta_nonfinite_after_every", [[1.25 * 2.0 ** -30, -1.5 * 2.0 ** -60], [-1.5 * 2.0 ** -60, -2.0 ** 61]], [-2.0 ** -59, -2.0 ** -60], 4, N, 2, 1, "direction:beta_nonfinite", ('every',), low=[[2.0 ** -59, -2.0 ** 31], [-2.0 ** 31, 1.25 * 2.0 ** 60]], dinv=[2.0 ** -1, 2.0 ** -1], rtol=2.0 ** -11, every=1),
    _m("m_update_alpha_nonfinite_after_every_every_estimate", [[2.0 ** 30, 2.0 ** -99], [2.0 ** -99, 1.25 * 2.0 ** -100]], [2.0 ** -30, -1.5], 6, N, 3, 3, "update:alpha_nonfinite", ('every', 'every', 'estimate'), atol=2.0 ** -8, every=1, drop=0.5),
    _m("m_update_alpha_nonfinite_after_every", [[2.0 ** 31, 1.25 * 2.0 ** -30], [1.25 * 2.0 ** -30, 1.25 * 2.0 ** 100]], [-1.5, -2], 5, N, 1, 1, "update:alpha_nonfinite", ('every',), low=[[2, -2.0 ** -29], [-2.0 ** -29, 2.0 ** -30]], dinv=[2.0 ** -1, 1], every=1, drop=0.5),
    _m("m_direction_beta_nonfinite_after_drop", [[2.0 ** -60, 0], [0, 1.25 * 2.0 ** 100]], [2.0 ** -60, -1], 4, N, 2, 1, "direction:beta_nonfinite", ('drop',), every=1, drop=0.25),
    _m("m_segment_nonfinite_after_every_every", [[-2.0 ** 61, -2.0 ** 60], [-2.0 ** 60, 2.0 ** 30]], [2.0 ** -29, 0], 6, N, 2, 2, "segment:nonfinite", ('every', 'every'), low=[[1.25 * 2.0 ** -30, -2.0 ** -60], [-2.0 ** -60, 2.0 ** 61]], x0=[-2, -1.5], every=1),
    _m("m_resume_nonfinite_after_every_every", [[2.0 ** -59, 0], [0, 2.0 ** -100]], [-2.0 ** 60, -2.0 ** 61], 2, N, 2, 1, "resume:nonfinite", ('every', 'every'), low=[[2.0 ** -58, 0], [0, 2.0 ** -99]], atol=2.0 ** 3, every=1, drop=0.5),
    _m("m_resume_nonfinite_after_drop_exact", [[1, 2.0 ** -59], [2.0 ** -59, 2.0 ** -99]], [-2.0 ** 100, 0], 5, N, 2, 1, "resume:nonfinite", ('drop', 'exact'), every=2),
    _m("m_update_alpha_nonfinite_after_every_drop", [[1.25 * 2.0 ** -60, 2.0 ** -99], [2.0 ** -99, 2.0 ** 31]], [1.25 * 2.0 ** 30, -2.0 ** -59], 6, N, 2, 2, "update:alpha_nonfinite", ('every', 'drop'), every=1, drop=0.25),
    _m("m_segment_zero_after_exact_exact", [[-2.0 ** -99, 2.0 ** -100], [2.0 ** -100, 1.25]], [0, -1.5 * 2.0 ** -100], 3, S, 2, 2, "segment:zero", ('exact', 'exact'), every=3),
    _m("m_direction_nonfinite_after_estimate", [[2.0 ** 30, 0], [0, 2.0 ** 31]], [-2.0 ** 61, 2.0 ** -29], 5, N, 3, 1, "direction:nonfinite", ('estimate',), x0=[-1.5, 0], atol=2.0 ** -5, every=3, drop=0.5),
    _m("m_resume_stagnated_after_drop_exact", [[2.0 ** 61, 1.25 * 2.0 ** -100], [1.25 * 2.0 ** -100, 2.0 ** 60]], [0, -2.0 ** 60], 6, S, 2, 1, "resume:stagnated", ('drop', 'exact'), every=3, drop=0.5),
    _m("m_direction_rz_breakdown_after_exact", [[-2.0 ** -99, 2.0 ** -29], [2.0 ** -29, 2.0 ** 30]], [2.0 ** -60, 0], 2, B, 2, 1, "direction:rz_breakdown", ('exact',), dinv=[-2.0 ** -1, 2.0 ** -1], x0=[1, -1]),
    _m("m_direction_beta_nonfinite_after_exact_drop", [[-2.0 ** -59, 2.0 ** -29], [2.0 ** -29, 1.25 * 2.0 ** 60]], [0, -1], 6, N, 3, 2, "direction:beta_nonfinite", ('exact', 'drop'), x0=[-1.5, 2], every=2, drop=0.5),
    _m("m_resume_nonfinite_after_drop_drop", [[2.0 ** -30, -1.5 * 2.0 ** -100], [-1.5 * 2.0 ** -100, 1.25 * 2.0 ** -100]], [1.25 * 2.0 ** 60, -1.5 * 2.0 ** 30], 6, N, 4, 1, "resume:nonfinite", ('drop', 'drop')),
    _m("m_resume_nonfinite_after_estimate_budget", [[1, 2.0 ** -100], [2.0 ** -100, -2.0 ** -100]], [-2.0 ** 61, -2.0 ** 31], 2, N, 2, 1, "resume:nonfinite", ('estimate', 'budget'), low=[[2, 2.0 ** -99], [2.0 ** -99, -2.0 ** -99]], x0=[-1.5, 1], rtol=2.0 ** -9, every=2),
    _m("m_direction_beta_nonfinite_after_every_estimate", [[1.25 * 2.0 ** -60, -2.0 ** -59], [-2.0 ** -59, 1.25 * 2.0 ** 60]], [-1.5 * 2.0 ** -30, 2.0 ** -59], 4, N, 4, 2, "direction:beta_nonfinite", ('every', 'estimate'), rtol=2.0 ** -3, every=2),
    _m("m_update_dot_nonfinite_after_exact", [[2.0 ** -29, -2.0 ** 61], [-2.0 ** 61, 1]], [0, 2], 4, N, 2, 1, "update:dot_nonfinite", ('exact',), x0=[1, -1], rtol=2.0 ** -2, drop=0.5),
    _m("m_direction_nonfinite_after_every_every_drop", [[1.25 * 2.0 ** 30, -2.0 ** -100], [-2.0 ** -100, 2.0 ** -60]], [-2, 2.0 ** 60], 4, N, 4, 3, "direction:nonfinite", ('every', 'every', 'drop'), low=[[1.25 * 2.0 ** 31, -2.0 ** -99], [-2.0 ** -99, 2.0 ** -59]], x0=[1.25, -2], rtol=2.0 ** -4, every=1),
    _m("m_start_nonfinite", [[2.0 ** 301, 0], [0, 2.0 ** 900]], [-2, -2], 4, N, 0, 0, "start:nonfinite", (), low=[[-1, 0], [0, 1.25]], x0=[1, 2]),
    _m("m_segment_nonfinite", [[0, -2.0 ** 300], [-2.0 ** 300, 2.0 ** -899]], [1, -1], 6, N, 0, 0, "segment:nonfinite", (), low=[[0, -1], [-1, 1.25]], x0=[-1.5, -1], every=3, drop=0.25),
    _m("m_segment_zero_after_every", [[2, 1.25 * 2.0 ** -300], [1.25 * 2.0 ** -300, 2.0 ** -599]], [-2, 0], 6, S, 1, 1, "segment:zero", ('every',), low=[[2, -1.5], [-1.5, 1]], x0=[-2, 0], every=1, drop=0.25),
    _m("m_resume_converged_after_budget", [[1, 1.25 * 2.0 ** -300], [1.25 * 2.0 ** -300, 1.25 * 2.0 ** -300]], [-2, 0], 1, C, 1, 1, "resume:converged", ('budget',), low=[[1, -1], [-1, 1.25]], x0=[1.25, -1.5], rtol=2.0 ** -5, every=2, drop=0.5),
    _m("m_update_pq_breakdown_after_exact_estimate", [[2, 2.0 ** -600], [2.0 ** -600, 1.25 * 2.0 ** -600]], [-1, 2], 6, B, 2, 2, "update:pq_breakdown", ('exact', 'estimate'), low=[[-1, -2], [-2, 2]], rtol=2.0 ** -1, every=3, drop=0.5),
    _m("m_segment_zero", [[-1.5, 2.0 ** -299], [2.0 ** -299, 0]], [-1.5, 0], 5, S, 0, 0, "segment:zero", (), low=[[-1, -1.5], [-1.5, 0]], x0=[1, 2]),
]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def options(case, **kw):
    """the keyword arguments of the model, and of Handle.cg_mixed, for the case's own run; kw replaces"""
    out = dict(rtol=case.rtol, atol=case.atol, max_iterations=case.budget, update_every=case.every, update_drop=case.drop)
    out.update(kw)
    return out


def system(case, reps):
    """-> (fp64 CSR of `reps` copies of `high` along the diagonal, float CSR of `low` on the same pattern, b, dinv (float) or None, x0 or None)"""
    high, low = np.array(case.high), np.array(case.low)
    i, j = np.nonzero(high)
    assert np.array_equal(np.nonzero(low), (i, j)), "high and low differ in pattern"
    base = 2 * np.arange(reps)[:, None]
    rows, cols = (base + i).ravel(), (base + j).ravel()
    hi = cgc._from_coo(2 * reps, rows, cols, np.tile(high[i, j], reps), np.float64)
    lo = cgc._from_coo(2 * reps, rows, cols, np.tile(low[i, j], reps), np.float32)
    assert np.array_equal(lo.val.astype(np.float64), np.tile(low[i, j], reps)), "an entry of low is not representable"
    assert np.array_equal(hi.rowptr, lo.rowptr) and np.array_equal(hi.colidx, lo.colidx)
    tiled = lambda v, t: None if v is None else np.tile(np.asarray(v, dtype=np.float64).astype(t), reps)
    return hi, lo, tiled(case.b, np.float64), tiled(case.dinv, np.float32), tiled(case.x0, np.float64)


def run(case, reps, multiply=None, watch=None, **kw):
    """the model on `reps` copies of the case (cg_cases.matvec on both sides unless a multiply is given) -> its result dict"""
    hi, lo, b, dinv, x0 = system(case, reps)
    mul = multiply or cgc.matvec
    return mix.cg_mixed(mul(hi), mul(lo), b, x0=x0, dinv=dinv, watch=watch, **options(case, **kw))


def true_rr(case, reps, x):
    """<b - high x, b - high x> on `reps` copies of the case, in the contract's order: the rr an update that tries x finds"""
    hi, _, b, _, _ = system(case, reps)
    with np.errstate(all="ignore"):
        r = b - cgc.matvec(hi)(x)
        return cgc.dot(r, r)


def traced(model):
    """model(watch) -> result dict.  -> (result, [(k, reason, rr before, rr tried, committed)] per segment end: the iteration behind which the
    update was tried, why the segment ended, the committed rr in front of it, the true rr of x + y, and whether that was committed).  Read
    through the model's watch hook, by the calls it names: what="iteration" behind cg_update, what="update" behind an update's residual."""
    tried, k, rs = [], [0], [None]

    def watch(*v, what=None):
        if what == "iteration":
            k[0] += 1
            rs.append(float(v[-1]))
        elif what == "update":
            tried.append((k[0], float(v[-1])))
    r = model(watch)
    r["rs"] = rs                                              # rs[k]: the recurrence's <r,r> after iteration k, also where the history holds a committed rr
    assert len(tried) == len(r["segments"]) and r["updates"] in (len(tried), len(tried) - 1)
    out, rr = [], float(r["history"][0])
    for n, ((at, rrn), reason) in enumerate(zip(tried, r["segments"])):
        committed = n < r["updates"]
        out.append((at, reason, rr, rrn, committed))
        if committed:
            rr = rrn
    return r, out


def rises(trace):
    """the reasons of the COMMITTED updates of a trace whose true residual did not fall"""
    return [reason for _, reason, before, after, committed in trace if committed and after >= before]


# ----------------------------------------------------------------------------- atol
def atol_probes(model):
    """model(atol, watch=None) -> result dict (rtol = 0).  -> [(a, k, where)]: atol = a decides at iteration k because a * a equals the value
    compared there and the test is <=, while the next double below a does not decide there.  where: "estimate" (the segment ends by the
    estimate test: a * a == rs) or "resume:converged" (a * a == the committed rr).  Candidates: the exact square roots of the free run's rs
    and committed rr; every one returned has been confirmed with the model."""
    free, trace = traced(lambda watch: model(0.0, watch))
    sums = {v for v in free["rs"][1:]} | {t[3] for t in trace if t[4]}
    out = []
    for h in sorted(sums, reverse=True):
        a = float(np.sqrt(h))
        if not (h > 0 and np.isfinite(h) and a * a == h):
            continue
        under = float(np.nextafter(a, 0.0))
        (at, t_at), (below, t_below) = traced(lambda watch: model(a, watch)), traced(lambda watch: model(under, watch))
        for k, reason, _, _, _ in t_at:
            if reason == "estimate" and at["rs"][k] == h and (k, "estimate") not in {(t[0], t[1]) for t in t_below}:
                out.append((a, k, "estimate"))
        same = (at["status"], at["iterations"], at["updates"], at["end"]) == (below["status"], below["iterations"], below["updates"], below["end"])
        if at["end"] == "resume:converged" and at["rr"] == h and not same:
            out.append((a, at["iterations"], "resume:converged"))
    return out


# ----------------------------------------------------------------------------- what the model can return
# every `end` of the model but "start:empty" (m = 0); tests/test_cg_mixed_ends_host.py compares the list with the model's text
ENDS = ("start:nonfinite", "start:bb_zero", "start:converged", "start:budget", "segment:nonfinite", "segment:zero", "segment:rz_breakdown",
        "update:dot_nonfinite", "update:pq_breakdown", "update:alpha_nonfinite", "direction:nonfinite", "direction:rz_breakdown",
        "direction:beta_nonfinite", "resume:nonfinite", "resume:stagnated", "resume:converged", "resume:budget")
ALLOWED_GAPS = ()
SEGMENT_ENDS = ("exact", "estimate", "drop", "every", "budget")
# the (end, reason of the segment in front of it) places the catalogue must reach
REQUIRED_PLACES = ({("resume:stagnated", r) for r in ("exact", "estimate", "drop")} | {("resume:converged", r) for r in SEGMENT_ENDS} |
                   {("resume:budget", r) for r in SEGMENT_ENDS} | {("rise", "every"), ("rise", "budget")} |
                   # a non-start end in a second or later segment, found by cg_update and by mix_direction: p kept behind "drop" and behind
                   # "every", p started afresh behind "exact"
                   {(kind, r) for kind in ("update", "direction") for r in ("drop", "every", "exact")})


def places_reached(traces):
    """-> the members of REQUIRED_PLACES that the catalogue meets: by its declarations, and ("rise", reason) by `traces` ({name: the trace of the
    case's run, from `traced`})"""
    got = set()
    for c in CASES:
        kind = c.end.split(":")[0]
        if kind == "resume" or (kind in ("update", "direction") and c.segments):
            got.add((c.end if kind == "resume" else kind, c.segments[-1]))
        for reason in rises(traces[c.name]):
            got.add(("rise", reason))
    return got & REQUIRED_PLACES


# ----------------------------------------------------------------------------- several cases in one pair of matrices
STATE_CASES = ("m_resume_converged_after_exact", "m_resume_stagnated_after_drop", "m_resume_budget_after_every", "m_update_pq_breakdown_after_every",
               "m_direction_rz_breakdown", "m_segment_rz_breakdown", "m_segment_zero", "m_start_converged", "m_start_bb_zero",
               "m_rise_resume_budget_after_every", "m_direction_nonfinite_after_every")


def mixed(cases, reps, tail):
    """solve_end_cases.mixed for a pair: `high` holds every case's fp64 block `reps` times -- block j of a group of len(cases) is case j's --
    and behind them `tail` rows of cg_cases.tri; `low` holds the cases' float blocks and the tail's float copy on the same pattern.
    -> (high CSR, low CSR, select): select(j) -> (b, dinv, x0) of case j on its own blocks and zero (Dinv one) everywhere else, where the
    recurrence then never leaves zero; select(None, seed) -> a right-hand side in (-1, 1) on the tail and zero on the blocks."""
    n = len(cases)
    parts = [system(c, 1) for c in cases]
    rows, cols, hv, lv = [], [], [], []
    for j, (hi, lo, _, _, _) in enumerate(parts):
        r = np.repeat(np.arange(2), np.diff(hi.rowptr))
        base = 2 * (j + n * np.arange(reps))[:, None]
        rows.append((base + r).ravel()), cols.append((base + hi.colidx).ravel())
        hv.append(np.tile(hi.val, reps)), lv.append(np.tile(lo.val.astype(np.float64), reps))
    head = 2 * n * reps
    band = cgc.tri(tail, np.float64)
    rows.append(head + np.repeat(np.arange(tail), np.diff(band.rowptr))), cols.append(head + band.colidx), hv.append(band.val), lv.append(band.val)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    high = cgc._from_coo(head + tail, rows, cols, np.concatenate(hv), np.float64)
    low = cgc._from_coo(head + tail, rows, cols, np.concatenate(lv), np.float32)
    assert high.val.size == low.val.size == rows.size and np.array_equal(high.colidx, low.colidx)

    def select(j, seed=0):
        b, dinv, x0 = np.zeros(head + tail), np.ones(head + tail, dtype=np.float32), np.zeros(head + tail)
        if j is None:
            b[head:] = np.random.default_rng(seed).uniform(-1, 1, tail)
            return b, None, None
        _, _, cb, cd, cx = parts[j]
        own = (2 * (j + n * np.arange(reps))[:, None] + np.arange(2)).ravel()
        b[own] = np.tile(cb, reps)
        if cd is not None:
            dinv[own] = np.tile(cd, reps)
        if cx is not None:
            x0[own] = np.tile(cx, reps)
        return b, None if cd is None else dinv, None if cx is None else x0
    return high, low, select


def state_system(m=1026):
    """-> (cases, high CSR of m rows, low CSR, select): `mixed` over STATE_CASES, about half of the rows in blocks and half in the tail; the
    last case turns non-finite inside the loop"""
    cases = [by_name(n) for n in STATE_CASES]
    reps = m // (4 * len(cases))
    return (cases,) + mixed(cases, reps, m - 2 * len(cases) * reps)
