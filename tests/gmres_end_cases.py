"""A catalogue of the ways spmv_hip_gmres can end (tests/test_gmres_ends_host.py, tests/test_gpu_gmres_ends.py), in the style of
tests/solve_end_cases.py.

A case is a small square block, a right-hand side of the block's size and, where it needs them, a Dinv, a guess and an atol: `system` repeats
them `reps` times along the diagonal, so every row, every workgroup and every size runs the same small recurrence and the loop ends where the
block's own ends.  A line says the restart R it runs with, the status, the iteration count and the `end` in the words of the model
(gmres_cases.gmres: result["end"]), and the cycle and the step j of that cycle at which the loop ends: a "rotate:converged" ends BEHIND the step
it applied, every other rotate end while making step j (iterations counts the steps applied before it), a restart end behind step R of its cycle.
tests/test_gmres_ends_host.py proves every line with the model alone; tests/test_gpu_gmres_ends.py then asks the device for the same bits.

Entries are a mantissa of {0, +-1, 1.25, -1.5, +-2} times a power of two (2^0, 2^+-30, 2^+-60, 2^+-100 in fp32; 2^0, 2^+-300, 2^+-600, 2^+-900 in
fp64), so that a dot or a product overflows without any operand being a subnormal number: denormal handling is not part of the contract.  The
lines below "found by search" come from a random search over 2 x 2 and 3 x 3 blocks of that set with R in {2, 3} (the fp32 rotate:nonfinite lines:
with a Dinv, and sometimes a guess, of the same set); a line was kept only where it
ends the same way at every size of `sizes`, under cg_cases.matvec and under solve_end_cases.matvec_wide, without a subnormal.  (Not among
them: [[-2, -1.5, 0], [-2, -2, 1], [-1, -2, 2]] with b = [2, 2, -1], R = 3 in fp32, whose restart:zero behind cycle 2 passed both and still
became a rotate:converged under a device multiply at 1026 rows: a true residual of exactly zero behind inexact steps moves with the rounding.)"""
from collections import namedtuple

import numpy as np

import cg_cases as cgc
import gmres_cases as gc

F32, F64 = np.float32, np.float64
BOTH = (F64, F32)
C, M, B, N = gc.CONVERGED, gc.MAX_ITERATIONS, gc.BREAKDOWN, gc.NONFINITE
G = gc.GROUP

# block: s rows of s; b, dinv, x0: s elements (None: none); zeros: the diagonal's zeros are entries too (a row of the chain would be empty);
# restart: R; atol: of the run (rtol is 0); budget: max_iterations of the run; status, iterations, end: what that run reports; cycle, step: where
Case = namedtuple("Case", "name block b dinv x0 dtypes restart atol budget zeros status iterations end cycle step")

BUDGET = 12                             # more than the iterations + 1 of every case that does not say otherwise


def _c(name, block, b, restart, status, iterations, end, cycle, step, dinv=None, x0=None, dtypes=BOTH, atol=0.0, budget=None, zeros=False):
    row = lambda v: None if v is None else tuple(float(e) for e in v)
    assert all(len(r) == len(block) for r in block) and len(b) == len(block)
    return Case(name, tuple(row(r) for r in block), row(b), row(dinv), row(x0), tuple(dtypes), restart, float(atol),
                max(BUDGET, iterations + 2) if budget is None else budget, zeros, status, iterations, end, cycle, step)


def chain(s):
    """A e_i = e_(i+1) for i < s - 1 and A e_(s-1) = 0: with b = e_0 the Krylov vectors are e_0 .. e_(s-1) up to scale, and step s finds w = 0
    and d = 0 exactly, whatever the scale's rounding"""
    a = np.zeros((s, s))
    a[np.arange(1, s), np.arange(s - 1)] = 1.0
    return a.tolist()


def cyclic(s):
    """the chain closed: A e_(s-1) = e_0.  With b = e_0 the estimate stays <b,b> for s - 1 steps and step s solves the system: the estimate is 0
    where 1 / sqrt(reps) is exact (reps a power of 4) and a rounding error of it elsewhere, which the lines' atol = 2^-20 lets pass"""
    a = np.array(chain(s))
    a[0, s - 1] = 1.0
    return a.tolist()


def e0(s):
    return [1.0] + [0.0] * (s - 1)


TINY = 2.0 ** -20


def tri(s):
    """s rows of gmres_cases.tri_ns as a block: a run that goes on past the budgets of the lines that use it"""
    return (2 * np.eye(s) - 1.5 * np.eye(s, k=1) - 0.5 * np.eye(s, k=-1)).tolist()


def ramp(s):
    return [1.0 + (i % 3) - (i % 2) for i in range(s)]


CASES = [
    # ---- the ends of iteration 0: a guess that solves the system, B = 0 (X is zeroed whatever the guess), a guess whose product overflows
    _c("g_begin_conv", [[-1, -2], [0, 1]], [2, 0], 3, C, 0, "begin:converged", 0, 0, x0=[-2, 0]),
    _c("g_begin_zero", [[-1, -2], [0, 1]], [0, 0], 3, C, 0, "begin:bb_zero", 0, 0, x0=[1, 2]),
    _c("g_begin_zero_nox0", [[-1, -2], [0, 1]], [0, 0], 3, C, 0, "begin:bb_zero", 0, 0),
    _c("g_begin_inf_32", [[2.0 ** 100, 0], [0, 1]], [1, 1], 3, N, 0, "begin:nonfinite", 0, 0, x0=[2.0 ** 100, 0], dtypes=(F32,)),
    _c("g_begin_inf_64", [[2.0 ** 900, 0], [0, 1]], [1, 1], 3, N, 0, "begin:nonfinite", 0, 0, x0=[2.0 ** 900, 0], dtypes=(F64,)),
    # ---- rotate:d_zero at steps 1, 2, G, G + 1 and R of the first cycle: the chain of s rows ends while making step s
    _c("g_chain_1", [[0]], [1], 3, B, 0, "rotate:d_zero", 1, 1, zeros=True),
    _c("g_chain_2", chain(2), e0(2), 3, B, 1, "rotate:d_zero", 1, 2, zeros=True),
    _c("g_chain_G", chain(G), e0(G), G + 4, B, G - 1, "rotate:d_zero", 1, G, zeros=True),
    _c("g_chain_G1", chain(G + 1), e0(G + 1), G + 4, B, G, "rotate:d_zero", 1, G + 1, zeros=True),
    _c("g_chain_R3", chain(3), e0(3), 3, B, 2, "rotate:d_zero", 1, 3, zeros=True),
    _c("g_chain_R10", chain(10), e0(10), 10, B, 9, "rotate:d_zero", 1, 10, zeros=True),
    _c("g_chain_R32", chain(32), e0(32), 32, B, 31, "rotate:d_zero", 1, 32, zeros=True),
    # ---- rotate:converged at steps 1, 2, G, G + 1 and R of the first cycle: the cyclic block of s rows is solved by step s
    _c("g_cyclic_1", [[1]], [1], 3, C, 1, "rotate:converged", 1, 1, atol=TINY),
    _c("g_cyclic_2", cyclic(2), e0(2), 3, C, 2, "rotate:converged", 1, 2, atol=TINY),
    _c("g_cyclic_G", cyclic(G), e0(G), G + 4, C, G, "rotate:converged", 1, G, atol=TINY),
    _c("g_cyclic_G1", cyclic(G + 1), e0(G + 1), G + 4, C, G + 1, "rotate:converged", 1, G + 1, atol=TINY),
    _c("g_cyclic_R3", cyclic(3), e0(3), 3, C, 3, "rotate:converged", 1, 3, atol=TINY),
    _c("g_cyclic_R10", cyclic(10), e0(10), 10, C, 10, "rotate:converged", 1, 10, atol=TINY),
    _c("g_cyclic_R32", cyclic(32), e0(32), 32, C, 32, "rotate:converged", 1, 32, atol=TINY),
    # ---- MAX_ITERATIONS with a budget that is 0, 1 and R - 1 (mod R): on a restart, one step behind it, one step before the next
    _c("g_budget_0_mod_R", tri(8), ramp(8), 3, M, 6, "budget", 2, 3, budget=6),
    _c("g_budget_1_mod_R", tri(8), ramp(8), 3, M, 7, "budget", 3, 1, budget=7),
    _c("g_budget_R1_mod_R", tri(8), ramp(8), 3, M, 5, "budget", 2, 2, budget=5),
    _c("g_budget_G1_mod_R", tri(32), ramp(32), G + 2, M, 2 * G + 5, "budget", 3, 1, budget=2 * G + 5, dinv=[0.5, 1, 2, 1] * 8, x0=[1, 1, -1, 0] * 8),
    # ---- found by search: the restart's own ends, and rotate ends in a later cycle (x is the restart's) or in the middle of one
    _c("g_restart_nonfinite_32_c1s2", [[2.0 ** -100, -2.0 ** -60, 2.0 ** -60], [-2.0 ** 61, 2.0 ** 61, -2.0 ** -99], [1.25 * 2.0 ** -30, 0, -2.0 ** -60]], [-2.0 ** -100, -2.0 ** -59, -1.5 * 2.0 ** 100], 2, N, 2, "restart:nonfinite", 1, 2, dtypes=(F32,)),
    _c("g_restart_nonfinite_32_c1s3", [[2.0 ** -29, 1.25, 2.0 ** 31], [-2.0 ** -99, 1.25 * 2.0 ** -100, -2], [0, 0, 1.25]], [2.0 ** -60, 1.25 * 2.0 ** 100, -2.0 ** 60], 3, N, 3, "restart:nonfinite", 1, 3, dtypes=(F32,)),
    _c("g_restart_nonfinite_64_c1s2", [[-2.0 ** 901, 2.0 ** -300, -1.5], [-2.0 ** -299, -1.5 * 2.0 ** -600, 0], [0, 1.25 * 2.0 ** 600, -1.5 * 2.0 ** -900]], [1.25 * 2.0 ** -600, -2.0 ** -900, -2.0 ** 300], 2, N, 2, "restart:nonfinite", 1, 2, dtypes=(F64,)),
    _c("g_restart_zero_32_c1s2", [[2, 1], [0, -1]], [1.25, -1], 2, C, 2, "restart:zero", 1, 2, dtypes=(F32,)),
    _c("g_restart_zero_32_c1s3", [[0, 1.25], [-1, -2]], [1.25, -2], 3, C, 3, "restart:zero", 1, 3, dtypes=(F32,)),
    _c("g_restart_zero_32_c5s2", [[-1, -1, -2], [0, -1, 0], [0, 1.25, 2]], [-2, -1, -2], 2, C, 10, "restart:zero", 5, 2, dtypes=(F32,)),
    _c("g_restart_zero_64_c1s2", [[-1, 1.25], [0, 2]], [2, 1.25], 2, C, 2, "restart:zero", 1, 2, dtypes=(F64,)),
    _c("g_restart_zero_64_c1s3", [[-1, 2], [0, -1.5]], [2, -1], 3, C, 3, "restart:zero", 1, 3, dtypes=(F64,)),
    _c("g_restart_zero_64_c2s2", [[-2, 0], [-2, 1]], [1.25, 2], 2, C, 4, "restart:zero", 2, 2, dtypes=(F64,)),
    _c("g_restart_zero_64_c2s3", [[-2, 0], [1.25, -1]], [-2, 1], 3, C, 6, "restart:zero", 2, 3, dtypes=(F64,)),
    _c("g_rotate_converged_32_c2s1", [[-1, 0], [0, 1.25]], [1.25, 2], 3, C, 4, "rotate:converged", 2, 1, dtypes=(F32,)),
    _c("g_rotate_converged_32_c2s2", [[0, -2], [1.25, 0]], [-2, 1.25], 2, C, 4, "rotate:converged", 2, 2, dtypes=(F32,)),
    _c("g_rotate_d_zero_32_c2s1", [[-1, 0, 0], [-1.5, 0, -2], [1, 0, -1]], [-1, -1, 1.25], 3, B, 3, "rotate:d_zero", 2, 1, dtypes=(F32,)),
    _c("g_rotate_d_zero_64_c2s1", [[-2.0 ** -599, 1.25 * 2.0 ** 900, -1.5 * 2.0 ** -600], [-2.0 ** 301, 0, -1.5 * 2.0 ** -600], [0, -1.5 * 2.0 ** -900, -2.0 ** -900]], [0, -1.5 * 2.0 ** -300, -2.0 ** 300], 2, B, 2, "rotate:d_zero", 2, 1, dtypes=(F64,)),
    # fp32 rotate:nonfinite: every line the search kept carries a Dinv (A (Dinv v) overflows where A v does not): at step 2 and 3 of the first
    # cycle, at step 1 of the second and at step 2 of it
    _c("g_rotate_nonfinite_32_c1s2", [[2.0 ** -30, 1.25 * 2.0 ** -30], [2.0 ** 100, 2.0 ** 30]], [-2.0 ** -99, -1.5 * 2.0 ** 60], 2, N, 1, "rotate:nonfinite", 1, 2, dinv=[1.25 * 2.0 ** 60, 2.0 ** 31], dtypes=(F32,)),
    _c("g_rotate_nonfinite_32_c1s2_b", [[2.0 ** 101, 2.0 ** 31], [-2, 1.25 * 2.0 ** -30]], [-1.5 * 2.0 ** -60, 1.25], 3, N, 1, "rotate:nonfinite", 1, 2, dinv=[2.0 ** 60, 1.25 * 2.0 ** 30], dtypes=(F32,)),
    _c("g_rotate_nonfinite_32_c1s3", [[2.0 ** 100, -2.0 ** 30, 2.0 ** 30], [2.0 ** 100, 2, -1.5 * 2.0 ** 100], [-2.0 ** 61, -2.0 ** -29, 2.0 ** -30]], [2.0 ** 100, -2.0 ** -99, 0], 3, N, 2, "rotate:nonfinite", 1, 3, dinv=[2, 2.0 ** 30, 2.0 ** 60], dtypes=(F32,)),
    _c("g_rotate_nonfinite_32_c1s3_b", [[1.25 * 2.0 ** -30, 2.0 ** 100, 1], [2.0 ** 100, -1.5, -1], [2.0 ** 61, 2.0 ** -30, -2.0 ** -100]], [-2.0 ** -60, -1.5 * 2.0 ** -60, 2.0 ** 30], 3, N, 2, "rotate:nonfinite", 1, 3, dinv=[-2.0 ** -30, 2.0 ** 100, 1.25 * 2.0 ** 30], dtypes=(F32,)),
    _c("g_rotate_nonfinite_32_c2s1", [[-2.0 ** -99, -2.0 ** -29, 2.0 ** 31], [-1.5, 1.25 * 2.0 ** 100, 2.0 ** -99], [1.25 * 2.0 ** 100, 1.25 * 2.0 ** 30, 0]], [2.0 ** 101, 2.0 ** -59, 2.0 ** 101], 2, N, 2, "rotate:nonfinite", 2, 1, dinv=[1.25 * 2.0 ** -30, -2.0 ** 60, 1.25 * 2.0 ** 60], dtypes=(F32,)),
    _c("g_rotate_nonfinite_32_c2s1_b", [[2.0 ** 101, 2.0 ** -99, -2], [2.0 ** 100, -1.5, 2.0 ** 101], [0, 1.25, 2.0 ** 31]], [-2.0 ** 61, 0, 0], 2, N, 2, "rotate:nonfinite", 2, 1, dinv=[-2.0 ** -100, -1.5 * 2.0 ** 100, -2.0 ** 100], dtypes=(F32,)),
    _c("g_rotate_nonfinite_32_c2s2", [[1, -2.0 ** 60, 1.25 * 2.0 ** -60], [2.0 ** 31, 2.0 ** 31, -2.0 ** -99], [2.0 ** 100, 2.0 ** 60, 0]], [0, 0, 1], 2, N, 3, "rotate:nonfinite", 2, 2, dinv=[1, 1.25 * 2.0 ** 100, -1.5], dtypes=(F32,)),
    _c("g_rotate_nonfinite_32_c2s2_b", [[-2.0 ** 61, 0, -1.5 * 2.0 ** 30], [-1.5, -1.5 * 2.0 ** 100, 1.25], [2.0 ** 31, 2.0 ** -29, -2.0 ** -29]], [-2.0 ** -59, 0, 0], 2, N, 3, "rotate:nonfinite", 2, 2, dinv=[2.0 ** -29, 1.25 * 2.0 ** 30, -1.5 * 2.0 ** 60], dtypes=(F32,)),
    _c("g_rotate_nonfinite_64_c1s1", [[2.0 ** 600, 0, 0], [2.0 ** 900, 2.0 ** -600, 1.25 * 2.0 ** -300], [1.25 * 2.0 ** -900, -2.0 ** 301, -2.0 ** 301]], [2.0 ** -299, -1.5 * 2.0 ** -600, 2.0 ** -299], 3, N, 0, "rotate:nonfinite", 1, 1, dtypes=(F64,)),
    _c("g_rotate_nonfinite_64_c1s2", [[1.25 * 2.0 ** 900, 2.0 ** -900, -2.0 ** 601], [-2.0 ** 600, 1, -2.0 ** -300], [2.0 ** 301, 2.0 ** 301, 0]], [-2.0 ** -299, -1.5 * 2.0 ** 300, 0], 2, N, 1, "rotate:nonfinite", 1, 2, dtypes=(F64,)),
    _c("g_rotate_nonfinite_64_c1s3", [[1.25 * 2.0 ** 900, 0, -2.0 ** -600], [2.0 ** -600, -1.5 * 2.0 ** -900, 0], [-1.5 * 2.0 ** -900, 2, 2.0 ** 301]], [1.25 * 2.0 ** -900, 1.25 * 2.0 ** 300, 1.25 * 2.0 ** 300], 3, N, 2, "rotate:nonfinite", 1, 3, dtypes=(F64,)),
    _c("g_rotate_nonfinite_64_c2s1", [[1, -1.5 * 2.0 ** 900, 0], [1.25 * 2.0 ** 300, -1, 0], [2.0 ** 300, 2, 2.0 ** 301]], [0, -2.0 ** -599, -1], 2, N, 2, "rotate:nonfinite", 2, 1, dtypes=(F64,)),
    _c("g_rotate_nonfinite_64_c2s2", [[0, -2.0 ** 301, 1.25], [-1.5 * 2.0 ** -600, 2.0 ** 600, 2.0 ** 601], [0, -1.5, -2.0 ** 900]], [1, -2.0 ** -899, 0], 2, N, 3, "rotate:nonfinite", 2, 2, dtypes=(F64,)),
]


MANTISSAS = (0.0, 1.0, -1.0, 1.25, -1.5, 2.0, -2.0)
EXPONENTS = {F32: (0, 30, -30, 60, -60, 100, -100), F64: (0, 300, -300, 600, -600, 900, -900)}


def random_systems(seed, n):
    """n random cases of the searches' kind: -> [(Case, dtype)], blocks of 2 to 4 rows without an empty row, every entry of the entry set"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        dtype = BOTH[rng.integers(2)]
        entry = lambda: float(MANTISSAS[rng.integers(7)] * 2.0 ** EXPONENTS[dtype][rng.integers(7)])
        s, R = int(rng.integers(2, 5)), int(rng.integers(2, 4))
        block = [[entry() for _ in range(s)] for _ in range(s)]
        if any(not any(row) for row in block):
            continue
        dinv = None if rng.integers(3) == 0 else [entry() or 1.0 for _ in range(s)]
        x0 = None if rng.integers(3) else [entry() for _ in range(s)]
        out.append((_c(f"random_{seed}_{len(out)}", block, [entry() for _ in range(s)], R, M, 0, "budget", 0, 0, dinv=dinv, x0=x0, dtypes=(dtype,)), dtype))
    return out


def by_name(name):
    return next(c for c in CASES if c.name == name)


def sizes(case):
    """the sizes of the GPU test for a block of s rows: one block, the most blocks in 1024 rows (one full workgroup of the dot), the fewest
    blocks that put rows into a second workgroup, about 4100 rows (five workgroups)"""
    s = len(case.block)
    return (s, 1024 // s * s, (1024 // s + 1) * s, 4100 // s * s)


# the case that also runs at two steps per workgroup (P = 1024): every Krylov vector is a unit vector times a scale, every dot of two of them an
# exact zero, so the run ends at step 2 whatever 1 / sqrt(reps) rounds to
BIG_CASE = "g_cyclic_2"
BIG = 2 ** 20 + 2


def system(case, reps, dtype):
    """-> (CSR of `reps` copies of the block along the diagonal, b, dinv or None, x0 or None) in `dtype`"""
    block = np.array(case.block, dtype=np.float64)
    s = block.shape[0]
    keep = block != 0
    if case.zeros:
        keep |= np.eye(s, dtype=bool)
    i, j = np.nonzero(keep)
    base = s * np.arange(reps)[:, None]
    csr = cgc._from_coo(s * reps, (base + i).ravel(), (base + j).ravel(), np.tile(block[i, j], reps), dtype)
    assert csr.val.size == i.size * reps and np.array_equal(csr.val.astype(np.float64), np.tile(block[i, j], reps)), "an entry is not representable"
    tiled = lambda v: None if v is None else np.tile(np.asarray(v, dtype=np.float64).astype(dtype), reps)
    return csr, tiled(case.b), tiled(case.dinv), tiled(case.x0)


def run(case, reps, dtype, multiply=None, watch=None, **kw):
    """the model on `reps` copies of the case (cg_cases.matvec unless a multiply is given) -> its result dict"""
    csr, b, dinv, x0 = system(case, reps, dtype)
    kw.setdefault("max_iterations", case.budget)
    kw.setdefault("atol", case.atol)
    return gc.gmres(multiply(csr) if multiply else cgc.matvec(csr), b, case.restart, x0=x0, dinv=dinv, watch=watch, **kw)


def place(restart, iterations, end):
    """-> (cycle, step) at which a run of `iterations` applied steps ended in `end`, cycles and steps counted from 1 ((0, 0): before the loop)"""
    k, R = iterations, restart
    if end.startswith("begin:"):
        return 0, 0
    if end.startswith("restart:"):
        return k // R, R
    if end in ("rotate:converged", "budget"):
        return (k - 1) // R + 1, (k - 1) % R + 1
    return k // R + 1, k % R + 1                              # found while making step k + 1


def found_making_a_step(case):
    """is the end found while making step iterations + 1 (d = 0, a non-finite h or d)?  A budget of `iterations` then never sees it"""
    return case.end.startswith("rotate:") and case.end != "rotate:converged"


# ----------------------------------------------------------------------------- what the model can return
# every `end` of the model but "begin:empty" (m = 0) and "budget"; tests/test_gmres_ends_host.py compares the list with the model's text
ENDS = ("begin:nonfinite", "begin:bb_zero", "begin:converged", "rotate:nonfinite", "rotate:d_zero", "rotate:rotation_nonfinite", "rotate:converged",
        "rotate:exhausted", "restart:nonfinite", "restart:zero")
# rotate:exhausted cannot fire (hn = 0 behind d != 0 makes s = 0 and the estimate 0, which the test before it takes).
# rotate:rotation_nonfinite needs a squared estimate that rounds to infinity behind a finite <r,r>: within a cycle |g_(j+1)| = |s g_j| <= |g_j| up
# to roundings, so the estimate stays at the cycle's <r,r>, which begin or the restart found finite.  random_systems(seed, n) below draws what the
# searches drew -- a block of 2 to 4 rows, b, a Dinv, sometimes a guess, all of the entry set, R in {2, 3}, either type, one copy -- and
# tests/test_gmres_ends_host.py runs a seeded sample of it and asserts that none ends there
ALLOWED_GAPS = ("rotate:exhausted", "rotate:rotation_nonfinite")
# the (cycle, step) places the catalogue must reach, per end: step 1, 2, G, G + 1 and R of the first cycle; step 1 and the middle of a later one
REQUIRED_PLACES = {
    "rotate:d_zero": {(1, 1), (1, 2), (1, G), (1, G + 1), "first:R", "later"},
    "rotate:converged": {(1, 1), (1, 2), (1, G), (1, G + 1), "first:R", "later:1", "later:middle"},
    "rotate:nonfinite": {"first:2+", "later"},
    "restart:zero": {"any"}, "restart:nonfinite": {"any"},
    "budget": {"0 mod R", "1 mod R", "R-1 mod R"},
}


def places_reached(cases=None):
    """-> {end: the members of REQUIRED_PLACES[end] that some line's declared (cycle, step) meets}"""
    out = {end: set() for end in REQUIRED_PLACES}
    for c in CASES + HISTORY_CASES if cases is None else cases:
        if c.end not in out:
            continue
        R, got = c.restart, out[c.end]
        if c.end == "budget":
            got.update(name for name, r in (("0 mod R", 0), ("1 mod R", 1 % R), ("R-1 mod R", R - 1)) if c.budget % R == r and R > 2)
            continue
        got.add("any")
        if c.cycle == 1:
            got.add((1, c.step))
            if c.step == R:
                got.add("first:R")
            if c.step >= 2:
                got.add("first:2+")
        elif c.cycle > 1:
            got.add("later")
            if c.step == 1:
                got.add("later:1")
            if 1 < c.step < R:
                got.add("later:middle")
    return {end: got & REQUIRED_PLACES[end] for end, got in out.items()}


# ----------------------------------------------------------------------------- rotate:converged by an atol taken from the model's own history
# gmres_cases.tri_ns(m) with b = gmres_cases.rhs(m): restart R, and the iteration k at which the derived atol ends the run: step 1 of a later
# cycle, and the middle of one
HistoryCase = namedtuple("HistoryCase", "name restart iterations cycle step end", defaults=("rotate:converged",))
HISTORY_CASES = [
    HistoryCase("g_tri_later_step_1", 3, 4, 2, 1),
    HistoryCase("g_tri_later_middle", 3, 5, 2, 2),
    HistoryCase("g_tri_later_middle_G1", G + 3, 2 * G + 4, 2, G + 1),
]
HISTORY_SIZES = (64, 1024, 1026, 4100)


def atol_for(history, k):
    """the smallest double a with a * a >= history[k]"""
    h = float(history[k])
    a = float(np.sqrt(h))
    while a * a < h:
        a = float(np.nextafter(a, np.inf))
    while float(np.nextafter(a, 0.0)) ** 2 >= h:
        a = float(np.nextafter(a, 0.0))
    return a


def history_probe(model, k):
    """model(atol) -> result dict (rtol = 0, a budget above k).  -> (a, at, below): atol = a ends the run at iteration k in rotate:converged and
    the next double below a does not end it there; asserted on the model"""
    free = model(0.0)
    assert free["iterations"] > k and free["history"][k] > 0, (free["iterations"], free["end"])
    a = atol_for(free["history"], k)
    at, below = model(a), model(float(np.nextafter(a, 0.0)))
    assert (at["status"], at["iterations"], at["end"]) == (C, k, "rotate:converged"), (at["iterations"], at["end"])
    assert (below["iterations"], below["end"]) != (k, "rotate:converged") and below["iterations"] > k, (below["iterations"], below["end"])
    return a, at, below


# ----------------------------------------------------------------------------- several cases in one matrix
def mixed(cases, reps, dtype, tail):
    """solve_end_cases.mixed for blocks of any size: one matrix that holds every case's block `reps` times -- a group is the cases' blocks one
    behind the other -- and behind the groups `tail` rows of gmres_cases.tri_ns, so that ONE handle can be driven into each case's end, and
    through an ordinary solve, by the right-hand side alone.  -> (CSR, select): select(j) -> (b, dinv, x0) of case j on its own blocks and zero
    (Dinv one) everywhere else, where the recurrence then never leaves zero; select(None, seed) -> a right-hand side in (-1, 1) on the tail
    and zero on the blocks."""
    parts = [system(c, 1, dtype) for c in cases]
    offs = np.concatenate([[0], np.cumsum([p[0].m for p in parts])])
    group = int(offs[-1])
    rows, cols, vals = [], [], []
    for j, (csr, _, _, _) in enumerate(parts):
        r = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
        base = (offs[j] + group * np.arange(reps))[:, None]
        rows.append((base + r).ravel()), cols.append((base + csr.colidx).ravel()), vals.append(np.tile(csr.val.astype(np.float64), reps))
    head = group * reps
    band = gc.tri_ns(tail, np.float64)
    rows.append(head + np.repeat(np.arange(tail), np.diff(band.rowptr))), cols.append(head + band.colidx), vals.append(band.val)
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    assert np.unique(rows * (head + tail) + cols).size == rows.size                   # explicit zeros stay entries: nothing is merged
    order = np.lexsort((cols, rows))
    rp = np.zeros(head + tail + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=head + tail), out=rp[1:])
    whole = gc.synth.CSR(head + tail, head + tail, rp, cols[order].astype(np.int32), vals[order].astype(dtype))

    def select(j, seed=0):
        b, dinv, x0 = np.zeros(head + tail, dtype=dtype), np.ones(head + tail, dtype=dtype), np.zeros(head + tail, dtype=dtype)
        if j is None:
            b[head:] = np.random.default_rng(seed).uniform(-1, 1, tail)
            return b, None, None
        csr, cb, cd, cx = parts[j]
        own = ((offs[j] + group * np.arange(reps))[:, None] + np.arange(csr.m)).ravel()
        b[own] = np.tile(cb, reps)
        if cd is not None:
            dinv[own] = np.tile(cd, reps)
        if cx is not None:
            x0[own] = np.tile(cx, reps)
        return b, None if cd is None else dinv, None if cx is None else x0
    return whole, select


def state_cases(dtype):
    """the cases of the test of state between solves: one of each end the loop has, the ends of iteration 0, and, last, one that turns
    non-finite inside the loop"""
    wide = dtype == np.float64
    names = ("g_cyclic_2", "g_chain_2", "g_chain_R3", "g_restart_zero_64_c1s2" if wide else "g_restart_zero_32_c1s2", "g_begin_conv", "g_begin_zero",
             "g_rotate_nonfinite_64_c1s2" if wide else "g_restart_nonfinite_32_c1s2")
    return [by_name(n) for n in names]


def state_system(dtype, m=1026):
    """-> (cases, CSR of m rows, select): `mixed` over state_cases, about half of the rows in blocks and half in the tridiagonal tail"""
    cases = state_cases(dtype)
    group = sum(len(c.block) for c in cases)
    reps = m // (2 * group)
    return (cases,) + mixed(cases, reps, dtype, m - group * reps)
