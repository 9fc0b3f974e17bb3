"""A catalogue of the ways spmv_hip_cg and spmv_hip_bicgstab can end (tests/test_solve_ends_host.py, tests/test_gpu_solve_ends.py), and its CG
cases as the columns of one spmv_hip_cg_columns call (columns_system; tests/test_cg_column_ends_host.py, tests/test_gpu_cg_column_ends.py).

A case is a 2 x 2 block, a right-hand side of two elements and, optionally, a Dinv of two: `system` repeats them `reps` times along the
diagonal, so every row, every workgroup and every size runs the same small recurrence and the loop ends where the block's own ends.  The
catalogue says for each case the status, the iteration count and the `end` -- the kernel and the test that stops the loop, in the words of
the models (cg_cases.cg, bicgstab_cases.bicgstab: result["end"]).  tests/test_solve_ends_host.py proves every line of it with the models
alone; tests/test_gpu_solve_ends.py then asks the device for the same bits.

Entries of the scaled cases are a mantissa of {0, +-1, 1.25, -1.5} times a power of two, so that alpha, omega or beta overflow or underflow
without any operand being a subnormal number: denormal handling is not part of the contract.  One case leaves that set:
b_omega_nonfinite_32_1 has a mantissa of 1.75 and exponents of -125 and 127, next to the ends of fp32's range, which is where omega alone
overflows; it meets no subnormal either."""
from collections import namedtuple

import numpy as np

import bicgstab_cases as bc
import cg_cases as cgc

F32, F64 = np.float32, np.float64
BOTH = (F64, F32)
C, M, B, N = cgc.CONVERGED, cgc.MAX_ITERATIONS, cgc.BREAKDOWN, cgc.NONFINITE

# solver: "cg" or "bicgstab"; block: two rows; b, dinv: two elements (dinv None: no preconditioner); dtypes: where the line holds;
# x0: two elements of an initial guess, or None; status, iterations, end: what a run with rtol = atol = 0 and a budget above `iterations`
# reports; exact: every operation of the run is exact in fp32, so fp32 and fp64 agree value for value and a fused multiply changes nothing
Case = namedtuple("Case", "name solver block b dinv x0 dtypes status iterations end exact")

# the sizes of the GPU test: one workgroup, one full workgroup, two elements in a second workgroup, five workgroups
SIZES = (2, 1024, 1026, 4098)
BIG = 2 ** 20 + 2                       # P = 1024, two steps per workgroup
BUDGET = 8                              # more than any case's iterations + 1
ATOL_SIZES = (2, 1024, 1026)            # 1, 512 and 513 copies: where the atol tests look for residuals that are squares

# BiCGStab cases also run with this power-of-two Dinv: the block's columns are divided by it, so A diag(Dinv) is the block as written, every
# scalar of the recurrence keeps its bits and x is the same numbers scaled by Dinv
PRE = (2.0, 0.5)


def _c(name, solver, block, b, status, iterations, end, dinv=None, x0=None, dtypes=BOTH, exact=False):
    pair = lambda v: None if v is None else tuple(float(e) for e in v)
    return Case(name, solver, tuple(pair(row) for row in block), pair(b), pair(dinv), pair(x0), tuple(dtypes), status, iterations, end, exact)


CASES = [
    # ---- BiCGStab, integer blocks
    _c("b_rv0_1", "bicgstab", [[-1, -1], [1, 1]], [0, -1], B, 1, "half:rv_zero", exact=True),
    _c("b_rv0_2", "bicgstab", [[2, -2], [2, -2]], [1, 2], B, 2, "half:rv_zero"),
    _c("b_rho0_2", "bicgstab", [[-1, -2], [1, -2]], [-1, 1], B, 2, "half:rho_zero"),
    _c("b_half_1", "bicgstab", [[-1, -2], [0, 1]], [2, 0], C, 1, "update:ss_converged", exact=True),
    _c("b_half_2", "bicgstab", [[-2, -2], [2, 1]], [0, 1], C, 2, "update:ss_converged", exact=True),
    _c("b_tt0_1", "bicgstab", [[0, -2], [0, -1]], [0, 1], B, 1, "update:tt_zero", exact=True),
    _c("b_tt0_2", "bicgstab", [[-1, -1], [-2, -2]], [-1, -1], B, 2, "update:tt_zero"),
    _c("b_ts0_1", "bicgstab", [[2, -1], [0, -1]], [-2, 2], B, 1, "update:ts_zero", exact=True),
    _c("b_ts0_2", "bicgstab", [[-2, 1], [-1, 2]], [-1, -2], B, 2, "update:ts_zero"),
    _c("b_rr_2", "bicgstab", [[2, 0], [-1, 2]], [2, -1], C, 2, "direction:converged"),
    _c("b_rr_1", "bicgstab", [[-2, -2], [0, -2]], [0, -1], C, 1, "direction:converged", exact=True),
    _c("b_rv0_0", "bicgstab", [[-2, -2], [-2, -2]], [-1, 1], B, 0, "half:rv_zero", exact=True),
    _c("b_half_3", "bicgstab", [[-1, -2], [3, 0]], [2, 1], C, 3, "update:ss_converged"),
    _c("b_ts0_3", "bicgstab", [[-2, -1], [-2, 0]], [2, -1], B, 3, "update:ts_zero"),
    # exact runs with a residual on the way that is the square of a double at 1, 512 or 513 copies: what the atol tests need
    _c("b_sq_half", "bicgstab", [[-2, -2], [-1, -2]], [-2, 0], C, 2, "update:ss_converged", exact=True),
    _c("b_sq_half_512", "bicgstab", [[-2, -1], [-1, 0]], [1, 1], B, 1, "update:ts_zero", exact=True),
    _c("b_sq_rr", "bicgstab", [[-2, -2], [-2, 2]], [-2, -2], C, 2, "update:ss_converged", exact=True),
    _c("b_sq_rr_512", "bicgstab", [[-2, -2], [-2, -2]], [-2, 1], B, 1, "half:rv_zero", exact=True),
    # the ends of iteration 0: a guess that solves the system (rr = 0, bb != 0: X keeps the guess), B = 0 (X is zeroed whatever the guess), and
    # a guess whose product overflows
    _c("b_begin_conv", "bicgstab", [[-1, -2], [0, 1]], [2, 0], C, 0, "begin:converged", x0=[-2, 0], exact=True),
    _c("b_begin_zero", "bicgstab", [[-1, -2], [0, 1]], [0, 0], C, 0, "begin:bb_zero", x0=[1, 2], exact=True),
    _c("b_begin_inf_32", "bicgstab", [[2.0 ** 100, 0], [0, 1]], [1, 1], N, 0, "begin:nonfinite", x0=[2.0 ** 100, 0], dtypes=(F32,)),
    _c("b_begin_inf_64", "bicgstab", [[2.0 ** 900, 0], [0, 1]], [1, 1], N, 0, "begin:nonfinite", x0=[2.0 ** 900, 0], dtypes=(F64,)),
    # ---- CG, symmetric integer blocks
    _c("c_rz_0", "cg", [[2, -2], [-2, -1]], [-1, -2], B, 0, "begin:rz_breakdown", dinv=[2, -1], exact=True),
    _c("c_rz_1", "cg", [[0, 1], [1, 1]], [-2, 1], B, 1, "direction:rz_breakdown", dinv=[1, -0.5]),
    _c("c_pq_0", "cg", [[-2, -2], [-2, -2]], [-2, -2], B, 0, "update:pq_breakdown", exact=True),
    _c("c_pq_1", "cg", [[-1, 1], [1, 1]], [1, 2], B, 1, "update:pq_breakdown"),
    _c("c_pq_1x", "cg", [[-2, -2], [-2, -1]], [-2, 2], B, 1, "update:pq_breakdown", exact=True),
    # not [[3, 3], [3, 3]] with b = [2, 1] and Dinv = [0.5, 2]: in fp64 its third <p,q> is a rounding error whose sign follows the multiply (a
    # row accumulated in long double runs one iteration more)
    _c("c_pq_2", "cg", [[1, -1], [-1, 1]], [-2, 1], B, 2, "update:pq_breakdown", dinv=[2, 0.5]),
    _c("c_rz_1x", "cg", [[-2, -2], [-2, 1]], [-2, -2], B, 1, "direction:rz_breakdown", dinv=[2, -1], exact=True),
    _c("c_rr_1", "cg", [[-2, -2], [-2, 1]], [-1, 2], C, 1, "direction:converged", exact=True),
    _c("c_rr_2", "cg", [[1, -1], [-1, 2]], [-2, -2], C, 2, "direction:converged", exact=True),
    _c("c_rr_2d", "cg", [[1, -1], [-1, 2]], [-2, -2], C, 2, "direction:converged", dinv=[2, 0.5], exact=True),
    _c("c_sq_rr", "cg", [[-2, -1], [-1, 2]], [0, -2], B, 1, "update:pq_breakdown", exact=True),
    _c("c_sq_rr_513", "cg", [[-2, -1], [-1, 2]], [-1, 2], B, 1, "update:pq_breakdown", exact=True),
    _c("c_sq_rr_512", "cg", [[-2, 3], [3, 0]], [1, 1], B, 1, "update:pq_breakdown", exact=True),
    _c("c_begin_conv", "cg", [[1, -1], [-1, 2]], [-2, -2], C, 0, "begin:converged", x0=[-6, -4], exact=True),
    _c("c_begin_zero", "cg", [[1, -1], [-1, 2]], [0, 0], C, 0, "begin:bb_zero", x0=[1, 2], exact=True),
    _c("c_begin_inf_32", "cg", [[2.0 ** 100, 0], [0, 1]], [1, 1], N, 0, "begin:nonfinite", x0=[2.0 ** 100, 0], dtypes=(F32,)),
    _c("c_begin_inf_64", "cg", [[2.0 ** 900, 0], [0, 1]], [1, 1], N, 0, "begin:nonfinite", x0=[2.0 ** 900, 0], dtypes=(F64,)),
    # ---- overflow and underflow: a mantissa of {0, +-1, 1.25, -1.5} times 2^e, e in {0, +-30, +-60, +-100} (fp32) or {0, +-300, +-600, +-900}
    # (fp64); the name ends in the type and the iteration count
    _c("b_nonfinite_64_0", "bicgstab", [[2.0 ** -900, 1], [1.25 * 2.0 ** 300, 1.25 * 2.0 ** 300]], [1.25 * 2.0 ** -900, -1.5 * 2.0 ** 900], N, 0, "begin:nonfinite", dtypes=(F64,)),
    _c("b_beta_nonfinite_32_1", "bicgstab", [[-2.0 ** -100, -2.0 ** 30], [-2.0 ** -60, -1.5 * 2.0 ** -30]], [1, 0], N, 1, "direction:beta_nonfinite", dtypes=(F32,)),
    _c("b_beta_nonfinite_32_2", "bicgstab", [[0, -1.5 * 2.0 ** 30], [1.25 * 2.0 ** -100, 1.25 * 2.0 ** 100]], [1.25, 1.25], N, 2, "direction:beta_nonfinite", dtypes=(F32,)),
    _c("b_beta_nonfinite_64_1", "bicgstab", [[2.0 ** -300, -1.5 * 2.0 ** -300], [-2.0 ** 300, 0]], [-2.0 ** -900, 1.25 * 2.0 ** -300], N, 1, "direction:beta_nonfinite", dtypes=(F64,)),
    _c("b_beta_nonfinite_64_2", "bicgstab", [[1, -1.5 * 2.0 ** -900], [-1, 0]], [2.0 ** -300, 1], N, 2, "direction:beta_nonfinite", dtypes=(F64,)),
    _c("b_alpha_nonfinite_32_0", "bicgstab", [[-1.5 * 2.0 ** -100, 0], [1.25 * 2.0 ** -60, 0]], [2.0 ** -60, -1.5 * 2.0 ** 100], N, 0, "half:alpha_nonfinite", dtypes=(F32,)),
    _c("b_alpha_nonfinite_32_1", "bicgstab", [[2.0 ** -30, 1.25 * 2.0 ** -30], [1.25 * 2.0 ** -100, -1.5 * 2.0 ** -60]], [1.25 * 2.0 ** 100, 1.25 * 2.0 ** -60], N, 1, "half:alpha_nonfinite", dtypes=(F32,)),
    _c("b_alpha_nonfinite_64_0", "bicgstab", [[0, 2.0 ** -900], [-2.0 ** -300, -2.0 ** -600]], [-1.5 * 2.0 ** 300, 2.0 ** -900], N, 0, "half:alpha_nonfinite", dtypes=(F64,)),
    _c("b_alpha_nonfinite_64_1", "bicgstab", [[1.25 * 2.0 ** -900, -2.0 ** -600], [1.25 * 2.0 ** -600, -2.0 ** -600]], [2.0 ** -600, -1.5 * 2.0 ** 300], N, 1, "half:alpha_nonfinite", dtypes=(F64,)),
    _c("b_dot_nonfinite_32_0", "bicgstab", [[2.0 ** 60, -1.5 * 2.0 ** 60], [2.0 ** -30, 0]], [-2.0 ** 100, -1.5], N, 0, "half:dot_nonfinite", dtypes=(F32,)),
    _c("b_dot_nonfinite_32_1", "bicgstab", [[2.0 ** -100, 1], [2.0 ** -100, -1.5 * 2.0 ** 30]], [2.0 ** 60, -2.0 ** -60], N, 1, "half:dot_nonfinite", dtypes=(F32,)),
    _c("b_dot_nonfinite_64_0", "bicgstab", [[0, -1.5 * 2.0 ** 900], [1.25 * 2.0 ** -900, 1.25]], [2.0 ** 300, 1.25], N, 0, "half:dot_nonfinite", dtypes=(F64,)),
    _c("b_dot_nonfinite_64_1", "bicgstab", [[1.25 * 2.0 ** -600, 2.0 ** 900], [2.0 ** -600, 1.25 * 2.0 ** 600]], [0, 1.25], N, 1, "half:dot_nonfinite", dtypes=(F64,)),
    _c("b_omega_zero_32_1", "bicgstab", [[0, -2.0 ** 30], [0, 2.0 ** -100]], [1.25 * 2.0 ** 100, 2.0 ** 60], B, 1, "update:omega_zero", dtypes=(F32,)),
    _c("b_omega_zero_32_2", "bicgstab", [[2.0 ** 30, -1.5 * 2.0 ** 30], [-1.5 * 2.0 ** 60, -2.0 ** -100]], [1.25 * 2.0 ** 30, 1], B, 2, "update:omega_zero", dtypes=(F32,)),
    _c("b_omega_zero_64_1", "bicgstab", [[0, -2.0 ** 600], [-1.5 * 2.0 ** -300, 1.25 * 2.0 ** -300]], [-1.5, -2.0 ** -600], B, 1, "update:omega_zero", dtypes=(F64,)),
    # omega = T(<t,s> / <t,t>) overflows behind finite dots only when A s is tiny beside s: a mantissa of 1.75 and exponents next to the ends
    # of the range, which the sets above do not hold.  fp32 alone: in fp64 the dots have the elements' own range, and <t,t> that far below a
    # finite <s,s> is zero or a subnormal
    _c("b_omega_nonfinite_32_1", "bicgstab", [[0, 1.75 * 2.0 ** -125], [0, -1.75 * 2.0 ** -125]], [0, 1.75 * 2.0 ** 127], N, 1, "update:omega_nonfinite", dtypes=(F32,)),
    _c("b_ss_nonfinite_32_1", "bicgstab", [[1.25 * 2.0 ** -100, -2.0 ** -100], [-1.5 * 2.0 ** 60, 1.25 * 2.0 ** 100]], [2.0 ** 30, 0], N, 1, "update:ss_nonfinite", dtypes=(F32,)),
    _c("b_ss_nonfinite_32_2", "bicgstab", [[1.25 * 2.0 ** 60, -1.5 * 2.0 ** 30], [-1.5 * 2.0 ** 60, -1]], [-2.0 ** 60, 1.25 * 2.0 ** -100], N, 2, "update:ss_nonfinite", dtypes=(F32,)),
    _c("b_ss_nonfinite_64_1", "bicgstab", [[1.25 * 2.0 ** -900, -1.5 * 2.0 ** -300], [1.25 * 2.0 ** 300, 0]], [2.0 ** -600, 1.25 * 2.0 ** 300], N, 1, "update:ss_nonfinite", dtypes=(F64,)),
    # (at 2 not [[2^-900, -2^-900], [1.25 * 2^-600, 1.25 * 2^-900]] with b = [-2^-300, -2^300]: its first row cancels, and under a fused multiply-add it runs on)
    _c("b_ss_nonfinite_64_2", "bicgstab", [[1, -1.5 * 2.0 ** -600], [1.25 * 2.0 ** 300, -2.0 ** -600]], [-1.5, 0], N, 2, "update:ss_nonfinite", dtypes=(F64,)),
    _c("b_ts_tt_nonfinite_32_1", "bicgstab", [[-2.0 ** -60, -1.5 * 2.0 ** 100], [1.25 * 2.0 ** 60, 0]], [2.0 ** 30, -2.0 ** -30], N, 1, "update:ts_tt_nonfinite", dtypes=(F32,)),
    _c("b_ts_tt_nonfinite_32_2", "bicgstab", [[0, 1.25 * 2.0 ** 100], [2.0 ** -100, 2.0 ** 100]], [-1.5, -2.0 ** -30], N, 2, "update:ts_tt_nonfinite", dtypes=(F32,)),
    _c("b_ts_tt_nonfinite_64_1", "bicgstab", [[-1.5 * 2.0 ** 600, -1.5], [1.25 * 2.0 ** 900, 2.0 ** 900]], [-1, -1.5], N, 1, "update:ts_tt_nonfinite", dtypes=(F64,)),
    _c("b_ts_tt_nonfinite_64_2", "bicgstab", [[-1.5 * 2.0 ** -900, 2.0 ** 300], [-1.5 * 2.0 ** -300, 2.0 ** 300]], [-1.5, -2.0 ** -300], N, 2, "update:ts_tt_nonfinite", dtypes=(F64,)),
    _c("c_nonfinite_64_0", "cg", [[2.0 ** 600, -1.5], [-1.5, -1]], [2.0 ** 600, 2.0 ** 900], N, 0, "begin:nonfinite", dtypes=(F64,)),
    _c("c_beta_nonfinite_32_1", "cg", [[2.0 ** -30, 2.0 ** 60], [2.0 ** 60, 2.0 ** 60]], [1.25 * 2.0 ** 30, 0], N, 1, "direction:beta_nonfinite", dinv=[0.5, 2], dtypes=(F32,)),
    _c("c_beta_nonfinite_32_2", "cg", [[1.25 * 2.0 ** 100, -2.0 ** 30], [-2.0 ** 30, 2.0 ** -100]], [-2.0 ** -100, -2.0 ** -60], N, 2, "direction:beta_nonfinite", dinv=[0.5, 2], dtypes=(F32,)),
    _c("c_beta_nonfinite_64_1", "cg", [[1.25 * 2.0 ** -300, -2.0 ** 300], [-2.0 ** 300, 0]], [-2.0 ** -300, 0], N, 1, "direction:beta_nonfinite", dinv=[1, 0.5], dtypes=(F64,)),
    _c("c_nonfinite_32_1", "cg", [[-2.0 ** -60, 2.0 ** 30], [2.0 ** 30, 2.0 ** -60]], [0, 1.25 * 2.0 ** 60], N, 1, "direction:nonfinite", dtypes=(F32,)),
    _c("c_nonfinite_32_2", "cg", [[2.0 ** 60, -2.0 ** 30], [-2.0 ** 30, 1.25 * 2.0 ** -100]], [2.0 ** 30, 2.0 ** 30], N, 2, "direction:nonfinite", dinv=[1, 0.5], dtypes=(F32,)),
    _c("c_nonfinite_64_1", "cg", [[2.0 ** -600, -1.5 * 2.0 ** -900], [-1.5 * 2.0 ** -900, -2.0 ** 600]], [-1.5 * 2.0 ** 300, 1.25 * 2.0 ** -300], N, 1, "direction:nonfinite", dinv=[1, 0.5], dtypes=(F64,)),
    _c("c_nonfinite_64_2", "cg", [[1.25 * 2.0 ** -900, -1], [-1, 1.25 * 2.0 ** 600]], [-1.5, 1], N, 2, "direction:nonfinite", dinv=[2, 1], dtypes=(F64,)),
    _c("c_alpha_nonfinite_32_0", "cg", [[0, -1.5 * 2.0 ** -30], [-1.5 * 2.0 ** -30, 0]], [-1, 1.25 * 2.0 ** 100], N, 0, "update:alpha_nonfinite", dtypes=(F32,)),
    _c("c_alpha_nonfinite_32_1", "cg", [[2.0 ** -30, 1.25 * 2.0 ** -100], [1.25 * 2.0 ** -100, 0]], [1.25 * 2.0 ** 60, 1], N, 1, "update:alpha_nonfinite", dtypes=(F32,)),
    _c("c_alpha_nonfinite_64_0", "cg", [[0, -1.5 * 2.0 ** -600], [-1.5 * 2.0 ** -600, 1.25 * 2.0 ** 300]], [1.25 * 2.0 ** 300, -2.0 ** -600], N, 0, "update:alpha_nonfinite", dinv=[2, 1], dtypes=(F64,)),
    _c("c_dot_nonfinite_32_0", "cg", [[-1.5 * 2.0 ** -30, -1.5 * 2.0 ** 100], [-1.5 * 2.0 ** 100, 2.0 ** -60]], [-2.0 ** 30, 1.25 * 2.0 ** 60], N, 0, "update:dot_nonfinite", dinv=[0.5, 2], dtypes=(F32,)),
    _c("c_dot_nonfinite_32_1", "cg", [[-2.0 ** -100, -1.5 * 2.0 ** 100], [-1.5 * 2.0 ** 100, -1.5 * 2.0 ** 30]], [2.0 ** -60, -1.5], N, 1, "update:dot_nonfinite", dinv=[1, 0.5], dtypes=(F32,)),
    _c("c_dot_nonfinite_64_0", "cg", [[-1.5 * 2.0 ** 600, 1.25 * 2.0 ** -300], [1.25 * 2.0 ** -300, 1]], [-1.5 * 2.0 ** 300, 2.0 ** -300], N, 0, "update:dot_nonfinite", dinv=[0.5, 2], dtypes=(F64,)),
    _c("c_dot_nonfinite_64_1", "cg", [[2.0 ** -600, 0], [0, -1.5 * 2.0 ** 600]], [1.25, -1.5 * 2.0 ** -900], N, 1, "update:dot_nonfinite", dtypes=(F64,)),
]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def solver(case):
    return cgc.cg if case.solver == "cg" else bc.bicgstab


def system(case, reps, dtype, pre=False):
    """-> (CSR of `reps` copies of the block along the diagonal, b, dinv or None, x0 or None) in `dtype`; pre: with PRE folded in (BiCGStab)"""
    block = np.array(case.block, dtype=np.float64)
    dinv = None if case.dinv is None else np.array(case.dinv, dtype=np.float64)
    x0 = None if case.x0 is None else np.array(case.x0, dtype=np.float64)
    if pre:
        assert case.solver == "bicgstab" and dinv is None
        dinv = np.array(PRE)
        block = block / dinv[None, :]
        x0 = None if x0 is None else x0 * dinv               # the same y = x / Dinv
    i, j = np.nonzero(block)
    base = 2 * np.arange(reps)[:, None]
    csr = cgc._from_coo(2 * reps, (base + i).ravel(), (base + j).ravel(), np.tile(block[i, j], reps), dtype)
    assert np.array_equal(csr.val.astype(np.float64), np.tile(block[i, j], reps)), "an entry is not representable"
    tiled = lambda v: None if v is None else np.tile(np.asarray(v, dtype=np.float64).astype(dtype), reps)
    return csr, tiled(case.b), tiled(dinv), tiled(x0)


def wide(dtype):
    return np.float64 if dtype == np.float32 else np.longdouble


def matvec_wide(csr):
    """cg_cases.matvec with every row accumulated in the next wider type and rounded to the matrix's type once"""
    W, T = wide(csr.val.dtype.type), csr.val.dtype.type
    val, starts = csr.val.astype(W), csr.rowptr[:-1].astype(np.int64)

    def multiply(x):
        with np.errstate(all="ignore"):
            return np.add.reduceat(val * x.astype(W)[csr.colidx], starts).astype(T)
    return multiply


def subnormal(*values):
    """is any element a non-zero subnormal of its own type?"""
    for v in values:
        a = np.abs(np.asarray(v))
        if ((a > 0) & (a < np.finfo(a.dtype).tiny)).any():
            return True
    return False


def run(case, reps, dtype, pre=False, multiply=None, watch=None, **kw):
    """the model on `reps` copies of the case (cg_cases.matvec unless a multiply is given) -> its result dict"""
    csr, b, dinv, x0 = system(case, reps, dtype, pre)
    kw.setdefault("max_iterations", BUDGET)
    return solver(case)(multiply(csr) if multiply else cgc.matvec(csr), b, x0=x0, dinv=dinv, watch=watch, **kw)


# ----------------------------------------------------------------------------- what a model can return
# every `end` of the two models but "begin:empty" (m = 0) and "budget"; tests/test_solve_ends_host.py compares these lists with the models' text
ENDS = {
    "bicgstab": ("begin:nonfinite", "begin:bb_zero", "begin:converged", "half:dot_nonfinite", "half:rv_zero", "half:rho_zero", "half:alpha_nonfinite",
                 "update:ss_nonfinite", "update:ss_converged", "update:ts_tt_nonfinite", "update:tt_zero", "update:ts_zero", "update:omega_nonfinite",
                 "update:omega_zero", "direction:nonfinite", "direction:converged", "direction:beta_nonfinite"),
    "cg": ("begin:nonfinite", "begin:bb_zero", "begin:converged", "begin:rz_breakdown", "update:dot_nonfinite", "update:pq_breakdown",
           "update:alpha_nonfinite", "direction:nonfinite", "direction:converged", "direction:rz_breakdown", "direction:beta_nonfinite"),
}
# reached by no block of the searches (integer entries; the scaled mantissas and exponents above, and exponents next to the ends of the
# range): a non-finite <r,r> or rho in bicg_direction, and, in fp64, omega non-finite behind finite <t,s> and <t,t>
ALLOWED_GAPS = {"bicgstab": ("direction:nonfinite", "update:omega_nonfinite"), "cg": ()}


def first_kernel(case):
    """does the end sit in the first kernel behind a multiply (bicg_half, cg_update)?  It is then found while STARTING iteration
    `iterations` + 1: a budget of `iterations` reports MAX_ITERATIONS"""
    return case.end.startswith("half:") or (case.solver == "cg" and case.end.startswith("update:"))


# ----------------------------------------------------------------------------- atol
def atol_probes(model):
    """model(atol) -> result dict (rtol = 0).  -> [(a, k, end)]: atol = a ends the run at iteration k in `end` because a * a == rr there and the
    test is <=, while the next double below a does not end it there.  Candidates: the exact square roots of the run's history and half-step
    sums; every one returned has been confirmed with the model."""
    free = model(0.0)
    sums = set(free["history"].tolist()) | set(free.get("halves", np.zeros(0)).tolist())
    out = []
    for h in sorted(sums, reverse=True):
        a = float(np.sqrt(h))
        if not (h > 0 and np.isfinite(h) and a * a == h):
            continue
        at, below = model(a), model(float(np.nextafter(a, 0.0)))
        if at["end"].endswith("converged") and at["rr"] == h and (below["iterations"], below["end"]) != (at["iterations"], at["end"]):
            out.append((a, at["iterations"], at["end"]))
    return out


# ----------------------------------------------------------------------------- several cases in one matrix
def mixed(cases, reps, dtype, tail):
    """One matrix that holds every case's block `reps` times -- block j of a group of len(cases) is case j's -- and behind them `tail` rows of
    a tridiagonal matrix (cg_cases.tri, or bicgstab_cases.tri_ns when the cases are BiCGStab's), so that ONE handle can be driven into each
    case's end, and through an ordinary solve, by the right-hand side alone.  -> (CSR, select): select(j) -> (b, dinv, x0) of case j on its
    own blocks and zero (Dinv one) everywhere else, where the recurrence then never leaves zero; select(None, seed) -> a right-hand side in
    (-1, 1) on the tail and zero on the blocks."""
    n = len(cases)
    parts = [system(c, 1, dtype) for c in cases]
    rows, cols, vals = [], [], []
    for j, (csr, _, _, _) in enumerate(parts):
        r = np.repeat(np.arange(2), np.diff(csr.rowptr))
        base = 2 * (j + n * np.arange(reps))[:, None]
        rows.append((base + r).ravel()), cols.append((base + csr.colidx).ravel()), vals.append(np.tile(csr.val.astype(np.float64), reps))
    head = 2 * n * reps
    band = cgc.tri(tail, np.float64) if cases[0].solver == "cg" else bc.tri_ns(tail, np.float64)
    rows.append(head + np.repeat(np.arange(tail), np.diff(band.rowptr))), cols.append(head + band.colidx), vals.append(band.val)
    whole = cgc._from_coo(head + tail, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), dtype)

    def select(j, seed=0):
        b, dinv, x0 = np.zeros(head + tail, dtype=dtype), np.ones(head + tail, dtype=dtype), np.zeros(head + tail, dtype=dtype)
        if j is None:
            b[head:] = np.random.default_rng(seed).uniform(-1, 1, tail)
            return b, None, None
        _, cb, cd, cx = parts[j]
        own = (2 * (j + n * np.arange(reps))[:, None] + np.arange(2)).ravel()
        b[own] = np.tile(cb, reps)
        if cd is not None:
            dinv[own] = np.tile(cd, reps)
        if cx is not None:
            x0[own] = np.tile(cx, reps)
        return b, None if cd is None else dinv, None if cx is None else x0
    return whole, select


# ----------------------------------------------------------------------------- the CG catalogue as the columns of one call
# spmv_hip_cg_columns (tests/test_cg_column_ends_host.py, tests/test_gpu_cg_column_ends.py): every CG case of a type is one column of a call
# on `mixed`, and behind them one ordinary column on the tridiagonal tail that is still running at BUDGET, so that every case ends -- and is
# frozen -- in company that runs on.  One call has one Dinv, so the cases are grouped by whether they carry one.
GROUPS = ("plain", "plain_nox0", "pre")
BIG_GROUP = ("c_rr_2", "c_pq_1x", "c_begin_zero")        # the group of the run at BIG: three ends at three iteration counts, one of them B = 0


def column_groups(dtype):
    """-> {"plain": the CG cases of `dtype` without a Dinv (they run with Dinv = NULL or all ones), "plain_nox0": those of them without a guess,
    "pre": the cases with a Dinv (they share one)}, in the catalogue's order"""
    mine = [c for c in CASES if c.solver == "cg" and dtype in c.dtypes]
    plain = [c for c in mine if c.dinv is None]
    return {"plain": plain, "plain_nox0": [c for c in plain if c.x0 is None], "pre": [c for c in mine if c.dinv is not None]}


def columns_shape(n, m):
    """-> (reps, tail) of `mixed` for n cases at the size m of SIZES or BIG; the smallest size is one copy of every block and four tail rows"""
    if m == SIZES[0]:
        return 1, 4
    reps = (m - 4) // (2 * n)
    return reps, m - 2 * n * reps


def columns_system(group, m, dtype):
    """group: a name of GROUPS or a list of CG cases.  -> (CSR, B, X0 or None, Dinv or None, cases): `mixed` over the cases with column j of B
    (and of X0) case j's right-hand side (guess) and, last, the ordinary column select(None, 1) on the tail.  X0: None when no case has a
    guess, zero in the columns of the cases without one.  Dinv: None when no case has one; every case's own on its own blocks -- the blocks
    do not touch, so no column's recurrence sees another's entries -- and 1 everywhere else."""
    cases = column_groups(dtype)[group] if isinstance(group, str) else list(group)
    n = len(cases)
    assert 1 <= n <= 15 and all(c.solver == "cg" and dtype in c.dtypes for c in cases)
    reps, tail = columns_shape(n, m)
    csr, select = mixed(cases, reps, dtype, tail)
    return (csr,) + columns_batch(csr, select, range(n), dtype) + (cases,)


def columns_batch(csr, select, picked, dtype):
    """-> (B, X0 or None, Dinv or None) of columns_system for the cases `picked` (indices into the cases `mixed` was built over) and the tail"""
    picks = [select(j) for j in picked]
    zero = np.zeros(csr.m, dtype=dtype)
    B = np.stack([p[0] for p in picks] + [select(None, 1)[0]], axis=1)
    X0 = None
    if any(p[2] is not None for p in picks):
        X0 = np.ascontiguousarray(np.stack([zero if p[2] is None else p[2] for p in picks] + [zero], axis=1))
    Dinv = None
    if any(p[1] is not None for p in picks):
        Dinv = np.ones(csr.m, dtype=dtype)
        for p in picks:
            if p[1] is not None:
                own = p[1] != 1
                assert (Dinv[own] == 1).all()                  # nobody else's rows
                Dinv[own] = p[1][own]
    return np.ascontiguousarray(B), X0, Dinv


def columns_state_system(dtype, m=1026):
    """the matrix of the test of state between calls: `mixed` over ALL CG cases of the type (more than one call holds), so that one handle runs
    the `plain` group, the `pre` group and ordinary columns on the tail.  -> (CSR, {group: (B, X0, Dinv, cases)}, tail_columns(k, seed) -> m x k
    generic right-hand sides on the tail rows, zero on the blocks)"""
    groups = column_groups(dtype)
    every = groups["plain"] + groups["pre"]
    reps, tail = columns_shape(len(every), m)
    csr, select = mixed(every, reps, dtype, tail)
    out = {g: columns_batch(csr, select, [every.index(c) for c in groups[g]], dtype) + (groups[g],) for g in ("plain", "pre")}

    def tail_columns(k, seed):
        return np.ascontiguousarray(np.stack([select(None, 1000 * seed + j)[0] for j in range(k)], axis=1))
    return csr, out, tail_columns


def column_runs(group, B, X0):
    """the (X0 or None, Dinv-is-all-ones) combinations a group is run with: `plain` with its guesses, also under an all-ones Dinv; `plain_nox0`
    from x = 0; `pre` from x = 0 and from all-zero guesses.  -> [(name, X0 of the call or None, ones: bool)]"""
    if group == "plain":
        return [("x0", X0, False), ("x0-ones", X0, True)]
    if group == "plain_nox0":
        return [("nox0", None, False)]
    return [("nox0", None, False), ("x0", np.zeros_like(B), False)]


def declared_columns(cases, budget=BUDGET):
    """-> what every column of columns_system reports under `budget`: (status, iterations, end) per case and the tail's (MAX_ITERATIONS, budget,
    "budget").  An end that ccg_alpha finds (first_kernel) is found while starting iteration `iterations` + 1: not with a budget of `iterations`"""
    out = []
    for c in cases:
        short = budget < c.iterations or (budget == c.iterations and first_kernel(c))
        out.append((M, budget, "budget") if short else (c.status, c.iterations, c.end))
    return out + [(M, budget, "budget")]


def state_cases(solver, dtype):
    """the cases of the test of state between solves: one of each breakdown, a convergence, and, last, one that turns non-finite inside the loop"""
    wide = dtype == np.float64
    names = {"bicgstab": ("b_rr_2", "b_rv0_1", "b_rho0_2", "b_tt0_1", "b_ts0_1", "b_half_1", "b_omega_zero_64_1" if wide else "b_omega_zero_32_1",
                          "b_ts_tt_nonfinite_64_1" if wide else "b_ts_tt_nonfinite_32_1"),
             "cg": ("c_rr_2", "c_pq_1x", "c_rz_1x", "c_rz_0", "c_nonfinite_64_1" if wide else "c_nonfinite_32_1")}[solver]
    return [by_name(n) for n in names]


def state_system(solver, dtype, m=1026):
    """-> (cases, CSR of m rows, select): `mixed` over state_cases, about half of the rows in blocks and half in the tridiagonal tail"""
    cases = state_cases(solver, dtype)
    reps = m // (4 * len(cases))
    return (cases,) + mixed(cases, reps, dtype, m - 2 * len(cases) * reps)


# ----------------------------------------------------------------------------- matrices for the solvers on every executor
def arrow(m, dtype, symmetric, per_row=4, seed=3):
    """m rows with a dense first row and a dense first column (a row longer than any long-row threshold) around a random pattern of about
    per_row entries per row; off-diagonal entries are multiples of 1/8 in [-1, 1] without 0.  symmetric: the pattern and the values are, and
    the diagonal is 2 * sum |off-diagonal| (for CG); otherwise 1.25 * sum |off-diagonal| (for BiCGStab).  Every entry is exact in fp32."""
    rng = np.random.default_rng(seed)

    def eighths(n):
        return rng.integers(1, 9, n) * rng.choice((-1.0, 1.0), n) / 8.0
    i = np.repeat(np.arange(1, m), per_row)
    j = rng.integers(1, m, i.size)
    keep = i != j
    i, j = i[keep], j[keep]
    v, first = eighths(i.size), np.arange(1, m)
    across, down = eighths(m - 1), eighths(m - 1)
    if symmetric:
        i, j, v, down = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([v, v]), across
    rows, cols = np.concatenate([i, np.zeros(m - 1, dtype=np.int64), first]), np.concatenate([j, first, np.zeros(m - 1, dtype=np.int64)])
    off = cgc._from_coo(m, rows, cols, np.concatenate([v, across, down]), np.float64)
    r = np.repeat(np.arange(m), np.diff(off.rowptr))
    diag = (2.0 if symmetric else 1.25) * np.bincount(r, weights=np.abs(off.val), minlength=m)
    return cgc._from_coo(m, np.concatenate([r, np.arange(m)]), np.concatenate([off.colidx, np.arange(m)]), np.concatenate([off.val, diag]), dtype)


def band32(m, dtype, every=0, tail=0, long_row=None, seed=4):
    """m rows of 32 entries: columns i - 16 .. i + 15 (mod m); in every `every`-th row (every > 0) and in the last `tail` rows the diagonal and 31
    random columns instead; row `long_row`, when given, holds the 544 columns i - 272 .. i + 271 (longer than the long-row threshold of 512
    at 8 lanes per row).
    Off-diagonal entries are multiples of 1/8 in [-1, 1], the diagonal is 24 (400 in the long row): row starts and lengths are multiples of 32 and every value is
    k * 2^-3, which is what the packed fp64 tiles ask for (tests/packed_cases.py: model_packed), and with random rows part of the entries has
    no column locality."""
    from spmv_amd import synth
    rng = np.random.default_rng(seed)
    i = np.arange(m, dtype=np.int64)[:, None]
    cols = (i - 16 + np.arange(32, dtype=np.int64)[None, :]) % m
    vals = rng.integers(-8, 9, (m, 32)) / 8.0
    vals[:, 16] = 24.0
    if every or tail:
        far = np.union1d(np.arange(0, m, every) if every else np.zeros(0, dtype=np.int64), np.arange(m - tail, m)).astype(np.int64)
        c = rng.integers(0, m, (far.size, 32))
        c[:, 0] = far
        order = np.argsort(c, axis=1, kind="stable")
        v = vals[far]
        v[:, 0], v[:, 16] = 24.0, 0.125
        cols[far], vals[far] = np.take_along_axis(c, order, axis=1), np.take_along_axis(v, order, axis=1)
    if long_row is None:
        return synth.CSR(m, m, (32 * np.arange(m + 1)).astype(np.int32), cols.ravel().astype(np.int32), vals.ravel().astype(dtype))
    lens = np.full(m, 32)
    lens[long_row] = 544
    rp = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=rp[1:])
    wide_c, wide_v = (long_row - 272 + np.arange(544)) % m, rng.integers(-8, 9, 544) / 8.0
    wide_v[272] = 400.0
    c = np.concatenate([cols[:long_row].ravel(), wide_c, cols[long_row + 1:].ravel()])
    v = np.concatenate([vals[:long_row].ravel(), wide_v, vals[long_row + 1:].ravel()])
    return synth.CSR(m, m, rp.astype(np.int32), c.astype(np.int32), v.astype(dtype))
