"""The host model of spmv_hip_cg_columns and the right-hand sides its tests share (tests/test_cg_columns_host.py, tests/test_gpu_cg_columns.py).

The per-column contract of include/spmv_hip.h says that column j of a call IS spmv_hip_cg's recurrence around another multiply, so the model is
cg_cases.cg -- unchanged, with cg_cases.dot over the column's m elements -- run once per column around a COLUMN multiply: on the GPU column 0
of Handle.spmm on a two-column probe (spmm's bits do not depend on the other column), on the CPU cg_cases.matvec."""
import numpy as np

import cg_cases as cgc


def solve(multiply, B, X0=None, dinv=None, **kw):
    """-> one cg_cases.cg result per column of B (m x k); multiply(v) -> A v for one column in B's dtype; X0: None or the m x k guesses"""
    return [cgc.cg(multiply, np.ascontiguousarray(B[:, j]), x0=None if X0 is None else np.ascontiguousarray(X0[:, j]), dinv=dinv, **kw) for j in range(B.shape[1])]


def spmm_column(h):
    """the model's multiply on the GPU: column 0 of this handle's spmm on the probe [v, 0]"""
    def multiply(v):
        probe = np.zeros((v.size, 2), dtype=v.dtype)
        probe[:, 0] = v
        return np.ascontiguousarray(h.spmm(probe)[:, 0])
    return multiply


def columns(m, k, dtype, seed=0):
    """k generic right-hand sides, column j the same whatever k is"""
    return np.stack([cgc.rhs(m, dtype, 1000 * seed + j) for j in range(k)], axis=1)


def eigenvector(g, dtype, a=1, b=2):
    """an eigenvector of lap2d(g): CG from x = 0 meets any modest rtol after ONE iteration"""
    i = np.arange(1, g + 1)
    return np.outer(np.sin(np.pi * a * i / (g + 1)), np.sin(np.pi * b * i / (g + 1))).ravel().astype(dtype)


MIXED = ("eigenvector", "generic", "zero", "nan", "generic2")


def mixed_ends(g, dtype):
    """m x 5 right-hand sides for lap2d(g) that end differently: an eigenvector (1 iteration), a generic column, zeros (x = 0 after 0
    iterations), a column with a NaN (NONFINITE at the start), another generic column"""
    m = g * g
    nan = cgc.rhs(m, dtype, 41)
    nan[m // 3] = np.nan
    return np.stack([eigenvector(g, dtype), cgc.rhs(m, dtype, 40), np.zeros(m, dtype=dtype), nan, cgc.rhs(m, dtype, 42)], axis=1)


def workspace_bytes(m, k, itemsize):
    """the documented size of the solver's workspace (include/spmv_hip.h)"""
    return 3 * ((m * k * itemsize + 255) // 256 * 256) + 4 * k * 8192 + 1024
