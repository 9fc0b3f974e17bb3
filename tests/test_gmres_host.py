"""CPU: the host model of tests/gmres_cases.py against the conditions the GPU tests rely on (tests/test_gpu_gmres.py): before the model is the
yardstick there, it has to meet them alone.  The dot it is built on is cg_cases.dot, which tests/test_cg_host.py holds against exact
arithmetic; the option and result structs are spmv_hip_cg's.

The one tolerance: GMRES reports the recurrence's ESTIMATE of <r,r>, not the norm of a residual vector.  test_the_estimate_follows_the_true_
residual measures, on the well-conditioned systems below, the ratio of the true <b - A x, b - A x> (longdouble) to the model's own rr."""
import numpy as np
import pytest

import gmres_cases as gc
from spmv_amd import api

# the well-conditioned solves: (matrix, dtype, rtol)
SOLVES = [("upwind32", np.float64, 1e-8), ("nonsym_dominant4096", np.float64, 1e-8), ("upwind32", np.float32, 1e-3), ("nonsym_dominant4096", np.float32, 1e-3)]


def build(name, dtype):
    return gc.upwind(32, dtype) if name == "upwind32" else gc.nonsym_dominant(4096, dtype)


def test_the_python_interface_exists():
    assert callable(api.gmres) and callable(api.time_gmres_iterations) and callable(api.Handle.gmres)
    assert "spmv_hip_gmres" in api.FUNCTIONS and "spmv_hip_time_gmres_iterations" in api.FUNCTIONS
    assert api.GMRES_RESTART_MAX == gc.RESTART_MAX == 32


@pytest.mark.parametrize("restart", [10, 30])
@pytest.mark.parametrize("name,dtype,rtol", SOLVES)
def test_the_estimate_follows_the_true_residual(name, dtype, rtol, restart):
    """measured here: true <r,r> / rr between 0.99997 and 1.0000048 over all eight runs; asserted with a factor of two (gmres_cases.RATIO_BOUND)"""
    csr = build(name, dtype)
    b = gc.rhs(csr.m, dtype)
    out = gc.gmres(gc.matvec(csr), b, restart, rtol=rtol, max_iterations=400)
    ratio = gc.true_rr(csr, b, out["x"]) / out["rr"]
    print(f"{name} {np.dtype(dtype).name} restart {restart}: {out['iterations']} iterations, rr/bb = {out['rr'] / out['bb']:.3e}, true <r,r> / rr = {ratio:.7f}")
    assert out["status"] == gc.CONVERGED and 3 < out["iterations"] < 400
    assert out["rr"] <= rtol * rtol * out["bb"] and len(out["history"]) == out["iterations"] + 1 == len(out["iterates"])
    assert out["rr"] == out["history"][-1] and np.array_equal(out["x"], out["iterates"][-1])
    assert ratio <= gc.RATIO_BOUND


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_history_does_not_rise_inside_a_cycle(dtype):
    csr = gc.upwind(32, dtype)
    b = gc.rhs(csr.m, dtype, 1)
    for restart in (3, 10):
        h = gc.gmres(gc.matvec(csr), b, restart, max_iterations=4 * restart + 1)["history"]
        assert len(h) == 4 * restart + 2
        for k in range(1, len(h)):
            if (k - 1) % restart:                         # k - 1 and k are steps of the same cycle
                assert h[k] <= h[k - 1], (restart, k)
        assert h[1] <= h[0]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [4, 1024])
def test_the_lucky_case_on_diagonal_matrices(m, dtype):
    """j distinct values: w = 0 exactly at step j (the vectors are chosen so that every operation is exact)"""
    ones = np.ones(m, dtype=dtype)
    one = gc.gmres(gc.matvec(gc.diag_of(np.full(m, 2.0), dtype)), ones, 5, max_iterations=9)
    assert (one["status"], one["iterations"], one["end"], one["rr"]) == (gc.CONVERGED, 1, "rotate:converged", 0.0)
    assert np.array_equal(one["x"], ones * dtype(0.5))
    two = gc.gmres(gc.matvec(gc.two_values(m, dtype)), ones, 5, max_iterations=9)
    assert (two["status"], two["iterations"], two["end"]) == (gc.CONVERGED, 2, "rotate:converged")
    assert np.array_equal(two["history"], [m, m, 0.0])
    assert np.array_equal(two["x"], np.where(np.arange(m) % 4 < 2, 0.5, -0.5).astype(dtype))


def test_breakdowns():
    guess = gc.rhs(8, np.float64, 3)
    zero = gc.gmres(gc.matvec(gc.zero_matrix(8)), np.ones(8), 5, x0=guess, max_iterations=9)
    assert (zero["status"], zero["iterations"], zero["end"]) == (gc.BREAKDOWN, 0, "rotate:d_zero") and np.array_equal(zero["x"], guess)
    assert np.array_equal(zero["history"], [8.0])
    e0 = np.zeros(8)
    e0[0] = 1
    for csr, b in ((gc.shift(8), e0), (gc.half_singular(4), np.ones(4))):       # singular, met at step 2 of a cycle of 5
        out = gc.gmres(gc.matvec(csr), b, 5, max_iterations=9)
        assert (out["status"], out["iterations"], out["end"]) == (gc.BREAKDOWN, 1, "rotate:d_zero")
        assert np.array_equal(out["x"], out["iterates"][1]) and np.isfinite(out["x"]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nonfinite(dtype):
    csr = gc.tri_ns(1025, dtype)
    bad = gc.rhs(csr.m, dtype)
    bad[7] = np.nan
    out = gc.gmres(gc.matvec(csr), bad, 5, max_iterations=9)
    assert (out["status"], out["iterations"], out["end"]) == (gc.NONFINITE, 0, "begin:nonfinite")
    e0 = np.zeros(8, dtype=dtype)
    e0[0] = 1
    out = gc.gmres(gc.matvec(gc.overflowing(8, dtype)), e0, 5, max_iterations=9)
    assert (out["status"], out["iterations"], out["end"]) == (gc.NONFINITE, 1, "rotate:nonfinite")
    assert np.array_equal(out["x"], out["iterates"][1]) and np.isfinite(out["x"]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_smaller_budget_stops_at_the_same_iterate_across_restarts(dtype):
    csr = gc.tri_ns(1025, dtype)
    b, guess = gc.rhs(csr.m, dtype), gc.rhs(csr.m, dtype, 9)
    mul = gc.matvec(csr)
    for restart in (1, 3):
        for x0 in (None, guess):
            full = gc.gmres(mul, b, restart, x0=x0, max_iterations=2 * restart + 2)
            assert full["iterations"] == 2 * restart + 2
            for k in range(2 * restart + 3):
                part = gc.gmres(mul, b, restart, x0=x0, max_iterations=k)
                assert (part["status"], part["iterations"]) == (gc.MAX_ITERATIONS, k)
                assert np.array_equal(part["x"], full["iterates"][k]) and np.array_equal(part["history"], full["history"][:k + 1])


def test_dinv_of_ones_is_no_preconditioner_and_a_real_one_is_a_right_one():
    csr = gc.tri_ns(1025)
    b = gc.rhs(csr.m, np.float64)
    mul = gc.matvec(csr)
    for x0 in (None, gc.rhs(csr.m, np.float64, 9)):
        none = gc.gmres(mul, b, 3, x0=x0, max_iterations=7)
        ones = gc.gmres(mul, b, 3, x0=x0, dinv=np.ones_like(b), max_iterations=7)
        assert none["iterations"] == 7 and np.array_equal(none["x"], ones["x"]) and np.array_equal(none["history"], ones["history"])
    sc = gc.scaled_upwind(16, 3)
    bs = gc.rhs(sc.m, np.float64)
    jac = gc.gmres(gc.matvec(sc), bs, 30, dinv=1.0 / gc.diagonal(sc), rtol=1e-8, max_iterations=2000)
    assert jac["status"] == gc.CONVERGED and gc.true_residual(sc, bs, jac["x"]) <= 1e-7    # x solves the ORIGINAL system


def test_zero_right_hand_side_and_the_workspace_formula():
    csr = gc.tri_ns(1025)
    b = gc.rhs(csr.m, np.float64)
    for x0 in (None, b):
        zero = gc.gmres(gc.matvec(csr), np.zeros_like(b), 4, x0=x0, max_iterations=5)
        assert zero["status"] == gc.CONVERGED and zero["iterations"] == 0 and not zero["x"].any() and zero["rr"] == 0 == zero["bb"]
    assert gc.workspace_bytes(100, 8, 5) == 8 * 1024 + 35 * 8192 + 10240
