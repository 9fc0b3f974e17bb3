"""CPU: the host model of tests/bicgstab_cases.py against the conditions the GPU tests rely on (tests/test_gpu_bicgstab.py): before the
model is the yardstick there, it has to meet them alone.  The dot it is built on is cg_cases.dot, which tests/test_cg_host.py holds against
exact arithmetic; the option and result structs are spmv_hip_cg's, whose mirrors that file holds against the header.

The true-residual bar ||b - A x|| / ||b|| <= 10 rtol is spmv_hip_cg's: the recurrence's residual meets rtol by construction, and the gap to
the true residual is the rounding of a few dozen updates in T, far below 9 rtol for the rtol used with each type (1e-8 in fp64, 1e-3 in
fp32)."""
import numpy as np
import pytest

import bicgstab_cases as bc
import cg_cases as cgc
from spmv_amd import api

# the two solves the GPU tests repeat: (matrix, dtype, rtol)
SOLVES = [("upwind32", np.float64, 1e-8), ("nonsym_dominant4096", np.float32, 1e-3)]


def build(name, dtype):
    return bc.upwind(32, dtype) if name == "upwind32" else bc.nonsym_dominant(4096, dtype)


def test_the_python_interface_exists():
    assert callable(api.bicgstab) and callable(api.time_bicgstab_iterations) and callable(api.Handle.bicgstab)
    assert "spmv_hip_bicgstab" in api.FUNCTIONS and "spmv_hip_time_bicgstab_iterations" in api.FUNCTIONS
    assert len(api.CG_STATUS) == 4                          # the statuses are spmv_hip_cg's


def test_the_matrices_are_what_their_names_say():
    a = bc.tri_ns(5)
    dense = np.zeros((5, 5))
    dense[np.repeat(np.arange(5), np.diff(a.rowptr)), a.colidx] = a.val
    assert np.array_equal(dense, 2.125 * np.eye(5) - 1.5 * np.eye(5, k=-1) - 0.5 * np.eye(5, k=1))
    u = bc.upwind(3)
    dense = np.zeros((9, 9))
    dense[np.repeat(np.arange(9), np.diff(u.rowptr)), u.colidx] = u.val
    assert dense[4].tolist() == [0, -1, 0, -1.5, 4.5, -1, 0, -1, 0] and dense[3, 2] == 0 and dense[2, 3] == 0    # no wrap between grid rows
    assert not np.array_equal(dense, dense.T)
    n = bc.nonsym_dominant(512)
    rows = np.repeat(np.arange(n.m), np.diff(n.rowptr))
    off = np.bincount(rows, weights=np.where(rows == n.colidx, 0, np.abs(n.val)), minlength=n.m)
    assert np.allclose(bc.diagonal(n), 1.25 * off) and (off > 0).all()
    s = bc.skew(6)
    dense = np.zeros((6, 6))
    dense[np.repeat(np.arange(6), np.diff(s.rowptr)), s.colidx] = s.val
    assert np.array_equal(dense, -dense.T) and dense[0, 1] == 1 and not bc.diagonal(s).any()
    assert np.array_equal(bc.twice_identity(4).val, np.full(4, 2.0))


@pytest.mark.parametrize("name,dtype,rtol", SOLVES)
def test_model_converges_and_the_true_residual_follows(name, dtype, rtol):
    csr = build(name, dtype)
    b = bc.rhs(csr.m, dtype)
    out = bc.bicgstab(bc.matvec(csr), b, rtol=rtol, max_iterations=500)
    res = bc.true_residual(csr, b, out["x"])
    print(f"{name}: {out['iterations']} iterations, rr/bb = {out['rr'] / out['bb']:.3e}, true residual = {res:.3e}")
    assert out["status"] == bc.CONVERGED and 3 < out["iterations"] < 500
    assert out["rr"] <= rtol * rtol * out["bb"] and len(out["history"]) == out["iterations"] + 1 == len(out["iterates"])
    assert out["rr"] == out["history"][-1] and np.array_equal(out["x"], out["iterates"][-1])
    assert res <= 10 * rtol
    # a smaller budget stops at the same iterate
    part = bc.bicgstab(bc.matvec(csr), b, rtol=rtol, max_iterations=3)
    assert part["status"] == bc.MAX_ITERATIONS and part["iterations"] == 3 and np.array_equal(part["x"], out["iterates"][3])
    assert np.array_equal(part["history"], out["history"][:4])


@pytest.mark.parametrize("name,dtype,rtol", SOLVES)
def test_conjugate_gradients_do_not_converge_on_the_same_systems(name, dtype, rtol):
    """why the solver exists: spmv_hip_cg's recurrence on a nonsymmetric matrix"""
    csr = build(name, dtype)
    b = bc.rhs(csr.m, dtype)
    out = cgc.cg(bc.matvec(csr), b, rtol=rtol, max_iterations=500)
    print(f"{name}: cg ends with status {out['status']} after {out['iterations']} iterations, true residual {bc.true_residual(csr, b, out['x']):.3e}")
    assert out["status"] != bc.CONVERGED


def test_jacobi_needs_strictly_fewer_iterations_on_the_scaled_stencil():
    csr = bc.scaled_upwind(16, 3)
    b = bc.rhs(csr.m, np.float64)
    plain = bc.bicgstab(bc.matvec(csr), b, rtol=1e-8, max_iterations=5000)
    jacobi = bc.bicgstab(bc.matvec(csr), b, dinv=1.0 / bc.diagonal(csr), rtol=1e-8, max_iterations=5000)
    print(f"scaled_upwind(16, 3): {plain['iterations']} iterations without, {jacobi['iterations']} with Jacobi")
    assert plain["status"] == jacobi["status"] == bc.CONVERGED
    assert jacobi["iterations"] < plain["iterations"]
    # x solves the ORIGINAL system whatever Dinv is: the preconditioner is a right one
    assert bc.true_residual(csr, b, jacobi["x"]) <= 1e-7


def test_dinv_of_ones_is_no_preconditioner():
    csr = bc.tri_ns(1025)
    b = bc.rhs(csr.m, np.float64)
    mul = bc.matvec(csr)
    for x0 in (None, bc.rhs(csr.m, np.float64, 9)):
        none = bc.bicgstab(mul, b, x0=x0, max_iterations=5)
        ones = bc.bicgstab(mul, b, x0=x0, dinv=np.ones_like(b), max_iterations=5)
        assert none["iterations"] == 5 and np.array_equal(none["x"], ones["x"]) and np.array_equal(none["history"], ones["history"])


def test_zero_and_nonfinite_right_hand_sides():
    csr = bc.tri_ns(1025)
    b = bc.rhs(csr.m, np.float64)
    mul = bc.matvec(csr)
    for x0 in (None, b):
        zero = bc.bicgstab(mul, np.zeros_like(b), x0=x0, max_iterations=5)
        assert zero["status"] == bc.CONVERGED and zero["iterations"] == 0 and not zero["x"].any() and zero["rr"] == 0 == zero["bb"]
        assert np.array_equal(zero["history"], np.zeros(1))
    nan = b.copy()
    nan[7] = np.nan
    bad = bc.bicgstab(mul, nan, max_iterations=5)
    assert bad["status"] == bc.NONFINITE and bad["iterations"] <= 1


def test_breakdown_on_the_skew_matrix():
    sk = bc.skew(1025)
    ones = np.ones(sk.m)
    v = bc.matvec(sk)(ones)
    assert v[0] == 1 and v[-1] == -1 and not v[1:-1].any()            # <rhat, v> is exactly 1 + (-1)
    brk = bc.bicgstab(bc.matvec(sk), ones, max_iterations=5)
    assert brk["status"] == bc.BREAKDOWN and brk["iterations"] == 0 and np.isfinite(brk["x"]).all() and not brk["x"].any()
    assert np.array_equal(brk["history"], [float(sk.m)]) and brk["rr"] == sk.m == brk["bb"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [1, 1025])
def test_the_half_step_ends_the_loop_on_twice_the_identity(m, dtype):
    csr = bc.twice_identity(m, dtype)
    b = bc.rhs(m, dtype, 2)
    out = bc.bicgstab(bc.matvec(csr), b, rtol=0.0, max_iterations=5)
    assert (out["status"], out["iterations"]) == (bc.CONVERGED, 1) and out["rr"] == 0.0
    assert len(out["history"]) == 2 and out["history"][1] == 0.0 and out["history"][0] == out["bb"] > 0
    assert np.array_equal(out["x"], b * dtype(0.5)) and np.array_equal(out["x"], out["iterates"][1])
