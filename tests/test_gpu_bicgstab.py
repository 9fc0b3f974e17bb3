"""GPU: spmv_hip_bicgstab, the BiCGStab solve that stays on the device (include/spmv_hip.h).

The yardstick is the host model of tests/bicgstab_cases.py -- a numpy restatement of the header's arithmetic contract -- driven by the SAME
handle's spmv(), so x, rr, bb and the history are compared BIT FOR BIT: no tolerance appears except the true-residual bound
||b - A x|| / ||b|| <= 10 rtol that tests/test_bicgstab_host.py shows the model alone to meet.  The bodies that the solvers share are in
tests/solve_harness.py."""
import functools

import numpy as np
import pytest

import bicgstab_cases as bc
import solve_harness as sh
from solve_harness import DEV, DTYPES, METHODS, SIZES, handle, same_bits
from spmv_amd import api

pytestmark = pytest.mark.gpu

ROW = sh.ROWS["bicgstab"]
solve = functools.partial(sh.solve, ROW)
check_same_end = functools.partial(sh.check_same_end, ROW)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return sh.library()


# ----------------------------------------------------------------------------- 1. bits against the model
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", SIZES)
def test_bits_against_the_model(m, dtype):
    sh.bits_against_the_model(ROW, m, dtype)


# ----------------------------------------------------------------------------- 2. every method
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_every_method_has_the_bits_of_the_model_on_its_own_spmv(method, dtype):
    sh.every_method(ROW, method, dtype)


# ----------------------------------------------------------------------------- 3. convergence
@pytest.mark.parametrize("name,dtype,rtol", [("upwind32", np.float64, 1e-8), ("nonsym_dominant4096", np.float32, 1e-3)])
def test_convergence_with_the_models_iteration_count(name, dtype, rtol):
    sh.convergence(ROW, name, dtype, rtol)


def test_jacobi_needs_fewer_iterations_on_the_scaled_stencil():
    csr = bc.scaled_upwind(16, 3)
    b = bc.rhs(csr.m, np.float64)
    with handle(csr) as h:
        _, plain = solve(h, b, rtol=1e-8, max_iterations=5000, check_every=64)
        xj, jacobi = solve(h, b, rtol=1e-8, max_iterations=5000, dinv=1.0 / bc.diagonal(csr))
    print(f"scaled_upwind(16, 3): {plain['iterations']} iterations without, {jacobi['iterations']} with Jacobi")
    assert plain["status"] == jacobi["status"] == bc.CONVERGED
    assert jacobi["iterations"] < plain["iterations"]
    assert bc.true_residual(csr, b, xj) <= 1e-7             # a right preconditioner: x solves the original system


# ----------------------------------------------------------------------------- 4. check_every
@pytest.mark.parametrize("dtype", DTYPES)
def test_check_every_changes_nothing(dtype):
    sh.check_every_changes_nothing(ROW, dtype)


# ----------------------------------------------------------------------------- 5. the early ends
@pytest.mark.parametrize("dtype", DTYPES)
def test_breakdown_half_step_nonfinite_and_zero_rhs(dtype):
    sk = bc.skew(1025, dtype)
    ones = np.ones(sk.m, dtype=dtype)
    with handle(sk) as h:
        model = ROW.model(h, ones, max_iterations=9)
        assert (model["status"], model["iterations"]) == (bc.BREAKDOWN, 0)
        for every in (1, 0):
            x, res = solve(h, ones, rtol=0.0, max_iterations=9, check_every=every)
            assert res["status_name"] == "breakdown" and np.isfinite(x).all()
            check_same_end(model, x, res)
    for m in (1, 1025):
        two = bc.twice_identity(m, dtype)
        b = bc.rhs(m, dtype, 2)
        with handle(two) as h:
            model = ROW.model(h, b, rtol=0.0, max_iterations=9)
            assert (model["status"], model["iterations"]) == (bc.CONVERGED, 1) and model["history"][1] == 0.0
            for every in (1, 0):
                x, res = solve(h, b, rtol=0.0, max_iterations=9, check_every=every)
                check_same_end(model, x, res)
            x, res = solve(h, b, rtol=0.0, max_iterations=9, dinv=np.full(m, 0.25, dtype=dtype))   # A Dinv = I / 2: the half step again
            check_same_end(ROW.model(h, b, dinv=np.full(m, 0.25, dtype=dtype), rtol=0.0, max_iterations=9), x, res)
            assert (res["status"], res["iterations"], res["rr"]) == (bc.CONVERGED, 1, 0.0)
    csr = bc.tri_ns(1025, dtype)
    b = bc.rhs(csr.m, dtype, 3)
    with handle(csr) as h:
        bad = b.copy()
        bad[700] = np.nan
        model = ROW.model(h, bad, rtol=1e-6, max_iterations=20)
        _, res = solve(h, bad, rtol=1e-6, max_iterations=20)
        assert res["status"] == bc.NONFINITE and res["status_name"] == "nonfinite" and res["iterations"] <= 1
        assert (res["status"], res["iterations"]) == (model["status"], model["iterations"])
        # a NaN that only the first multiply brings in: x0 with a NaN and a finite B
        _, res = solve(h, b, bad, rtol=1e-6, max_iterations=20)
        assert res["status"] == bc.NONFINITE and res["iterations"] == 0
        for x0 in (None, b):
            model = ROW.model(h, np.zeros_like(b), x0=x0, rtol=1e-6, max_iterations=20)
            x, res = solve(h, np.zeros_like(b), x0, rtol=1e-6, max_iterations=20)
            assert sh.converged_at_zero(res)
            assert not x.any() and same_bits(res["history"], np.zeros(1))
            check_same_end(model, x, res)


# ----------------------------------------------------------------------------- 6. pointers
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1025, 70001])
def test_host_device_and_unaligned_pointers_give_the_same_bits(m, dtype):
    rng = np.random.default_rng(m + 1)
    b, guess, jac = bc.rhs(m, dtype, 4), rng.uniform(-1, 1, m).astype(dtype), rng.uniform(0.5, 1.5, m).astype(dtype)
    sh.pointers_give_the_same_bits(ROW, bc.tri_ns(m, dtype), b, guess, dict(rtol=0.0, max_iterations=6), lambda res: res["iterations"] == 6, dinv=jac)


# ----------------------------------------------------------------------------- 7. handle rules
def test_argument_errors_leave_x_untouched(_lib):
    sh.argument_errors(ROW, _lib, bc.tri_ns(300))


def test_m_zero_is_converged():
    sh.m_zero_is_converged(ROW)


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_spmv_and_timer(dtype):
    import torch
    csr = bc.upwind(48, dtype)
    b = bc.rhs(csr.m, dtype, 5)
    item = np.dtype(dtype).itemsize
    with handle(csr) as h:
        fresh = h.info()["device_bytes"]
        y0 = h.spmv(b, np.empty_like(b))                                           # host vectors: spmv()'s own staging buffers appear here
        before = h.info()["device_bytes"]
        bd = torch.from_numpy(b).to(DEV)
        xd, res = h.bicgstab(bd, rtol=1e-6, max_iterations=300)                   # device operands: no staging buffer is added
        assert res["status"] == bc.CONVERGED and xd.device.type == "cuda"
        grown = h.info()["device_bytes"] - before
        assert grown == ROW.workspace(csr.m, item)
        x2, res2 = h.bicgstab(bd, rtol=1e-6, max_iterations=300)
        assert h.info()["device_bytes"] == before + grown and same_bits(x2.cpu().numpy(), xd.cpu().numpy()) and res2 == res
        mean, runs = ROW.timer(h.h, bd, xd, 10, warmup=1, iters=3)
        assert mean > 0 and runs.shape == (3,) and (runs > 0).all()
        assert h.info()["device_bytes"] == before + grown
        xc = torch.empty_like(bd)
        _, cres = h.cg(bd, xc, rtol=1e-6, max_iterations=5)                        # spmv_hip_cg's workspace is its own, neither shared nor grown
        both = h.info()["device_bytes"]
        assert both - (before + grown) == sh.ROWS["cg"].workspace(csr.m, item)
        x3, res3 = h.bicgstab(bd, rtol=1e-6, max_iterations=300)                   # ... and the two solvers do not disturb each other
        assert h.info()["device_bytes"] == both and same_bits(x3.cpu().numpy(), x2.cpu().numpy()) and res3 == res
        assert same_bits(h.spmv(b, np.empty_like(b)), y0)                          # spmv() computes what it did before the solves
        # copies of the CSR arrays: spmv() re-inspects, which frees both workspaces with everything else on the device and leaves what
        # `before` saw; the next solve allocates the workspace again
        rp, ci, va = csr.rowptr.copy(), csr.colidx.copy(), csr.val.copy()
        y1 = np.empty_like(b)
        api.spmv(h.h, csr.m, rp, ci, va, b, y1)
        shrunk = h.info()["device_bytes"]
        print(f"device_bytes: fresh {fresh}, before {before}, with the workspace {before + grown}, with cg's {both}, re-inspected {shrunk}")
        assert same_bits(y1, y0) and shrunk == before
        x4 = torch.empty_like(bd)
        _, res4 = api.bicgstab(h.h, csr.m, rp, ci, va, bd, x4, rtol=1e-6, max_iterations=300)
        assert h.info()["device_bytes"] == before + grown and same_bits(x4.cpu().numpy(), x2.cpu().numpy()) and res4 == res
    with handle(csr) as h:                                                          # destroyed and created again: nothing is carried over
        assert h.info()["device_bytes"] == fresh


def test_a_reordered_handle_solves_the_permuted_system():
    sh.a_reordered_handle_solves_the_permuted_system(ROW)
