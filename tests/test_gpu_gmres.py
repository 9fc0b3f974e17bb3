"""GPU: spmv_hip_gmres, the restarted GMRES solve that stays on the device (include/spmv_hip.h).

The yardstick is the host model of tests/gmres_cases.py -- a numpy restatement of the header's arithmetic contract -- driven by the SAME
handle's spmv(), so x, rr, bb and the history are compared BIT FOR BIT.  The one tolerance is the bound on true <r,r> / rr that
tests/test_gmres_host.py measures on the model alone (gmres_cases.RATIO_BOUND).  The bodies that the solvers share are in
tests/solve_harness.py."""
import functools

import numpy as np
import pytest

import cg_cases as cgc
import gmres_cases as gc
import solve_harness as sh
from solve_harness import BIG, CANARY, DEV, DTYPES, E_ARG, METHODS, handle, same_bits
from spmv_amd import api

pytestmark = pytest.mark.gpu

ROW = sh.ROWS["gmres"]
G = gc.GROUP
SIZES = sh.SIZES[:-1]            # the dot's edges; BIG has a test of its own
# a group boundary of the multi-dot kernel (G, G + 1) and the maximum
RESTARTS = [1, 2, 3, G, G + 1, gc.RESTART_MAX]
check_same_end = functools.partial(sh.check_same_end, ROW)
check_against = functools.partial(sh.check_against, ROW)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return sh.library()


def solve(h, b, restart, x0=None, **kw):
    return sh.solve(ROW, h, b, x0, restart=restart, **kw)


def model_of(h, b, restart, **kw):
    return ROW.model(h, b, restart, **kw)


def budgets(restart):
    return sorted({0, 1, restart - 1, restart, restart + 1, 2 * restart + 1})


# ----------------------------------------------------------------------------- 0. the square root
def test_the_device_square_root_is_correctly_rounded():
    """about 2^20 fp64 inputs through gmres_sqrt_kernel (spmv_solve.hip's flags), bit for bit against np.sqrt: random mantissas over the whole
    exponent range, exact squares and their two neighbours, subnormals, and the special values"""
    import torch
    rng = np.random.default_rng(7)
    n = 1 << 18
    anywhere = (rng.integers(0, 1 << 52, n, dtype=np.uint64) | (rng.integers(1, 0x7ff, n, dtype=np.uint64) << np.uint64(52))).view(np.float64)
    roots = rng.integers(1, 1 << 26, n).astype(np.float64) * 2.0 ** rng.integers(-400, 400, n)       # 26-bit mantissas: the squares are exact
    squares = roots * roots
    subnormal = rng.integers(1, 1 << 52, n, dtype=np.uint64).view(np.float64)
    special = np.array([0.0, -0.0, np.inf, 1.0, 2.0, 4.0, np.finfo(np.float64).max, np.finfo(np.float64).tiny, 5e-324])
    values = np.concatenate([anywhere, squares, np.nextafter(squares, np.inf), np.nextafter(squares, 0.0), subnormal, special])
    assert np.isfinite(squares).all() and (squares > 0).all()
    dev = torch.from_numpy(values).to(DEV)
    got = api.gmres_device_sqrt(dev, torch.empty_like(dev)).cpu().numpy()
    want = np.sqrt(values)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    print(f"{values.size} inputs, {bad.size} differ" + (f"; first: sqrt({values[bad[0]]!r}) = {got[bad[0]]!r}, correctly rounded {want[bad[0]]!r}" if bad.size else ""))
    assert bad.size == 0
    assert same_bits(got[n:2 * n], roots)


# ----------------------------------------------------------------------------- 1. bits against the model
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("restart", RESTARTS)
@pytest.mark.parametrize("m", SIZES)
def test_bits_against_the_model(m, restart, dtype):
    csr = gc.tri_ns(m, dtype)
    rng = np.random.default_rng(m)
    b, guess = gc.rhs(m, dtype), rng.uniform(-1, 1, m).astype(dtype)
    jac = rng.uniform(0.5, 1.5, m).astype(dtype)
    ones = np.ones(m, dtype=dtype)
    top = 2 * restart + 1
    with handle(csr) as h:
        plain = model_of(h, b, restart, max_iterations=top)
        pre = model_of(h, b, restart, x0=guess, dinv=jac, max_iterations=top)
        for k in budgets(restart):
            x_none, r_none = solve(h, b, restart, rtol=0.0, max_iterations=k)
            check_against(plain, k, x_none, r_none)
            x_ones, r_ones = solve(h, b, restart, rtol=0.0, max_iterations=k, dinv=ones)
            assert same_bits(x_ones, x_none) and same_bits(r_ones["history"], r_none["history"]) and r_ones["iterations"] == r_none["iterations"]
            x_jac, r_jac = solve(h, b, restart, guess, rtol=0.0, max_iterations=k, dinv=jac)
            check_against(pre, k, x_jac, r_jac)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("restart", [3, G + 1])
def test_bits_with_empty_workgroups(restart, dtype):
    csr = gc.tri_ns(BIG, dtype)
    rng = np.random.default_rng(restart)
    b, guess, jac = gc.rhs(BIG, dtype), rng.uniform(-1, 1, BIG).astype(dtype), rng.uniform(0.5, 1.5, BIG).astype(dtype)
    with handle(csr) as h:
        pre = model_of(h, b, restart, x0=guess, dinv=jac, max_iterations=restart + 1)
        for k in (0, restart - 1, restart + 1):
            x, res = solve(h, b, restart, guess, rtol=0.0, max_iterations=k, dinv=jac)
            check_against(pre, k, x, res)


# ----------------------------------------------------------------------------- 2. every method
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_every_method_has_the_bits_of_the_model_on_its_own_spmv(method, dtype):
    sh.every_method(ROW, method, dtype, restart=5)


# ----------------------------------------------------------------------------- 3. convergence
@pytest.mark.parametrize("restart", [10, 30])
@pytest.mark.parametrize("name,dtype,rtol", [("upwind32", np.float64, 1e-8), ("nonsym_dominant4096", np.float32, 1e-3)])
def test_convergence_with_the_models_iteration_count(name, dtype, rtol, restart):
    csr = gc.upwind(32, dtype) if name == "upwind32" else gc.nonsym_dominant(4096, dtype)
    b = gc.rhs(csr.m, dtype)
    with handle(csr) as h:
        model = model_of(h, b, restart, rtol=rtol, max_iterations=400)
        x, res = solve(h, b, restart, rtol=rtol, max_iterations=400)
    assert model["status"] == gc.CONVERGED
    assert res["status_name"] == "converged"
    check_same_end(model, x, res)
    hist = res["history"]
    assert all(hist[k] <= hist[k - 1] for k in range(1, len(hist)) if (k - 1) % restart)     # the estimate never rises inside a cycle
    ratio = gc.true_rr(csr, b, x) / res["rr"]
    print(f"{name} restart {restart}: {res['iterations']} iterations, true <r,r> / rr = {ratio:.7f}")
    assert ratio <= gc.RATIO_BOUND


def test_jacobi_is_a_right_preconditioner():
    csr = gc.scaled_upwind(16, 3)
    b = gc.rhs(csr.m, np.float64)
    with handle(csr) as h:
        xj, jacobi = solve(h, b, 30, rtol=1e-8, max_iterations=2000, dinv=1.0 / gc.diagonal(csr))
    assert jacobi["status"] == gc.CONVERGED
    assert gc.true_residual(csr, b, xj) <= 1e-7             # x solves the original system


# ----------------------------------------------------------------------------- 4. check_every
@pytest.mark.parametrize("dtype", DTYPES)
def test_check_every_changes_nothing(dtype):
    csr = gc.upwind(32, dtype)
    b = gc.rhs(csr.m, dtype, 2)
    rtol = 1e-8 if dtype == np.float64 else 1e-4
    restart = 5
    with handle(csr) as h:
        model = model_of(h, b, restart, rtol=rtol, max_iterations=600)
        assert model["status"] == gc.CONVERGED and 2 * restart < model["iterations"] < 600
        for every in (1, 3, restart, 64, 0):
            x, res = solve(h, b, restart, rtol=rtol, max_iterations=600, check_every=every)
            # the early exit really exits: nothing is applied behind the step that met the test, however many were enqueued
            check_same_end(model, x, res)
        for short in (model["iterations"] // 2 // restart * restart + 2, model["iterations"] // 2 // restart * restart):   # in a cycle; on a restart
            for every in (1, 3, restart, 64):
                x, res = solve(h, b, restart, rtol=rtol, max_iterations=short, check_every=every)
                assert res["status_name"] == "max_iterations"
                check_against(model, short, x, res)


# ----------------------------------------------------------------------------- 5. every end
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_end(dtype):
    def both(csr, b, restart, x0=None, **kw):
        with handle(csr) as h:
            model = model_of(h, b, restart, x0=x0, **kw)
            for every in (1, 0):
                x, res = solve(h, b, restart, x0, check_every=every, **kw)
                check_same_end(model, x, res)
        return model, x, res

    tri = gc.tri_ns(1025, dtype)
    b = gc.rhs(tri.m, dtype, 3)
    # converged at the start: the guess is good enough
    model, x, res = both(tri, b, 4, x0=np.zeros_like(b), rtol=1.0, max_iterations=9)
    assert (model["end"], res["iterations"]) == ("begin:converged", 0) and not x.any()
    # bb = 0
    for x0 in (None, b):
        model, x, res = both(tri, np.zeros_like(b), 4, x0=x0, rtol=1e-6, max_iterations=9)
        assert (model["end"], res["rr"], res["bb"]) == ("begin:bb_zero", 0.0, 0.0) and not x.any()
    # the lucky case
    for m in (4, 1024):
        model, x, res = both(gc.two_values(m, dtype), np.ones(m, dtype=dtype), 5, max_iterations=9)
        assert (model["end"], res["status"], res["iterations"], res["rr"]) == ("rotate:converged", gc.CONVERGED, 2, 0.0)
    # BREAKDOWN: the zero matrix at step 1 (x stays the guess); a singular matrix at step 2 of a cycle of 5
    model, x, res = both(gc.zero_matrix(1025, dtype), b, 5, x0=b, max_iterations=9)
    assert (model["end"], res["status_name"], res["iterations"]) == ("rotate:d_zero", "breakdown", 0) and same_bits(x, b)
    e0 = np.zeros(1025, dtype=dtype)
    e0[0] = 1
    model, x, res = both(gc.shift(1025, dtype), e0, 5, max_iterations=9)
    assert (model["end"], res["status"], res["iterations"]) == ("rotate:d_zero", gc.BREAKDOWN, 1) and np.isfinite(x).all()
    model, x, res = both(gc.half_singular(1024, dtype), np.ones(1024, dtype=dtype), 5, max_iterations=9)
    assert (model["end"], res["status"], res["iterations"]) == ("rotate:d_zero", gc.BREAKDOWN, 1) and np.isfinite(x).all()
    # NONFINITE: a NaN in B; an infinity that A's values bring in at step 2
    bad = b.copy()
    bad[700] = np.nan
    model, x, res = both(tri, bad, 4, rtol=1e-6, max_iterations=9)
    assert (model["end"], res["status_name"], res["iterations"]) == ("begin:nonfinite", "nonfinite", 0)
    model, x, res = both(gc.overflowing(1025, dtype), e0, 5, max_iterations=9)
    assert (model["end"], res["status"], res["iterations"]) == ("rotate:nonfinite", gc.NONFINITE, 1) and np.isfinite(x).all()
    # MAX_ITERATIONS in the middle of a cycle: x holds the columns of the unfinished cycle
    model, x, res = both(tri, b, 5, max_iterations=7)
    assert (model["end"], res["status_name"], res["iterations"]) == ("budget", "max_iterations", 7)
    assert not same_bits(x, model["iterates"][5])


def test_m_zero_is_converged():
    sh.m_zero_is_converged(ROW, restart=5)


# ----------------------------------------------------------------------------- 6. pointers
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1025, 70001])
def test_host_device_and_unaligned_pointers_give_the_same_bits(m, dtype):
    rng = np.random.default_rng(m + 1)
    b, guess, jac = gc.rhs(m, dtype, 4), rng.uniform(-1, 1, m).astype(dtype), rng.uniform(0.5, 1.5, m).astype(dtype)
    sh.pointers_give_the_same_bits(ROW, gc.tri_ns(m, dtype), b, guess, dict(restart=3, rtol=0.0, max_iterations=7), lambda res: res["iterations"] == 7, dinv=jac,
                                   shift_dinv=True)


# ----------------------------------------------------------------------------- 7. handle rules
def test_argument_errors_leave_x_untouched(_lib):
    def restarts(call, options, res, h):
        for restart in (0, -1, gc.RESTART_MAX + 1):
            assert call(h.h, options(), res, restart=restart) == E_ARG, restart
    sh.argument_errors(ROW, _lib, gc.tri_ns(300), more=restarts, good=dict(restart=gc.RESTART_MAX))


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_and_timer(dtype):
    import torch
    csr = gc.upwind(48, dtype)
    b = gc.rhs(csr.m, dtype, 5)
    item = np.dtype(dtype).itemsize
    with handle(csr) as h:
        fresh = h.info()["device_bytes"]
        y0 = h.spmv(b, np.empty_like(b))                                           # host vectors: spmv()'s own staging buffers appear here
        before = h.info()["device_bytes"]
        bd = torch.from_numpy(b).to(DEV)
        xd, res = h.gmres(bd, restart=5, rtol=1e-6, max_iterations=300)            # device operands: no staging buffer is added
        assert res["status"] == gc.CONVERGED and xd.device.type == "cuda"
        small = ROW.workspace(csr.m, item, 5)
        assert h.info()["device_bytes"] - before == small
        x2, res2 = h.gmres(bd, restart=3, rtol=1e-6, max_iterations=300)           # a smaller restart runs in the workspace that is there
        assert h.info()["device_bytes"] == before + small and res2["iterations"] > 0
        x3, res3 = h.gmres(bd, restart=9, rtol=1e-6, max_iterations=300)           # a larger one allocates it anew
        large = ROW.workspace(csr.m, item, 9)
        assert h.info()["device_bytes"] == before + large and res3["iterations"] > 0
        x4, res4 = h.gmres(bd, restart=5, rtol=1e-6, max_iterations=300)           # ... and the bits do not depend on the workspace's size
        assert same_bits(x4.cpu().numpy(), xd.cpu().numpy()) and res4 == res
        mean, runs = ROW.timer(h.h, bd, xd, 12, restart=5, warmup=1, iters=3)
        assert mean > 0 and runs.shape == (3,) and (runs > 0).all()
        assert h.info()["device_bytes"] == before + large
        xc = torch.empty_like(bd)
        h.bicgstab(bd, xc, rtol=1e-6, max_iterations=5)                            # the other solvers' workspaces are their own
        assert h.info()["device_bytes"] == before + large + sh.ROWS["bicgstab"].workspace(csr.m, item)
        assert same_bits(h.spmv(b, np.empty_like(b)), y0)                          # spmv() computes what it did before the solves
        # copies of the CSR arrays: spmv() re-inspects, which frees every workspace with everything else on the device (what clear and destroy
        # do as well) and leaves what `before` saw; the next solve allocates the workspace again, for the restart it is called with
        rp, ci, va = csr.rowptr.copy(), csr.colidx.copy(), csr.val.copy()
        y1 = np.empty_like(b)
        api.spmv(h.h, csr.m, rp, ci, va, b, y1)
        assert same_bits(y1, y0) and h.info()["device_bytes"] == before
        x5 = torch.empty_like(bd)
        _, res5 = api.gmres(h.h, csr.m, rp, ci, va, bd, x5, 5, rtol=1e-6, max_iterations=300)
        assert h.info()["device_bytes"] == before + small and same_bits(x5.cpu().numpy(), x4.cpu().numpy()) and res5 == res      # the timer has written into xd
    with handle(csr) as h:                                                          # destroyed and created again: nothing is carried over
        assert h.info()["device_bytes"] == fresh


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_company(dtype):
    """cg, gmres, bicgstab, gmres with a larger restart, cg on ONE handle: each call has the bits it has on a fresh handle"""
    csr = cgc.lap2d(24, dtype)
    b = gc.rhs(csr.m, dtype, 6)
    calls = [("cg", {}), ("gmres", dict(restart=4)), ("bicgstab", {}), ("gmres", dict(restart=11)), ("cg", {})]

    def run(h, name, kw):
        x = np.full(b.size, CANARY, dtype=dtype)
        x, res, hist = getattr(h, name)(b, x, rtol=0.0, max_iterations=13, history=True, **kw)
        return x, res, hist

    with handle(csr) as shared:
        for name, kw in calls:
            x, res, hist = run(shared, name, kw)
            with handle(csr) as alone:
                x1, res1, hist1 = run(alone, name, kw)
            assert same_bits(x, x1) and res == res1 and same_bits(hist, hist1), (name, kw)
            assert res["iterations"] == 13


def test_a_reordered_handle_solves_the_permuted_system():
    sh.a_reordered_handle_solves_the_permuted_system(ROW, restart=10)
