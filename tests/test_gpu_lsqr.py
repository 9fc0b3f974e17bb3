"""GPU: spmv_hip_lsqr, the least-squares solve for a matrix of any shape that stays on the device (include/spmv_hip.h).

The yardstick is the host model of tests/lsqr_cases.py -- a numpy restatement of the header's arithmetic contract -- driven by the SAME
handle's spmv() and spmv_transpose(), so x, rr, bb, ar, anorm and the history are compared BIT FOR BIT.  No tolerance enters.
The bodies that the solvers share are in tests/solve_harness.py."""
import functools

import numpy as np
import pytest

import cg_cases as cgc
import lsqr_cases as lc
import solve_harness as sh
from solve_harness import CANARY, DEV, DTYPES, E_ARG, M, handle, same_bits
from spmv_amd import api, synth

pytestmark = pytest.mark.gpu

ROW = sh.ROWS["lsqr"]
# (m, n) -> the model's end without and with (an initial guess and damp = 0.5), under rtol = ls_tol = TOL: a consistent system converges (wide,
# undamped), an inconsistent one meets the normal-equations test once its Krylov space is exhausted, the largest runs out of budget
SHAPES = {
    (1, 1): ("step:converged", "step:least_squares"),                  # smallest
    (5, 3): ("step:least_squares", "step:least_squares"),              # tall
    (3, 5): ("step:converged", "step:least_squares"),                  # wide
    (1025, 3): ("step:least_squares", "step:least_squares"),           # the two dots' geometries differ: P(m) = 2, P(n) = 1
    (3, 1025): ("step:converged", "step:least_squares"),               # ... P(m) = 1, P(n) = 2
    (4099, 1030): ("budget", "budget"),                                # both past one workgroup, neither a multiple of 4
}
BUDGET = 6
BIG = (2 ** 20 + 5, 7)                                                  # P(m) = 1024, L = 2048: a second step per thread, empty workgroups


def tol_of(dtype):
    return 1e-9 if dtype == np.float64 else 1e-4


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return sh.library()


model_of = ROW.model
solve = functools.partial(sh.solve, ROW)
check_same_end = functools.partial(sh.check_same_end, ROW)
check_against = functools.partial(sh.check_against, ROW)


# ----------------------------------------------------------------------------- 1. bits against the model
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bits_against_the_model(shape, dtype):
    """every budget up to the model's end, damp = 0 from x = 0 and damp > 0 from a guess, host pointers, two runs"""
    m, n = shape
    csr = lc.sparse_rect(m, n, dtype)
    empty_col = n - 2 if n >= 3 else None
    assert m < 5 or np.diff(csr.rowptr)[[1, m - 1]].tolist() == [0, 0]
    assert empty_col is None or not (csr.colidx == empty_col).any()
    b, guess, tol = lc.rhs(m, dtype, 1), lc.rhs(n, dtype, 2), tol_of(dtype)
    with handle(csr) as h:
        for x0, damp, end in ((None, 0.0, SHAPES[shape][0]), (guess, 0.5, SHAPES[shape][1])):
            kw = dict(damp=damp, rtol=tol, ls_tol=tol)
            model = model_of(h, b, x0=x0, max_iterations=BUDGET, **kw)
            print(f"{shape} {np.dtype(dtype).name} damp {damp}: {model['end']} after {model['iterations']} iterations, rr {model['rr']:.3e} ar {model['ar']:.3e} anorm {model['anorm']:.3e}")
            assert model["end"] == end and model["iterations"] >= 1
            for k in range(min(model["iterations"] + 1, BUDGET) + 1):              # one past an end that a test brought, never past the model's budget
                x, res = solve(h, b, x0, max_iterations=k, **kw)
                check_against(model, k, x, res)
                if x0 is None and empty_col is not None:
                    assert x[empty_col] == 0 and not np.signbit(x[empty_col])
            again, res2 = solve(h, b, x0, max_iterations=k, **kw)
            assert same_bits(again, x) and same_bits(res2.pop("history"), res.pop("history")) and res2 == res


@pytest.mark.parametrize("dtype", DTYPES)
def test_bits_with_a_second_step_per_thread(dtype):
    m, n = BIG
    csr = lc.two_per_row(m, n, dtype)
    b = lc.rhs(m, dtype, 1)
    assert cgc.geometry(m) == (1024, 2048) and cgc.geometry(n) == (1, 1024)
    with handle(csr) as h:
        model = model_of(h, b, max_iterations=3)                                       # every tolerance 0: seven well-separated columns are fitted at once
        assert (model["end"], model["iterations"]) == ("budget", 3)
        x, res = solve(h, b, rtol=0.0, ls_tol=0.0, max_iterations=3)
        check_same_end(model, x, res)


# ----------------------------------------------------------------------------- 2. every method
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", [M.Method_Parallel, M.Method_Serial], ids=lambda mth: mth.name)
def test_a_method_has_the_bits_of_the_model_on_its_own_multiplies(method, dtype):
    csr = lc.sparse_rect(4099, 1030, dtype, per_row=5, seed=3)
    b = lc.rhs(csr.m, dtype, 4)
    with handle(csr, method) as h:
        model = model_of(h, b, damp=0.25, max_iterations=7)
        x, res = solve(h, b, damp=0.25, rtol=0.0, ls_tol=0.0, max_iterations=7)
        assert (model["end"], res["iterations"]) == ("budget", 7)
        check_same_end(model, x, res)


# ----------------------------------------------------------------------------- 3. check_every
@pytest.mark.parametrize("dtype", DTYPES)
def test_check_every_changes_nothing(dtype):
    csr = lc.sparse_rect(1025, 40, dtype, per_row=4, seed=5)
    b, tol = lc.rhs(csr.m, dtype, 5), tol_of(dtype)
    with handle(csr) as h:
        model = model_of(h, b, ls_tol=tol, max_iterations=200)
        assert model["end"] == "step:least_squares" and 3 < model["iterations"] < 200 and model["iterations"] % 8   # the end falls inside a default batch
        for every in (1, 3, 0, 64):
            # the early exit really exits: nothing is applied behind the step that met the test, however many were enqueued
            x, res = solve(h, b, rtol=0.0, ls_tol=tol, max_iterations=200, check_every=every)
            check_same_end(model, x, res)
            assert res["status_name"] == "least_squares"
        short = model["iterations"] // 2
        for every in (1, 3, 0):
            x, res = solve(h, b, rtol=0.0, ls_tol=tol, max_iterations=short, check_every=every)
            assert res["status_name"] == "max_iterations"
            check_against(model, short, x, res)


# ----------------------------------------------------------------------------- 4. every end
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_end(dtype):
    """CONVERGED on a consistent system, LEAST_SQUARES on an inconsistent one and at 0 iterations, the beta == 0 end, bb == 0, MAX_ITERATIONS,
    NONFINITE from a NaN in B and from the overflows that the dtype can reach: lsqr_cases.end_cases, the table that the host test holds the
    model against"""
    for name, (csr, b, kw, end) in lc.end_cases(dtype).items():
        x0 = kw.get("x0")
        rest = {key: v for key, v in kw.items() if key != "x0"}
        rest.setdefault("rtol", 0.0)
        rest.setdefault("ls_tol", 0.0)
        with handle(csr) as h:
            model = model_of(h, b, **kw)
            assert model["end"] == end, name
            for every in (1, 0):
                x, res = solve(h, b, x0, check_every=every, **rest)
                check_same_end(model, x, res)
        if end in ("step:converged", "step:least_squares", "step:nonfinite"):
            assert res["iterations"] >= 1, name
        if name == "zero_b":
            assert (res["rr"], res["bb"]) == (0.0, 0.0) and not x.any()
        if name == "orthogonal_b":
            assert (res["status_name"], res["iterations"], res["ar"]) == ("least_squares", 0, 0.0)
        if name == "beta_zero":
            assert (res["status_name"], res["iterations"], res["rr"], x.tolist()) == ("converged", 1, 0.0, [3.0, 0.0, 0.0, 0.0])
        if name == "nan_in_b":
            assert res["status_name"] == "nonfinite" and not x.any()


def test_no_rows_no_entries():
    sh.m_zero_is_converged(ROW)
    with handle(sh.empty_csr(n=5)) as h:
        x, res = h.lsqr(np.zeros(0), np.full(5, CANARY), max_iterations=5)
    assert sh.converged_at_zero(res) and not x.any()
    nnz0 = synth.CSR(7, 5, np.zeros(8, np.int32), np.zeros(0, np.int32), np.zeros(0))
    b = lc.rhs(7, np.float64)
    with handle(nnz0) as h:
        model = model_of(h, b, max_iterations=5)
        x, res = solve(h, b, max_iterations=5)
    assert model["end"] == "first:alpha_zero" and not x.any()
    check_same_end(model, x, res)


# ----------------------------------------------------------------------------- 5. pointers
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_device_and_unaligned_pointers_give_the_same_bits(dtype):
    import torch
    m, n = 4099, 1030
    b, guess = lc.rhs(m, dtype, 6), lc.rhs(n, dtype, 7)
    kw = dict(damp=0.125, rtol=0.0, ls_tol=0.0, max_iterations=5)

    def x_allocated_like_b(h):
        xa, _ = h.lsqr(torch.from_numpy(b).to(DEV), **kw)
        assert xa.shape == (n,) and xa.device.type == "cuda"
    sh.pointers_give_the_same_bits(ROW, lc.sparse_rect(m, n, dtype, seed=6), b, guess, kw, lambda res: res["iterations"] == 5, last=x_allocated_like_b)


# ----------------------------------------------------------------------------- 6. the values change
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_values_reaches_both_multiplies(dtype):
    csr = lc.sparse_rect(1025, 40, dtype, per_row=4, seed=8)
    b = lc.rhs(csr.m, dtype, 8)
    new = (csr.val * np.linspace(0.5, 1.5, csr.val.size)).astype(dtype)
    with handle(csr) as h:
        x_old, res_old = solve(h, b, rtol=0.0, ls_tol=0.0, max_iterations=6)
        h.update_values(new)
        x_new, res_new = solve(h, b, rtol=0.0, ls_tol=0.0, max_iterations=6)          # before the model's spmv_transpose() could refresh anything
        model = model_of(h, b, max_iterations=6)
        check_same_end(model, x_new, res_new)
        assert not same_bits(x_new, x_old)
    changed = synth.CSR(csr.m, csr.n, csr.rowptr, csr.colidx, new)
    with handle(changed) as fresh:                                                       # ... and what a handle created with the new values computes
        x_fresh, res_fresh = solve(fresh, b, rtol=0.0, ls_tol=0.0, max_iterations=6)
    assert same_bits(x_new, x_fresh) and same_bits(res_new["history"], res_fresh["history"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_has_the_same_bits_before_and_after_an_lsqr_call(dtype):
    csr = cgc.lap2d(24, dtype)
    b = cgc.rhs(csr.m, dtype, 6)

    def run_cg(h):
        x = np.full(b.size, CANARY, dtype=dtype)
        return h.cg(b, x, rtol=0.0, max_iterations=13, history=True)

    with handle(csr) as h:
        x1, res1, hist1 = run_cg(h)
        model = model_of(h, b, damp=0.5, max_iterations=9)
        x, res = solve(h, b, damp=0.5, rtol=0.0, ls_tol=0.0, max_iterations=9)
        check_same_end(model, x, res)
        assert res["iterations"] == 9
        x2, res2, hist2 = run_cg(h)
    assert same_bits(x1, x2) and res1 == res2 and same_bits(hist1, hist2) and res1["iterations"] == 13


# ----------------------------------------------------------------------------- 7. handle rules
def test_argument_errors_leave_x_untouched(_lib):
    nan = float("nan")
    bad = (dict(max_iterations=-1), dict(check_every=-1), dict(rtol=-1e-3), dict(atol=-1.0), dict(ls_tol=-1e-3), dict(damp=-0.5), dict(rtol=nan), dict(atol=nan),
           dict(ls_tol=nan), dict(damp=nan))

    def a_reordered_handle(call, options, res):
        square = cgc.dominant(4096)
        xs, bs = np.full(square.m, CANARY), cgc.rhs(square.m, np.float64)
        with handle(square, reorder=1) as h:
            assert h.index is not None
            assert call(h.h, options(), res, B=bs, X=xs, mat=square) == E_ARG
        assert (xs == CANARY).all()
    sh.argument_errors(ROW, _lib, lc.sparse_rect(300, 40), bad=bad, square=False, after=a_reordered_handle)


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_transpose_and_timer(dtype):
    """device_bytes rises by the transpose and the workspace at the first call, by nothing afterwards, and falls back when the matrix is
    inspected again; Method_Serial (CSR-scalar): no timed choice enters the transpose's size"""
    import torch
    csr = lc.sparse_rect(4099, 1030, dtype, seed=9)
    b = lc.rhs(csr.m, dtype, 9)
    item = np.dtype(dtype).itemsize
    ws = ROW.workspace(csr.m, csr.n, item)
    bd = torch.from_numpy(b).to(DEV)
    with handle(csr, M.Method_Serial) as h:
        before = h.info()["device_bytes"]
        assert api.prepare_transpose(h.h) == 0
        transpose = h.info()["device_bytes"] - before
        assert transpose > 0
        xd, res = h.lsqr(bd, rtol=0.0, ls_tol=0.0, max_iterations=4)                   # device operands: no staging buffer is added
        assert res["iterations"] == 4 and h.info()["device_bytes"] == before + transpose + ws
    with handle(csr, M.Method_Serial) as h:
        assert h.info()["device_bytes"] == before
        x1, res1 = h.lsqr(bd, rtol=0.0, ls_tol=0.0, max_iterations=4)                  # the first call builds the transpose itself
        assert h.info()["device_bytes"] == before + transpose + ws
        assert same_bits(x1.cpu().numpy(), xd.cpu().numpy()) and res1 == res
        x2, res2 = h.lsqr(bd, rtol=0.0, ls_tol=0.0, max_iterations=4)
        assert h.info()["device_bytes"] == before + transpose + ws and same_bits(x2.cpu().numpy(), x1.cpu().numpy())
        mean, runs = ROW.timer(h.h, bd, x2, 6, warmup=1, iters=3)
        assert mean > 0 and runs.shape == (3,) and (runs > 0).all()
        assert h.info()["device_bytes"] == before + transpose + ws
        xc = torch.empty(csr.n, dtype=bd.dtype, device=DEV)
        _, hist_res, hist = h.lsqr(bd, xc, rtol=0.0, ls_tol=0.0, max_iterations=4, history=True)
        assert h.info()["device_bytes"] == before + transpose + ws + 8 * 5 and same_bits(xc.cpu().numpy(), x1.cpu().numpy())
        # copies of the CSR arrays: spmv() re-inspects, which frees the workspace and the transpose with everything else on the device
        rp, ci, va = csr.rowptr.copy(), csr.colidx.copy(), csr.val.copy()
        yd = torch.empty(csr.m, dtype=bd.dtype, device=DEV)
        api.spmv(h.h, csr.m, rp, ci, va, torch.from_numpy(lc.rhs(csr.n, dtype)).to(DEV), yd)
        assert h.info()["device_bytes"] == before
        x3 = torch.empty(csr.n, dtype=bd.dtype, device=DEV)
        _, res3 = api.lsqr(h.h, csr.m, rp, ci, va, bd, x3, rtol=0.0, ls_tol=0.0, max_iterations=4)
        assert h.info()["device_bytes"] == before + transpose + ws and same_bits(x3.cpu().numpy(), x1.cpu().numpy()) and res3 == res
