"""GPU: spmv_hip_cg_mixed, fp64 solutions from fp32 conjugate-gradient iterations on a pair of handles (include/spmv_hip.h).

The yardstick is the host model of tests/cg_mixed_cases.py -- a numpy restatement of the header's arithmetic contract -- driven by the two
handles' OWN spmv(), so X, status, iterations, updates, rr, bb and the history are compared BIT FOR BIT; the only tolerance is the true-residual
bound ||b - A x|| / ||b|| <= 2 rtol that tests/test_cg_mixed_host.py shows the model alone to meet.  The bodies that the solvers share are in
tests/solve_harness.py; there a pair (hi, lo) stands where the other solvers have a handle."""
import ctypes as C

import numpy as np
import pytest

import cg_cases as cgc
import cg_mixed_cases as mix
import solve_harness as sh
from solve_harness import CANARY, DEV, E_ARG, E_NOSTATE, M, SIZES, handle, pair, same_bits
from spmv_amd import api

pytestmark = pytest.mark.gpu

ROW = sh.ROWS["cg_mixed"]
BUDGETS = [0, 1, 2, 5, 9]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return sh.library()


def solve(hi, lo, b, x0=None, **kw):
    return sh.solve(ROW, (hi, lo), b, x0, **kw)


def model_of(hi, lo, b, **kw):
    return ROW.model((hi, lo), b, **kw)


def check_against(model, x, res):
    sh.check_same_end(ROW, model, x, res)


# ----------------------------------------------------------------------------- 1. bits against the model, updates inside small budgets
@pytest.mark.parametrize("with_x0", [False, True])
@pytest.mark.parametrize("m", SIZES)
def test_bits_against_the_model(m, with_x0):
    csr = cgc.tri(m)
    rng = np.random.default_rng(m)
    b, guess = cgc.rhs(m, np.float64), rng.uniform(-1, 1, m)
    jac = rng.uniform(0.5, 1.5, m).astype(np.float32)
    x0 = guess if with_x0 else None
    kw = dict(rtol=0.0, update_every=2, update_drop=0.5)
    with pair(csr) as (hi, lo):
        seen = set()
        for k in BUDGETS:
            plain = model_of(hi, lo, b, x0=x0, max_iterations=k, **kw)
            pre = model_of(hi, lo, b, x0=x0, dinv=jac, max_iterations=k, **kw)
            seen.update(plain["segments"])
            x_none, r_none = solve(hi, lo, b, x0, max_iterations=k, **kw)
            check_against(plain, x_none, r_none)
            x_ones, r_ones = solve(hi, lo, b, x0, max_iterations=k, dinv=np.ones(m, dtype=np.float32), **kw)
            assert same_bits(x_ones, x_none) and same_bits(r_ones["history"], r_none["history"])
            assert {key: v for key, v in r_ones.items() if key != "history"} == {key: v for key, v in r_none.items() if key != "history"}
            x_jac, r_jac = solve(hi, lo, b, x0, max_iterations=k, dinv=jac, **kw)
            check_against(pre, x_jac, r_jac)
        if m >= 1023:                                  # updates fell inside the budgets and at their ends
            assert plain["updates"] >= 2 and "budget" in seen and ("every" in seen or "drop" in seen)


# ----------------------------------------------------------------------------- 2. a full solve
@pytest.fixture(scope="module")
def full_solve():
    """lap2d(32) to rtol 1e-12: the matrix, b, a pair of handles and the model's run on that pair's own multiplies, computed once"""
    csr = cgc.lap2d(32)
    b = cgc.rhs(csr.m, np.float64)
    with pair(csr) as (hi, lo):
        model = model_of(hi, lo, b, rtol=1e-12, max_iterations=1000)
        assert model["status"] == mix.CONVERGED and model["updates"] > 3
        yield csr, b, model, hi, lo


def test_full_solve_has_the_models_bits_and_an_fp64_residual(full_solve):
    csr, b, model, hi, lo = full_solve
    x, res = solve(hi, lo, b, rtol=1e-12, max_iterations=1000)
    check_against(model, x, res)
    assert res["status_name"] == "converged"
    true = cgc.true_residual(csr, b, x)
    print(f"lap2d(32): {res['iterations']} iterations, {res['updates']} updates, true residual {true:.3e}")
    assert true <= 2e-12


def test_check_every_changes_nothing(full_solve):
    csr, b, model, hi, lo = full_solve
    short = model["iterations"] // 2
    cut = model_of(hi, lo, b, rtol=1e-12, max_iterations=short)
    assert cut["status"] == mix.MAX_ITERATIONS
    for every in (1, 2, 3, 8, 64):
        # the early exit really exits: nothing is applied behind a segment's end or the solve's, however many iterations were enqueued
        x, res = solve(hi, lo, b, rtol=1e-12, max_iterations=1000, check_every=every)
        check_against(model, x, res)
        x, res = solve(hi, lo, b, rtol=1e-12, max_iterations=short, check_every=every)
        check_against(cut, x, res)
        assert res["status_name"] == "max_iterations"


# ----------------------------------------------------------------------------- 3. pointers
@pytest.mark.parametrize("m", [1025, 70001])
def test_host_device_and_unaligned_pointers_give_the_same_bits(m):
    import torch
    rng = np.random.default_rng(m + 1)
    b, guess, jac = cgc.rhs(m, np.float64, 4), rng.uniform(-1, 1, m), rng.uniform(0.5, 1.5, m).astype(np.float32)
    kw = dict(rtol=0.0, max_iterations=7, update_every=3)

    def host_b_device_x_host_dinv(h, x0, want):
        xd = torch.full((m,), CANARY, dtype=torch.float64, device=DEV) if x0 is None else torch.from_numpy(x0).to(DEV)
        h[0].cg_mixed(h[1], b, xd, x0=x0 is not None, dinv=jac, **kw)
        assert same_bits(xd.cpu().numpy(), want)
    sh.pointers_give_the_same_bits(ROW, cgc.tri(m), b, guess, kw, lambda res: res["updates"] >= 2, dinv=jac, shift_dinv=True, each=host_b_device_x_host_dinv)


# ----------------------------------------------------------------------------- 4. schedules
@pytest.mark.parametrize("method", [M.Method_Parallel, M.Method_SellCSigma, M.Method_CSR5SPMV])
def test_schedules_have_the_bits_of_the_model_on_their_own_spmv(method):
    csr = cgc.lap2d(32)
    b = cgc.rhs(csr.m, np.float64, 1)
    kw = dict(rtol=1e-12, max_iterations=40, update_every=6)
    with pair(csr, method=method) as (hi, lo):
        model = model_of(hi, lo, b, **kw)
        x, res = solve(hi, lo, b, **kw)
    assert model["updates"] >= 3
    check_against(model, x, res)


# ----------------------------------------------------------------------------- 5. every status and segment end
@pytest.mark.parametrize("name", mix.named_cases())
def test_every_status_and_segment_end(name):
    csr, low_csr, b, kw, status, what = mix.named_cases()[name]
    with pair(csr, low_csr) as (hi, lo):
        model = model_of(hi, lo, b, **kw)
        assert model["status"] == status and (what in model["segments"] or what == model["end"]), (model["end"], model["segments"])
        x, res = solve(hi, lo, b, **kw)
    check_against(model, x, res)
    assert res["status_name"] == ("converged", "max_iterations", "breakdown", "nonfinite", "stagnated")[status]


def test_zero_rhs_and_m_zero(_lib):
    csr = cgc.tri(1025)
    b = cgc.rhs(csr.m, np.float64, 3)
    with pair(csr) as (hi, lo):
        for x0 in (None, b):
            x, res = solve(hi, lo, np.zeros_like(b), x0, rtol=1e-6, max_iterations=20)
            assert sh.converged_at_zero(res, "updates")
            assert not x.any() and same_bits(res["history"], np.zeros(1))
    with handle(sh.empty_csr()) as hi, handle(sh.empty_csr(np.float32)) as lo:
        rc, res = api.cg_mixed(hi.h, lo.h, None, None, max_iterations=5)
    assert rc == 0 and sh.converged_at_zero(res, "updates")


# ----------------------------------------------------------------------------- 6. argument and handle rules
def test_argument_errors_leave_x_untouched(_lib):
    import torch
    lib = _lib
    csr = cgc.tri(300)
    b = cgc.rhs(csr.m, np.float64)
    x = np.full(csr.m, CANARY)

    call = sh.caller(lib, lambda hi, lo, opt, res, B=b, X=x: lib.spmv_hip_cg_mixed(hi, lo, api._ptr(B), api._ptr(X), opt, res))
    options = sh.options_of(ROW)
    res = C.byref(ROW.result())
    with pair(csr) as (hi, lo):
        assert call(hi.h, lo.h, None, res) == E_ARG and call(hi.h, lo.h, options(), None) == E_ARG
        assert call(hi.h, lo.h, options(), res, B=None) == E_ARG and call(hi.h, lo.h, options(), res, X=None) == E_ARG
        for bad in sh.BAD_OPTIONS + (dict(update_drop=-0.1), dict(update_drop=1.0), dict(update_drop=2.0), dict(update_drop=float("nan")), dict(update_every=-1)):
            assert call(hi.h, lo.h, options(**bad), res) == E_ARG, bad
        assert call(None, lo.h, options(), res) == E_ARG and call(hi.h, None, options(), res) == E_ARG
        # the types: `high` must be fp64 and `low` fp32
        assert call(lo.h, lo.h, options(), res) == E_ARG and call(hi.h, hi.h, options(), res) == E_ARG and call(lo.h, hi.h, options(), res) == E_ARG
        # m, n, nnz
        for other in (cgc.tri(301, np.float32), cgc.synth.CSR(csr.m, csr.m + 1, csr.rowptr, csr.colidx, csr.val.astype(np.float32)),
                      cgc.signs(300, np.float32)):
            with handle(other) as lo2:
                assert call(hi.h, lo2.h, options(), res) == E_ARG, (other.m, other.n)
        # another stream
        stream = torch.cuda.Stream()
        with handle(mix.narrowed(csr)) as lo2:
            api.set_stream(lo2.h, stream.cuda_stream, async_=False)
            assert call(hi.h, lo2.h, options(), res) == E_ARG
            api.set_stream(hi.h, stream.cuda_stream, async_=False)           # the same stream on both: the pair solves
            assert call(hi.h, lo2.h, options(), res) == 0 and not (x == CANARY).any()
            api.set_stream(hi.h, None, async_=False)
            x[:] = CANARY
        # another device, where the machine has one
        if lib.spmv_hip_device_count() > 1:
            with torch.cuda.device(1):
                lo2 = handle(mix.narrowed(csr))
            assert call(hi.h, lo2.h, options(), res) == E_ARG
            lo2.close()
        assert (x == CANARY).all()
        assert call(hi.h, lo.h, options(), res) == 0 and not (x == CANARY).any()      # the same call with good arguments runs
    x[:] = CANARY
    wide = cgc.synth.CSR(csr.m, csr.m + 1, csr.rowptr, csr.colidx, csr.val)          # m != n on both
    with pair(wide) as (hi, lo):
        assert call(hi.h, lo.h, options(), res) == E_ARG
    # multi-GPU, host_rows and reordered handles, on either side
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        with pair(csr) as (hi, lo), handle(csr, M.Method_Serial, way, **{key: 1}) as hi2, handle(mix.narrowed(csr), M.Method_Serial, way, **{key: 1}) as lo2:
            assert call(hi2.h, lo.h, options(), res) == E_ARG and call(hi.h, lo2.h, options(), res) == E_ARG, key
    big = cgc.dominant(4096)
    bb, xb = cgc.rhs(big.m, np.float64), np.full(big.m, CANARY)
    with pair(big) as (hi, lo), handle(big, reorder=1) as hi2, handle(mix.narrowed(big), reorder=1) as lo2:
        assert hi2.index is not None and lo2.index is not None
        assert call(hi2.h, lo.h, options(), res, B=bb, X=xb) == E_ARG and call(hi.h, lo2.h, options(), res, B=bb, X=xb) == E_ARG
    assert (xb == CANARY).all()
    # a cleared handle on either side
    with pair(csr) as (hi, lo), pair(csr) as (hi2, lo2):
        api.spmv_clear_handle(hi2.h)
        api.spmv_clear_handle(lo2.h)
        assert call(hi2.h, lo.h, options(), res) == E_NOSTATE and call(hi.h, lo2.h, options(), res) == E_NOSTATE
    assert (x == CANARY).all()


# ----------------------------------------------------------------------------- 7. the workspace
def test_workspace_is_highs_own_and_leaves_the_other_solves_alone():
    import torch
    csr = cgc.lap2d(48)
    m = csr.m
    b = cgc.rhs(m, np.float64, 5)
    b32 = b.astype(np.float32)
    with pair(csr) as (hi, lo):
        fresh = hi.info()["device_bytes"]
        bd, bd32 = torch.from_numpy(b).to(DEV), torch.from_numpy(b32).to(DEV)
        x64, r64 = hi.cg(bd, rtol=1e-8, max_iterations=300)                    # the two handles' own CG workspaces appear here
        x32, r32 = lo.cg(bd32, rtol=1e-4, max_iterations=300)
        before_hi, before_lo = hi.info()["device_bytes"], lo.info()["device_bytes"]
        xd, res = hi.cg_mixed(lo, bd, rtol=1e-10, max_iterations=500)          # device operands: no staging buffer is added
        assert res["status"] == mix.CONVERGED and xd.device.type == "cuda" and xd.dtype == torch.float64
        grown = hi.info()["device_bytes"] - before_hi
        assert grown == ROW.workspace(m)
        assert lo.info()["device_bytes"] == before_lo
        x2, res2 = hi.cg_mixed(lo, bd, rtol=1e-10, max_iterations=500)
        assert hi.info()["device_bytes"] == before_hi + grown and lo.info()["device_bytes"] == before_lo
        assert same_bits(x2.cpu().numpy(), xd.cpu().numpy()) and res2 == res
        mean, runs = ROW.timer(hi.h, lo.h, bd, x2, 10, update_every=4, warmup=1, iters=3)
        assert mean > 0 and runs.shape == (3,) and (runs > 0).all()
        assert hi.info()["device_bytes"] == before_hi + grown and lo.info()["device_bytes"] == before_lo
        # Handle.cg on either handle computes what it did before the mixed solves
        y64, s64 = hi.cg(bd, rtol=1e-8, max_iterations=300)
        y32, s32 = lo.cg(bd32, rtol=1e-4, max_iterations=300)
        assert same_bits(y64.cpu().numpy(), x64.cpu().numpy()) and s64 == r64 and same_bits(y32.cpu().numpy(), x32.cpu().numpy()) and s32 == r32
        assert hi.info()["device_bytes"] == before_hi + grown and lo.info()["device_bytes"] == before_lo
        # clear gives the device state back, the workspace in it (a cleared handle has no device_bytes to read: the re-inspection below goes
        # through the same destroy, and there they can be read); `low` is untouched by it and solves on with another `high`
        api.spmv_clear_handle(hi.h)
        with handle(csr) as hi2:
            _, res3 = hi2.cg_mixed(lo, bd, rtol=1e-10, max_iterations=500)
            assert res3["status"] == mix.CONVERGED and lo.info()["device_bytes"] == before_lo
    with pair(csr) as (hi, lo):                                                 # created again: nothing is carried over
        assert hi.info()["device_bytes"] == fresh
        hi.spmv(b, np.empty_like(b))                                           # host vectors: spmv()'s own staging buffers appear here
        base = hi.info()["device_bytes"]
        hi.cg_mixed(lo, torch.from_numpy(b).to(DEV), rtol=1e-10, max_iterations=500)
        assert hi.info()["device_bytes"] == base + grown
        rp, ci, va = csr.rowptr.copy(), csr.colidx.copy(), csr.val.copy()      # copies of the CSR arrays: spmv() re-inspects, which frees the workspace
        api.spmv(hi.h, m, rp, ci, va, b, np.empty_like(b))
        assert hi.info()["device_bytes"] == base
