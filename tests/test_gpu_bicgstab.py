"""GPU: spmv_hip_bicgstab, the BiCGStab solve that stays on the device (include/spmv_hip.h).

The yardstick is the host model of tests/bicgstab_cases.py -- a numpy restatement of the header's arithmetic contract -- driven by the SAME
handle's spmv(), so x, rr, bb and the history are compared BIT FOR BIT: no tolerance appears except the true-residual bound
||b - A x|| / ||b|| <= 10 rtol that tests/test_bicgstab_host.py shows the model alone to meet."""
import ctypes as C

import numpy as np
import pytest

import bicgstab_cases as bc
from spmv_amd import api, build

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
DTYPES = [np.float64, np.float32]
E_ARG, E_NOSTATE = 3, 5
DEV = "cuda:0"
CANARY = -7.25
# slot, step and workgroup edges: P = 1, 2 and 3 workgroups, two steps per workgroup and empty workgroups (2^20 + 1: P = 1024, L = 2048)
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2049, 1024 * 1024 + 1]
BIG = 1024 * 1024 + 1
BUDGETS = (0, 1, 2, 5)
PARTIAL_ARRAYS = 8            # <rhat,v>, <s,s>, <t,s>, <t,t>, rho twice, <r,r>, <b,b>


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def handle(csr, method=M.Method_Parallel, way=api.VECTORIZED_WAY.VECTOR_HIP, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method, way=way)
    finally:
        api.clear_thread_options()


def multiply_of(h):
    """the model's multiply: this handle's spmv() on host vectors"""
    def multiply(x):
        return h.spmv(np.ascontiguousarray(x), np.empty_like(x))
    return multiply


def solve(h, b, x0=None, **kw):
    """through host pointers -> (x, result dict with history)"""
    x = np.full(b.size, CANARY, dtype=b.dtype) if x0 is None else x0.copy()
    x, res, hist = h.bicgstab(b, x, x0=x0 is not None, history=True, **kw)
    res["history"] = hist
    return x, res


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against(model, k, x, res):
    """a run with max_iterations = k against a model run with a budget of at least k that ended as CONVERGED or MAX_ITERATIONS"""
    assert model["status"] in (bc.CONVERGED, bc.MAX_ITERATIONS)
    its = min(k, model["iterations"])
    status = bc.MAX_ITERATIONS if k < model["iterations"] or model["status"] == bc.MAX_ITERATIONS else model["status"]
    assert (res["status"], res["iterations"]) == (status, its)
    assert same_bits(x, model["iterates"][its])
    assert res["bb"] == model["bb"] and res["rr"] == model["history"][its]
    assert same_bits(res["history"], model["history"][:its + 1])


def check_same_end(model, x, res):
    """a run with the model's own budget, whatever way the model ended"""
    assert (res["status"], res["iterations"]) == (model["status"], model["iterations"])
    assert same_bits(x, model["x"])
    if model["status"] != bc.NONFINITE:
        assert res["bb"] == model["bb"] and res["rr"] == model["rr"] and same_bits(res["history"], model["history"])


# ----------------------------------------------------------------------------- 1. bits against the model
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", SIZES)
def test_bits_against_the_model(m, dtype):
    csr = bc.tri_ns(m, dtype)
    rng = np.random.default_rng(m)
    b, guess = bc.rhs(m, dtype), rng.uniform(-1, 1, m).astype(dtype)
    jac = rng.uniform(0.5, 1.5, m).astype(dtype)
    ones = np.ones(m, dtype=dtype)
    with handle(csr) as h:
        mul = multiply_of(h)
        if m == BIG:                                         # one x0 / Dinv combination: a guess and a random Dinv
            pre = bc.bicgstab(mul, b, x0=guess, dinv=jac, max_iterations=5)
            for k in BUDGETS:
                x_jac, r_jac = solve(h, b, guess, rtol=0.0, max_iterations=k, dinv=jac)
                check_against(pre, k, x_jac, r_jac)
            return
        for x0 in (None, guess):
            plain = bc.bicgstab(mul, b, x0=x0, max_iterations=5)
            pre = bc.bicgstab(mul, b, x0=x0, dinv=jac, max_iterations=5)
            for k in BUDGETS:
                x_none, r_none = solve(h, b, x0, rtol=0.0, max_iterations=k)
                check_against(plain, k, x_none, r_none)
                x_ones, r_ones = solve(h, b, x0, rtol=0.0, max_iterations=k, dinv=ones)
                assert same_bits(x_ones, x_none) and same_bits(r_ones["history"], r_none["history"]) and r_ones["iterations"] == r_none["iterations"]
                x_jac, r_jac = solve(h, b, x0, rtol=0.0, max_iterations=k, dinv=jac)
                check_against(pre, k, x_jac, r_jac)


# ----------------------------------------------------------------------------- 2. every method
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", [mth for mth in M if mth != M.Method_Total_Size])
def test_every_method_has_the_bits_of_the_model_on_its_own_spmv(method, dtype):
    csr = bc.upwind(32, dtype)
    b = bc.rhs(csr.m, dtype, 1)
    with handle(csr, method) as h:
        model = bc.bicgstab(multiply_of(h), b, max_iterations=12)
        x, res = solve(h, b, rtol=0.0, max_iterations=12)
        check_against(model, 12, x, res)


# ----------------------------------------------------------------------------- 3. convergence
@pytest.mark.parametrize("name,dtype,rtol", [("upwind32", np.float64, 1e-8), ("nonsym_dominant4096", np.float32, 1e-3)])
def test_convergence_with_the_models_iteration_count(name, dtype, rtol):
    csr = bc.upwind(32, dtype) if name == "upwind32" else bc.nonsym_dominant(4096, dtype)
    b = bc.rhs(csr.m, dtype)
    with handle(csr) as h:
        model = bc.bicgstab(multiply_of(h), b, rtol=rtol, max_iterations=500)
        x, res = solve(h, b, rtol=rtol, max_iterations=500)
    assert model["status"] == bc.CONVERGED
    assert res["status"] == bc.CONVERGED and res["status_name"] == "converged" and res["iterations"] == model["iterations"]
    assert same_bits(x, model["x"]) and same_bits(res["history"], model["history"]) and res["rr"] == model["rr"] and res["bb"] == model["bb"]
    true = bc.true_residual(csr, b, x)
    print(f"{name}: {res['iterations']} iterations, true residual {true:.3e}")
    assert true <= 10 * rtol


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
    csr = bc.upwind(32, dtype)
    b = bc.rhs(csr.m, dtype, 2)
    rtol = 1e-8 if dtype == np.float64 else 1e-4
    with handle(csr) as h:
        model = bc.bicgstab(multiply_of(h), b, rtol=rtol, max_iterations=400)
        assert model["status"] == bc.CONVERGED and 8 < model["iterations"] < 400
        for every in (1, 3, 64, 0):
            x, res = solve(h, b, rtol=rtol, max_iterations=400, check_every=every)
            # the early exit really exits: nothing is applied behind the iteration that met the test, however many were enqueued
            assert (res["status"], res["iterations"]) == (bc.CONVERGED, model["iterations"]), every
            assert same_bits(x, model["x"]) and same_bits(res["history"], model["history"]) and res["rr"] == model["rr"], every
        short = model["iterations"] // 2
        for every in (1, 3, 64):
            x, res = solve(h, b, rtol=rtol, max_iterations=short, check_every=every)
            assert (res["status"], res["status_name"], res["iterations"]) == (bc.MAX_ITERATIONS, "max_iterations", short), every
            assert same_bits(x, model["iterates"][short]) and same_bits(res["history"], model["history"][:short + 1]), every


# ----------------------------------------------------------------------------- 5. the early ends
@pytest.mark.parametrize("dtype", DTYPES)
def test_breakdown_half_step_nonfinite_and_zero_rhs(dtype):
    sk = bc.skew(1025, dtype)
    ones = np.ones(sk.m, dtype=dtype)
    with handle(sk) as h:
        model = bc.bicgstab(multiply_of(h), ones, max_iterations=9)
        assert (model["status"], model["iterations"]) == (bc.BREAKDOWN, 0)
        for every in (1, 0):
            x, res = solve(h, ones, rtol=0.0, max_iterations=9, check_every=every)
            assert res["status_name"] == "breakdown" and np.isfinite(x).all()
            check_same_end(model, x, res)
    for m in (1, 1025):
        two = bc.twice_identity(m, dtype)
        b = bc.rhs(m, dtype, 2)
        with handle(two) as h:
            model = bc.bicgstab(multiply_of(h), b, rtol=0.0, max_iterations=9)
            assert (model["status"], model["iterations"]) == (bc.CONVERGED, 1) and model["history"][1] == 0.0
            for every in (1, 0):
                x, res = solve(h, b, rtol=0.0, max_iterations=9, check_every=every)
                check_same_end(model, x, res)
            x, res = solve(h, b, rtol=0.0, max_iterations=9, dinv=np.full(m, 0.25, dtype=dtype))   # A Dinv = I / 2: the half step again
            check_same_end(bc.bicgstab(multiply_of(h), b, dinv=np.full(m, 0.25, dtype=dtype), rtol=0.0, max_iterations=9), x, res)
            assert (res["status"], res["iterations"], res["rr"]) == (bc.CONVERGED, 1, 0.0)
    csr = bc.tri_ns(1025, dtype)
    b = bc.rhs(csr.m, dtype, 3)
    with handle(csr) as h:
        bad = b.copy()
        bad[700] = np.nan
        model = bc.bicgstab(multiply_of(h), bad, rtol=1e-6, max_iterations=20)
        _, res = solve(h, bad, rtol=1e-6, max_iterations=20)
        assert res["status"] == bc.NONFINITE and res["status_name"] == "nonfinite" and res["iterations"] <= 1
        assert (res["status"], res["iterations"]) == (model["status"], model["iterations"])
        # a NaN that only the first multiply brings in: x0 with a NaN and a finite B
        _, res = solve(h, b, bad, rtol=1e-6, max_iterations=20)
        assert res["status"] == bc.NONFINITE and res["iterations"] == 0
        for x0 in (None, b):
            model = bc.bicgstab(multiply_of(h), np.zeros_like(b), x0=x0, rtol=1e-6, max_iterations=20)
            x, res = solve(h, np.zeros_like(b), x0, rtol=1e-6, max_iterations=20)
            assert (res["status"], res["iterations"], res["rr"], res["bb"]) == (bc.CONVERGED, 0, 0.0, 0.0)
            assert not x.any() and same_bits(res["history"], np.zeros(1))
            check_same_end(model, x, res)


# ----------------------------------------------------------------------------- 6. pointers
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1025, 70001])
def test_host_device_and_unaligned_pointers_give_the_same_bits(m, dtype):
    import torch
    csr = bc.tri_ns(m, dtype)
    rng = np.random.default_rng(m + 1)
    b, guess, jac = bc.rhs(m, dtype, 4), rng.uniform(-1, 1, m).astype(dtype), rng.uniform(0.5, 1.5, m).astype(dtype)
    pad = 16 // np.dtype(dtype).itemsize                 # canaries of one 16-byte unit each side keep X aligned; + 1 element: not
    with handle(csr) as h:
        for x0 in (None, guess):
            want, wres = solve(h, b, x0, rtol=0.0, max_iterations=6, dinv=jac)
            assert wres["iterations"] == 6
            for shift_b, shift_x in ((0, 0), (1, 0), (0, 1), (1, 1)):
                bd = torch.zeros(m + 1, dtype=torch.from_numpy(b).dtype, device=DEV)[shift_b:shift_b + m]
                bd.copy_(torch.from_numpy(b))
                jd = torch.from_numpy(jac).to(DEV)
                buf = torch.full((m + 2 * pad + 1,), CANARY, dtype=bd.dtype, device=DEV)
                xd = buf[pad + shift_x:pad + shift_x + m]
                assert (bd.data_ptr() % 16 != 0) == bool(shift_b) and (xd.data_ptr() % 16 != 0) == bool(shift_x)
                if x0 is not None:
                    xd.copy_(torch.from_numpy(x0))
                got, res, hist = h.bicgstab(bd, xd, x0=x0 is not None, rtol=0.0, max_iterations=6, dinv=jd, history=True)
                torch.cuda.synchronize()
                assert got is xd and same_bits(xd.cpu().numpy(), want), (shift_b, shift_x)
                assert same_bits(hist, wres["history"]) and res["rr"] == wres["rr"]
                out = buf.cpu().numpy()
                assert (out[:pad + shift_x] == CANARY).all() and (out[pad + shift_x + m:] == CANARY).all(), "written outside X"
            # mixed: device B, host X, device Dinv
            xh = np.full(m, CANARY, dtype=dtype) if x0 is None else x0.copy()
            h.bicgstab(torch.from_numpy(b).to(DEV), xh, x0=x0 is not None, rtol=0.0, max_iterations=6, dinv=torch.from_numpy(jac).to(DEV))
            assert same_bits(xh, want)


# ----------------------------------------------------------------------------- 7. handle rules
def test_argument_errors_leave_x_untouched(_lib):
    lib = _lib
    csr = bc.tri_ns(300)
    b = bc.rhs(csr.m, np.float64)
    x = np.full(csr.m, CANARY)
    rp, ci, va = csr.rowptr, csr.colidx, csr.val

    def call(h, opt, res, B=b, X=x):
        lib.spmv_hip_clear_error()
        rc = lib.spmv_hip_bicgstab(h, csr.m, api._ptr(rp), api._ptr(ci), api._ptr(va), api._ptr(B), api._ptr(X), opt, res)
        assert lib.spmv_hip_last_error() == rc
        lib.spmv_hip_clear_error()
        return rc

    def options(**kw):
        base = dict(rtol=1e-8, atol=0.0, max_iterations=10, check_every=0, use_x0=0)
        base.update(kw)
        return C.byref(api.spmv_hip_cg_options(**base))

    res = C.byref(api.spmv_hip_cg_result())
    with handle(csr) as h:
        assert call(h.h, None, res) == E_ARG and call(h.h, options(), None) == E_ARG
        assert call(h.h, options(), res, B=None) == E_ARG and call(h.h, options(), res, X=None) == E_ARG
        for bad in (dict(max_iterations=-1), dict(check_every=-1), dict(rtol=-1e-3), dict(atol=-1.0), dict(rtol=float("nan")), dict(atol=float("nan"))):
            assert call(h.h, options(**bad), res) == E_ARG, bad
        assert call(None, options(), res) == E_ARG
        assert (x == CANARY).all()
        assert call(h.h, options(), res) == 0 and not (x == CANARY).any()      # the same call with good arguments runs
    x[:] = CANARY
    wide = bc.synth.CSR(csr.m, csr.m + 1, rp, ci, va)                           # m != n at create
    with handle(wide) as h:
        assert call(h.h, options(), res) == E_ARG
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        with handle(csr, M.Method_Serial, way, **{key: 1}) as h:
            assert call(h.h, options(), res) == E_ARG, key
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert call(h.h, options(), res) == E_NOSTATE
    h.close()
    assert (x == CANARY).all()


def test_m_zero_is_converged():
    empty = bc.synth.CSR(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    with handle(empty) as h:
        rc, res = api.bicgstab(h.h, 0, empty.rowptr, empty.colidx, empty.val, None, None, max_iterations=5)
    assert rc == 0 and (res["status"], res["iterations"], res["rr"], res["bb"]) == (bc.CONVERGED, 0, 0.0, 0.0)


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
        vec = (csr.m * item + 255) // 256 * 256
        assert grown == 6 * vec + PARTIAL_ARRAYS * 1024 * 8 + 256                  # r, rhat, p, v, t, y, the partial arrays, the state
        x2, res2 = h.bicgstab(bd, rtol=1e-6, max_iterations=300)
        assert h.info()["device_bytes"] == before + grown and same_bits(x2.cpu().numpy(), xd.cpu().numpy()) and res2 == res
        mean, runs = api.time_bicgstab_iterations(h.h, bd, xd, 10, warmup=1, iters=3)
        assert mean > 0 and runs.shape == (3,) and (runs > 0).all()
        assert h.info()["device_bytes"] == before + grown
        xc = torch.empty_like(bd)
        _, cres = h.cg(bd, xc, rtol=1e-6, max_iterations=5)                        # spmv_hip_cg's workspace is its own, neither shared nor grown
        both = h.info()["device_bytes"]
        assert both - (before + grown) == 3 * vec + 5 * 1024 * 8 + 256
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
    csr = bc.nonsym_dominant(4096, np.float64)
    b = bc.rhs(csr.m, np.float64, 6)
    with handle(csr, reorder=1) as h:
        perm = h.index
        assert perm is not None and sorted(perm.tolist()) == list(range(csr.m))
        bp = np.ascontiguousarray(b[perm])                                         # XX[i] = X[index[i]], as for spmv()
        model = bc.bicgstab(multiply_of(h), bp, rtol=1e-10, max_iterations=200)
        xp, res = solve(h, bp, rtol=1e-10, max_iterations=200)
    assert res["status"] == bc.CONVERGED and res["iterations"] == model["iterations"] and same_bits(xp, model["x"])
    x = np.empty_like(xp)
    x[perm] = xp
    assert bc.true_residual(csr, b, x) <= 1e-9
