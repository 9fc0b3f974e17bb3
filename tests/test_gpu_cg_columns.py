"""GPU: spmv_hip_cg_columns, conjugate gradients for k right-hand sides in one pass over A per iteration (include/spmv_hip.h).

The yardstick is the per-column host model of tests/cg_columns_cases.py: cg_cases.cg, unchanged, around column 0 of the SAME handle's spmm on a
two-column probe.  X, status, iterations, rr, bb and the history of every column are compared BIT FOR BIT; no tolerance appears except the
true-residual bound that tests/test_cg_columns_host.py shows the model alone to meet.  A column's model does not depend on k, so it is computed
once per matrix and shared by every k and position.  The helpers that the solvers share are in tests/solve_harness.py."""
import ctypes as C

import numpy as np
import pytest

import cg_cases as cgc
import cg_columns_cases as ccc
import solve_harness as sh
from solve_harness import CANARY, DEV, DTYPES, E_ARG, METHODS, check_column, check_columns, handle, run_bits, same_bits, same_values
from solve_harness import solve_columns as solve
from spmv_amd import api

pytestmark = pytest.mark.gpu

ROW = sh.ROWS["cg_columns"]
SIZES = sh.SIZES[:-1]     # slot, block and workgroup edges: P = 1, 2 and 3 workgroups; BIG has a test of its own
KS = [2, 3, 5, 8, 16]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = sh.library()
    assert hasattr(lib, "spmv_hip_cg_columns")
    return lib


def same_results(a, b):
    """two lists of result dicts, rr and bb by same_values"""
    return len(a) == len(b) and all((p["status"], p["iterations"]) == (q["status"], q["iterations"]) and same_values([p["rr"], p["bb"]], [q["rr"], q["bb"]]) for p, q in zip(a, b))


# ----------------------------------------------------------------------------- 1. bits against the model
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", SIZES)
def test_bits_against_the_model(m, dtype):
    run_bits(cgc.tri(m, dtype), dtype, KS, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bits_against_the_model_past_one_step(dtype):
    run_bits(cgc.tri(sh.BIG, dtype), dtype, [3], 1)      # P = 1024, L = 2048: two steps, empty workgroups


# ----------------------------------------------------------------------------- 2. a column does not know its company
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_column_has_the_same_bits_in_every_company_and_position(dtype):
    csr = cgc.lap2d(40, dtype)                                     # m = 1600: two workgroups
    m = csr.m
    B = ccc.columns(m, 5, dtype, 2)
    other = ccc.columns(m, 16, dtype, 3)
    with handle(csr) as h:
        X5, res5, hist5 = solve(h, B, rtol=0.0, max_iterations=9)
        for pair in ((0, 1), (2, 3), (4, 0), (3, 1)):
            X, res, hist = solve(h, B[:, pair], rtol=0.0, max_iterations=9)
            for at, j in enumerate(pair):
                assert same_bits(X[:, at], X5[:, j]) and res[at] == res5[j] and same_bits(hist[:, at], hist5[:, j]), pair
        where = [13, 2, 7, 0, 15]                                  # the five columns among eleven others
        B16 = other.copy()
        B16[:, where] = B
        X, res, hist = solve(h, B16, rtol=0.0, max_iterations=9)
        for j, at in enumerate(where):
            assert same_bits(X[:, at], X5[:, j]) and res[at] == res5[j] and same_bits(hist[:, at], hist5[:, j]), at


# ----------------------------------------------------------------------------- 3. columns that end differently, in one call
@pytest.mark.parametrize("dtype", DTYPES)
def test_columns_end_on_their_own_and_stay_frozen(_lib, dtype):
    g = 24
    csr = cgc.lap2d(g, dtype)
    B = ccc.mixed_ends(g, dtype)
    k = B.shape[1]
    rtol = 1e-6 if dtype == np.float64 else 1e-4
    with handle(csr) as h:
        models = ccc.solve(ccc.spmm_column(h), B, rtol=rtol, max_iterations=400)
        X, res, hist = solve(h, B, rtol=rtol, max_iterations=400)
        check_columns(models, 400, X, res, hist)
        by = dict(zip(ccc.MIXED, res))
        assert (by["eigenvector"]["status"], by["eigenvector"]["iterations"]) == (cgc.CONVERGED, 1)
        assert (by["zero"]["status"], by["zero"]["iterations"], by["zero"]["rr"], by["zero"]["bb"]) == (cgc.CONVERGED, 0, 0.0, 0.0) and not X[:, 2].any()
        assert (by["nan"]["status"], by["nan"]["status_name"], by["nan"]["iterations"]) == (cgc.NONFINITE, "nonfinite", 0)
        assert by["generic"]["status"] == by["generic2"]["status"] == cgc.CONVERGED and by["generic"]["iterations"] > 10
        assert len({r["iterations"] for r in res}) >= 3
        # the early column is what it was when it ended: a call that stops there returns the same column
        X1, res1, _ = solve(h, B, rtol=rtol, max_iterations=1)
        assert same_bits(X1[:, 0], X[:, 0]) and res1[0] == res[0] and res1[1]["status"] == cgc.MAX_ITERATIONS
        # the NaN touched no other column: the same call without it
        clean = B.copy()
        clean[:, 3] = B[:, 1]
        Xc, resc, _ = solve(h, clean, rtol=rtol, max_iterations=400)
        for j in (0, 1, 2, 4):
            assert same_bits(Xc[:, j], X[:, j]) and resc[j] == res[j]
        # the caller's history keeps what it held behind every column's end
        budget = 400
        raw = np.full((budget + 1, k), CANARY)
        out = (api.spmv_hip_cg_result * k)()
        opt = api.spmv_hip_cg_options(rtol, 0.0, budget, 0, 0, None, raw.ctypes.data_as(C.POINTER(C.c_double)))
        Xr = np.full(B.shape, CANARY, dtype=dtype)
        rp, ci, va = csr.rowptr, csr.colidx, csr.val
        assert _lib.spmv_hip_cg_columns(h.h, csr.m, api._ptr(rp), api._ptr(ci), api._ptr(va), k, api._ptr(B), k, api._ptr(Xr), k, C.byref(opt), out) == 0
        assert same_bits(Xr, X)
        for j in range(k):
            its = out[j].iterations
            assert its == res[j]["iterations"] and same_values(raw[:its + 1, j], models[j]["history"]) and (raw[its + 1:, j] == CANARY).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_breakdown_and_a_nan_in_the_guess(dtype):
    sg = cgc.signs(1025, dtype)
    B = np.ones((sg.m, 3), dtype=dtype)
    B[:, 1] = cgc.rhs(sg.m, dtype, 7)
    with handle(sg) as h:
        models = ccc.solve(ccc.spmm_column(h), B, max_iterations=9)
        assert models[0]["status"] == models[2]["status"] == cgc.BREAKDOWN
        X, res, hist = solve(h, B, rtol=0.0, max_iterations=9)
        check_columns(models, 9, X, res, hist)
        assert res[0]["status_name"] == "breakdown" and np.isfinite(X[:, 0]).all()
    csr = cgc.tri(1025, dtype)
    B = ccc.columns(csr.m, 3, dtype, 4)
    G = ccc.columns(csr.m, 3, dtype, 5)
    G[17, 1] = np.nan
    with handle(csr) as h:
        models = ccc.solve(ccc.spmm_column(h), B, G, max_iterations=6)
        X, res, hist = solve(h, B, G, rtol=0.0, max_iterations=6)
        assert res[1]["status"] == cgc.NONFINITE and res[1]["iterations"] == 0 and same_bits(X[:, 1], G[:, 1])     # the guess is left as it was
        for j in (0, 2):
            check_column(models[j], 6, X[:, j], res[j], hist[:, j])


# ----------------------------------------------------------------------------- 4. check_every, methods, one column
@pytest.mark.parametrize("dtype", DTYPES)
def test_check_every_changes_nothing(dtype):
    g = 24
    csr = cgc.lap2d(g, dtype)
    B = ccc.mixed_ends(g, dtype)
    rtol = 1e-6 if dtype == np.float64 else 1e-4
    with handle(csr) as h:
        want = solve(h, B, rtol=rtol, max_iterations=400, check_every=1)
        assert max(r["iterations"] for r in want[1]) > 8
        short = max(r["iterations"] for r in want[1]) // 2
        want_short = solve(h, B, rtol=rtol, max_iterations=short, check_every=1)
        assert cgc.MAX_ITERATIONS in [r["status"] for r in want_short[1]]
        for every in (3, 64, 0):
            for budget, ref in ((400, want), (short, want_short)):
                X, res, hist = solve(h, B, rtol=rtol, max_iterations=budget, check_every=every)
                assert same_bits(X, ref[0]) and same_results(res, ref[1]) and same_values(hist, ref[2]), (every, budget)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_method_gives_the_same_bits_and_one_column_is_cg(dtype):
    csr = cgc.lap2d(32, dtype)
    B = ccc.columns(csr.m, 4, dtype, 6)
    b = np.ascontiguousarray(B[:, 0])
    want = None
    for method in METHODS:
        with handle(csr, method) as h:
            got = solve(h, B, rtol=0.0, max_iterations=12)
            if want is None:
                want = got
                check_columns(ccc.solve(ccc.spmm_column(h), B, max_iterations=12), 12, *got)
            assert same_bits(got[0], want[0]) and got[1] == want[1] and same_bits(got[2], want[2]), method
            # k = 1, ldb = ldx = 1 is spmv_hip_cg: this method's own multiply
            x, res, hist = h.cg(b, np.full(csr.m, CANARY, dtype=dtype), rtol=0.0, max_iterations=12, history=True)
            X1, res1, hist1 = solve(h, B[:, :1], rtol=0.0, max_iterations=12)
            assert same_bits(X1[:, 0], x) and res1 == [res] and same_bits(hist1[:, 0], hist), method
            # ... and with a leading dimension above 1 it is a column like any other
            wide = np.full((csr.m, 2), CANARY, dtype=dtype)
            Xw, resw = h.cg_columns(np.ascontiguousarray(B[:, :1]), wide[:, :1], rtol=0.0, max_iterations=12)
            assert same_bits(Xw[:, 0], want[0][:, 0]) and resw[0] == want[1][0] and (wide[:, 1] == CANARY).all(), method


# ----------------------------------------------------------------------------- 5. pointers and leading dimensions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 8])
def test_host_device_unaligned_and_padded_operands_give_the_same_bits(k, dtype):
    import torch
    m = 2049
    csr = cgc.tri(m, dtype)
    rng = np.random.default_rng(k)
    B, G, jac = ccc.columns(m, k, dtype, 8), rng.uniform(-1, 1, (m, k)).astype(dtype), rng.uniform(0.5, 1.5, m).astype(dtype)
    tdt = torch.from_numpy(B).dtype
    with handle(csr) as h:
        for X0 in (None, G):
            want, wres, whist = solve(h, B, X0, rtol=0.0, max_iterations=6, dinv=jac)
            # host views into wider arrays: ldb = k + 3, ldx = k + 1; B's padding is NaN, X's a canary
            Bw = np.full((m, k + 3), np.nan, dtype=dtype)
            Bw[:, 2:2 + k] = B
            Xw = np.full((m, k + 1), CANARY, dtype=dtype)
            if X0 is not None:
                Xw[:, 1:] = X0
            got, res, hist = h.cg_columns(Bw[:, 2:2 + k], Xw[:, 1:], x0=X0 is not None, rtol=0.0, max_iterations=6, dinv=jac, history=True)
            assert same_bits(got, want) and res == wres and same_bits(hist, whist) and (Xw[:, 0] == CANARY).all()
            for shift_b, shift_x, pad_b, pad_x in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, 3, 1), (1, 1, 3, 1)):
                ldb, ldx = k + pad_b, k + pad_x
                bbuf = torch.full((m * ldb + 1,), float("nan"), dtype=tdt, device=DEV)
                Bd = bbuf[shift_b:shift_b + m * ldb].view(m, ldb)[:, :k]
                Bd.copy_(torch.from_numpy(B))
                edge = 16 // np.dtype(dtype).itemsize                 # one 16-byte unit of canaries each side keeps X aligned; + 1 element: not
                xbuf = torch.full((m * ldx + 2 * edge + 1,), CANARY, dtype=tdt, device=DEV)
                Xd = xbuf[edge + shift_x:edge + shift_x + m * ldx].view(m, ldx)[:, :k]
                assert (Bd.data_ptr() % 16 != 0) == bool(shift_b) and (Xd.data_ptr() % 16 != 0) == bool(shift_x)
                if X0 is not None:
                    Xd.copy_(torch.from_numpy(X0))
                got, res, hist = h.cg_columns(Bd, Xd, x0=X0 is not None, rtol=0.0, max_iterations=6, dinv=torch.from_numpy(jac).to(DEV), history=True)
                torch.cuda.synchronize()
                case = (shift_b, shift_x, pad_b, pad_x)
                assert got is Xd and same_bits(Xd.cpu().numpy(), want) and res == wres and same_bits(hist, whist), case
                out = xbuf.cpu().numpy()
                body = out[edge + shift_x:edge + shift_x + m * ldx].reshape(m, ldx)
                assert (out[:edge + shift_x] == CANARY).all() and (out[edge + shift_x + m * ldx:] == CANARY).all() and (body[:, k:] == CANARY).all(), case
            # mixed: device B, host X, device Dinv
            Xh = np.full((m, k), CANARY, dtype=dtype) if X0 is None else X0.copy()
            h.cg_columns(torch.from_numpy(B).to(DEV), Xh, x0=X0 is not None, rtol=0.0, max_iterations=6, dinv=torch.from_numpy(jac).to(DEV))
            assert same_bits(Xh, want)


# ----------------------------------------------------------------------------- 6. handle rules
def test_argument_errors_leave_x_untouched(_lib):
    lib = _lib
    csr = cgc.tri(300)
    k = 3
    B = ccc.columns(csr.m, k, np.float64, 9)
    X = np.full((csr.m, k), CANARY)
    rp, ci, va = csr.rowptr, csr.colidx, csr.val
    results = (api.spmv_hip_cg_result * 16)()
    call = sh.caller(lib, lambda h, opt, res, B=B, X=X, kk=k, ldb=k, ldx=k: lib.spmv_hip_cg_columns(
        h, csr.m, api._ptr(rp), api._ptr(ci), api._ptr(va), kk, api._ptr(B), ldb, api._ptr(X), ldx, opt, res))
    options = sh.options_of(ROW)

    def shapes(h):
        for bad in (dict(kk=0), dict(kk=-1), dict(kk=17, ldb=17, ldx=17), dict(ldb=k - 1), dict(ldx=k - 1), dict(ldb=0), dict(ldx=0)):
            assert call(h.h, options(), results, **bad) == E_ARG, bad
    sh.common_argument_errors(csr, X, call, options, results, more=shapes)


def test_m_zero_is_converged():
    empty = sh.empty_csr()
    with handle(empty) as h:
        rc, res = api.cg_columns(h.h, 0, empty.rowptr, empty.colidx, empty.val, np.zeros((0, 3)), np.zeros((0, 3)), max_iterations=5)
    assert rc == 0 and len(res) == 3 and all(sh.converged_at_zero(r) for r in res)


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_other_solvers_multiplies_and_timer(dtype):
    import torch
    csr = cgc.lap2d(48, dtype)
    m, item = csr.m, np.dtype(dtype).itemsize
    B = ccc.columns(m, 8, dtype, 10)
    b = np.ascontiguousarray(B[:, 0])
    with handle(csr) as h:
        fresh = h.info()["device_bytes"]
        y0 = h.spmv(b, np.empty_like(b))                                           # host operands: the multiplies' staging buffers and spmm's tables appear here
        with_spmv = h.info()["device_bytes"]
        Y0 = h.spmm(B)
        before = h.info()["device_bytes"]
        Bd = torch.from_numpy(B).to(DEV)
        X3, res3 = h.cg_columns(Bd[:, :3].contiguous(), rtol=1e-6, max_iterations=300)   # device operands: no staging buffer is added
        assert all(r["status"] == cgc.CONVERGED for r in res3) and X3.device.type == "cuda"
        assert h.info()["device_bytes"] - before == ROW.workspace(m, 3, item)
        h.cg_columns(Bd[:, :2].contiguous(), rtol=1e-6, max_iterations=300)            # fewer columns: the same block
        assert h.info()["device_bytes"] - before == ROW.workspace(m, 3, item)
        X8, res8 = h.cg_columns(Bd, rtol=1e-6, max_iterations=300)                   # more: allocated anew
        grown = ROW.workspace(m, 8, item)
        assert h.info()["device_bytes"] - before == grown
        assert same_bits(X8[:, :3].cpu().numpy(), X3.cpu().numpy()) and res8[:3] == res3
        X3b, res3b = h.cg_columns(Bd[:, :3].contiguous(), rtol=1e-6, max_iterations=300)   # in the larger block: the same bits
        assert h.info()["device_bytes"] - before == grown and same_bits(X3b.cpu().numpy(), X3.cpu().numpy()) and res3b == res3
        cg_block, bicgstab_block = sh.ROWS["cg"].workspace(m, item), sh.ROWS["bicgstab"].workspace(m, item)
        bd = torch.from_numpy(b).to(DEV)
        h.cg(bd, rtol=1e-6, max_iterations=300)
        assert h.info()["device_bytes"] - before == grown + cg_block            # spmv_hip_cg's own pinned block
        h.bicgstab(bd, rtol=1e-6, max_iterations=300)
        both = grown + cg_block + bicgstab_block                  # ... and spmv_hip_bicgstab's
        assert h.info()["device_bytes"] - before == both
        assert same_bits(h.spmv(b, np.empty_like(b)), y0) and same_bits(h.spmm(B), Y0)              # the multiplies compute what they did
        Xt = torch.empty_like(Bd)
        mean, runs = ROW.timer(h.h, Bd, Xt, 10, warmup=1, iters=3)
        assert mean > 0 and runs.shape == (3,) and (runs > 0).all() and h.info()["device_bytes"] - before == both
        X8b, res8b = h.cg_columns(Bd, rtol=1e-6, max_iterations=300)
        assert same_bits(X8b.cpu().numpy(), X8.cpu().numpy()) and res8b == res8
        # copies of the CSR arrays: spmv() re-inspects, which frees every workspace with everything else on the device
        rp, ci, va = csr.rowptr.copy(), csr.colidx.copy(), csr.val.copy()
        y1 = np.empty_like(b)
        api.spmv(h.h, m, rp, ci, va, b, y1)
        assert same_bits(y1, y0) and h.info()["device_bytes"] == with_spmv < before
        Xa = torch.empty_like(Bd)
        _, resa = api.cg_columns(h.h, m, rp, ci, va, Bd, Xa, rtol=1e-6, max_iterations=300)
        assert same_bits(Xa.cpu().numpy(), X8.cpu().numpy()) and resa == res8
    with handle(csr) as h:                                                          # destroyed and created again: nothing is carried over
        assert h.info()["device_bytes"] == fresh


def test_a_reordered_handle_solves_the_permuted_system():
    csr = cgc.dominant(4096, np.float64)
    B = ccc.columns(csr.m, 3, np.float64, 11)
    with handle(csr, reorder=1) as h:
        perm = h.index
        assert perm is not None and sorted(perm.tolist()) == list(range(csr.m))
        Bp = np.ascontiguousarray(B[perm])                                         # XX[i] = X[index[i]], as for spmv()
        models = ccc.solve(ccc.spmm_column(h), Bp, rtol=1e-10, max_iterations=200)
        Xp, res, hist = solve(h, Bp, rtol=1e-10, max_iterations=200)
        check_columns(models, 200, Xp, res, hist)
    X = np.empty_like(Xp)
    X[perm] = Xp
    for j in range(3):
        assert res[j]["status"] == cgc.CONVERGED and cgc.true_residual(csr, B[:, j], X[:, j]) <= 1e-9


# ----------------------------------------------------------------------------- 7. convergence
@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", ["lap2d32", "dominant4096"])
def test_convergence_with_the_models_iteration_counts(name, rtol):
    csr = cgc.lap2d(32) if name == "lap2d32" else cgc.dominant(4096)
    B = ccc.columns(csr.m, 4, np.float64, 12)
    with handle(csr) as h:
        models = ccc.solve(ccc.spmm_column(h), B, rtol=rtol, max_iterations=500)
        X, res, hist = solve(h, B, rtol=rtol, max_iterations=500)
    check_columns(models, 500, X, res, hist)
    print(f"{name} rtol {rtol}: iterations {[r['iterations'] for r in res]}")
    for j in range(4):
        assert res[j]["status"] == cgc.CONVERGED and res[j]["iterations"] == models[j]["iterations"]
        assert cgc.true_residual(csr, B[:, j], X[:, j]) <= 10 * rtol
