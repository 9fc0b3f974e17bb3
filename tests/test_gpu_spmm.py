"""GPU: spmv_hip_spmm, Y = A X for k right-hand sides in one pass over A per panel (include/spmv_hip.h).

Bars: exact-arithmetic ("eighths") inputs -> every column BIT-EXACT against the oracle (and column 0 against the golden y_ref);
random inputs -> the per-row bar of test_gpu_parity.check, column by column.  Results must not depend on ldx / ldy, the pointers'
kind, the stream or async setting; k = 1 with ldx = ldy = 1 is spmv() itself."""
import json
import os
import warnings

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_golden
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    NAMES = sorted(json.load(_f)["cases"].keys())
ALL_METHODS = [M.Method_Serial, M.Method_Parallel, M.Method_Balanced, M.Method_Balanced2,
               M.Method_Balanced_Yid, M.Method_SellCSigma, M.Method_CSR5SPMV]
TOL = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-3}
SHARP = {np.dtype(np.float64): 64 * 2.3e-16, np.dtype(np.float32): 64 * 1.2e-7}
E_ARG, E_NOSTATE = 3, 5
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def block_x(csr, x, k, seed=11):
    """n x k: column 0 is x, the others seeded vectors of the same value kind."""
    kind = "eighths" if np.all(x * 8 == np.round(x * 8)) and np.all(x >= 0) else "uniform"
    X = np.empty((csr.n, k), dtype=x.dtype)
    if csr.n:
        X[:, 0] = x
        for c in range(1, k):
            X[:, c] = synth.fill_x(csr.n, kind, x.dtype, seed + 101 * c)
    return X


def check_block(Y, csr, X, exact, y_ref=None):
    assert not np.isnan(Y).any(), f"{int(np.isnan(Y).sum())} entries left unwritten"
    for c in range(X.shape[1]):
        xc = np.ascontiguousarray(X[:, c])
        ye = oracle.spmv_exact(csr, xc)
        yc = np.ascontiguousarray(Y[:, c])
        if exact:
            assert np.array_equal(yc.view(np.uint8), ye.astype(Y.dtype).view(np.uint8)), c
            if c == 0 and y_ref is not None:
                assert np.array_equal(yc.view(np.uint8), y_ref.view(np.uint8))
            continue
        s = oracle.row_abs_sum(csr, xc)
        err = np.abs(yc.astype(np.float64) - ye)
        assert (err <= TOL[Y.dtype] * s + 1e-300).all(), (c, float((err / np.maximum(s, 1e-300)).max()))
        assert (err <= SHARP[Y.dtype] * np.maximum(1, np.diff(csr.rowptr)) * s + 1e-300).all(), c


def spmm_host(h, csr, X):
    Y = np.full((csr.m, X.shape[1]), np.nan, dtype=X.dtype)
    api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, X, Y)
    return Y


# ----------------------------------------------------------------------------- 1. golden cases, host pointers
@pytest.mark.parametrize("method", ALL_METHODS, ids=lambda m: m.name)
@pytest.mark.parametrize("name", NAMES)
def test_golden_host_pointers(name, method):
    csr, x, y_ref = load_golden(name)
    exact = name.endswith("eighths")
    with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method) as h:
        for k in (1, 3, 8, 17):
            X = block_x(csr, x, k)
            check_block(spmm_host(h, csr, X), csr, X, exact, y_ref)


# ----------------------------------------------------------------------------- 2. device pointers: the host run's bits
@pytest.mark.parametrize("method", ALL_METHODS, ids=lambda m: m.name)
@pytest.mark.parametrize("name", ["banded_f64_eighths", "powerlaw_f32_uniform", "empty_mix_f64_uniform", "dense_row0_f32_uniform",
                                  "skewed_f64_uniform", "single_long_f32_uniform", "nnz0_f64_uniform"])
def test_golden_device_pointers(name, method):
    import torch
    csr, x, _ = load_golden(name)
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    with api.Handle(csr.m, csr.n, rp, ci, va, method) as h:
        for k in (3, 17, 33):
            X = block_x(csr, x, k)
            Yd = h.spmm(torch.from_numpy(X).to(DEV))
            torch.cuda.synchronize()
            with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method) as hh:
                Yh = spmm_host(hh, csr, X)
            assert np.array_equal(Yd.cpu().numpy().view(np.uint8), Yh.view(np.uint8)), k
            check_block(Yh, csr, X, name.endswith("eighths"))


# ----------------------------------------------------------------------------- 3. padding and leading dimensions
@pytest.mark.parametrize("name", ["skewed_f64_uniform", "powerlaw_f32_uniform", "banded_wide_f32_uniform", "single_long_f64_uniform"])
def test_padding_and_leading_dimensions(name):
    import torch
    csr, x, _ = load_golden(name)
    with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Parallel) as h:
        for k in (2, 5, 16, 19):
            X = block_x(csr, x, k)
            base = spmm_host(h, csr, X)
            check_block(base, csr, X, False)
            # NaN in X's padding never reaches Y; Y's padding keeps its bits
            Xp = np.full((csr.n, k + 3), np.nan, dtype=X.dtype)
            Xp[:, :k] = X
            Yp = np.full((csr.m, k + 5), np.nan, dtype=X.dtype)
            Yp[:, k:] = -7.25
            api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Xp[:, :k], Yp[:, :k])
            assert not np.isnan(Yp[:, :k]).any()
            assert np.array_equal(Yp[:, :k], base)
            assert (Yp[:, k:] == -7.25).all()
            # odd / even leading dimensions, 16-byte aligned or not: identical bits (host and device)
            for ld, off in ((k, 0), (k + 1, 0), (k + 2, 0), (k + 1, 1), (k + 4, 1)):
                Xo = np.full((csr.n, ld + off), np.nan, dtype=X.dtype)
                Xo[:, off:off + k] = X
                Yo = np.full((csr.m, ld + off), np.nan, dtype=X.dtype)
                api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Xo[:, off:off + k], Yo[:, off:off + k])
                assert np.array_equal(np.ascontiguousarray(Yo[:, off:off + k]).view(np.uint8), np.ascontiguousarray(base).view(np.uint8)), (ld, off)
                Xd = torch.from_numpy(Xo).to(DEV)
                Yd = torch.full((csr.m, ld + off), float("nan"), dtype=Xd.dtype, device=DEV)
                api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Xd[:, off:off + k], Yd[:, off:off + k])
                torch.cuda.synchronize()
                got = Yd.cpu().numpy()
                assert np.array_equal(np.ascontiguousarray(got[:, off:off + k]).view(np.uint8), np.ascontiguousarray(base).view(np.uint8)), (ld, off)
                assert np.isnan(got[:, :off]).all() and np.isnan(got[:, off + k:]).all()
                assert np.isnan(Yo[:, :off]).all() and np.isnan(Yo[:, off + k:]).all()


# ----------------------------------------------------------------------------- 4. k = 1, ld = 1 is spmv()
@pytest.mark.parametrize("method", ALL_METHODS, ids=lambda m: m.name)
@pytest.mark.parametrize("name", ["skewed_f64_uniform", "powerlaw_f32_uniform", "uniformk32_f64_uniform", "banded_wide_f32_uniform"])
def test_k1_is_spmv(name, method):
    csr, x, _ = load_golden(name)
    with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method) as h:
        y = np.full(csr.m, np.nan, dtype=x.dtype)
        h.spmv(x, y)
        Y = spmm_host(h, csr, x.reshape(-1, 1).copy())
        assert np.array_equal(Y[:, 0].view(np.uint8), y.view(np.uint8))


# ----------------------------------------------------------------------------- 5. repeat calls, stream and async
def test_repeat_and_async_are_bit_identical():
    import torch
    m, n, rp, ci, va = synth.from_row_lengths_device(synth.powerlaw_lengths_device(300_000, 6.0, 3000, 1.7, DEV, 3), 300_000, "uniform",
                                                     torch.float64, DEV, 3)
    g = torch.Generator(device=DEV); g.manual_seed(5)
    X = torch.rand((n, 12), generator=g, device=DEV, dtype=torch.float64)
    with api.Handle(m, n, rp, ci, va, M.Method_CSR5SPMV) as h:
        a = h.spmm(X)
        b = h.spmm(X)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        s = torch.cuda.Stream()
        h.attach_stream(s.cuda_stream, async_=True)
        c = torch.full_like(a, float("nan"))
        with torch.cuda.stream(s):
            api.spmm(h.h, m, rp, ci, va, X, c)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert torch.equal(a.view(torch.int64), c.view(torch.int64))
        Xh = X.cpu().numpy()
        assert np.array_equal(h.spmm(Xh).view(np.uint8), a.cpu().numpy().view(np.uint8))


# ----------------------------------------------------------------------------- 6. released column copy
def _per_column_spmv(h, X):
    import torch
    ys = []
    for c in range(X.shape[1]):
        y = torch.full((h.m,), float("nan"), dtype=X.dtype, device=DEV)
        h.spmv(X[:, c].contiguous(), y)
        ys.append(y)
    torch.cuda.synchronize()
    return torch.stack(ys, 1)


def _released_fixture():
    import torch
    m, n, rp, ci, va = synth.banded_holes_device(400_000, 400_000, 24, 0.25, "eighths", torch.float64, DEV, 7)
    g = torch.Generator(device=DEV); g.manual_seed(2)
    X = (torch.randint(0, 8, (n, 6), generator=g, device=DEV) * 0.125).double()
    return m, n, rp, ci, va, X


def test_released_columns_are_restored():
    import torch
    m, n, rp, ci, va, X = _released_fixture()
    nnz = int(rp[-1].item())
    api.set_thread_option("keep_columns", 1)
    try:
        with api.Handle(m, n, rp, ci, va, M.Method_Parallel) as hk:
            kept = hk.info()["device_bytes"]
    finally:
        api.clear_thread_options()
    with api.Handle(m, n, rp, ci, va, M.Method_Parallel) as h:
        before = h.info()["device_bytes"]
        assert before <= kept - 4 * nnz, (before, kept)          # create() gave the column copy back
        x0 = X[:, 0].contiguous()
        y_before = torch.empty(m, dtype=torch.float64, device=DEV)
        h.spmv(x0, y_before)
        Y = h.spmm(X)
        torch.cuda.synchronize()
        want = (va[:, None] * X[ci.long()]).view(m, 24, X.shape[1]).sum(1)
        assert torch.equal(Y, want)
        grown = h.info()["device_bytes"] - before
        assert 4 * nnz <= grown <= 4 * nnz + nnz // 64 + 65536, (grown, nnz)
        y_after = torch.empty_like(y_before)
        h.spmv(x0, y_after)
        torch.cuda.synchronize()
        assert torch.equal(y_before.view(torch.int64), y_after.view(torch.int64))


def test_released_columns_are_restored_permuted_on_reorder_handles():
    import torch
    m, n, rp, ci, va, X = _released_fixture()
    nnz = int(rp[-1].item())
    want = (va[:, None] * X[ci.long()]).view(m, 24, X.shape[1]).sum(1)
    api.set_thread_option("reorder", 1)
    try:
        h = api.Handle(m, n, rp, ci, va, M.Method_Parallel)
    finally:
        api.clear_thread_options()
    with h:
        idx = h.index
        assert idx is not None
        idx_d = torch.from_numpy(idx).long().to(DEV)
        before = h.info()["device_bytes"]
        x0 = X[idx_d, 0].contiguous()
        y_before = torch.empty(m, dtype=torch.float64, device=DEV)
        h.spmv(x0, y_before)
        YY = h.spmm(X[idx_d].contiguous())                        # gather X rows by index ...
        torch.cuda.synchronize()
        Y = torch.empty_like(YY)
        Y[idx_d] = YY                                             # ... scatter Y rows by index
        assert torch.equal(Y, want)
        grown = h.info()["device_bytes"] - before
        assert grown <= 4 * nnz + nnz // 64 + 65536, grown
        y_after = torch.empty_like(y_before)
        h.spmv(x0, y_after)
        torch.cuda.synchronize()
        assert torch.equal(y_before.view(torch.int64), y_after.view(torch.int64))


# ----------------------------------------------------------------------------- 7. other handle kinds, value changes, other matrices
def test_split_and_cache_blocked_handles():
    import torch
    m, k = 1_000_000, 32
    _, _, rp, cb, va = synth.banded_device(m, m, k, "eighths", torch.float64, DEV, 1)
    _, _, _, cr, _ = synth.uniform_k_device(m, m, k, "eighths", torch.float64, DEV, 1)
    rows = torch.arange(m, device=DEV)
    ci = torch.where((rows % 10 == 0).repeat_interleave(k), cr, cb)   # partly local: every tenth row random
    g = torch.Generator(device=DEV); g.manual_seed(4)
    X = (torch.randint(0, 8, (m, 5), generator=g, device=DEV) * 0.125).double()
    want = (va[:, None] * X[ci.long()]).view(m, k, 5).sum(1)
    for opts in ({}, {"cache_block": 2}):
        for key, v in opts.items():
            api.set_thread_option(key, v)
        try:
            h = api.Handle(m, m, rp, ci, va, M.Method_Parallel)
        finally:
            api.clear_thread_options()
        with h:
            info = h.info()
            if opts:
                assert info["cache_blocked"] == 1, info
            Y = h.spmm(X)
            torch.cuda.synchronize()
            assert torch.equal(Y, want), (opts, info["far_nnz"])
            assert torch.equal(_per_column_spmv(h, X), want)


def test_value_changes_and_other_matrices():
    import torch
    csr, x, _ = load_golden("skewed_f64_eighths")
    X = block_x(csr, x, 6)
    with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Balanced2) as h:
        check_block(spmm_host(h, csr, X), csr, X, True)
        # spmv_hip_update_values
        v2 = (csr.val * 2).astype(csr.val.dtype)
        h.update_values(v2)
        c2 = synth.CSR(csr.m, csr.n, csr.rowptr, csr.colidx, v2)
        Y = np.full((csr.m, 6), np.nan)
        api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, v2, X, Y)
        check_block(Y, c2, X, True)
    # a host in-place change of the whole value array (option check_values, default 2)
    val = csr.val.copy()
    with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, val, M.Method_Parallel) as h:
        check_block(spmm_host(h, csr, X), csr, X, True)
        val *= 0.5
        check_block(spmm_host(h, synth.CSR(csr.m, csr.n, csr.rowptr, csr.colidx, val), X), synth.CSR(csr.m, csr.n, csr.rowptr, csr.colidx, val), X, True)
        # other CSR pointers (copies, other values): re-inspected, that matrix multiplied
        other = synth.CSR(csr.m, csr.n, csr.rowptr.copy(), csr.colidx.copy(), (csr.val * 0.25).astype(csr.val.dtype))
        Yo = np.full((other.m, 6), np.nan)
        api.spmm(h.h, other.m, other.rowptr, other.colidx, other.val, X, Yo)
        check_block(Yo, other, X, True)


# ----------------------------------------------------------------------------- 8. errors and degenerate shapes
def test_errors_leave_y_untouched():
    import torch
    lib = api.load()
    csr, x, _ = load_golden("banded_f64_uniform")
    X = block_x(csr, x, 4)
    with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Parallel) as h:
        def call(k, px, ldx, py, ldy):
            lib.spmv_hip_clear_error()
            return lib.spmv_hip_spmm(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, k, px, ldx, py, ldy)
        Y = np.full((csr.m, 4), -3.0)
        for args in ((0, X.ctypes.data, 4, Y.ctypes.data, 4), (4, X.ctypes.data, 3, Y.ctypes.data, 4), (4, X.ctypes.data, 4, Y.ctypes.data, 3),
                     (4, None, 4, Y.ctypes.data, 4), (4, X.ctypes.data, 4, None, 4)):
            assert call(*args) == E_ARG, args
            assert lib.spmv_hip_last_error() == E_ARG
            assert (Y == -3.0).all()
    # multi-GPU handle (option gpus) and host_rows handle
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            Y = np.full((csr.m, 4), -3.0)
            assert api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, X, Y, check=False) == E_ARG, key
            api.load().spmv_hip_clear_error()
            assert (Y == -3.0).all()
    # cleared handle
    h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Parallel)
    api.spmv_clear_handle(h.h)
    Y = np.full((csr.m, 4), -3.0)
    assert api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, X, Y, check=False) == E_NOSTATE
    api.load().spmv_hip_clear_error()
    assert (Y == -3.0).all()
    h.close()


def test_empty_shapes_give_zeros():
    for csr in (synth.CSR(0, 5, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)),
                synth.CSR(7, 5, np.zeros(8, np.int32), np.zeros(0, np.int32), np.zeros(0)),
                synth.with_empty_rows(synth.banded(50, 50), lead=3, trail=4, every=5)):
        X = np.random.default_rng(1).uniform(-1, 1, (csr.n, 9))
        with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Parallel) as h:
            Y = spmm_host(h, csr, X)
            assert Y.shape == (csr.m, 9)
            empty = np.diff(csr.rowptr) == 0
            assert (Y[empty] == 0).all() and not np.signbit(Y[empty]).any()
            if csr.nnz:
                check_block(Y, csr, X, False)


# ----------------------------------------------------------------------------- 9. 64-bit offsets
def test_offsets_beyond_int32():
    import torch
    m = 1 << 22
    k, ld = 2, 520
    _, _, rp, ci, va = synth.banded_device(m, m, 8, "eighths", torch.float32, DEV, 5)
    X = torch.zeros((m, ld), dtype=torch.float32, device=DEV)
    g = torch.Generator(device=DEV); g.manual_seed(9)
    X[:, :k] = torch.randint(0, 8, (m, k), generator=g, device=DEV).float() * 0.125
    X[:, k:] = float("nan")
    Y = torch.full((m, ld), float("nan"), dtype=torch.float32, device=DEV)
    assert m * ld > 2**31
    with api.Handle(m, m, rp, ci, va, M.Method_Parallel) as h:
        api.spmm(h.h, m, rp, ci, va, X[:, :k], Y[:, :k])
        torch.cuda.synchronize()
    for r0 in (0, m // 2 - 3, m - 16):
        rows = torch.arange(r0, r0 + 16, device=DEV)
        cols = ci.view(m, 8)[rows].long()
        want = (va.view(m, 8)[rows][:, :, None] * X[cols][:, :, :k]).sum(1)
        assert torch.equal(Y[rows, :k], want), r0
        assert torch.isnan(Y[rows, k:]).all()
    del X, Y
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 10. fuzz
def _fuzz_matrix(rng, seed):
    kind = seed % 5
    m = int(rng.integers(1, 3000))
    n = int(rng.integers(1, 3000))
    dt = np.float64 if seed % 2 else np.float32
    if kind == 0:
        return synth.powerlaw(m, n, 3.0, min(n, 2000), 1.6, "uniform", dt, seed)
    if kind == 1:
        lens = rng.integers(0, 40, m)
        lens[rng.random(m) < 0.02] = rng.integers(500, 3000)
        return synth.from_row_lengths(np.minimum(lens, n), n, "uniform", dt, seed)
    if kind == 2:
        return synth.dense_rows(m, n, sorted(set(rng.integers(0, m, 3).tolist())), 3, "uniform", dt, seed)
    if kind == 3:
        return synth.with_empty_rows(synth.from_row_lengths(rng.integers(0, 20, m), n, "uniform", dt, seed), lead=2, trail=2, every=3)
    return synth.from_row_lengths(rng.integers(0, 60, m), n, "uniform", dt, seed, local=int(rng.integers(1, 50)))


@pytest.mark.parametrize("chunk", range(4))
def test_fuzz(chunk):
    for seed in range(chunk * 50, chunk * 50 + 50):
        rng = np.random.default_rng(seed)
        csr = _fuzz_matrix(rng, seed)
        k = int(rng.integers(1, 41))
        ldx, ldy = k + int(rng.integers(0, 4)), k + int(rng.integers(0, 4))
        X = np.full((csr.n, ldx), np.nan, dtype=csr.val.dtype)
        X[:, :k] = rng.uniform(-1, 1, (csr.n, k))
        Y = np.full((csr.m, ldy), np.nan, dtype=csr.val.dtype)
        method = ALL_METHODS[seed % len(ALL_METHODS)]
        with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method) as h:
            api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, X[:, :k], Y[:, :k])
        check_block(Y[:, :k], csr, X[:, :k], False)
        assert np.isnan(Y[:, k:]).all(), seed


# ----------------------------------------------------------------------------- 11. full size, config-2 shape
def test_config2_shape_k8():
    import torch
    m, k = 10_000_000, 8
    _, _, rp, ci, va = synth.banded_device(m, m, 32, "uniform", torch.float64, DEV, 1)
    g = torch.Generator(device=DEV); g.manual_seed(8)
    X = torch.rand((m, k), generator=g, device=DEV, dtype=torch.float64) * 2 - 1
    with api.Handle(m, m, rp, ci, va, M.Method_Parallel) as h:
        Y = h.spmm(X)
        ref = _per_column_spmv(h, X)
        torch.cuda.synchronize()
        err = (Y - ref).abs()
        assert not torch.isnan(Y).any()
        assert float(err.max()) <= 1e-12 * 32, float(err.max())   # |a|, |x| <= 1: row magnitude <= 32
        t_spmm = float(api.time_spmm_launches(h.h, X, Y, 3, 10)[1].min())
        xs, ys = X[:, 0].contiguous(), torch.empty(m, dtype=torch.float64, device=DEV)
        t_spmv = float(api.time_launches(h.h, xs, ys, 3, 10)[1].min())
    ok = t_spmm <= 0.5 * k * t_spmv
    msg = f"config-2 k=8: spmm {t_spmm:.3f} ms vs 8 x spmv {k * t_spmv:.3f} ms"
    if not ok:
        if os.environ.get("SPMV_TEST_TIMING") == "1":
            raise AssertionError(msg)
        warnings.warn("timing expectation missed (not enforced without SPMV_TEST_TIMING=1): " + msg)
