"""GPU: spmv_hip_spmm_transpose, Y = A^T X for k right-hand sides through the k-column executor on the device-built transpose
(include/spmv_hip.h).

Bars: every column against oracle.spmv_exact on the host-built transpose (stable argsort of ColIdx: entries in ascending row of A) --
BIT-EXACT on exact-arithmetic ("eighths") cases, the per-row bars of test_gpu_spmm.check_block otherwise.  Every column has the bits of
Handle(A^T).spmm under the same method; k = 1 with ld = 1 has the bits of spmv_transpose; results do not depend on ld, alignment, the
pointers' kind or the order in which the transpose entry points are first called."""
import json
import os

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
KS = (1, 3, 8, 17, 33)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def transposed(csr):
    """A^T as a CSR whose rows list their entries in ascending row of A (the stable order by column)"""
    order = np.argsort(csr.colidx, kind="stable")
    rows = np.repeat(np.arange(csr.m, dtype=np.int32), np.diff(csr.rowptr))
    rp = np.zeros(csr.n + 1, dtype=np.int32)
    np.cumsum(np.bincount(csr.colidx, minlength=csr.n), out=rp[1:])
    return synth.CSR(csr.n, csr.m, rp, rows[order].astype(np.int32), csr.val[order].copy())


_CACHE = {}


def case(name):
    """(csr, A^T on the host, exact?) of a golden case: computed once, shared, never changed"""
    if name not in _CACHE:
        csr, _, _ = load_golden(name)
        _CACHE[name] = (csr, transposed(csr), name.endswith("eighths"))
    return _CACHE[name]


def block_x(csr, k, exact, seed=11):
    """m x k operand of A^T X in the value kind of the case"""
    X = np.empty((csr.m, k), dtype=csr.val.dtype)
    for c in range(k):
        X[:, c] = synth.fill_x(csr.m, "eighths" if exact else "uniform", csr.val.dtype, seed + 101 * c)
    return X


def check_block(Y, csr, X, exact):
    """test_gpu_spmm.check_block: csr is the matrix that multiplies (here A^T)"""
    assert not np.isnan(Y).any(), f"{int(np.isnan(Y).sum())} entries left unwritten"
    for c in range(X.shape[1]):
        xc = np.ascontiguousarray(X[:, c])
        ye = oracle.spmv_exact(csr, xc)
        yc = np.ascontiguousarray(Y[:, c])
        if exact:
            assert np.array_equal(yc.view(np.uint8), ye.astype(Y.dtype).view(np.uint8)), c
            continue
        s = oracle.row_abs_sum(csr, xc)
        err = np.abs(yc.astype(np.float64) - ye)
        assert (err <= TOL[Y.dtype] * s + 1e-300).all(), (c, float((err / np.maximum(s, 1e-300)).max()))
        assert (err <= SHARP[Y.dtype] * np.maximum(1, np.diff(csr.rowptr)) * s + 1e-300).all(), c


def handle(csr, method=M.Method_Parallel, **opts):
    for k, v in opts.items():
        api.set_thread_option(k, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method)
    finally:
        api.clear_thread_options()


def spmmt_host(h, csr, X):
    Y = np.full((csr.n, X.shape[1]), np.nan, dtype=X.dtype)
    api.spmm_transpose(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, X, Y)
    return Y


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ----------------------------------------------------------------------------- 1. golden cases x methods
@pytest.mark.parametrize("method", ALL_METHODS, ids=lambda m: m.name)
@pytest.mark.parametrize("name", NAMES)
def test_golden(name, method):
    csr, t, exact = case(name)
    with handle(csr, method) as h:
        for k in KS:
            X = block_x(csr, k, exact)
            Y = spmmt_host(h, csr, X)
            assert Y.shape == (csr.n, k)
            check_block(Y, t, X, exact)


# ----------------------------------------------------------------------------- 2. the bits of spmm on a handle created from A^T
@pytest.mark.parametrize("method", ALL_METHODS, ids=lambda m: m.name)
@pytest.mark.parametrize("name", ["banded_wide_f64_uniform", "powerlaw_f32_uniform", "empty_mix_f64_uniform", "dense_row0_f32_uniform",
                                  "single_long_f64_uniform", "nnz0_f32_uniform"])
def test_bits_of_spmm_on_the_explicit_transpose(name, method):
    csr, t, exact = case(name)
    with handle(csr, method) as h, handle(t, method) as ht:
        for k in (3, 17, 33):
            X = block_x(csr, k, exact)
            want = np.full((t.m, k), np.nan, dtype=X.dtype)
            api.spmm(ht.h, t.m, t.rowptr, t.colidx, t.val, X, want)
            assert same_bits(spmmt_host(h, csr, X), want), k


# ----------------------------------------------------------------------------- 3. one vector is spmv_transpose
@pytest.mark.parametrize("method", ALL_METHODS, ids=lambda m: m.name)
@pytest.mark.parametrize("name", ["skewed_f64_uniform", "powerlaw_f32_uniform", "banded_wide_f32_uniform"])
def test_k1_ld1_is_spmv_transpose(name, method):
    csr, _, exact = case(name)
    x = block_x(csr, 1, exact)
    with handle(csr, method) as h:
        y = h.spmv_transpose(np.ascontiguousarray(x[:, 0]))
        assert same_bits(spmmt_host(h, csr, x)[:, 0], y)


# ----------------------------------------------------------------------------- 4. pointers' kind
@pytest.mark.parametrize("name", ["skewed_f32_uniform", "dense_row0_f64_uniform", "empty_mix_f32_uniform"])
def test_device_pointers_give_the_host_bits(name):
    import torch
    csr, t, exact = case(name)
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    with api.Handle(csr.m, csr.n, rp, ci, va, M.Method_Parallel) as hd, handle(csr) as hh:
        for k in (3, 17):
            X = block_x(csr, k, exact)
            Yd = hd.spmm_transpose(torch.from_numpy(X).to(DEV))
            torch.cuda.synchronize()
            assert tuple(Yd.shape) == (csr.n, k)
            Yh = hh.spmm_transpose(X)
            assert same_bits(Yd.cpu().numpy(), Yh), k
            check_block(Yh, t, X, exact)


# ----------------------------------------------------------------------------- 5. padding, leading dimensions, alignment
@pytest.mark.parametrize("name", ["skewed_f64_uniform", "powerlaw_f32_uniform", "banded_wide_f32_uniform"])
def test_padding_and_leading_dimensions(name):
    import torch
    csr, t, exact = case(name)
    with handle(csr) as h:
        for k in (2, 5, 16, 19):
            X = block_x(csr, k, exact)
            base = spmmt_host(h, csr, X)
            check_block(base, t, X, exact)
            for ld, off in ((k, 0), (k + 1, 0), (k + 3, 0), (k + 1, 1), (k + 4, 1)):   # odd ld; off = 1: an 8-byte (fp64) / 4-byte offset view
                Xo = np.full((csr.m, ld + off), np.nan, dtype=X.dtype)
                Xo[:, off:off + k] = X
                Yo = np.full((csr.n, ld + off), -7.25, dtype=X.dtype)
                api.spmm_transpose(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Xo[:, off:off + k], Yo[:, off:off + k])
                assert same_bits(Yo[:, off:off + k], base), (ld, off)          # NaN in X's padding never arrives
                assert (Yo[:, :off] == -7.25).all() and (Yo[:, off + k:] == -7.25).all()   # Y's padding keeps its bits
                Xd = torch.from_numpy(Xo).to(DEV)
                Yd = torch.full((csr.n, ld + off), -7.25, dtype=Xd.dtype, device=DEV)
                api.spmm_transpose(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Xd[:, off:off + k], Yd[:, off:off + k])
                torch.cuda.synchronize()
                got = Yd.cpu().numpy()
                assert same_bits(got[:, off:off + k], base), (ld, off)
                assert (got[:, :off] == -7.25).all() and (got[:, off + k:] == -7.25).all()


# ----------------------------------------------------------------------------- 6. call order, released columns, memory
def _released_fixture():
    import torch
    m, n, rp, ci, va = synth.banded_holes_device(200_000, 200_000, 24, 0.25, "eighths", torch.float64, DEV, 7)
    g = torch.Generator(device=DEV); g.manual_seed(2)
    X = (torch.randint(0, 8, (m, 6), generator=g, device=DEV) * 0.125).double()
    want = torch.zeros((n, 6), dtype=torch.float64, device=DEV).index_add_(0, ci.long(), va[:, None] * X.repeat_interleave(24, 0))
    return m, n, rp, ci, va, X, want


@pytest.mark.parametrize("first", ["spmm_transpose", "spmv_transpose", "prepare_transpose"])
def test_call_orders_and_restored_columns(first):
    import torch
    m, n, rp, ci, va, X, want = _released_fixture()
    nnz = int(rp[-1].item())
    x0 = X[:, 0].contiguous()
    with api.Handle(m, n, rp, ci, va, M.Method_Parallel) as h:          # option keep_columns = 0 (default)
        y_before = torch.empty(m, dtype=torch.float64, device=DEV)
        h.spmv(x0, y_before)
        if first == "spmm_transpose":
            Y = h.spmm_transpose(X)
            yt = h.spmv_transpose(x0)
        else:
            if first == "prepare_transpose":
                api.prepare_transpose(h.h)
            yt = h.spmv_transpose(x0)
            before = h.info()["device_bytes"]
            tinfo = api.get_transpose_info(h.h)
            Y = h.spmm_transpose(X)
            torch.cuda.synchronize()
            grown = h.info()["device_bytes"] - before
            spmm_state = api.get_transpose_info(h.h)["device_bytes"] - tinfo["device_bytes"]
            assert grown == spmm_state, (grown, spmm_state)              # everything new belongs to the transpose
            # the transposed schedule released its columns (every tile of a banded matrix stages): 4 B per non-zero come back (with the
            # 1 KiB tail pad every resident index array has for 16-byte loads); the rest is spmm's batch table (an int per 2048 entries + 1)
            table = 4 * ((nnz + 2047) // 2048 + 1)
            assert 4 * nnz <= grown - table <= 4 * nnz + 2048, (grown, table, nnz)
            again = h.info()["device_bytes"]
            h.spmm_transpose(X)
            assert h.info()["device_bytes"] == again                      # resident from then on
        torch.cuda.synchronize()
        assert torch.equal(Y, want)                                       # eighths: every order gives the same bits
        assert torch.equal(yt, want[:, 0])
        y_after, yt_after = torch.empty_like(y_before), torch.empty_like(yt)
        h.spmv(x0, y_after)
        h.spmv_transpose(x0, yt_after)
        torch.cuda.synchronize()
        assert torch.equal(y_before.view(torch.int64), y_after.view(torch.int64))
        assert torch.equal(yt.view(torch.int64), yt_after.view(torch.int64))


def test_destroy_returns_the_memory():
    import torch
    csr, _, _ = case("skewed_f64_eighths")
    big = synth.from_row_lengths(np.full(40000, 24), 40000, "eighths", np.float64, seed=3)
    Xs = {id(mat): block_x(mat, 5, True) for mat in (csr, big)}

    def cycle():
        for mat in (csr, big):
            for method in ALL_METHODS:
                h = handle(mat, method)
                Y = np.empty((mat.n, 5))
                api.spmm_transpose(h.h, mat.m, mat.rowptr, mat.colidx, mat.val, Xs[id(mat)], Y)      # host staging, batch table, restored columns
                if method == M.Method_CSR5SPMV:
                    api.spmv_clear_handle(h.h)
                h.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    first = cycle()
    for _ in range(2):
        last = cycle()
    assert last >= first - (1 << 20), (first, last)      # nothing accumulates (1 MiB slack for the runtime)


# ----------------------------------------------------------------------------- 7. values follow updates; other handle kinds
def test_values_follow_updates():
    csr, t, _ = case("skewed_f64_eighths")
    X = block_x(csr, 6, True)
    with handle(csr, M.Method_Balanced2) as h:
        check_block(spmmt_host(h, csr, X), t, X, True)
        v2 = (csr.val * 2).astype(csr.val.dtype)
        h.update_values(v2)
        c2 = synth.CSR(csr.m, csr.n, csr.rowptr, csr.colidx, v2)
        Y = np.full((csr.n, 6), np.nan)
        api.spmm_transpose(h.h, csr.m, csr.rowptr, csr.colidx, v2, X, Y)
        check_block(Y, transposed(c2), X, True)
    val = csr.val.copy()  # a host in-place change of the whole array (option check_values, default 2)
    with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, val, M.Method_Parallel) as h:
        Y = np.full((csr.n, 6), np.nan)
        api.spmm_transpose(h.h, csr.m, csr.rowptr, csr.colidx, val, X, Y)
        check_block(Y, t, X, True)
        val *= 0.5
        api.spmm_transpose(h.h, csr.m, csr.rowptr, csr.colidx, val, X, Y)
        check_block(Y, transposed(synth.CSR(csr.m, csr.n, csr.rowptr, csr.colidx, val)), X, True)
        # other CSR pointers: re-inspected, the transpose dropped and rebuilt, that matrix multiplied
        other = synth.CSR(csr.m, csr.n, csr.rowptr.copy(), csr.colidx.copy(), (csr.val * 0.25).astype(csr.val.dtype))
        api.spmm_transpose(h.h, other.m, other.rowptr, other.colidx, other.val, X, Y)
        check_block(Y, transposed(other), X, True)


def test_stream_and_async_are_bit_identical():
    import torch
    csr, t, _ = case("powerlaw_f64_uniform")
    X = block_x(csr, 12, False)
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    Xd = torch.from_numpy(X).to(DEV)
    with api.Handle(csr.m, csr.n, rp, ci, va, M.Method_CSR5SPMV) as h:
        a = h.spmm_transpose(Xd)
        b = h.spmm_transpose(Xd)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        s = torch.cuda.Stream()
        h.attach_stream(s.cuda_stream, async_=True)     # changed after the transpose was built
        c = torch.full_like(a, float("nan"))
        with torch.cuda.stream(s):
            api.spmm_transpose(h.h, csr.m, rp, ci, va, Xd, c)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert torch.equal(a.view(torch.int64), c.view(torch.int64))
        check_block(a.cpu().numpy(), t, X, False)


def test_reorder_handle_index_protocol():
    import torch
    m, n, rp, ci, va, X, want = _released_fixture()
    api.set_thread_option("reorder", 1)
    try:
        h = api.Handle(m, n, rp, ci, va, M.Method_Parallel)
    finally:
        api.clear_thread_options()
    with h:
        idx_d = torch.from_numpy(h.index).long().to(DEV)
        YY = h.spmm_transpose(X[idx_d].contiguous())    # gather X rows by index ...
        torch.cuda.synchronize()
        Y = torch.empty_like(YY)
        Y[idx_d] = YY                                   # ... scatter Y rows by index
        assert torch.equal(Y, want)


# ----------------------------------------------------------------------------- 8. errors and degenerate shapes
def test_errors_leave_y_untouched():
    lib = api.load()
    csr, _, _ = case("banded_f64_uniform")
    X = block_x(csr, 4, False)
    with handle(csr) as h:
        def call(k, px, ldx, py, ldy):
            lib.spmv_hip_clear_error()
            return lib.spmv_hip_spmm_transpose(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, k, px, ldx, py, ldy)
        Y = np.full((csr.n, 4), -3.0)
        for args in ((0, X.ctypes.data, 4, Y.ctypes.data, 4), (4, X.ctypes.data, 3, Y.ctypes.data, 4), (4, X.ctypes.data, 4, Y.ctypes.data, 3),
                     (4, None, 4, Y.ctypes.data, 4), (4, X.ctypes.data, 4, None, 4)):
            assert call(*args) == E_ARG, args
            assert lib.spmv_hip_last_error() == E_ARG
            assert (Y == -3.0).all()
        lib.spmv_hip_clear_error()
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            Y = np.full((csr.n, 4), -3.0)
            assert api.spmm_transpose(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, X, Y, check=False) == E_ARG, key
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
            assert (Y == -3.0).all()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    Y = np.full((csr.n, 4), -3.0)
    assert api.spmm_transpose(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, X, Y, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert (Y == -3.0).all()
    h.close()


def test_empty_shapes_give_zeros():
    for csr in (synth.CSR(0, 5, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)),
                synth.CSR(7, 5, np.zeros(8, np.int32), np.zeros(0, np.int32), np.zeros(0)),
                synth.with_empty_rows(synth.banded(50, 50), lead=3, trail=4, every=5)):
        X = np.random.default_rng(1).uniform(-1, 1, (csr.m, 9))
        with handle(csr) as h:
            Y = spmmt_host(h, csr, X)
            assert Y.shape == (csr.n, 9)
            empty = np.bincount(csr.colidx, minlength=csr.n) == 0
            assert (Y[empty] == 0).all() and not np.signbit(Y[empty]).any()
            if csr.nnz:
                check_block(Y, transposed(csr), X, False)
