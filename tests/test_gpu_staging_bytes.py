"""GPU: the accounting of the HBM staging buffers behind host operands, and the six launch timers, on one small handle per precision.

Every operation on the resident matrix takes host or device operands.  A host operand is staged through a handle-owned HBM buffer -- one per
operand, allocated at the first host call and grown only when a later call needs more -- and `spmv_hip_info.device_bytes` counts it.  The
figures asserted here follow from the code, none is measured: an allocation adds exactly the bytes asked for, a buffer that grows gives back
what it held and adds the new size.  With s the value size, A m x n with nnz entries:
  spmv                    s (n + m) at the first host call, nothing afterwards
  spmm, k columns         s k (n + m); a smaller k reuses the buffers, a larger k replaces them
  spmm_transpose, k       s k (m + n), held by the attached transpose and therefore part of the parent's figure
  sddmm, k                s (k m + k n + nnz)
  row_softmax             2 s nnz (S and Out); its backward adds s nnz (G)
Each operation runs on device operands first, so that whatever it builds once per matrix (the batch table, the transpose) exists before the
bytes are read, and the host-operand result must have the bits of that device-operand result.  Method_Serial (CSR-scalar) keeps the resident
ColIdx, so no restore enters the count.

The timers: `warmup = 1`, `iters = 3` give three positive times whose mean is the returned mean, leave no error behind, allocate nothing and
leave the handle synchronous: a host-operand spmv afterwards returns finished data."""
import numpy as np
import pytest
import torch

from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS, COLS = 67, 53
EMPTY_ROWS = (13, ROWS - 1)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def small_matrix(dtype):
    """67 x 53, 3 to 7 entries in a row (5 on average), rows 13 and 66 empty"""
    rng = np.random.default_rng(67053)
    lens = rng.integers(3, 8, size=ROWS)
    lens[list(EMPTY_ROWS)] = 0
    rowptr = np.zeros(ROWS + 1, dtype=np.int32)
    np.cumsum(lens, out=rowptr[1:])
    colidx = np.concatenate([np.sort(rng.choice(COLS, size=n, replace=False)) for n in lens]).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, size=int(rowptr[-1])).astype(dtype)
    return synth.CSR(ROWS, COLS, rowptr, colidx, val)


def dense(rng, shape, dtype):
    return rng.uniform(-1.0, 1.0, size=shape).astype(dtype)


def on_device(a):
    return torch.from_numpy(a).to(DEV)


def same_bits(host, device):
    torch.cuda.synchronize()
    return np.array_equal(np.ascontiguousarray(host).view(np.uint8), device.cpu().numpy().view(np.uint8))


def device_bytes(h):
    return int(h.info()["device_bytes"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_staging_bytes_and_timers(dtype):
    csr = small_matrix(dtype)
    m, n, nnz, s = csr.m, csr.n, int(csr.rowptr[-1]), np.dtype(dtype).itemsize
    assert np.diff(csr.rowptr).min() == 0 and 4.5 <= nnz / m <= 5.5
    rng = np.random.default_rng(5)
    lib = api.load()
    lib.spmv_hip_clear_error()
    with api.Handle(m, n, csr.rowptr, csr.colidx, csr.val, api.SPMV_METHODS.Method_Serial) as h:
        assert h.info()["schedule_name"] == "csr-scalar"

        # ---- spmv: x_stage / y_stage, allocated once
        x = dense(rng, n, dtype)
        xd = on_device(x)
        yd = h.spmv(xd, torch.empty(m, dtype=xd.dtype, device=DEV))
        before = device_bytes(h)
        y = h.spmv(x, np.full(m, np.nan, dtype=dtype))
        assert device_bytes(h) - before == s * (n + m), "spmv"
        assert same_bits(y, yd), "spmv"
        h.spmv(x, y)
        assert device_bytes(h) - before == s * (n + m), "spmv, second host call"

        # ---- spmm: grown only when too small
        X = {k: dense(rng, (n, k), dtype) for k in (4, 2, 8)}
        Yd = {k: h.spmm(on_device(X[k])) for k in X}
        before = device_bytes(h)
        for k, total in ((4, s * 4 * (n + m)), (2, s * 4 * (n + m)), (8, s * 8 * (n + m))):
            Y = h.spmm(X[k], np.full((m, k), np.nan, dtype=dtype))
            assert device_bytes(h) - before == total, ("spmm", k)
            assert same_bits(Y, Yd[k]), ("spmm", k)

        # ---- spmm_transpose: the child's buffers, seen through the parent's info
        Xt = dense(rng, (m, 4), dtype)
        Ytd = h.spmm_transpose(on_device(Xt))
        before = device_bytes(h)
        child_before = int(api.get_transpose_info(h.h)["device_bytes"])
        Yt = h.spmm_transpose(Xt, np.full((n, 4), np.nan, dtype=dtype))
        assert device_bytes(h) - before == s * 4 * (n + m), "spmm_transpose"
        assert int(api.get_transpose_info(h.h)["device_bytes"]) - child_before == s * 4 * (n + m), "spmm_transpose, the child's own figure"
        assert same_bits(Yt, Ytd), "spmm_transpose"

        # ---- sddmm
        U, V = dense(rng, (m, 3), dtype), dense(rng, (n, 3), dtype)
        Od = h.sddmm(on_device(U), on_device(V))
        before = device_bytes(h)
        O = h.sddmm(U, V, np.full(nnz, np.nan, dtype=dtype))
        assert device_bytes(h) - before == s * (3 * m + 3 * n + nnz), "sddmm"
        assert same_bits(O, Od), "sddmm"

        # ---- row_softmax, then its backward
        S, G = dense(rng, nnz, dtype), dense(rng, nnz, dtype)
        Pd = h.row_softmax(on_device(S))
        Bd = h.row_softmax_backward(Pd, on_device(G))
        before = device_bytes(h)
        P = h.row_softmax(S, np.full(nnz, np.nan, dtype=dtype))
        assert device_bytes(h) - before == 2 * s * nnz, "row_softmax"
        assert same_bits(P, Pd), "row_softmax"
        B = h.row_softmax_backward(P, G, np.full(nnz, np.nan, dtype=dtype))
        assert device_bytes(h) - before == 3 * s * nnz, "row_softmax_backward"
        assert same_bits(B, Bd), "row_softmax_backward"

        # ---- the six timers, on device operands of the same handle
        Xd, Xtd, Ud, Vd, Sd = (on_device(a) for a in (X[4], Xt, U, V, S))
        before = device_bytes(h)
        timed = {
            "time_launches": lambda: api.time_launches(h.h, xd, yd, 1, 3),
            "time_spmm_launches": lambda: api.time_spmm_launches(h.h, Xd, Yd[4], 1, 3),
            "time_transpose_launches": lambda: api.time_transpose_launches(h.h, Xtd[:, 0].contiguous(), torch.empty(n, dtype=xd.dtype, device=DEV), 1, 3),
            "time_spmm_transpose_launches": lambda: api.time_spmm_transpose_launches(h.h, Xtd, Ytd, 1, 3),
            "time_sddmm_launches": lambda: api.time_sddmm_launches(h.h, Ud, Vd, Od, 1, 3),
            "time_row_softmax_launches": lambda: api.time_row_softmax_launches(h.h, Sd, Pd, 1, 3),
        }
        for name, run in timed.items():
            mean, ms = run()
            assert ms.shape == (3,) and ms.dtype == np.float32 and (ms > 0).all(), (name, ms)
            # the mean is the double sum of the three floats over 3: to fp32 rounding whatever the order of the additions
            assert abs(float(ms.astype(np.float64).mean()) - mean) <= 2.0 ** -23 * mean, (name, mean, ms)
            assert lib.spmv_hip_last_error() == 0, (name, api.last_error())
            assert device_bytes(h) == before, name
            # the timer switched the handle to asynchronous launches for its own loop only
            again = h.spmv(x, np.full(m, np.nan, dtype=dtype))
            assert np.array_equal(again.view(np.uint8), y.view(np.uint8)), name
