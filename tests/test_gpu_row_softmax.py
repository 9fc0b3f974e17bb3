"""GPU: spmv_hip_row_softmax and spmv_hip_row_softmax_backward over the handle's row structure (include/spmv_hip.h).

Reference: every row in float64 (fp32 handles) or np.longdouble (fp64 handles).  The bars are derived, not measured (u = unit roundoff 2^-24 /
2^-53, d_p = S[p] - M_i, E = 2 ulp for exp / expf -- HIP's math documentation states 1, the second is margin --, tiny = the smallest normal):

forward   |Out[p] - ref[p]| <= 2 u ref[p] (|d_p| + sum_q ref[q] |d_q| + 4 E + len_i) + tiny.
          One rounding in S - M is an absolute error u |d_p| of the exponent, i.e. a relative error u |d_p| of e_p = exp(d_p); exp adds E ulp =
          2 E u; so e_p has relative error u (|d_p| + 2 E).  Z sums len positive terms: (len - 1) u from the additions (any order) plus the
          terms' own errors weighted by their share ref[q], u (sum_q ref[q] |d_q| + 2 E).  One division: u.  The sum of these is at most
          u (|d_p| + sum_q ref[q] |d_q| + 4 E + len); the leading factor 2 covers the second-order terms.
backward  |Out[p] - ref[p]| <= u P[p] (3 (|G[p]| + |D_i|) + (len_i + 2) sum_q |P[q] G[q]|): D is a length-len inner product, gamma_len bound
          len u sum |P G| (any order, fma or not), doubled by the rounding of G - D and of the product (first-order: u |G - D| each, and
          |G - D| <= |G| + |D|), which the factor 3 and the + 2 cover.

Exact properties carry no tolerance: shift invariance on the eighths grid, rows of length 1, -inf beside finite scores, NaN rows and their
neighbours, untouched canaries, and the bits of a row wherever it sits and however the call is made."""
import numpy as np
import pytest

from conftest import load_golden
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
METHODS = [M.Method_Parallel, M.Method_Balanced, M.Method_Balanced_Yid, M.Method_CSR5SPMV, M.Method_SellCSigma]
DTYPES = [np.float64, np.float32]
UNIT = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
WIDE = {np.dtype(np.float64): np.longdouble, np.dtype(np.float32): np.float64}
SPREAD = {np.dtype(np.float64): 600.0, np.dtype(np.float32): 60.0}   # |S - M| at most this: no result is subnormal
E_ULP = 2
E_ARG, E_NOSTATE = 3, 5
DEV = "cuda:0"
CANARY = -7.25
PAD = 8
# every width of the lane groups (1 .. 64), the register chain (64 per step up to 512), the long-row threshold (512), the workgroup (256) and
# the batch (2048) lie between two of these
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65,
           127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025,
           2047, 2048, 2049, 4095, 4096, 4097, 5000, 20000]
GOLDENS = ["rowlen_sweep", "single_long", "powerlaw", "empty_mix", "nnz0", "tiny"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def layout(lengths, order_seed, runs, filler_every, dtype=np.float64, n=64):
    """CSR holding the rows `lengths` in a shuffled order, with runs of empty rows at the start, in the middle and at the end and a filler row
    (length 1 .. 40) after every `filler_every` rows.  -> (csr, where): where[k] = the matrix row of lengths[k]."""
    rng = np.random.default_rng(order_seed)
    order = rng.permutation(len(lengths))
    lens, where = [0] * runs[0], np.zeros(len(lengths), dtype=np.int64)
    for pos, k in enumerate(order):
        if pos == len(order) // 2:
            lens += [0] * runs[1]
        if filler_every and pos % filler_every == filler_every - 1:
            lens.append(int(rng.integers(1, 41)))
        where[k] = len(lens)
        lens.append(lengths[k])
    lens += [0] * runs[2]
    rp = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    nnz = int(rp[-1])
    ci = (np.arange(nnz) * 7 % n).astype(np.int32)   # never read by the operation
    return synth.CSR(len(lens), n, rp, ci, rng.uniform(-1, 1, nnz).astype(dtype)), where


_PAT = {}


def pattern(dtype):
    """the test pattern of one dtype: built once, shared, never changed"""
    key = np.dtype(dtype)
    if key not in _PAT:
        _PAT[key] = layout(LENGTHS, 11, (5, 9, 6), 0, dtype)
    return _PAT[key]


def row_scores(length, dtype, seed, grid=False):
    """scores of one row: a row offset plus a spread of at most SPREAD below it (grid: multiples of 1/8 in [-8, 8])"""
    rng = np.random.default_rng(1000 + seed)
    if grid:
        return (rng.integers(-64, 65, length) * 0.125).astype(dtype)
    return (rng.uniform(-50, 50) - rng.uniform(0, SPREAD[np.dtype(dtype)], length)).astype(dtype)


def scores_for(csr, dtype, seed=0, grid=False):
    S = np.empty(csr.nnz, dtype=dtype)
    for i in range(csr.m):
        a, b = csr.rowptr[i], csr.rowptr[i + 1]
        S[a:b] = row_scores(b - a, dtype, seed * 100003 + i, grid)
    return S


def handle(csr, method=M.Method_Parallel, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method)
    finally:
        api.clear_thread_options()


def forward_host(h, csr, S):
    """through host pointers, into a canary-filled Out with PAD extra elements behind RowPtr[m]"""
    buf = np.full(csr.nnz + PAD, CANARY, dtype=S.dtype)
    api.row_softmax(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, S, buf[:csr.nnz])
    assert (buf[csr.nnz:] == CANARY).all(), "written past the end of Out"
    return buf[:csr.nnz].copy()


def backward_host(h, csr, P, G):
    buf = np.full(csr.nnz + PAD, CANARY, dtype=P.dtype)
    api.row_softmax_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, P, G, buf[:csr.nnz])
    assert (buf[csr.nnz:] == CANARY).all(), "written past the end of Out"
    return buf[:csr.nnz].copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_forward(out, csr, S):
    dt = np.dtype(S.dtype)
    wide, u, tiny = WIDE[dt], UNIT[dt], np.finfo(dt).tiny
    assert out.shape == (csr.nnz,) and out.dtype == dt
    worst = 0.0
    for i in range(csr.m):
        a, b = int(csr.rowptr[i]), int(csr.rowptr[i + 1])
        if a == b:
            continue
        d = S[a:b].astype(wide)
        d = d - d.max()
        e = np.exp(d)
        ref = e / e.sum()
        bar = 2 * u * ref * (np.abs(d) + (ref * np.abs(d)).sum() + 4 * E_ULP + (b - a)) + tiny
        err = np.abs(out[a:b].astype(wide) - ref)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (i, b - a, float((err / bar).max()))
    print(f"forward {dt}: max err / bar = {worst:.3f}")


def check_backward(out, csr, P, G):
    dt = np.dtype(P.dtype)
    wide, u = WIDE[dt], UNIT[dt]
    worst = 0.0
    for i in range(csr.m):
        a, b = int(csr.rowptr[i]), int(csr.rowptr[i + 1])
        if a == b:
            continue
        p, g = P[a:b].astype(wide), G[a:b].astype(wide)
        D = (p * g).sum()
        ref = p * (g - D)
        bar = u * p * (3 * (np.abs(g) + abs(D)) + (b - a + 2) * np.abs(p * g).sum())
        err = np.abs(out[a:b].astype(wide) - ref)
        worst = max(worst, float((err / np.maximum(bar, np.finfo(wide).tiny)).max()))
        assert (err <= bar).all(), (i, b - a)
    print(f"backward {dt}: max err / bar = {worst:.3f}")


def golden_csr(name, dtype):
    return load_golden(f"{name}_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}_uniform")[0]


def one_row(dtype):
    rp = np.array([0, 37], dtype=np.int32)
    return synth.CSR(1, 64, rp, np.arange(37, dtype=np.int32), np.ones(37, dtype=dtype))


# ----------------------------------------------------------------------------- 1. + 4. accuracy, forward and backward
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("method", METHODS, ids=lambda m: m.name)
def test_accuracy_on_the_pattern(method, dtype):
    csr, _ = pattern(dtype)
    S = scores_for(csr, dtype)
    G = np.random.default_rng(8).uniform(-1, 1, csr.nnz).astype(dtype)
    with handle(csr, method) as h:
        P = forward_host(h, csr, S)
        dS = backward_host(h, csr, P, G)
    check_forward(P, csr, S)
    check_backward(dS, csr, P, G)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", GOLDENS + ["one_row"])
def test_accuracy_on_goldens(name, dtype):
    csr = one_row(dtype) if name == "one_row" else golden_csr(name, dtype)
    S = scores_for(csr, dtype, seed=2)
    G = np.random.default_rng(9).uniform(-1, 1, csr.nnz).astype(dtype)
    with handle(csr) as h:
        P = forward_host(h, csr, S)
        dS = backward_host(h, csr, P, G)
        assert h.row_softmax(S).shape == (csr.nnz,)
    check_forward(P, csr, S)
    check_backward(dS, csr, P, G)


# ----------------------------------------------------------------------------- 2. exact properties
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_shift_invariance_is_exact_on_the_eighths_grid(dtype):
    csr, _ = pattern(dtype)
    S = scores_for(csr, dtype, seed=3, grid=True)
    shifts = [1024.0, -4096.0] + ([2.0 ** 20] if dtype == np.float32 else [])   # exp(2^20) overflows fp32: the maximum must be subtracted
    with handle(csr) as h:
        base = forward_host(h, csr, S)
        for c in shifts:
            Sc = (S + dtype(c)).astype(dtype)
            assert np.array_equal(Sc.astype(np.float64) - c, S.astype(np.float64)), "S + c must be exact"
            assert same_bits(forward_host(h, csr, Sc), base), c
    assert np.isfinite(base).all()
    check_forward(base, csr, S)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_rows_of_length_one_give_exactly_one(dtype):
    lens = [1, 0, 1, 1, 5, 1, 0, 0, 1] + [1] * 70 + [600, 1]
    csr, _ = layout(lens, 1, (0, 0, 0), 0, dtype)
    S = scores_for(csr, dtype, seed=4)
    S[0] = np.finfo(dtype).max          # any finite score
    with handle(csr) as h:
        P = forward_host(h, csr, S)
    ones = np.flatnonzero(np.diff(csr.rowptr) == 1)
    assert len(ones) == lens.count(1)
    assert same_bits(P[csr.rowptr[ones]], np.ones(len(ones), dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_special_values_stay_in_their_row(dtype):
    csr, where = pattern(dtype)
    S = scores_for(csr, dtype, seed=5)
    span = lambda length: slice(int(csr.rowptr[where[LENGTHS.index(length)]]), int(csr.rowptr[where[LENGTHS.index(length)] + 1]))
    T = S.copy()
    nan_rows = []
    for length, kind in ((5, "nan"), (65, "nan"), (513, "nan"), (33, "+inf"), (1025, "+inf"), (17, "-inf all"), (129, "-inf all"), (5000, "-inf all"),
                         (1, "nan"), (2, "+inf")):
        sl = span(length)
        if kind == "nan":
            T[sl.start + (length * 2) // 3] = np.nan
        elif kind == "+inf":
            T[sl.start + length // 2] = np.inf
        else:
            T[sl] = -np.inf
        nan_rows.append(sl)
    zero_at = []
    for length in (3, 64, 257, 511, 2049):      # -inf beside finite scores
        sl = span(length)
        for p in (sl.start, sl.start + length // 2, sl.stop - 1)[: 2 if length == 3 else 3]:
            T[p] = -np.inf
            zero_at.append(p)
    touched = np.zeros(csr.nnz, dtype=bool)
    for sl in nan_rows + [span(l) for l in (3, 64, 257, 511, 2049)]:
        touched[sl] = True
    for method in (M.Method_Parallel, M.Method_CSR5SPMV):
        with handle(csr, method) as h:
            base = forward_host(h, csr, S)
            out = forward_host(h, csr, T)
        for sl in nan_rows:
            assert np.isnan(out[sl]).all(), sl
        assert same_bits(out[~touched], base[~touched])              # no other row is affected, bit for bit
        z = out[zero_at]
        assert (z == 0).all() and not np.signbit(z).any()            # exactly +0
        for length in (3, 64, 257, 511, 2049):
            sl = span(length)
            finite = np.isfinite(T[sl])
            assert np.isfinite(out[sl]).all() and (out[sl][finite] > 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_nothing_stored_nothing_written(dtype):
    import torch
    lib = api.load()
    for csr in (golden_csr("nnz0", dtype), synth.CSR(0, 64, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))):
        with handle(csr) as h:
            host = np.full(PAD, CANARY, dtype=dtype)
            dev = torch.full((PAD,), CANARY, dtype=torch.from_numpy(host).dtype, device=DEV)
            for buf in (host, dev):
                lib.spmv_hip_clear_error()
                assert api.row_softmax(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, buf, buf) == 0
                assert api.row_softmax_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, buf, buf, buf) == 0
            assert lib.spmv_hip_row_softmax(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, None, None) == 0
            assert lib.spmv_hip_last_error() == 0
            torch.cuda.synchronize()
            assert (host == CANARY).all() and bool((dev == CANARY).all())
            assert h.row_softmax(host[:0]).shape == (0,)
    # a matrix of empty rows around two stored ones: the canary behind RowPtr[m] stays, on the device too
    csr, _ = layout([0, 0, 3, 0, 0, 0, 70, 0], 2, (4, 3, 5), 0, dtype)
    S = scores_for(csr, dtype, seed=6)
    with handle(csr) as h:
        want = forward_host(h, csr, S)
        dev = torch.full((csr.nnz + PAD,), CANARY, dtype=torch.from_numpy(S).dtype, device=DEV)
        dev[:csr.nnz] = torch.from_numpy(S).to(DEV)
        api.row_softmax(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, dev[:csr.nnz], dev[:csr.nnz])
        torch.cuda.synchronize()
        assert bool((dev[csr.nnz:] == CANARY).all())
        assert same_bits(dev[:csr.nnz].cpu().numpy(), want)
    check_forward(want, csr, S)


# ----------------------------------------------------------------------------- 3. position independence, forward and backward
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_rows_bits_do_not_depend_on_where_it_sits_or_how_it_is_called(dtype):
    import torch
    tdt = torch.from_numpy(np.zeros(1, dtype=dtype)).dtype
    A, whereA = pattern(dtype)
    B, whereB = layout(LENGTHS, 29, (1, 17, 2), 3, dtype)       # another order, other empty-row runs, filler rows between
    assert not np.array_equal(whereA, whereB) and B.m > A.m
    rows = {k: (row_scores(L, dtype, 7000 + k), np.random.default_rng(9000 + k).uniform(-1, 1, L).astype(dtype)) for k, L in enumerate(LENGTHS)}

    def fill(csr, where):
        S, G = scores_for(csr, dtype, seed=12), np.random.default_rng(13).uniform(-1, 1, csr.nnz).astype(dtype)
        for k, L in enumerate(LENGTHS):
            a = int(csr.rowptr[where[k]])
            S[a:a + L], G[a:a + L] = rows[k]
        return S, G

    def gather(csr, where, v):
        return np.concatenate([v[int(csr.rowptr[where[k]]):int(csr.rowptr[where[k]]) + L] for k, L in enumerate(LENGTHS)])

    SA, GA = fill(A, whereA)
    SB, GB = fill(B, whereB)
    with handle(A) as h:
        PA = forward_host(h, A, SA)
        # the backward's P is the same multiset of rows in both matrices: the forward's bits of matrix A, laid out again
        dA = backward_host(h, A, PA, GA)
    want_p, want_d = gather(A, whereA, PA), gather(A, whereA, dA)
    check_forward(PA, A, SA)
    PB_in = np.full(B.nnz, 0.5, dtype=dtype)                    # the filler rows' P: any values
    for k, L in enumerate(LENGTHS):
        a, b = int(A.rowptr[whereA[k]]), int(B.rowptr[whereB[k]])
        PB_in[b:b + L] = PA[a:a + L]
    for method in METHODS:
        with handle(B, method) as h:
            assert same_bits(gather(B, whereB, forward_host(h, B, SB)), want_p), method
            assert same_bits(gather(B, whereB, backward_host(h, B, PB_in, GB)), want_d), method
    for method in METHODS[1:]:
        with handle(A, method) as h:
            assert same_bits(forward_host(h, A, SA), PA), method
            assert same_bits(backward_host(h, A, PA, GA), dA), method
    with handle(A) as h:
        Sd, Pd, Gd = (torch.from_numpy(v).to(DEV) for v in (SA, PA, GA))

        def device_calls(tag):
            out = torch.full((A.nnz + PAD,), CANARY, dtype=tdt, device=DEV)
            api.row_softmax(h.h, A.m, A.rowptr, A.colidx, A.val, Sd, out[:A.nnz])                       # device, out of place
            s2 = Sd.clone()
            api.row_softmax(h.h, A.m, A.rowptr, A.colidx, A.val, s2, s2)                                # device, in place
            bo = torch.full((A.nnz + PAD,), CANARY, dtype=tdt, device=DEV)
            api.row_softmax_backward(h.h, A.m, A.rowptr, A.colidx, A.val, Pd, Gd, bo[:A.nnz])
            g2 = Gd.clone()
            api.row_softmax_backward(h.h, A.m, A.rowptr, A.colidx, A.val, Pd, g2, g2)                   # Out = G
            assert api.load().spmv_hip_synchronize(h.h) == 0
            torch.cuda.synchronize()
            assert bool((out[A.nnz:] == CANARY).all()) and bool((bo[A.nnz:] == CANARY).all())
            for got, want in ((out[:A.nnz], PA), (s2, PA), (bo[:A.nnz], dA), (g2, dA)):
                assert same_bits(got.cpu().numpy(), want), tag

        device_calls("default stream")
        device_calls("second run")
        s_in, g_in = SA.copy(), GA.copy()                                                               # host, in place
        api.row_softmax(h.h, A.m, A.rowptr, A.colidx, A.val, s_in, s_in)
        api.row_softmax_backward(h.h, A.m, A.rowptr, A.colidx, A.val, PA, g_in, g_in)
        assert same_bits(s_in, PA) and same_bits(g_in, dA)
        assert same_bits(h.row_softmax_backward(PA, GA), dA) and same_bits(h.row_softmax(Sd).cpu().numpy(), PA)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        h.attach_stream(side.cuda_stream, async_=True)
        with torch.cuda.stream(side):
            device_calls("side stream, async")
            assert same_bits(forward_host(h, A, SA), PA)


# ----------------------------------------------------------------------------- 5. errors and memory
def test_errors_leave_out_untouched():
    lib = api.load()
    csr = golden_csr("tiny", np.float64)
    S = scores_for(csr, np.float64, seed=1)
    G = np.ones(csr.nnz)
    rp, ci, va = csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data
    with handle(csr) as h:
        out = np.full(csr.nnz, CANARY)
        for f, args in ((lib.spmv_hip_row_softmax, (None, out.ctypes.data)), (lib.spmv_hip_row_softmax, (S.ctypes.data, None)),
                        (lib.spmv_hip_row_softmax_backward, (None, G.ctypes.data, out.ctypes.data)),
                        (lib.spmv_hip_row_softmax_backward, (S.ctypes.data, None, out.ctypes.data)),
                        (lib.spmv_hip_row_softmax_backward, (S.ctypes.data, G.ctypes.data, None))):
            lib.spmv_hip_clear_error()
            assert f(h.h, csr.m, rp, ci, va, *args) == E_ARG, args
            assert lib.spmv_hip_last_error() == E_ARG
            assert (out == CANARY).all()
        lib.spmv_hip_clear_error()
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            out = np.full(csr.nnz, CANARY)
            assert api.row_softmax(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, S, out, check=False) == E_ARG, key
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
            assert api.row_softmax_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, S, G, out, check=False) == E_ARG, key
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
            assert (out == CANARY).all()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    out = np.full(csr.nnz, CANARY)
    assert api.row_softmax(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, S, out, check=False) == E_NOSTATE
    assert api.row_softmax_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, S, G, out, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert (out == CANARY).all()
    h.close()


def test_reorder_handle_is_an_argument_error():
    import torch
    lib = api.load()
    m, n, rp, ci, va = synth.banded_holes_device(100_000, 100_000, 24, 0.25, "eighths", torch.float64, DEV, 7)
    api.set_thread_option("reorder", 1)
    try:
        h = api.Handle(m, n, rp, ci, va, M.Method_Parallel)
    finally:
        api.clear_thread_options()
    with h:
        assert h.index is not None
        nnz = int(rp[-1].item())
        S = torch.zeros(nnz, dtype=torch.float64, device=DEV)
        out = torch.full((nnz,), CANARY, dtype=torch.float64, device=DEV)
        lib.spmv_hip_clear_error()
        assert api.row_softmax(h.h, m, rp, ci, va, S, out, check=False) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        assert api.row_softmax_backward(h.h, m, rp, ci, va, S, S, out, check=False) == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all())


@pytest.mark.parametrize("keep", [0, 1])
def test_only_the_row_structure_is_resident(keep):
    """4096 x 32 banded: the first call builds the batch table, never a ColIdx copy -- device_bytes grows by less than 4 B per non-zero"""
    import torch
    m, k = 4096, 32
    rp = (np.arange(m + 1) * k).astype(np.int32)
    ci = ((np.arange(m)[:, None] + np.arange(k)[None, :]) % m).astype(np.int32).reshape(-1)
    csr = synth.CSR(m, m, rp, ci, np.random.default_rng(1).uniform(-1, 1, m * k))
    S = scores_for(csr, np.float64, seed=7)
    with handle(csr, keep_columns=keep) as h:
        x, y = np.ones(m), np.empty(m)
        h.spmv(x, y)
        before = int(h.info()["device_bytes"])
        Sd = torch.from_numpy(S).to(DEV)
        P = h.row_softmax(Sd)
        dS = h.row_softmax_backward(P, Sd)
        torch.cuda.synchronize()
        grown = int(h.info()["device_bytes"]) - before
        assert 0 <= grown < 4 * csr.nnz, grown
        y2 = np.empty(m)
        h.spmv(x, y2)
        assert same_bits(y, y2)                                      # spmv() computes what it did before
        check_forward(P.cpu().numpy(), csr, S)
        assert dS.shape == (csr.nnz,)
