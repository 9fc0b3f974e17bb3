"""GPU: spmv_hip_attention_heads -- `heads` attention heads, stored side by side in the rows of Q, K, V and O, in one pass over A's pattern
(include/spmv_hip.h).

The contract is exact: head h's block of O has the bits of spmv_hip_attention on the h-th column slices of the same arrays.  So the oracle
throughout is api.attention on column-slice VIEWS of the very arrays the heads call gets -- no tolerance anywhere.

1. Bits: heads 1, 2, 3, 5; head widths with aligned and misaligned head bases; scale 0.125 and the default 1 / sqrt(k).
2. Padding and alignment: ld = width + 3 with NaN in every padding element, canaries around O, base pointers one element in.
3. Pointer kinds and settings: host and device operands, every method, an attached stream, K and V one buffer, the same call twice.
4. Head isolation: NaN / inf in one head leave the other heads of the same row as they are.
5. Memory: device_bytes does not depend on heads; spmv() is unchanged; keep_columns = 0.
6. Golden patterns.   7. Handle rules."""
import numpy as np
import pytest

from conftest import load_golden
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
METHODS = [M.Method_Parallel, M.Method_Balanced, M.Method_Balanced_Yid, M.Method_CSR5SPMV, M.Method_SellCSigma]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
HEADS = [1, 2, 3, 5]
E_ARG, E_NOSTATE = 3, 5
DEV = "cuda:0"
CANARY = -7.25
N = 300
STREAM_PAD = 4 * 64 + 8   # elements behind the resident ColIdx (kernels/csr_vector4.hpp)
# both sides of: the lane groups (1 .. 64), the register chain (64 per step), the long-row threshold and the LDS chunk (512), the chunk's
# packing of several rows (575 .. 577 beside their neighbours), the 2048 batch and the 64-segment split (ceil(len / 64) changes at 4097)
LENGTHS = [0, 1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64, 65, 511, 512, 513, 575, 576, 577, 1025, 2047, 2048, 2049, 4097, 5000]
GOLDENS = ["rowlen_sweep", "single_long", "powerlaw", "empty_mix", "nnz0", "tiny"]


def widths(dtype):
    """(k, dv) of ONE head: width 1; the 16-byte unit (every head base aligned: the wide access form); one element more (head bases
    misaligned: element accesses when heads > 1); more than a chunk of columns and more than two panels"""
    W, KP = (2, 16) if np.dtype(dtype) == np.float64 else (4, 32)
    return [(1, 1), (W, 16 // np.dtype(dtype).itemsize), (W + 1, KP + 1), (8 * W + 1, 2 * KP + 3)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


_PAT = {}


def pattern(dtype):
    """the rows LENGTHS in a shuffled order, with runs of empty rows at the start, in the middle and at the end; columns in [0, N).  Built
    once per dtype, shared, never changed."""
    key = np.dtype(dtype)
    if key not in _PAT:
        rng = np.random.default_rng(11)
        order = rng.permutation(len(LENGTHS))
        lens = [0] * 5
        for pos, i in enumerate(order):
            if pos == len(order) // 2:
                lens += [0] * 70   # more empty rows than a wave looks at in one step
            lens.append(LENGTHS[i])
        lens += [0] * 6
        rp = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(lens, out=rp[1:])
        nnz = int(rp[-1])
        ci = rng.integers(0, N, nnz).astype(np.int32)
        _PAT[key] = synth.CSR(len(lens), N, rp, ci, rng.uniform(-1, 1, nnz).astype(dtype))
        assert set(np.diff(rp).tolist()) == set(LENGTHS)
    return _PAT[key]


def operands(csr, heads, k, dv, seed=0):
    """Q (m x heads*k), K (n x heads*k), V (n x heads*dv), uniform in [-1, 1]"""
    rng = np.random.default_rng(1000 * heads + 100 * k + dv + seed)
    dt = csr.val.dtype
    return (rng.uniform(-1, 1, (csr.m, heads * k)).astype(dt), rng.uniform(-1, 1, (csr.n, heads * k)).astype(dt),
            rng.uniform(-1, 1, (csr.n, heads * dv)).astype(dt))


def handle(csr, method=M.Method_Parallel, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method)
    finally:
        api.clear_thread_options()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def heads_host(h, csr, heads, Q, K, V, scale, pad=3):
    """the heads call through host pointers, into a canary-filled O with `pad` extra elements behind every row and a row behind the last"""
    w = V.shape[1]
    buf = np.full((csr.m + 1, w + pad), CANARY, dtype=csr.val.dtype)
    api.attention_heads(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, buf[:csr.m, :w], scale)
    assert (buf[:, w:] == CANARY).all() and (buf[csr.m] == CANARY).all(), "written outside O's m x heads*dv elements"
    return buf[:csr.m, :w].copy()


def head_by_head(h, csr, heads, Q, K, V, scale):
    """the oracle: spmv_hip_attention, once per head, on column-slice views of the same arrays, into the column slices of one O"""
    k, dv = Q.shape[1] // heads, V.shape[1] // heads
    out = np.full((csr.m, heads * dv), CANARY, dtype=csr.val.dtype)
    for hd in range(heads):
        ck, cv = slice(hd * k, (hd + 1) * k), slice(hd * dv, (hd + 1) * dv)
        api.attention(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q[:, ck], K[:, ck], V[:, cv], out[:, cv], scale)
    return out


def check_bits(out, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan)
    assert same_bits(out[~nan], want[~nan])


def check_heads(h, csr, heads, k, dv, seed=0):
    """every head block bit for bit, for scale 0.125 and for the default (1 / sqrt(k) of ONE head's k); heads = 1 against the whole arrays"""
    Q, K, V = operands(csr, heads, k, dv, seed)
    for scale in (0.125, None):
        out = heads_host(h, csr, heads, Q, K, V, scale)
        want = head_by_head(h, csr, heads, Q, K, V, 1.0 / np.sqrt(k) if scale is None else scale)
        assert same_bits(out, want), (heads, k, dv, scale)
        if heads == 1:
            whole = np.full_like(out, CANARY)
            api.attention(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q, K, V, whole, scale)
            assert same_bits(out, whole), (k, dv, scale)
        if csr.nnz == 0:
            assert (out == 0).all() and not np.signbit(out).any()
    return out


# ----------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_head_has_the_single_head_bits(dtype, heads):
    csr = pattern(dtype)
    with handle(csr) as h:
        for k, dv in widths(dtype):
            out = check_heads(h, csr, heads, k, dv)
            lens = np.diff(csr.rowptr)
            assert (out[lens == 0] == 0).all() and not np.signbit(out[lens == 0]).any()   # empty rows: +0 in every head


# ----------------------------------------------------------------------------- 2. padding and alignment
@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padding_is_neither_read_nor_written(dtype, heads):
    import torch
    csr = pattern(dtype)
    scale = 0.125
    with handle(csr) as h:
        for k, dv in widths(dtype)[1:3]:   # aligned head bases (the offset view takes the wide form away), misaligned head bases
            Q, K, V = operands(csr, heads, k, dv)
            base = head_by_head(h, csr, heads, Q, K, V, scale)
            w = heads * dv
            for pad, off in ((3, 0), (2, 1)):   # ld = width + 3; off: a view that many elements into the row
                wide = [np.full((a.shape[0], a.shape[1] + pad + off), np.nan, dtype=dtype) for a in (Q, K, V)]   # NaN in every padding element
                views = []
                for wd, a in zip(wide, (Q, K, V)):
                    wd[:, off:off + a.shape[1]] = a
                    views.append(wd[:, off:off + a.shape[1]])
                assert same_bits(heads_host(h, csr, heads, *views, scale, pad=pad + off), base), (k, dv, pad, off)
                dev = [torch.from_numpy(wd).to(DEV) for wd in wide]
                Od = torch.full((csr.m + 1, w + pad + off), CANARY, dtype=dev[0].dtype, device=DEV)
                api.attention_heads(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, *(d[:, off:off + a.shape[1]] for d, a in zip(dev, (Q, K, V))),
                                    Od[:csr.m, off:off + w], scale)
                torch.cuda.synchronize()
                Oh = Od.cpu().numpy()
                assert same_bits(Oh[:csr.m, off:off + w], base), (k, dv, pad, off)
                Oh[:csr.m, off:off + w] = CANARY
                assert (Oh == CANARY).all(), "written outside O's m x heads*dv elements"


# ----------------------------------------------------------------------------- 3. pointer kinds and settings
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pointer_kind_method_and_stream_change_no_bit(dtype):
    import torch
    csr = pattern(dtype)
    heads = 3
    k = dv = widths(dtype)[2][0]   # misaligned head bases
    Q, K, V = operands(csr, heads, k, dv)
    scale = 0.125
    with handle(csr) as h:
        base = head_by_head(h, csr, heads, Q, K, V, scale)
        assert same_bits(heads_host(h, csr, heads, Q, K, V, scale), base)
        assert same_bits(heads_host(h, csr, heads, Q, K, V, scale), base)          # the same call twice: nothing of the last head is left over
        Qd, Kd, Vd = (torch.from_numpy(a).to(DEV) for a in (Q, K, V))
        for q, kk, v in ((Qd, K, V), (Q, Kd, V), (Q, K, Vd), (Qd, Kd, Vd)):        # each operand on its own side
            assert same_bits(heads_host(h, csr, heads, q, kk, v, scale), base)
        od = h.attention_heads(Qd, Kd, Vd, heads, scale)                           # all four on the device, twice
        od2 = h.attention_heads(Qd, Kd, Vd, heads, scale)
        torch.cuda.synchronize()
        assert tuple(od.shape) == (csr.m, heads * dv) and same_bits(od.cpu().numpy(), base) and same_bits(od2.cpu().numpy(), base)
        # K and V the same buffer (k == dv)
        kv = head_by_head(h, csr, heads, Q, K, K.copy(), scale)
        assert same_bits(heads_host(h, csr, heads, Q, K, K, scale), kv)
        okv = h.attention_heads(Qd, Kd, Kd, heads, scale)
        torch.cuda.synchronize()
        assert same_bits(okv.cpu().numpy(), kv)
        # an attached stream with async
        s = torch.cuda.Stream()
        h.attach_stream(s.cuda_stream, async_=True)
        with torch.cuda.stream(s):
            o = h.attention_heads(Qd, Kd, Vd, heads, scale)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert same_bits(o.cpu().numpy(), base)
        assert same_bits(heads_host(h, csr, heads, Q, K, V, scale), base)          # host operands on an asynchronous handle
    for method in METHODS:
        with handle(csr, method) as h:
            assert same_bits(heads_host(h, csr, heads, Q, K, V, scale), base), method


# ----------------------------------------------------------------------------- 4. head isolation
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values_stay_in_their_head(dtype):
    """k = 1, three heads, Q and K > 0.  Head 1: NaN in Q at a row of 3 and at a row of 513 entries.  Head 2: +inf in Q at a row of 65.  Head
    0: -inf in K at one column (a -inf score beside finite ones, and the only score of a row of length 1)."""
    base = pattern(dtype)
    rng = np.random.default_rng(5)
    heads, dv, jstar = 3, 5, 17
    lens = np.diff(base.rowptr)
    r1, r3, r65, r513, r5000 = (int(np.flatnonzero(lens == n)[0]) for n in (1, 3, 65, 513, 5000))
    ci = base.colidx.copy()
    ci[base.rowptr[r1]] = jstar
    ci[base.rowptr[r65] + 40] = jstar
    ci[base.rowptr[r5000] + 4000] = jstar
    csr = synth.CSR(base.m, base.n, base.rowptr, ci, base.val)
    Q = rng.uniform(0.5, 1, (csr.m, heads)).astype(dtype)
    K = rng.uniform(0.5, 1, (csr.n, heads)).astype(dtype)
    V = rng.uniform(-1, 1, (csr.n, heads * dv)).astype(dtype)
    Qs, Ks = Q.copy(), K.copy()
    Qs[r3, 1] = Qs[r513, 1] = np.nan
    Qs[r65, 2] = np.inf
    Ks[jstar, 0] = -np.inf
    with handle(csr) as h:
        clean = heads_host(h, csr, heads, Q, K, V, 1.0)
        out = heads_host(h, csr, heads, Qs, Ks, V, 1.0)
        want = head_by_head(h, csr, heads, Qs, Ks, V, 1.0)
    check_bits(out, want)
    blocks = [out[:, hd * dv:(hd + 1) * dv] for hd in range(heads)]
    has_j = np.array([jstar in ci[csr.rowptr[i]:csr.rowptr[i + 1]] for i in range(csr.m)])
    expect = [has_j & (lens == 1), np.isin(np.arange(csr.m), [r3, r513]), np.arange(csr.m) == r65]   # the NaN rows of each head: those and only those
    for hd in range(heads):
        nan_rows = np.isnan(blocks[hd]).any(1)
        assert np.array_equal(nan_rows, expect[hd]), hd
        assert np.isnan(blocks[hd][nan_rows]).all()
    # the heads that were not touched: the bits of the clean run -- head 0 wherever column jstar is not in the row, heads 1 and 2 outside their rows
    untouched = [~has_j, ~expect[1], ~expect[2]]
    for hd in range(heads):
        assert same_bits(blocks[hd][untouched[hd]], clean[:, hd * dv:(hd + 1) * dv][untouched[hd]]), hd
    assert not np.isnan(blocks[2][[r3, r513]]).any() and not np.isnan(blocks[1][r65]).any() and not np.isnan(blocks[0][r65]).any()


# ----------------------------------------------------------------------------- 5. memory
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_memory_does_not_depend_on_heads(dtype):
    import torch
    csr = pattern(dtype)
    s = np.dtype(dtype).itemsize
    k, dv = 4, 8
    x = np.random.default_rng(1).uniform(-1, 1, csr.n).astype(dtype)
    lens = np.diff(csr.rowptr)
    nlong, long_sum = int((lens > 512).sum()), int(lens[lens > 512].sum())
    nb = -(-csr.nnz // 2048)
    tables = 4 * (nb + 1) + 4 * nlong + 4 * (nlong + 1) + s * long_sum   # spmm's batch table and long-row list, the parked rows' offsets and space
    restored = 4 * (csr.nnz + STREAM_PAD)
    for keep in (1, 0):
        grown = {}
        for heads in (4, 1):
            Qd, Kd, Vd = (torch.from_numpy(a).to(DEV) for a in operands(csr, heads, k, dv))
            with handle(csr, keep_columns=keep) as h:
                y0 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
                b0 = h.info()["device_bytes"]
                od = h.attention_heads(Qd, Kd, Vd, heads, 0.5)
                torch.cuda.synchronize()
                grown[heads] = h.info()["device_bytes"] - b0
                od2 = h.attention_heads(Qd, Kd, Vd, heads, 0.5)
                torch.cuda.synchronize()
                assert h.info()["device_bytes"] - b0 == grown[heads]   # once: nothing grows with use
                assert same_bits(od.cpu().numpy(), od2.cpu().numpy())
                y1 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
                assert same_bits(y0, y1), "spmv() after the call must multiply the handle's own values"
        assert grown[4] == grown[1], (keep, grown)
        assert grown[4] in ((tables,) if keep else (tables, tables + restored)), (keep, grown, tables)   # spmv_hip_attention's rule
    with handle(csr, keep_columns=0) as h, handle(csr, keep_columns=0) as h1:   # ... and exactly what the single-head call adds
        b0, b1 = h.info()["device_bytes"], h1.info()["device_bytes"]
        Qd, Kd, Vd = (torch.from_numpy(a).to(DEV) for a in operands(csr, 4, k, dv))
        h.attention_heads(Qd, Kd, Vd, 4, 0.5)
        h1.attention(Qd, Kd, Vd, 0.5)
        torch.cuda.synchronize()
        assert h.info()["device_bytes"] - b0 == h1.info()["device_bytes"] - b1


# ----------------------------------------------------------------------------- 6. golden patterns
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", GOLDENS)
def test_golden_patterns(name, dtype):
    csr = load_golden(f"{name}_{'f64' if dtype == np.float64 else 'f32'}_uniform")[0]
    with handle(csr) as h:
        for k, dv in widths(dtype):
            check_heads(h, csr, 2, k, dv)


# ----------------------------------------------------------------------------- 7. handle rules
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
        Q = torch.ones((m, 6), dtype=torch.float64, device=DEV)
        out = torch.full((m, 6), CANARY, dtype=torch.float64, device=DEV)
        lib.spmv_hip_clear_error()
        assert api.attention_heads(h.h, m, rp, ci, va, 2, Q, Q, Q, out, check=False) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all())


def test_errors_leave_o_untouched_and_another_matrix_is_inspected_first():
    lib = api.load()
    csr = load_golden("banded_f64_uniform")[0]
    heads, k, dv = 2, 4, 3
    Q, K, V = operands(csr, heads, k, dv)
    with handle(csr) as h:
        O = np.full((csr.m, heads * dv), CANARY)
        q, kk, v, o = Q.ctypes.data, K.ctypes.data, V.ctypes.data, O.ctypes.data

        def call(nh, k, dv, pq, ldq, pk, ldk, pv, ldv, po, ldo):
            lib.spmv_hip_clear_error()
            return lib.spmv_hip_attention_heads(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, nh, k, dv, 1.0,
                                                pq, ldq, pk, ldk, pv, ldv, po, ldo)
        for args in ((0, 4, 3, q, 8, kk, 8, v, 6, o, 6), (2, 0, 3, q, 8, kk, 8, v, 6, o, 6), (2, 4, 0, q, 8, kk, 8, v, 6, o, 6),
                     (2, 4, 3, q, 7, kk, 8, v, 6, o, 6), (2, 4, 3, q, 8, kk, 7, v, 6, o, 6), (2, 4, 3, q, 8, kk, 8, v, 5, o, 6),
                     (2, 4, 3, q, 8, kk, 8, v, 6, o, 5), (2 ** 30, 4, 3, q, 2 ** 40, kk, 2 ** 40, v, 2 ** 40, o, 2 ** 40),
                     (2, 4, 3, None, 8, kk, 8, v, 6, o, 6), (2, 4, 3, q, 8, None, 8, v, 6, o, 6), (2, 4, 3, q, 8, kk, 8, None, 6, o, 6),
                     (2, 4, 3, q, 8, kk, 8, v, 6, None, 6)):
            assert call(*args) == E_ARG, args
            assert lib.spmv_hip_last_error() == E_ARG
            assert (O == CANARY).all()
        lib.spmv_hip_clear_error()
        # other CSR arrays (a copy of the pattern with other columns): re-inspected first, that matrix's attention computed
        rng = np.random.default_rng(3)
        other = synth.CSR(csr.m, csr.n, csr.rowptr.copy(), np.sort(rng.integers(0, csr.n, csr.nnz).astype(np.int32)), csr.val.copy())
        got = heads_host(h, other, heads, Q, K, V, 0.25)
        with handle(other) as ho:
            assert same_bits(got, head_by_head(ho, other, heads, Q, K, V, 0.25))
        with handle(csr) as hc:
            assert not same_bits(got, head_by_head(hc, csr, heads, Q, K, V, 0.25))
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            O = np.full((csr.m, heads * dv), CANARY)
            assert api.attention_heads(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, O, check=False) == E_ARG, key
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
            assert (O == CANARY).all()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    O = np.full((csr.m, heads * dv), CANARY)
    assert api.attention_heads(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, O, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert (O == CANARY).all()
    h.close()


def test_timer_runs_on_device_operands():
    import torch
    csr = pattern(np.float32)
    heads, k, dv = 4, 8, 8
    Qh, Kh, Vh = operands(csr, heads, k, dv)
    Q, K, V = (torch.from_numpy(a).to(DEV) for a in (Qh, Kh, Vh))
    with handle(csr) as h:
        O = torch.empty((csr.m, heads * dv), dtype=torch.float32, device=DEV)
        mean, ms = api.time_attention_heads_launches(h.h, heads, Q, K, V, O, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        assert same_bits(O.cpu().numpy(), head_by_head(h, csr, heads, Qh, Kh, Vh, 1.0 / np.sqrt(k)))
        with pytest.raises(api.SpmvError):   # device pointers only
            api.time_attention_heads_launches(h.h, heads, Qh, Kh, Vh, O, warmup=0, iters=1)
