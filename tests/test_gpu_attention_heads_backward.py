"""GPU: spmv_hip_attention_heads_backward -- dQ, dK, dV of `heads` attention heads in two passes per group of heads (include/spmv_hip.h).

The oracle throughout is api.attention_backward on column-slice views of the same arrays, with NO tolerance: the call promises, head by head, the
bits of the single-head call on the h-th column slices (pointers advanced by h*k and h*dv, the same leading dimensions), and that call's own
bits are pinned to the composition by test_gpu_attention_backward.py.  pattern_a / pattern_b are that file's generators restated: rows (a) and
columns (b) of the lengths LENGTHS cross every boundary of the row pass and of the column pass.

1. every head has the single-head bits   2. rounds (option "attention_backward_heads") change no bit, only device_bytes
3. need, pointer kind, ld / alignment (element and 16-byte form), method, stream change no bit   4. special values stay in their head
5. memory rules on one handle   6. golden patterns   7. handle rules   8. autograd backward="fused"   9. the timer"""
import itertools

import numpy as np
import pytest

from conftest import load_golden
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
METHODS = [M.Method_Parallel, M.Method_Balanced, M.Method_Balanced_Yid, M.Method_CSR5SPMV, M.Method_SellCSigma]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
E_ARG, E_NOSTATE = 3, 5
DEV = "cuda:0"
CANARY = -7.25
N = 300
STREAM_PAD = 4 * 64 + 8   # elements behind the resident ColIdx (kernels/csr_vector4.hpp)
LENGTHS = [0, 1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64, 65, 511, 512, 513, 575, 576, 577, 1025, 2047, 2048, 2049, 4097, 5000]
GOLDENS = ["rowlen_sweep", "single_long", "powerlaw", "empty_mix", "nnz0", "tiny"]
NEEDS = [n for n in itertools.product((True, False), repeat=3)]
OPTION = "attention_backward_heads"


def shapes(dtype):
    """(k, dv) of one head: width 1, an odd width that forces element access, a head wider than a panel in each role"""
    W, KP = (2, 16) if np.dtype(dtype) == np.float64 else (4, 32)
    return [(1, 1), (W + 1, 16 // np.dtype(dtype).itemsize), (8 * W + 1, KP + 1), (KP, 2)]


def scales(dtype, k):
    return [1.0, 0.125, float(dtype(1.0 / np.sqrt(k)))]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


_PAT = {}


def pattern_a(dtype):
    """the rows LENGTHS in a shuffled order, with runs of empty rows at the start, in the middle and at the end; columns in [0, N).  Built
    once per dtype, shared, never changed."""
    key = ("a", np.dtype(dtype))
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


def pattern_b(dtype):
    """pattern A transposed on the host (a stable sort by column): the COLUMNS have the lengths LENGTHS, with the runs of empty columns"""
    key = ("b", np.dtype(dtype))
    if key not in _PAT:
        a = pattern_a(dtype)
        rows = np.repeat(np.arange(a.m, dtype=np.int32), np.diff(a.rowptr))
        order = np.argsort(a.colidx, kind="stable")
        rp = np.zeros(a.n + 1, dtype=np.int32)
        np.cumsum(np.bincount(a.colidx, minlength=a.n), out=rp[1:])
        _PAT[key] = synth.CSR(a.n, a.m, rp, rows[order].copy(), a.val[order].copy())
        assert set(np.bincount(_PAT[key].colidx, minlength=a.m).tolist()) == set(LENGTHS)
    return _PAT[key]


PATTERNS = {"rows": pattern_a, "cols": pattern_b}


def operands(csr, heads, k, dv, seed=0):
    """Q, K, V, G at the full widths, uniform in [-1, 1]"""
    rng = np.random.default_rng(1000 * heads + 100 * k + dv + seed)
    dt = csr.val.dtype
    return tuple(rng.uniform(-1, 1, shape).astype(dt) for shape in ((csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv), (csr.m, heads * dv)))


def handle(csr, method=M.Method_Parallel, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method)
    finally:
        api.clear_thread_options()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def all_same(got, want):
    return all((g is None and w is None) or (g is not None and w is not None and same_bits(g, w)) for g, w in zip(got, want))


def out_shapes(csr, Q, V):
    return (csr.m, Q.shape[1]), (csr.n, Q.shape[1]), (csr.n, V.shape[1])


def heads_host(h, csr, heads, Q, K, V, G, scale, need=(True, True, True), pad=3):
    """the heads call through host pointers, into canary-filled outputs with `pad` extra elements behind every row and a row behind the last;
    -> (dQ, dK, dV)"""
    bufs = [np.full((rows + 1, w + pad), CANARY, dtype=csr.val.dtype) if want else None for want, (rows, w) in zip(need, out_shapes(csr, Q, V))]
    views = [None if b is None else b[:rows, :w] for b, (rows, w) in zip(bufs, out_shapes(csr, Q, V))]
    api.attention_heads_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, G, *views, scale=scale)
    for b, v in zip(bufs, views):
        if b is not None:
            assert (b[:, v.shape[1]:] == CANARY).all() and (b[v.shape[0]] == CANARY).all(), "written outside an output's elements"
    return tuple(None if v is None else v.copy() for v in views)


def head_by_head(h, csr, heads, Q, K, V, G, scale, need=(True, True, True)):
    """the oracle: api.attention_backward once per head on column-slice views of the same arrays, written into slices of full-width outputs"""
    k, dv = Q.shape[1] // heads, V.shape[1] // heads
    outs = [np.full(shape, CANARY, dtype=csr.val.dtype) if want else None for want, shape in zip(need, out_shapes(csr, Q, V))]
    for hd in range(heads):
        ck, cv = slice(hd * k, (hd + 1) * k), slice(hd * dv, (hd + 1) * dv)
        api.attention_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q[:, ck], K[:, ck], V[:, cv], G[:, cv],
                               None if outs[0] is None else outs[0][:, ck], None if outs[1] is None else outs[1][:, ck],
                               None if outs[2] is None else outs[2][:, cv], scale=scale)
    return tuple(outs)


# ----------------------------------------------------------------------------- 1. every head has the single-head bits
@pytest.mark.parametrize("heads", [1, 2, 3, 5])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", list(PATTERNS))
def test_every_head_has_the_single_head_bits(which, dtype, heads):
    csr = PATTERNS[which](dtype)
    with handle(csr) as h:
        for k, dv in shapes(dtype):
            Q, K, V, G = operands(csr, heads, k, dv)
            for scale in scales(dtype, k):
                got = heads_host(h, csr, heads, Q, K, V, G, scale)
                want = head_by_head(h, csr, heads, Q, K, V, G, scale)
                for name, g, w in zip(("dQ", "dK", "dV"), got, want):
                    assert not np.isnan(w).any(), (name, k, dv)
                    assert same_bits(g, w), (name, heads, k, dv, scale)


# ----------------------------------------------------------------------------- 2. rounds change no bit
def device_ops(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def heads_device(h, heads, ops, scale, need=(True, True, True)):
    import torch
    got = h.attention_heads_backward(*ops, heads, scale, need=need)
    torch.cuda.synchronize()
    return tuple(None if g is None else g.cpu().numpy() for g in got)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rounds_change_no_bit_only_memory(dtype):
    import torch
    csr = pattern_a(dtype)
    s = np.dtype(dtype).itemsize
    heads, k, dv = 5, 3, 2
    # the automatic rule on the CPU: the largest HG <= heads with 2 * HG * s * nnz within an eighth of the device's memory
    eighth = torch.cuda.mem_get_info()[1] // 8
    assert min(heads, eighth // (2 * s * csr.nnz)) == 5
    host = operands(csr, heads, k, dv)
    ops = device_ops(host)
    one = [o[:, :w].contiguous() for o, w in zip(ops, (k, k, dv, dv))]
    base = None
    for n in (0, 1, 2, 3, 5, 8):   # rounds of 5, 1+1+1+1+1, 2+2+1, 3+2, 5 and 5
        with handle(csr, **{OPTION: n}) as h:
            assert h.option(OPTION) == n
            h.attention_backward(*one, 0.5)   # a single-head call first: the tables, the transpose and one plane of each array
            torch.cuda.synchronize()
            b0 = h.info()["device_bytes"]
            got = heads_device(h, heads, ops, 0.5)
            planes = heads if n == 0 else min(n, heads)
            assert h.info()["device_bytes"] - b0 == 2 * (planes - 1) * s * csr.nnz, n
            if base is None:
                base = got
                assert all_same(base, head_by_head(h, csr, heads, *host, 0.5))
            assert all_same(got, base), n


# ----------------------------------------------------------------------------- 3. what changes no bit
def _wide(arrays, dtype, pad, off):
    """every array inside a wider one: `off` elements in front of and `pad` behind every row, NaN in every padding element"""
    wide, views = [], []
    for a in arrays:
        wd = np.full((a.shape[0], a.shape[1] + pad + off), np.nan, dtype=dtype)
        wd[:, off:off + a.shape[1]] = a
        wide.append(wd)
        views.append(wd[:, off:off + a.shape[1]])
    return wide, views


def heads_device_wide(h, csr, heads, wide, off, widths, scale, need=(True, True, True)):
    """device operands cut out of the wide arrays; outputs with the same padding, canary-filled; -> (dQ, dK, dV) on the host"""
    import torch
    dev = [torch.from_numpy(wd).to(DEV) for wd in wide]
    ins = [d[:, off:off + w] for d, w in zip(dev, widths)]
    extra = wide[0].shape[1] - widths[0]
    outs, views = [], []
    for want, rows, w in zip(need, (csr.m, csr.n, csr.n), (widths[0], widths[0], widths[2])):
        outs.append(torch.full((rows + 1, w + extra), CANARY, dtype=dev[0].dtype, device=DEV) if want else None)
        views.append(outs[-1][:rows, off:off + w] if want else None)
    api.attention_heads_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, *ins, *views, scale=scale)
    torch.cuda.synchronize()
    res = []
    for o, v in zip(outs, views):
        if o is None:
            res.append(None)
            continue
        oh = o.cpu().numpy()
        res.append(oh[:v.shape[0], off:off + v.shape[1]].copy())
        oh[:v.shape[0], off:off + v.shape[1]] = CANARY
        assert (oh == CANARY).all(), "written outside an output's elements"
    return tuple(res)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_need_pointer_kind_layout_method_and_stream_change_no_bit(dtype):
    import torch
    csr = pattern_a(dtype)
    s = np.dtype(dtype).itemsize
    heads, k, dv = 3, 3 * (16 // s), 2 * (16 // s)   # k * s and dv * s multiples of 16: aligned operands take the 16-byte form
    Q, K, V, G = host = operands(csr, heads, k, dv)
    widths = (heads * k, heads * k, heads * dv, heads * dv)
    scale = 0.125
    with handle(csr) as h:
        base = head_by_head(h, csr, heads, *host, scale)
        assert all(not np.isnan(b).any() for b in base)
        assert all_same(heads_host(h, csr, heads, *host, scale, pad=0), base)       # host pointers
        for need in NEEDS:                                                          # every subset of the wanted outputs
            got = heads_host(h, csr, heads, *host, scale, need=need)
            assert all_same(got, [b if n else None for b, n in zip(base, need)]), need
            got = heads_device_wide(h, csr, heads, host, 0, widths, scale, need=need)
            assert all_same(got, [b if n else None for b, n in zip(base, need)]), need
        # (0, 0), (4, 0): every address and ld a multiple of 16 bytes in fp32, of 32 / 16 in fp64 -- the 16-byte form; an odd pad or an offset
        # of one element: the element form
        for pad, off in ((0, 0), (4, 0), (1, 0), (3, 0), (0, 1), (1, 1), (2, 2)):
            wide, views = _wide(host, dtype, pad, off)
            assert all_same(heads_host(h, csr, heads, *views, scale, pad=pad + off), base), (pad, off)
            assert all_same(heads_device_wide(h, csr, heads, wide, off, widths, scale), base), (pad, off)
        ops = device_ops(host)
        for mix in ((ops[0], K, V, G), (Q, ops[1], V, G), (Q, K, ops[2], G), (Q, K, V, ops[3]), (ops[0], ops[1], V, ops[3])):
            assert all_same(heads_host(h, csr, heads, *mix, scale), base)           # each operand on its own side
        st = torch.cuda.Stream()                                                    # a non-default stream with async
        h.attach_stream(st.cuda_stream, async_=True)
        with torch.cuda.stream(st):
            got = h.attention_heads_backward(*ops, heads, scale)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert [tuple(g.shape) for g in got] == [(csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv)]
        assert all_same([g.cpu().numpy() for g in got], base)
        assert all_same(heads_host(h, csr, heads, *host, scale), base)              # host operands on an asynchronous handle
        want_default = heads_host(h, csr, heads, *host, float(1.0 / np.sqrt(k)))
    for method in METHODS:
        with handle(csr, method) as h:
            assert all_same(heads_host(h, csr, heads, *host, scale), base), method
            assert all_same(h.attention_heads_backward(Q, K, V, G, heads), want_default), method   # scale=None: 1 / sqrt(k) of one head
            got = h.attention_heads_backward(Q, K, V, G, heads, scale, need=(False, True, False))
            assert got[0] is None and got[2] is None and same_bits(got[1], base[1])


# ----------------------------------------------------------------------------- 4. special values stay in their head
def check_bits(out, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan)
    assert same_bits(out[~nan], want[~nan])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values_stay_in_their_head(dtype):
    """heads = 3, k = 1, Q > 0 and K > 0.  In head 1 only: a NaN in Q[i] makes row i's scores NaN, +inf in Q[i] makes them +inf, K[j*] = -inf
    makes a row that holds only column j* all -inf and puts a -inf beside finite scores elsewhere -- each in a short row and in a long one"""
    base = pattern_a(dtype)
    rng = np.random.default_rng(5)
    jstar = 17
    lens = np.diff(base.rowptr)
    row = {n: int(np.flatnonzero(lens == n)[0]) for n in (1, 3, 64, 65, 513, 1025, 2049, 5000)}
    ci = base.colidx.copy()
    ci[base.rowptr[row[1]]] = jstar                                   # only -inf: the short row
    ci[base.rowptr[row[2049]]:base.rowptr[row[2049] + 1]] = jstar     # ... and the long one
    ci[base.rowptr[row[64]] + 40] = jstar                             # -inf beside finite scores
    ci[base.rowptr[row[5000]] + 4000] = jstar
    csr = synth.CSR(base.m, base.n, base.rowptr, ci, base.val)
    heads, dv = 3, 5
    Q = rng.uniform(0.5, 1, (csr.m, heads)).astype(dtype)
    K = rng.uniform(0.5, 1, (csr.n, heads)).astype(dtype)
    V = rng.uniform(-1, 1, (csr.n, heads * dv)).astype(dtype)
    G = rng.uniform(-1, 1, (csr.m, heads * dv)).astype(dtype)
    K[jstar, 1] = -np.inf
    Q[[row[3], row[1025]], 1] = np.nan
    Q[[row[65], row[513]], 1] = np.inf
    with handle(csr) as h:
        got = heads_host(h, csr, heads, Q, K, V, G, 1.0)
        want = head_by_head(h, csr, heads, Q, K, V, G, 1.0)
    for g, w, width in zip(got, want, (1, 1, dv)):
        for hd in (0, 2):
            cols = slice(hd * width, (hd + 1) * width)
            assert not np.isnan(w[:, cols]).any() and not np.isnan(g[:, cols]).any()
            assert same_bits(g[:, cols], w[:, cols]), hd
        cols = slice(width, 2 * width)
        check_bits(g[:, cols], w[:, cols])
        assert np.isnan(w[:, cols]).any()
    assert np.isnan(got[0][[row[1], row[2049], row[3], row[1025], row[65], row[513]], 1]).all()   # all -inf, NaN, +inf: dQ's element of head 1


# ----------------------------------------------------------------------------- 5. memory rules
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_memory_rules(dtype):
    import torch
    lib = api.load()
    csr = pattern_a(dtype)
    s = np.dtype(dtype).itemsize
    heads, k, dv = 3, 5, 4
    host = operands(csr, heads, k, dv)
    ops = device_ops(host)
    one_host = [a[:, :w] for a, w in zip(host, (k, k, dv, dv))]
    one = device_ops(one_host)
    two = 2 * s * csr.nnz
    restored = 4 * (csr.nnz + STREAM_PAD)
    rng = np.random.default_rng(1)
    x, xt, X = rng.uniform(-1, 1, csr.n).astype(dtype), rng.uniform(-1, 1, csr.m).astype(dtype), rng.uniform(-1, 1, (csr.n, 3)).astype(dtype)
    for opts in ({"keep_columns": 1}, {"keep_columns": 0}):
        with handle(csr, **opts) as h:
            h.row_softmax(torch.zeros(csr.nnz, dtype=ops[0].dtype, device=DEV))   # spmm's tables, without touching the columns
            torch.cuda.synchronize()
            y0 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
            b0 = h.info()["device_bytes"]
            # 1. a single-head call: one plane of each array, as before
            dq1 = h.attention_backward(*one, 0.5, need=(True, False, False))[0]
            torch.cuda.synchronize()
            b1 = h.info()["device_bytes"]
            assert b1 - b0 in ((two,) if opts["keep_columns"] else (two, two + restored)), (opts, b1 - b0, two)
            # 2. heads = 3, option 0: three planes
            dq3 = heads_device(h, heads, ops, 0.5, need=(True, False, False))[0]
            b2 = h.info()["device_bytes"]
            assert b2 - b1 == 2 * two   # from 2 * s * nnz to 2 * 3 * s * nnz
            # 3. a second identical call: + 0, the same bits
            assert same_bits(heads_device(h, heads, ops, 0.5, need=(True, False, False))[0], dq3) and h.info()["device_bytes"] == b2
            # 4. dQ alone never builds the transpose
            with pytest.raises(api.SpmvError, match=r"\[5\]"):
                api.get_transpose_info(h.h)
            lib.spmv_hip_clear_error()
            # 5. / 6. the handle's products and every input, before and after a full call through host pointers
            yt0, Y0 = h.spmv_transpose(xt), h.spmm(X)
            keep = h._keep[2]
            bits = [a.tobytes() for a in (*host, csr.rowptr, csr.colidx, csr.val)]
            out = heads_host(h, csr, heads, *host, 0.5)
            assert [a.tobytes() for a in (*host, csr.rowptr, csr.colidx, csr.val)] == bits
            assert same_bits(out[0], dq3) and all_same(out, head_by_head(h, csr, heads, *host, 0.5))
            b3 = h.info()["device_bytes"]
            assert all_same(heads_host(h, csr, heads, *host, 0.5), out) and h.info()["device_bytes"] == b3   # nothing grows with use
            assert h._keep[2] is keep
            assert same_bits(h.spmv(x, np.full(csr.m, np.nan, dtype=dtype)), y0), "spmv() after the call must multiply the handle's own values"
            assert same_bits(h.spmv_transpose(xt), yt0) and same_bits(h.spmm(X), Y0)
            # 7. a single-head call afterwards: its earlier bits, and no plane given back
            again = h.attention_backward(*one, 0.5, need=(True, False, False))[0]
            torch.cuda.synchronize()
            assert same_bits(again.cpu().numpy(), dq1.cpu().numpy()) and h.info()["device_bytes"] == b3
            assert same_bits(dq1.cpu().numpy(), dq3[:, :k])


# ----------------------------------------------------------------------------- 6. golden patterns
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", GOLDENS)
def test_golden_patterns(name, dtype):
    csr = load_golden(f"{name}_{'f64' if dtype == np.float64 else 'f32'}_uniform")[0]
    heads, k, dv = 2, 3, 2
    with handle(csr) as h:
        host = operands(csr, heads, k, dv)
        got = heads_host(h, csr, heads, *host, 0.5)
        want = head_by_head(h, csr, heads, *host, 0.5)
        for g, w in zip(got, want):
            assert not np.isnan(w).any()
            assert same_bits(g, w)
            if csr.nnz == 0:
                assert (g == 0).all() and not np.signbit(g).any()


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
        outs = [torch.full((m, 6), CANARY, dtype=torch.float64, device=DEV) for _ in range(3)]
        lib.spmv_hip_clear_error()
        assert api.attention_heads_backward(h.h, m, rp, ci, va, 2, Q, Q, Q, Q, *outs, check=False) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert all(bool((o == CANARY).all()) for o in outs)


def test_another_matrix_is_inspected_first():
    csr = load_golden("banded_f64_uniform")[0]
    heads, k, dv = 2, 4, 3
    host = operands(csr, heads, k, dv)
    rng = np.random.default_rng(3)
    other = synth.CSR(csr.m, csr.n, csr.rowptr.copy(), np.sort(rng.integers(0, csr.n, csr.nnz).astype(np.int32)), csr.val.copy())
    with handle(csr) as h:
        got = heads_host(h, other, heads, *host, 0.25)   # other CSR arrays: re-inspected first, that matrix's gradients computed
    with handle(other) as ho:
        assert all_same(got, head_by_head(ho, other, heads, *host, 0.25))
    with handle(csr) as hc:
        assert not all_same(got, head_by_head(hc, csr, heads, *host, 0.25))


def test_m0_writes_zero_rows_of_dk_and_dv_at_the_full_widths():
    n, heads, k, dv = 70, 3, 3, 5
    csr = synth.CSR(0, n, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    rng = np.random.default_rng(3)
    Q, G = np.zeros((0, heads * k)), np.zeros((0, heads * dv))
    K, V = rng.uniform(-1, 1, (n, heads * k)), rng.uniform(-1, 1, (n, heads * dv))
    with handle(csr) as h:
        dQ, dK, dV = heads_host(h, csr, heads, Q, K, V, G, 1.0)
    assert dQ.shape == (0, heads * k) and dK.shape == (n, heads * k) and dV.shape == (n, heads * dv)
    for g in (dK, dV):
        assert (g == 0).all() and not np.signbit(g).any()


# ----------------------------------------------------------------------------- 8. autograd
def _device_handle(csr):
    import torch
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    return api.Handle(csr.m, csr.n, rp, ci, va, M.Method_Parallel)


def _small_pattern():
    """12 x 10 with an empty row, a row of one entry and a full row among rows of 2 .. 6 entries"""
    rng = np.random.default_rng(4)
    m, n = 12, 10
    lens = rng.integers(2, 7, m)
    lens[7], lens[3], lens[9] = 0, 1, 10
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(n, int(l), replace=False)) for l in lens]).astype(np.int32)
    return synth.CSR(m, n, rp, ci, rng.uniform(-1, 1, int(rp[-1])))


def _rand(shape, seed):
    import torch
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.rand(shape, generator=g, device=DEV, dtype=torch.float64) * 2 - 1


@pytest.mark.parametrize("heads", [1, 3])
def test_autograd_fused_has_the_default_modes_bits(heads):
    import torch
    from spmv_amd import autograd
    csr = pattern_a(np.float64)
    k, dv = 5, 4
    with _device_handle(csr) as h:
        W = _rand((csr.m, heads * dv), 9)
        for req in ((True, True, True), (False, False, True)):
            grads = {}
            for mode in ("per_head", "fused"):
                Q, K, V = (_rand(shp, i).requires_grad_(r) for i, (shp, r) in enumerate(zip(((csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv)), req)))
                (autograd.attention_heads(h, Q, K, V, heads, backward=mode) * W).sum().backward()
                torch.cuda.synchronize()
                grads[mode] = [t.grad for t in (Q, K, V)]
            for a, b, r in zip(grads["per_head"], grads["fused"], req):
                assert (a is None) == (b is None) == (not r)
                if r:
                    assert not torch.isnan(a).any() and torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_autograd_fused_gradcheck():
    import torch
    from spmv_amd import autograd
    csr = _small_pattern()
    heads, k, dv = 2, 3, 2
    with _device_handle(csr) as h:
        Q, K, V = (_rand(s, i).requires_grad_(True) for i, s in enumerate(((csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv))))
        assert torch.autograd.gradcheck(lambda q, kk, v: autograd.attention_heads(h, q, kk, v, heads, backward="fused"), (Q, K, V))   # default eps / atol / rtol


# ----------------------------------------------------------------------------- 9. the timer
def test_timer_runs_on_device_operands_and_rejects_host_ones():
    import torch
    lib = api.load()
    csr = pattern_a(np.float32)
    heads = 2
    host = operands(csr, heads, 8, 8)
    ops = device_ops(host)
    with handle(csr) as h:
        outs = [torch.empty((rows, heads * 8), dtype=torch.float32, device=DEV) for rows in (csr.m, csr.n, csr.n)]
        mean, ms = api.time_attention_heads_backward_launches(h.h, heads, *ops, *outs, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        assert all_same([o.cpu().numpy() for o in outs], head_by_head(h, csr, heads, *host, 1.0 / np.sqrt(8)))
        mean, ms = api.time_attention_heads_backward_launches(h.h, heads, *ops, outs[0], None, None, warmup=1, iters=2)   # dQ alone
        assert mean > 0
        with pytest.raises(api.SpmvError):
            api.time_attention_heads_backward_launches(h.h, heads, host[0], *ops[1:], *outs, warmup=1, iters=1)
        with pytest.raises(api.SpmvError):
            api.time_attention_heads_backward_launches(h.h, heads, *ops, outs[0], np.empty((csr.n, heads * 8), dtype=np.float32), None, warmup=1, iters=1)
        lib.spmv_hip_clear_error()
