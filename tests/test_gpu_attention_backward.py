"""GPU: spmv_hip_attention_backward -- dQ, dK, dV of O = softmax_rows(scale * Q K^T on A's pattern) V in two passes over A (include/spmv_hip.h).

1. Bits.  The call promises the composition's result step by step, so dQ, dK and dV are compared BIT FOR BIT with the composition made from
   the library's own calls on numpy arrays: Handle.sddmm(Q, K), `* dtype(scale)`, Handle.row_softmax, Handle.sddmm(G, V),
   Handle.row_softmax_backward, `* dtype(scale)`, api.spmm on a second handle holding dS, api.spmm_transpose on second handles holding P and
   dS (every second-handle output has ld = width + 2, so that width 1 does not take the spmv schedule).  With these inputs the composition
   holds no NaN, which is asserted: the comparison leaves no element out.
   Pattern A has the row lengths that cross every boundary of the row pass; pattern B is its transpose, so its COLUMNS have those lengths
   and cross every boundary of the column pass.
2. Special scores: a NaN, a +inf and a -inf placed as in test_gpu_fused_attention.py; NaN positions and all other bits equal the composition's.
3. Invariance: host and device pointers, padded ld with NaN in every padding element, misaligned base pointers, every method, stream and
   async settings, K and V the same pointer, repeated calls, every subset of the wanted outputs -- identical bits.
4. Memory rules: canaries, inputs, spmv() / spmv_transpose() / spmm before and after, the handle's values, device_bytes.
5. Golden patterns through 1.   6. Handle rules."""
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
# both sides of: the lane groups (1 .. 64), the register chain (64 per step), the long-row threshold and the LDS chunk (512), the chunk's
# packing of several rows (575 .. 577 beside their neighbours), the 2048 batch and the 64-segment split (ceil(len / 64) changes at 4097)
LENGTHS = [0, 1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64, 65, 511, 512, 513, 575, 576, 577, 1025, 2047, 2048, 2049, 4097, 5000]
GOLDENS = ["rowlen_sweep", "single_long", "powerlaw", "empty_mix", "nnz0", "tiny"]
NEEDS = [n for n in itertools.product((True, False), repeat=3)]


def shapes(dtype):
    """(k, dv, scale) triples: test_gpu_fused_attention.py's rule"""
    W, KP = (2, 16) if np.dtype(dtype) == np.float64 else (4, 32)
    ks = [1, W, W + 1, 4 * W + 1, 8 * W, 8 * W + 1, 33]
    dvs = [1, 16 // np.dtype(dtype).itemsize, KP - 1, KP, KP + 1, 2 * KP + 3, 2 * KP + 3]
    scales = [1.0, 0.125, None, 1.0, 0.125, None, None]   # None: 1 / sqrt(k) rounded to dtype
    return [(k, dv, float(dtype(1.0 / np.sqrt(k))) if s is None else s) for k, dv, s in zip(ks, dvs, scales)]


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
    """pattern A transposed on the host (a stable sort by column): N rows of about 75 entries; the COLUMNS have the lengths LENGTHS, with the runs
    of empty columns"""
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


def operands(csr, k, dv, seed=0):
    """Q, K, V, G uniform in [-1, 1]"""
    rng = np.random.default_rng(100 * k + dv + seed)
    dt = csr.val.dtype
    return tuple(rng.uniform(-1, 1, shape).astype(dt) for shape in ((csr.m, k), (csr.n, k), (csr.n, dv), (csr.m, dv)))


def handle(csr, method=M.Method_Parallel, val=None, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val if val is None else val, method)
    finally:
        api.clear_thread_options()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def all_same(got, want):
    return all((g is None and w is None) or same_bits(g, w) for g, w in zip(got, want))


def fused_host(h, csr, Q, K, V, G, scale, need=(True, True, True), pad=3):
    """through host pointers, into canary-filled outputs with `pad` extra elements behind every row and a row behind the last; -> (dQ, dK, dV)"""
    k, dv = Q.shape[1], V.shape[1]
    bufs = []
    for want, rows, width in zip(need, (csr.m, csr.n, csr.n), (k, k, dv)):
        bufs.append(np.full((rows + 1, width + pad), CANARY, dtype=csr.val.dtype) if want else None)
    views = [None if b is None else b[:rows, :width] for b, rows, width in zip(bufs, (csr.m, csr.n, csr.n), (k, k, dv))]
    api.attention_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q, K, V, G, *views, scale=scale)
    for b, v in zip(bufs, views):
        if b is not None:
            assert (b[:, v.shape[1]:] == CANARY).all() and (b[v.shape[0]] == CANARY).all(), "written outside an output's elements"
    return tuple(None if v is None else v.copy() for v in views)


def composition(h, csr, Q, K, V, G, scale):
    """the calls the fused one replaces, on the library's kernels; P and dS live on second handles; -> (dQ, dK, dV)"""
    dt, k, dv = Q.dtype.type, Q.shape[1], V.shape[1]
    if csr.nnz == 0:
        return np.zeros((csr.m, k), dtype=dt), np.zeros((csr.n, k), dtype=dt), np.zeros((csr.n, dv), dtype=dt)
    with np.errstate(all="ignore"):
        P = h.row_softmax(h.sddmm(Q, K) * dt(scale))
        dS = h.row_softmax_backward(P, h.sddmm(G, V)) * dt(scale)
    dQ, dK, dV = (np.full((rows, w + 2), CANARY, dtype=dt) for rows, w in ((csr.m, k), (csr.n, k), (csr.n, dv)))
    with handle(csr, val=dS) as hs:
        api.spmm(hs.h, csr.m, csr.rowptr, csr.colidx, dS, K, dQ[:, :k])
        api.spmm_transpose(hs.h, csr.m, csr.rowptr, csr.colidx, dS, Q, dK[:, :k])
    with handle(csr, val=P) as hp:
        api.spmm_transpose(hp.h, csr.m, csr.rowptr, csr.colidx, P, G, dV[:, :dv])
    return dQ[:, :k].copy(), dK[:, :k].copy(), dV[:, :dv].copy()


def check_bits(out, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan)
    assert same_bits(out[~nan], want[~nan])


# ----------------------------------------------------------------------------- 1. the composition's bits
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", list(PATTERNS))
def test_bits_equal_the_composition(which, dtype):
    csr = PATTERNS[which](dtype)
    with handle(csr) as h:
        for k, dv, scale in shapes(dtype):
            Q, K, V, G = operands(csr, k, dv)
            got = fused_host(h, csr, Q, K, V, G, scale)
            want = composition(h, csr, Q, K, V, G, scale)
            for name, g, w in zip(("dQ", "dK", "dV"), got, want):
                assert not np.isnan(w).any(), (name, k, dv)
                assert same_bits(g, w), (name, k, dv, scale)


# ----------------------------------------------------------------------------- 2. special scores
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_scores(dtype):
    """k = 1, Q > 0: a NaN in Q[i] makes row i's scores NaN, +inf in Q[i] makes them +inf (or -inf), K[j*] = -inf puts a -inf beside finite scores
    in every row that holds column j* and makes a row that holds nothing else all -inf"""
    base = pattern_a(dtype)
    rng = np.random.default_rng(5)
    jstar = 17
    lens = np.diff(base.rowptr)
    rows = [int(np.flatnonzero(lens == n)[0]) for n in (1, 3, 65, 513, 5000)]
    ci = base.colidx.copy()
    ci[base.rowptr[rows[0]]] = jstar          # the row of length 1: only -inf
    ci[base.rowptr[rows[2]] + 40] = jstar     # -inf beside finite scores, short and long rows
    ci[base.rowptr[rows[4]] + 4000] = jstar
    csr = synth.CSR(base.m, base.n, base.rowptr, ci, base.val)
    dv = 5
    Q = rng.uniform(0.5, 1, (csr.m, 1)).astype(dtype)
    K = rng.uniform(0.5, 1, (csr.n, 1)).astype(dtype)
    V = rng.uniform(-1, 1, (csr.n, dv)).astype(dtype)
    G = rng.uniform(-1, 1, (csr.m, dv)).astype(dtype)
    K[jstar] = -np.inf
    Q[rows[1]] = np.nan
    Q[rows[3]] = np.inf
    with handle(csr) as h:
        got = fused_host(h, csr, Q, K, V, G, 1.0)
        want = composition(h, csr, Q, K, V, G, 1.0)
    for g, w in zip(got, want):
        check_bits(g, w)
    assert np.isnan(got[0][[rows[0], rows[1], rows[3]]]).all()   # all -inf, NaN, +inf: the whole row of dQ
    assert np.isnan(got[0][[rows[2], rows[4]]]).all()            # a -inf K row met by an exact zero dS: 0 * inf in dQ's chain
    assert all(np.isnan(w).any() and not np.isnan(w).all() for w in want)


# ----------------------------------------------------------------------------- 3. invariance
def _wide(arrays, dtype, pad, off):
    """every array inside a wider one: `off` elements in front of and `pad` behind every row, NaN in every padding element"""
    wide, views = [], []
    for a in arrays:
        wd = np.full((a.shape[0], a.shape[1] + pad + off), np.nan, dtype=dtype)
        wd[:, off:off + a.shape[1]] = a
        wide.append(wd)
        views.append(wd[:, off:off + a.shape[1]])
    return wide, views


def fused_device(h, csr, wide, off, widths, scale, need=(True, True, True)):
    """device operands cut out of the wide arrays; outputs with the same padding, canary-filled; -> (dQ, dK, dV) on the host"""
    import torch
    dev = [torch.from_numpy(wd).to(DEV) for wd in wide]
    ins = [d[:, off:off + w] for d, w in zip(dev, widths)]
    extra = wide[0].shape[1] - widths[0]
    outs, views = [], []
    for want, rows, w in zip(need, (csr.m, csr.n, csr.n), (widths[0], widths[0], widths[2])):
        outs.append(torch.full((rows + 1, w + extra), CANARY, dtype=dev[0].dtype, device=DEV) if want else None)
        views.append(outs[-1][:rows, off:off + w] if want else None)
    api.attention_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, *ins, *views, scale=scale)
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
def test_layout_pointer_kind_method_stream_and_need_change_no_bit(dtype):
    import torch
    csr = pattern_a(dtype)
    KP = 16 if dtype == np.float64 else 32
    k = dv = KP + 1
    Q, K, V, G = operands(csr, k, dv)
    scale = 0.125
    with handle(csr) as h:
        base = fused_host(h, csr, Q, K, V, G, scale)
        assert all_same(fused_host(h, csr, Q, K, V, G, scale), base)                # repeated
        for need in NEEDS:                                                          # a gradient asked for alone or beside others: the same bits
            got = fused_host(h, csr, Q, K, V, G, scale, need=need)
            assert all_same(got, [b if n else None for b, n in zip(base, need)]), need
        for pad, off in ((0, 0), (1, 0), (3, 0), (4, 0), (1, 1), (2, 2), (3, 3)):   # off: a view that many elements into the row
            wide, views = _wide((Q, K, V, G), dtype, pad, off)
            assert all_same(fused_host(h, csr, *views, scale, pad=pad + off), base), (pad, off)
            assert all_same(fused_device(h, csr, wide, off, (k, k, dv, dv), scale), base), (pad, off)
        wide, _ = _wide((Q, K, V, G), dtype, 0, 0)
        for need in ((True, False, False), (False, True, False), (False, False, True)):
            assert all_same(fused_device(h, csr, wide, 0, (k, k, dv, dv), scale, need=need), [b if n else None for b, n in zip(base, need)]), need
        # each operand on its own side
        Qd, Kd, Vd, Gd = (torch.from_numpy(a).to(DEV) for a in (Q, K, V, G))
        for ops in ((Qd, K, V, G), (Q, Kd, V, G), (Q, K, Vd, G), (Q, K, V, Gd), (Qd, Kd, V, Gd)):
            assert all_same(fused_host(h, csr, *ops, scale), base)
        # K and V the same pointer (k == dv)
        kv = fused_host(h, csr, Q, K, K.copy(), G, scale)
        assert all_same(fused_host(h, csr, Q, K, K, G, scale), kv)
        got = h.attention_backward(Qd, Kd, Kd, Gd, scale)
        torch.cuda.synchronize()
        assert all_same([g.cpu().numpy() for g in got], kv)
        # an attached stream with async
        s = torch.cuda.Stream()
        h.attach_stream(s.cuda_stream, async_=True)
        with torch.cuda.stream(s):
            got = h.attention_backward(Qd, Kd, Vd, Gd, scale)                       # Handle.attention_backward allocates like Q
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert [tuple(g.shape) for g in got] == [(csr.m, k), (csr.n, k), (csr.n, dv)] and all_same([g.cpu().numpy() for g in got], base)
        assert all_same(fused_host(h, csr, Q, K, V, G, scale), base)                # host operands on an asynchronous handle
        want_default = fused_host(h, csr, Q, K, V, G, None)
    for method in METHODS:
        with handle(csr, method) as h:
            assert all_same(fused_host(h, csr, Q, K, V, G, scale), base), method
            assert all_same(h.attention_backward(Q, K, V, G), want_default), method  # scale=None: 1 / sqrt(k)
            got = h.attention_backward(Q, K, V, G, scale, need=(False, True, False))
            assert got[0] is None and got[2] is None and same_bits(got[1], base[1])
    with handle(csr) as h:
        assert all_same(want_default, fused_host(h, csr, Q, K, V, G, 1.0 / np.sqrt(k)))


# ----------------------------------------------------------------------------- 4. memory rules
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_memory_rules(dtype):
    import torch
    lib = api.load()
    csr = pattern_a(dtype)
    s = np.dtype(dtype).itemsize
    k, dv = 9, 7
    Q, K, V, G = operands(csr, k, dv)
    two = 2 * s * csr.nnz
    restored = 4 * (csr.nnz + STREAM_PAD)
    rng = np.random.default_rng(1)
    x, xt, X = rng.uniform(-1, 1, csr.n).astype(dtype), rng.uniform(-1, 1, csr.m).astype(dtype), rng.uniform(-1, 1, (csr.n, 3)).astype(dtype)
    want = None
    for method in (M.Method_Parallel, M.Method_CSR5SPMV):
        for opts in ({"keep_columns": 1}, {"keep_columns": 0}):
            with handle(csr, method, **opts) as h:
                Qd, Kd, Vd, Gd = (torch.from_numpy(a).to(DEV) for a in (Q, K, V, G))
                h.row_softmax(torch.zeros(csr.nnz, dtype=Qd.dtype, device=DEV))   # spmm's tables, without touching the columns
                torch.cuda.synchronize()
                y0 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
                b0 = h.info()["device_bytes"]
                keep = h._keep[2]
                dq = h.attention_backward(Qd, Kd, Vd, Gd, 0.5, need=(True, False, False))[0]
                torch.cuda.synchronize()
                b1 = h.info()["device_bytes"]
                assert b1 - b0 in ((two,) if opts["keep_columns"] else (two, two + restored)), (method, opts, b1 - b0, two)
                with pytest.raises(api.SpmvError, match=r"\[5\]"):                     # dQ alone: no transpose, E_NOSTATE
                    api.get_transpose_info(h.h)
                lib.spmv_hip_clear_error()
                got = h.attention_backward(Qd, Kd, Vd, Gd, 0.5, need=(False, False, True))
                torch.cuda.synchronize()
                assert api.get_transpose_info(h.h)["nnz"] == csr.nnz                 # dV wanted: built now
                b2 = h.info()["device_bytes"]
                assert b2 > b1
                again = h.attention_backward(Qd, Kd, Vd, Gd, 0.5, need=(False, False, True))
                torch.cuda.synchronize()
                assert h.info()["device_bytes"] == b2 and same_bits(again[2].cpu().numpy(), got[2].cpu().numpy())   # a second identical call: + 0
                # the transpose's own products, before and after a full call through host pointers
                yt0, Y0 = h.spmv_transpose(xt), h.spmm(X)
                b2 = h.info()["device_bytes"]
                bits = [a.tobytes() for a in (Q, K, V, G, csr.rowptr, csr.colidx, csr.val)]
                out = fused_host(h, csr, Q, K, V, G, 0.5)
                assert [a.tobytes() for a in (Q, K, V, G, csr.rowptr, csr.colidx, csr.val)] == bits   # the inputs keep their bits
                assert same_bits(out[0], dq.cpu().numpy()) and same_bits(out[2], got[2].cpu().numpy())
                b3 = h.info()["device_bytes"]
                assert b3 - b2 == s * (csr.m * k + csr.n * k + csr.n * dv + csr.m * dv + csr.m * k + csr.n * k + csr.n * dv)   # the staging buffers
                assert all_same(fused_host(h, csr, Q, K, V, G, 0.5), out) and h.info()["device_bytes"] == b3       # nothing grows with use
                assert h._keep[2] is keep
                assert same_bits(h.spmv(x, np.full(csr.m, np.nan, dtype=dtype)), y0), "spmv() after the call must multiply the handle's own values"
                assert same_bits(h.spmv_transpose(xt), yt0) and same_bits(h.spmm(X), Y0)
                want = out if want is None else want
                assert all_same(out, want), (method, opts)


# ----------------------------------------------------------------------------- 5. golden patterns
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", GOLDENS)
def test_golden_patterns(name, dtype):
    csr = load_golden(f"{name}_{'f64' if dtype == np.float64 else 'f32'}_uniform")[0]
    KP = 16 if dtype == np.float64 else 32
    with handle(csr) as h:
        for k, dv, scale in ((33, 2 * KP + 3, float(dtype(1 / np.sqrt(33)))), (3, 5, 1.0)):
            Q, K, V, G = operands(csr, k, dv)
            got = fused_host(h, csr, Q, K, V, G, scale)
            want = composition(h, csr, Q, K, V, G, scale)
            for g, w in zip(got, want):
                assert not np.isnan(w).any()
                assert same_bits(g, w), (k, dv)
                if csr.nnz == 0:
                    assert (g == 0).all() and not np.signbit(g).any()


# ----------------------------------------------------------------------------- 6. handle rules
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
        Q = torch.ones((m, 3), dtype=torch.float64, device=DEV)
        outs = [torch.full((m, 3), CANARY, dtype=torch.float64, device=DEV) for _ in range(3)]
        lib.spmv_hip_clear_error()
        assert api.attention_backward(h.h, m, rp, ci, va, Q, Q, Q, Q, *outs, check=False) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert all(bool((o == CANARY).all()) for o in outs)


def test_errors_leave_the_outputs_untouched_and_no_output_is_no_work():
    lib = api.load()
    csr = load_golden("banded_f64_uniform")[0]
    Q, K, V, G = operands(csr, 4, 3)
    outs = [np.full((csr.m, 4), CANARY), np.full((csr.n, 4), CANARY), np.full((csr.n, 3), CANARY)]
    ptr = [a.ctypes.data for a in (Q, K, V, G, *outs)]
    good_ld = [4, 4, 3, 3, 4, 4, 3]

    def call(h, k, dv, ptrs, ld):
        lib.spmv_hip_clear_error()
        args = [v for pair in zip(ptrs, ld) for v in pair]
        return lib.spmv_hip_attention_backward(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, k, dv, 1.0, *args)

    with handle(csr) as h:
        bad = [(0, 3, ptr, good_ld), (4, 0, ptr, good_ld)]
        bad += [(4, 3, ptr, [l - (i == j) for j, l in enumerate(good_ld)]) for i in range(7)]
        bad += [(4, 3, [None if i == j else p for j, p in enumerate(ptr)], good_ld) for i in range(4)]
        for args in bad:
            assert call(h, *args) == E_ARG, args
            assert lib.spmv_hip_last_error() == E_ARG
            assert all((o == CANARY).all() for o in outs)
        b0 = h.info()["device_bytes"]
        assert call(h, 4, 3, ptr[:4] + [None] * 3, good_ld) == 0 and call(h, 4, 3, ptr[:4] + [None] * 3, [4, 4, 3, 3, 0, 0, 0]) == 0   # nothing wanted
        assert h.info()["device_bytes"] == b0 and all((o == CANARY).all() for o in outs)
        lib.spmv_hip_clear_error()
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            assert api.attention_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q, K, V, G, *outs, check=False) == E_ARG, key
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
            assert all((o == CANARY).all() for o in outs)
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert api.attention_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q, K, V, G, *outs, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert all((o == CANARY).all() for o in outs)
    h.close()


def test_m0_writes_zero_rows_of_dk_and_dv():
    """spmv_hip_spmm_transpose's rule: a matrix without rows has n empty columns"""
    n, k, dv = 70, 3, 5
    csr = synth.CSR(0, n, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    rng = np.random.default_rng(3)
    Q, G = np.zeros((0, k)), np.zeros((0, dv))
    K, V = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, dv))
    with handle(csr) as h:
        dQ, dK, dV = fused_host(h, csr, Q, K, V, G, 1.0)
    assert dQ.shape == (0, k)
    for g in (dK, dV):
        assert (g == 0).all() and not np.signbit(g).any()


def test_timer_runs_on_device_operands_and_rejects_host_ones():
    import torch
    lib = api.load()
    csr = pattern_a(np.float32)
    ops = operands(csr, 8, 8)
    Q, K, V, G = (torch.from_numpy(a).to(DEV) for a in ops)
    with handle(csr) as h:
        outs = [torch.empty((rows, 8), dtype=torch.float32, device=DEV) for rows in (csr.m, csr.n, csr.n)]
        mean, ms = api.time_attention_backward_launches(h.h, Q, K, V, G, *outs, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        assert all_same([o.cpu().numpy() for o in outs], fused_host(h, csr, *ops, 1.0 / np.sqrt(8)))
        mean, ms = api.time_attention_backward_launches(h.h, Q, K, V, G, outs[0], None, None, warmup=1, iters=2)   # dQ alone
        assert mean > 0
        with pytest.raises(api.SpmvError):
            api.time_attention_backward_launches(h.h, ops[0], K, V, G, *outs, warmup=1, iters=1)
        with pytest.raises(api.SpmvError):
            api.time_attention_backward_launches(h.h, Q, K, V, G, outs[0], np.empty((csr.n, 8), dtype=np.float32), None, warmup=1, iters=1)
        lib.spmv_hip_clear_error()
