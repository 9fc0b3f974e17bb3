"""GPU: spmv_hip_attention_gqa -- `heads` query heads over `kv_heads` K / V heads in the one forward pass (include/spmv_hip.h).

No tolerance anywhere.  The oracles are api.attention_bias with ONE head on the slices the contract names (Q + h*k, K + (h/gs)*k, V + (h/gs)*dv,
O + h*dv, plane h of B) and api.attention_bias / api.attention_heads on K and V expanded by this file's own numpy indexing (gqa_cases.expand).
The patterns and shapes are test_gpu_attention_heads_backward.py's, restated in gqa_cases.py.

1. bits per head   2. kv_heads = heads is the bias call, B = NULL the heads call   3. pointer kind, ld, alignment, method, stream change no bit
4. special values stay in their head   5. goldens and m = 0   6. handle rules   7. the timer"""
import numpy as np
import pytest

from conftest import load_golden
from gqa_cases import (BIASES, CANARY, COMBOS, COMBO_IDS, DEV, DTYPES, E_ARG, E_NOSTATE, GOLDENS, IDS, METHODS, PATTERNS, M, all_same, bias_of, device_ops,
                       expand, forward_head_by_head, gqa_host, handle, operands, pattern_a, plane, same_bits, shapes)
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


# ----------------------------------------------------------------------------- 1. bits per head
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", list(PATTERNS))
def test_every_head_has_the_single_head_bits(which, dtype, combo):
    heads, kv = combo
    csr = PATTERNS[which](dtype)
    with handle(csr) as h:
        for k, dv in shapes(dtype):
            Q, K, V, _ = operands(csr, heads, kv, k, dv)
            scale = float(dtype(1.0 / np.sqrt(k)))
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                got = gqa_host(h, csr, heads, kv, Q, K, V, B, scale)
                want = forward_head_by_head(h, csr, heads, kv, Q, K, V, B, scale)
                assert not np.isnan(want).any()
                assert same_bits(got, want), (heads, kv, k, dv, kind)
                # the caller's other option today: K and V repeated, the bias call on all heads
                O = np.full_like(want, CANARY)
                api.attention_bias(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, expand(K, heads, kv), expand(V, heads, kv), B, O, scale=scale)
                assert same_bits(got, O), (heads, kv, k, dv, kind)


# ----------------------------------------------------------------------------- 2. the existing calls
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kv_heads_equal_to_heads_is_the_bias_call_and_no_bias_the_heads_call(dtype):
    csr = pattern_a(dtype)
    heads = 3
    with handle(csr) as h:
        for k, dv in shapes(dtype):
            Q, K, V, _ = operands(csr, heads, heads, k, dv)
            B = bias_of(csr, heads, "planes")
            O = np.full((csr.m, heads * dv), CANARY, dtype=dtype)
            api.attention_bias(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, B, O, scale=0.5)
            assert same_bits(gqa_host(h, csr, heads, heads, Q, K, V, B, 0.5), O)
            O2 = np.full_like(O, CANARY)
            api.attention_heads(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, O2, scale=0.5)
            assert same_bits(gqa_host(h, csr, heads, heads, Q, K, V, None, 0.5), O2)
            assert same_bits(h.attention_gqa(Q, K, V, heads, heads, scale=0.5), O2)
        # grouped, without a bias: the heads call on the expanded operands
        Q, K, V, _ = operands(csr, 6, 2, 5, 3)
        O3 = np.full((csr.m, 18), CANARY, dtype=dtype)
        api.attention_heads(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, 6, Q, expand(K, 6, 2), expand(V, 6, 2), O3)
        assert same_bits(h.attention_gqa(Q, K, V, 6, 2), O3)   # scale None: 1 / sqrt(k) of one head


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


def gqa_device_wide(h, csr, heads, kv, wide, off, widths, B, scale):
    """device operands cut out of the wide arrays; O with the same padding, canary-filled"""
    import torch
    dev = [torch.from_numpy(wd).to(DEV) for wd in wide]
    ins = [d[:, off:off + w] for d, w in zip(dev, widths)]
    extra = wide[0].shape[1] - widths[0]
    wo = heads * (widths[2] // kv)
    out = torch.full((csr.m + 1, wo + extra), CANARY, dtype=dev[0].dtype, device=DEV)
    Bd = None if B is None else torch.from_numpy(B).to(DEV)
    api.attention_gqa(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *ins, Bd, out[:csr.m, off:off + wo], scale=scale)
    torch.cuda.synchronize()
    oh = out.cpu().numpy()
    res = oh[:csr.m, off:off + wo].copy()
    oh[:csr.m, off:off + wo] = CANARY
    assert (oh == CANARY).all(), "written outside O's elements"
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pointer_kind_layout_method_and_stream_change_no_bit(dtype):
    import torch
    csr = pattern_a(dtype)
    s = np.dtype(dtype).itemsize
    heads, kv, k, dv = 6, 2, 3 * (16 // s), 2 * (16 // s)   # k * s and dv * s multiples of 16: aligned operands take the 16-byte form
    Q, K, V, _ = operands(csr, heads, kv, k, dv)
    host = (Q, K, V)
    widths = (heads * k, kv * k, kv * dv)
    B = bias_of(csr, heads, "planes")
    scale = 0.125
    with handle(csr) as h:
        base = forward_head_by_head(h, csr, heads, kv, Q, K, V, B, scale)
        assert not np.isnan(base).any()
        assert same_bits(gqa_host(h, csr, heads, kv, Q, K, V, B, scale, pad=0), base)
        # (0, 0), (4, 0): every address and ld a multiple of 16 bytes -- the 16-byte form; an odd pad or an offset of one element: the element form
        for pad, off in ((0, 0), (4, 0), (1, 0), (3, 0), (0, 1), (1, 1), (2, 2)):
            wide, views = _wide(host, dtype, pad, off)
            assert same_bits(gqa_host(h, csr, heads, kv, *views, B, scale, pad=pad + off), base), (pad, off)
            assert same_bits(gqa_device_wide(h, csr, heads, kv, wide, off, widths, B, scale), base), (pad, off)
        # padded bias planes with canaries behind each: ldb > nnz
        Bw = np.full((heads, csr.nnz + 5), np.nan, dtype=dtype)
        Bw[:, :csr.nnz] = B
        assert same_bits(gqa_host(h, csr, heads, kv, Q, K, V, Bw[:, :csr.nnz], scale), base)
        ops = device_ops(host)
        for mix in ((ops[0], K, V), (Q, ops[1], V), (Q, K, ops[2]), (ops[0], ops[1], V)):
            assert same_bits(gqa_host(h, csr, heads, kv, *mix, B, scale), base)     # each operand on its own side
        st = torch.cuda.Stream()                                                    # a non-default stream with async
        h.attach_stream(st.cuda_stream, async_=True)
        with torch.cuda.stream(st):
            got = h.attention_gqa(*ops, heads, kv, torch.from_numpy(B).to(DEV), scale)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert tuple(got.shape) == (csr.m, heads * dv)
        assert same_bits(got.cpu().numpy(), base)
        assert same_bits(gqa_host(h, csr, heads, kv, Q, K, V, B, scale), base)      # host operands on an asynchronous handle
    for method in METHODS:
        with handle(csr, method) as h:
            assert same_bits(gqa_host(h, csr, heads, kv, Q, K, V, B, scale), base), method


# ----------------------------------------------------------------------------- 4. special values
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values_stay_in_their_query_head(dtype):
    """heads = 4 over 2.  A NaN in one row of head 1's Q and a bias plane of -inf for head 2: O is NaN in those heads' blocks only, and head 0
    (the NaN head's group mate) and head 3 (the masked head's) are finite and have the single-head bits"""
    csr = pattern_a(dtype)
    heads, kv, k, dv = 4, 2, 3, 5
    Q, K, V, _ = operands(csr, heads, kv, k, dv)
    B = bias_of(csr, heads, "planes")
    lens = np.diff(csr.rowptr)
    rows = [int(np.flatnonzero(lens == n)[0]) for n in (3, 1025)]   # a short row and a long one
    Q[rows, 1 * k] = np.nan
    B[2] = -np.inf
    with handle(csr) as h:
        got = gqa_host(h, csr, heads, kv, Q, K, V, B, 1.0)
        want = forward_head_by_head(h, csr, heads, kv, Q, K, V, B, 1.0)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and same_bits(got[~nan], want[~nan])
    for hd in (0, 3):
        assert not nan[:, hd * dv:(hd + 1) * dv].any()
    assert nan[rows, dv:2 * dv].all() and nan[:, dv:2 * dv].sum() == len(rows) * dv        # head 1: those rows and no other
    assert np.array_equal(nan[:, 2 * dv:3 * dv].all(axis=1), lens > 0)                     # head 2: every row with an entry (all -inf), empty rows +0


# ----------------------------------------------------------------------------- 5. goldens, m = 0
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", GOLDENS)
def test_golden_patterns(name, dtype):
    csr = load_golden(f"{name}_{'f64' if dtype == np.float64 else 'f32'}_uniform")[0]
    heads, kv, k, dv = 6, 2, 3, 2
    Q, K, V, _ = operands(csr, heads, kv, k, dv)
    with handle(csr) as h:
        for kind in ("none", "planes"):
            B = bias_of(csr, heads, kind)
            got = gqa_host(h, csr, heads, kv, Q, K, V, B, 0.5)
            want = forward_head_by_head(h, csr, heads, kv, Q, K, V, B, 0.5)
            assert not np.isnan(want).any() and same_bits(got, want)
            if csr.nnz == 0:
                assert (got == 0).all() and not np.signbit(got).any()


def test_m0_is_no_work():
    n, heads, kv, k, dv = 70, 4, 2, 3, 5
    csr = synth.CSR(0, n, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    rng = np.random.default_rng(3)
    Q = np.zeros((0, heads * k))
    K, V = rng.uniform(-1, 1, (n, kv * k)), rng.uniform(-1, 1, (n, kv * dv))
    with handle(csr) as h:
        assert gqa_host(h, csr, heads, kv, Q, K, V, None, 1.0).shape == (0, heads * dv)


# ----------------------------------------------------------------------------- 6. handle rules
def test_handle_rules():
    import torch
    lib = api.load()
    csr = load_golden("banded_f64_uniform")[0]
    heads, kv, k, dv = 4, 2, 3, 2
    Q, K, V, _ = operands(csr, heads, kv, k, dv)
    O = np.full((csr.m, heads * dv), CANARY)
    rng = np.random.default_rng(1)
    x, xt = rng.uniform(-1, 1, csr.n), rng.uniform(-1, 1, csr.m)
    with handle(csr) as h:
        y0, yt0 = h.spmv(x, np.full(csr.m, np.nan)), h.spmv_transpose(xt)
        b0 = h.info()["device_bytes"]
        # errors found once the handle is looked at leave O untouched too: a plane stride below nnz
        assert api.attention_gqa(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, np.zeros(heads * csr.nnz), O, check=False, ldb=csr.nnz - 1) == E_ARG
        lib.spmv_hip_clear_error()
        for bad_kv in (0, 3, 8):
            assert lib.spmv_hip_attention_gqa(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, heads, bad_kv, k, dv, 1.0, Q.ctypes.data, 2 ** 20,
                                              K.ctypes.data, 2 ** 20, V.ctypes.data, 2 ** 20, None, 0, O.ctypes.data, 2 ** 20) == E_ARG
            lib.spmv_hip_clear_error()
        assert (O == CANARY).all()
        got = gqa_host(h, csr, heads, kv, Q, K, V, None, 0.5)
        assert same_bits(got, forward_head_by_head(h, csr, heads, kv, Q, K, V, None, 0.5))
        assert same_bits(h.spmv(x, np.full(csr.m, np.nan)), y0) and same_bits(h.spmv_transpose(xt), yt0)
        b1 = h.info()["device_bytes"]
        # device operands: nothing beyond what the heads call allocates (here: nothing new at all after the first call)
        ops = device_ops((Q, K, V))
        h.attention_gqa(*ops, heads, kv, None, 0.5)
        torch.cuda.synchronize()
        assert h.info()["device_bytes"] == b1 and b1 >= b0
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            assert api.attention_gqa(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, O, check=False) == E_ARG, key
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
            assert (O == CANARY).all()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert api.attention_gqa(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, O, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert (O == CANARY).all()
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
        Q = torch.ones((m, 8), dtype=torch.float64, device=DEV)
        KV = torch.ones((n, 4), dtype=torch.float64, device=DEV)
        O = torch.full((m, 8), CANARY, dtype=torch.float64, device=DEV)
        lib.spmv_hip_clear_error()
        assert api.attention_gqa(h.h, m, rp, ci, va, 4, 2, Q, KV, KV, None, O, check=False) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert bool((O == CANARY).all())


# ----------------------------------------------------------------------------- 7. the timer
def test_timer_runs_on_device_operands_and_leaves_the_calls_bits():
    import torch
    lib = api.load()
    csr = pattern_a(np.float32)
    heads, kv = 4, 2
    Q, K, V, _ = operands(csr, heads, kv, 8, 8)
    B = bias_of(csr, heads, "planes")
    ops = device_ops((Q, K, V, B))
    with handle(csr) as h:
        O = torch.empty((csr.m, heads * 8), dtype=torch.float32, device=DEV)
        mean, ms = api.time_attention_gqa_launches(h.h, heads, kv, *ops, O, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        assert same_bits(O.cpu().numpy(), gqa_host(h, csr, heads, kv, Q, K, V, B, float(1.0 / np.sqrt(8))))
        with pytest.raises(api.SpmvError):
            api.time_attention_gqa_launches(h.h, heads, kv, Q, *ops[1:], O, warmup=1, iters=1)   # a host Q
        lib.spmv_hip_clear_error()
