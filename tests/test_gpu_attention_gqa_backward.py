"""GPU: spmv_hip_attention_gqa_backward -- dQ, dK, dV and dB of `heads` query heads over `kv_heads` K / V heads (include/spmv_hip.h).

No tolerance anywhere.  dQ and dB of head h are the single-head backward's bits (api.attention_bias_backward with ONE head on Q + h*k,
K + (h/gs)*k, V + (h/gs)*dv, G + h*dv and plane h of B) and also those of api.attention_bias_backward on K and V expanded by numpy indexing;
dK and dV of a K / V head are the single-head terms of its group added by an explicit left-to-right numpy loop in the handle's dtype
(gqa_cases.chain): the first term as it is, then one plain addition per head, ascending.  A group of three or four is in every case list: with
two terms the order cannot be wrong.

1. the bit chain   2. kv_heads = heads is the bias call, B = NULL the heads call   3. rounds (option "attention_backward_heads") change no bit
4. need, pointer kind, ld / alignment, method, stream change no bit   5. special values reach their group's K / V head only
6. the test sees the order of the sum   7. goldens and m = 0   8. handle rules   9. the timer"""
import itertools

import numpy as np
import pytest

from conftest import load_golden
from gqa_cases import (BIASES, CANARY, COMBOS, COMBO_IDS, DEV, DTYPES, E_ARG, E_NOSTATE, GOLDENS, IDS, METHODS, OPTION, PATTERNS, M, all_same, backward_oracle, bias_of,
                       chain, device_ops, expand, gqa_bwd_host, group_sums, handle, operands, out_shapes, pattern_a, per_head_terms, same_bits, shapes)
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu
NAMES = ("dQ", "dK", "dV", "dB")
NEEDS = [n for n in itertools.product((True, False), repeat=4)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


# ----------------------------------------------------------------------------- 1. the bit chain
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", list(PATTERNS))
def test_bits_per_head_and_the_chain_per_group(which, dtype, combo):
    heads, kv = combo
    csr = PATTERNS[which](dtype)
    with handle(csr) as h:
        for k, dv in shapes(dtype):
            Q, K, V, G = operands(csr, heads, kv, k, dv)
            scale = float(dtype(1.0 / np.sqrt(k)))
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                got = gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, scale)
                want = backward_oracle(h, csr, heads, kv, Q, K, V, B, G, scale)
                for name, g, w in zip(NAMES, got, want):
                    assert not np.isnan(w).any(), (name, k, dv)
                    assert same_bits(g, w), (name, heads, kv, k, dv, kind)
            # dQ and dB once more, from the bias call on K and V repeated (B as left by the loop: one shared plane)
            outs = [np.full(s, CANARY, dtype=dtype) for s in ((csr.m, heads * k), (heads, csr.nnz))]
            api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, expand(K, heads, kv), expand(V, heads, kv), B, G, outs[0], None, None, outs[1],
                                        scale=scale)
            assert same_bits(got[0], outs[0]) and same_bits(got[3], outs[1]), (heads, kv, k, dv)


# ----------------------------------------------------------------------------- 2. the existing calls
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kv_heads_equal_to_heads_is_the_bias_call_and_no_bias_the_heads_call(dtype):
    csr = pattern_a(dtype)
    heads = 3
    with handle(csr) as h:
        for k, dv in shapes(dtype):
            Q, K, V, G = operands(csr, heads, heads, k, dv)
            B = bias_of(csr, heads, "planes")
            want = [np.full(s, CANARY, dtype=dtype) for s in out_shapes(csr, heads, Q, K, V)]
            api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, B, G, *want, scale=0.5)
            assert all_same(gqa_bwd_host(h, csr, heads, heads, Q, K, V, B, G, 0.5), want), (k, dv)
            want3 = [np.full(s, CANARY, dtype=dtype) for s in out_shapes(csr, heads, Q, K, V)[:3]]
            api.attention_heads_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, G, *want3, scale=0.5)
            assert all_same(gqa_bwd_host(h, csr, heads, heads, Q, K, V, None, G, 0.5)[:3], want3), (k, dv)
            assert all_same(h.attention_gqa_backward(Q, K, V, None, G, heads, heads, 0.5, need=(True, True, True, False))[:3], want3)


# ----------------------------------------------------------------------------- 3. rounds change no bit
def gqa_device(h, heads, kv, ops, B, scale, need=(True, True, True, True)):
    import torch
    got = h.attention_gqa_backward(*ops[:3], B, ops[3], heads, kv, scale, need=need)
    torch.cuda.synchronize()
    return tuple(None if g is None else g.cpu().numpy() for g in got)


@pytest.mark.parametrize("combo", [(6, 2), (4, 1)], ids=["6over2", "4over1"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rounds_change_no_bit_only_memory(dtype, combo):
    """rounds that end inside a group continue the chain from the dK / dV they find: HG in {1, gs - 1, gs, gs + 1, heads} and the default"""
    import torch
    heads, kv = combo
    gs = heads // kv
    s = np.dtype(dtype).itemsize
    k, dv = 3, 16 // s + 1
    eighth = torch.cuda.mem_get_info()[1] // 8
    for which in PATTERNS:   # short and long columns
        csr = PATTERNS[which](dtype)
        assert eighth // (2 * s * csr.nnz) >= heads   # the automatic rule takes every head: a multiple of gs
        host = operands(csr, heads, kv, k, dv)
        B = bias_of(csr, heads, "planes")
        ops, Bd = device_ops(host), device_ops([B])[0]
        one = [o[:, :w].contiguous() for o, w in zip(ops, (k, k, dv, dv))]
        base = None
        for n in (0, 1, gs - 1, gs, gs + 1, heads, heads + 3):
            with handle(csr, **{OPTION: n}) as h:
                assert h.option(OPTION) == n
                h.attention_backward(*one, 0.5)   # a single-head call first: the tables, the transpose and one plane of each array
                torch.cuda.synchronize()
                b0 = h.info()["device_bytes"]
                got = gqa_device(h, heads, kv, ops, Bd, 0.5)
                planes = heads if n == 0 else min(n, heads)
                assert h.info()["device_bytes"] - b0 == 2 * (planes - 1) * s * csr.nnz, n   # 2 * HG * s * nnz in all: the heads backward's, indexed by QUERY head
                if n == 0:
                    assert planes % gs == 0
                    # the heads backward reports the same for the same heads
                    with handle(csr) as h2:
                        h2.attention_backward(*one, 0.5)
                        torch.cuda.synchronize()
                        b2 = h2.info()["device_bytes"]
                        h2.attention_heads_backward(ops[0], torch.from_numpy(expand(host[1], heads, kv)).to(DEV), torch.from_numpy(expand(host[2], heads, kv)).to(DEV),
                                                    ops[3], heads, 0.5)
                        torch.cuda.synchronize()
                        assert h2.info()["device_bytes"] - b2 == h.info()["device_bytes"] - b0
                    base = got
                    assert all_same(base, backward_oracle(h, csr, heads, kv, *host[:3], B, host[3], 0.5))
                assert all_same(got, base), (which, n)
                # only dK: the read-back chain without dV's, and through host pointers
                if n in (1, gs + 1):
                    assert same_bits(gqa_bwd_host(h, csr, heads, kv, *host[:3], B, host[3], 0.5, need=(False, True, False, False))[1], base[1]), (which, n)


# ----------------------------------------------------------------------------- 4. what changes no bit
def _wide(arrays, dtype, pad, off):
    """every array inside a wider one: `off` elements in front of and `pad` behind every row, NaN in every padding element"""
    wide, views = [], []
    for a in arrays:
        wd = np.full((a.shape[0], a.shape[1] + pad + off), np.nan, dtype=dtype)
        wd[:, off:off + a.shape[1]] = a
        wide.append(wd)
        views.append(wd[:, off:off + a.shape[1]])
    return wide, views


def gqa_device_wide(h, csr, heads, kv, wide, off, widths, B, scale, need=(True, True, True, True)):
    """device operands cut out of the wide arrays; outputs with the same padding (dB: `extra` elements behind every plane), canary-filled"""
    import torch
    dev = [torch.from_numpy(wd).to(DEV) for wd in wide]
    ins = [d[:, off:off + w] for d, w in zip(dev, widths)]
    extra = wide[0].shape[1] - widths[0]
    outs, views = [], []
    for want, rows, w in zip(need, (csr.m, csr.n, csr.n, heads), (widths[0], widths[1], widths[2], csr.nnz)):
        outs.append(torch.full((rows + 1, w + extra), CANARY, dtype=dev[0].dtype, device=DEV) if want else None)
        views.append(outs[-1][:rows, off:off + w] if want else None)
    Bd = None if B is None else torch.from_numpy(B).to(DEV)
    api.attention_gqa_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *ins[:3], Bd, ins[3], *views, scale=scale)
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
    lib = api.load()
    csr = pattern_a(dtype)
    s = np.dtype(dtype).itemsize
    heads, kv, k, dv = 6, 2, 3 * (16 // s), 2 * (16 // s)   # k * s and dv * s multiples of 16: aligned operands take the 16-byte form
    Q, K, V, G = host = operands(csr, heads, kv, k, dv)
    widths = (heads * k, kv * k, kv * dv, heads * dv)
    B = bias_of(csr, heads, "planes")
    scale = 0.125

    def sub(base, need):
        return [b if n else None for b, n in zip(base, need)]

    with handle(csr) as h:
        base = backward_oracle(h, csr, heads, kv, Q, K, V, B, G, scale)
        assert all(not np.isnan(b).any() for b in base)
        # only dB (or dQ and dB) wanted, on a handle that has computed no dK or dV yet: the row pass alone, no transpose is built
        with handle(csr) as h2:
            got = gqa_bwd_host(h2, csr, heads, kv, Q, K, V, B, G, scale, need=(False, False, False, True))
            assert all_same(got, sub(base, (False, False, False, True)))
            got = gqa_bwd_host(h2, csr, heads, kv, Q, K, V, B, G, scale, need=(True, False, False, True))
            assert all_same(got, sub(base, (True, False, False, True)))
            with pytest.raises(api.SpmvError, match=r"\[5\]"):
                api.get_transpose_info(h2.h)
            lib.spmv_hip_clear_error()
            assert all_same(gqa_bwd_host(h2, csr, heads, kv, Q, K, V, B, G, scale, need=(False, True, False, False)), sub(base, (False, True, False, False)))
            api.get_transpose_info(h2.h)   # dK wanted: now it is there
        assert all_same(gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, scale, pad=0), base)       # host pointers
        for need in NEEDS:                                                                        # every subset of the wanted outputs
            assert all_same(gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, scale, need=need), sub(base, need)), need
            assert all_same(gqa_device_wide(h, csr, heads, kv, host, 0, widths, B, scale, need=need), sub(base, need)), need
        # (0, 0), (4, 0): every address and ld a multiple of 16 bytes -- the 16-byte form; an odd pad or an offset of one element: the element form
        for pad, off in ((0, 0), (4, 0), (1, 0), (3, 0), (0, 1), (1, 1), (2, 2)):
            wide, views = _wide(host, dtype, pad, off)
            assert all_same(gqa_bwd_host(h, csr, heads, kv, *views[:3], B, views[3], scale, pad=pad + off), base), (pad, off)
            assert all_same(gqa_device_wide(h, csr, heads, kv, wide, off, widths, B, scale), base), (pad, off)
        ops = device_ops(host)
        for mix in ((ops[0], K, V, G), (Q, ops[1], V, G), (Q, K, ops[2], G), (Q, K, V, ops[3]), (ops[0], ops[1], V, ops[3])):
            assert all_same(gqa_bwd_host(h, csr, heads, kv, *mix[:3], B, mix[3], scale), base)    # each operand on its own side
        st = torch.cuda.Stream()                                                                  # a non-default stream with async
        h.attach_stream(st.cuda_stream, async_=True)
        with torch.cuda.stream(st):
            got = h.attention_gqa_backward(*ops[:3], torch.from_numpy(B).to(DEV), ops[3], heads, kv, scale)
        assert lib.spmv_hip_synchronize(h.h) == 0
        assert [tuple(g.shape) for g in got] == [(csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv), (heads, csr.nnz)]
        assert all_same([g.cpu().numpy() for g in got], base)
        assert all_same(gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, scale), base)              # host operands on an asynchronous handle
    for method in METHODS:
        with handle(csr, method) as h:
            assert all_same(gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, scale), base), method


# ----------------------------------------------------------------------------- 5. special values
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values_reach_their_groups_kv_head_only(dtype):
    """heads = 6 over 2 (groups of three).  Head 1 (group 0): a NaN in two rows of Q; head 2 (group 0): a bias plane of -inf.  dQ and dB are NaN in
    heads 1 and 2 only; dK and dV are NaN in K / V head 0 only, and K / V head 1 has the chain's bits"""
    csr = pattern_a(dtype)
    heads, kv, k, dv = 6, 2, 3, 5
    Q, K, V, G = operands(csr, heads, kv, k, dv)
    B = bias_of(csr, heads, "planes")
    lens = np.diff(csr.rowptr)
    rows = [int(np.flatnonzero(lens == n)[0]) for n in (3, 1025)]   # a short row and a long one
    Q[rows, 1 * k] = np.nan
    B[2] = -np.inf
    with handle(csr) as h:
        got = gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, 1.0)
        want = backward_oracle(h, csr, heads, kv, Q, K, V, B, G, 1.0)
    for name, g, w in zip(NAMES, got, want):
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), name
        assert same_bits(g[~nan], w[~nan]), name
    dQ, dK, dV, dB = (np.isnan(g) for g in got)
    assert not dQ[:, :k].any() and not dQ[:, 3 * k:].any() and dQ[rows, k:2 * k].all() and dQ[:, 2 * k:3 * k].any()
    assert not dB[[0, 3, 4, 5]].any() and dB[1].any() and dB[2].all()
    assert dK[:, :k].any() and not dK[:, k:].any()
    assert dV[:, :dv].any() and not dV[:, dv:].any()


# ----------------------------------------------------------------------------- 6. the order of the sum is visible
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_order_of_the_sum_is_part_of_the_bits(dtype):
    """groups whose per-head dK terms differ by many orders of magnitude: the group's first query head has its Q scaled by 2^-40, its last by 2^20
    (dK = A_dS^T Q is linear in Q for given dS; scale = 2^-20 keeps the large head's softmax away from saturation, so its dS does not vanish).
    The call has the ascending chain's bits.  In the group of four the two heads in between are of one magnitude, so the host-side restatement in
    another order has other bits -- asserted, in both precisions: the test sees the order.  In the group of three the smallest term lies 2^40
    below the next one and fp32 absorbs it in every order, so there a differing order is not demanded, only told apart where it exists."""
    csr = pattern_a(dtype)
    scale = 2.0 ** -20
    for heads, kv in ((4, 1), (6, 2)):
        gs, k, dv = heads // kv, 3, 2
        Q, K, V, G = operands(csr, heads, kv, k, dv)
        Q[:, 0:k] *= dtype(2.0 ** -40)
        Q[:, (gs - 1) * k:gs * k] *= dtype(2.0 ** 20)
        with handle(csr) as h:
            dQ, dB, tK, tV = per_head_terms(h, csr, heads, kv, Q, K, V, None, G, scale)
            got = gqa_bwd_host(h, csr, heads, kv, Q, K, V, None, G, scale)
        want = group_sums(tK, heads, kv)
        assert not np.isnan(want).any()
        mags = [float(np.abs(t).max()) for t in tK[:gs]]
        assert mags[gs - 1] > 2.0 ** 40 * mags[0] > 0, mags   # the inputs do what the case is about
        assert same_bits(got[1], want) and same_bits(got[2], group_sums(tV, heads, kv))
        assert same_bits(got[0], dQ)
        others = [list(reversed(range(gs))), [gs - 1] + list(range(gs - 1)), list(range(1, gs)) + [0]]
        differing = [o for o in others if not same_bits(group_sums(tK, heads, kv, o), want)]
        if gs == 4:
            assert list(reversed(range(gs))) in differing, "the reversed sum has the chain's bits: the operands do not exercise the order"
        for o in differing:
            assert not same_bits(got[1], group_sums(tK, heads, kv, o)), o
    # a sum that starts from a zero is not the chain where the first term is -0: (+0) + (-0) = +0
    z = np.array([-0.0], dtype=dtype)
    assert np.signbit(chain([z, z]))[0] and not np.signbit(np.zeros(1, dtype=dtype) + z + z)[0]


# ----------------------------------------------------------------------------- 7. goldens, m = 0
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", GOLDENS)
def test_golden_patterns(name, dtype):
    csr = load_golden(f"{name}_{'f64' if dtype == np.float64 else 'f32'}_uniform")[0]
    heads, kv, k, dv = 6, 2, 3, 2
    Q, K, V, G = operands(csr, heads, kv, k, dv)
    with handle(csr) as h:
        for kind in ("none", "planes"):
            B = bias_of(csr, heads, kind)
            got = gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, 0.5)
            want = backward_oracle(h, csr, heads, kv, Q, K, V, B, G, 0.5)
            for g, w in zip(got, want):
                assert not np.isnan(w).any()
                assert same_bits(g, w)
                if csr.nnz == 0:
                    assert (g == 0).all() and not np.signbit(g).any()
        # empty columns: every per-head term is +0 there, so the sums are +0
        empty = np.bincount(csr.colidx, minlength=csr.n) == 0
        for g in got[1:3]:
            assert (g[empty] == 0).all() and not np.signbit(g[empty]).any()


def test_m0_writes_zero_rows_of_dk_and_dv_at_the_kv_widths():
    n, heads, kv, k, dv = 70, 6, 2, 3, 5
    csr = synth.CSR(0, n, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    rng = np.random.default_rng(3)
    Q, G = np.zeros((0, heads * k)), np.zeros((0, heads * dv))
    K, V = rng.uniform(-1, 1, (n, kv * k)), rng.uniform(-1, 1, (n, kv * dv))
    with handle(csr) as h:
        dQ, dK, dV, dB = gqa_bwd_host(h, csr, heads, kv, Q, K, V, None, G, 1.0)
    assert dQ.shape == (0, heads * k) and dK.shape == (n, kv * k) and dV.shape == (n, kv * dv) and dB.shape == (heads, 0)
    for g in (dK, dV):
        assert (g == 0).all() and not np.signbit(g).any()


# ----------------------------------------------------------------------------- 8. handle rules
def test_handle_rules():
    lib = api.load()
    csr = load_golden("banded_f64_uniform")[0]
    heads, kv, k, dv = 4, 2, 3, 2
    Q, K, V, G = operands(csr, heads, kv, k, dv)
    outs = [np.full(s, CANARY) for s in out_shapes(csr, heads, Q, K, V)]
    rng = np.random.default_rng(1)
    x, xt = rng.uniform(-1, 1, csr.n), rng.uniform(-1, 1, csr.m)
    with handle(csr) as h:
        y0, yt0 = h.spmv(x, np.full(csr.m, np.nan)), h.spmv_transpose(xt)
        for bad_kv in (0, 3, 8):
            assert lib.spmv_hip_attention_gqa_backward(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, heads, bad_kv, k, dv, 1.0,
                                                       Q.ctypes.data, 2 ** 20, K.ctypes.data, 2 ** 20, V.ctypes.data, 2 ** 20, None, 0, G.ctypes.data, 2 ** 20,
                                                       outs[0].ctypes.data, 2 ** 20, outs[1].ctypes.data, 2 ** 20, outs[2].ctypes.data, 2 ** 20, outs[3].ctypes.data,
                                                       2 ** 20) == E_ARG
            lib.spmv_hip_clear_error()
        assert api.attention_gqa_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, G, *outs, check=False, lddb=csr.nnz - 1) == E_ARG
        lib.spmv_hip_clear_error()
        assert all((o == CANARY).all() for o in outs)
        got = gqa_bwd_host(h, csr, heads, kv, Q, K, V, None, G, 0.5)
        assert all_same(got, backward_oracle(h, csr, heads, kv, Q, K, V, None, G, 0.5))
        assert same_bits(h.spmv(x, np.full(csr.m, np.nan)), y0) and same_bits(h.spmv_transpose(xt), yt0)
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            assert api.attention_gqa_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, G, *outs, check=False) == E_ARG, key
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
            assert all((o == CANARY).all() for o in outs)
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert api.attention_gqa_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, G, *outs, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert all((o == CANARY).all() for o in outs)
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
        outs = [torch.full((m, w), CANARY, dtype=torch.float64, device=DEV) for w in (8, 4, 4)]
        lib.spmv_hip_clear_error()
        assert api.attention_gqa_backward(h.h, m, rp, ci, va, 4, 2, Q, KV, KV, None, Q, *outs, check=False) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert all(bool((o == CANARY).all()) for o in outs)


# ----------------------------------------------------------------------------- 9. the timer
def test_timer_runs_on_device_operands_and_leaves_the_calls_bits():
    import torch
    lib = api.load()
    csr = pattern_a(np.float32)
    heads, kv = 6, 2
    host = operands(csr, heads, kv, 8, 8)
    B = bias_of(csr, heads, "planes")
    ops, Bd = device_ops(host), device_ops([B])[0]
    with handle(csr) as h:
        outs = [torch.empty(s, dtype=torch.float32, device=DEV) for s in out_shapes(csr, heads, *host[:3])]
        mean, ms = api.time_attention_gqa_backward_launches(h.h, heads, kv, *ops[:3], Bd, ops[3], *outs, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        assert all_same([o.cpu().numpy() for o in outs], gqa_bwd_host(h, csr, heads, kv, *host[:3], B, host[3], float(1.0 / np.sqrt(8))))
        mean, ms = api.time_attention_gqa_backward_launches(h.h, heads, kv, *ops[:3], None, ops[3], outs[0], None, None, None, warmup=1, iters=2)   # dQ alone
        assert mean > 0
        with pytest.raises(api.SpmvError):
            api.time_attention_gqa_backward_launches(h.h, heads, kv, host[0], *ops[1:3], Bd, ops[3], *outs, warmup=1, iters=1)
        lib.spmv_hip_clear_error()
