"""GPU: spmv_hip_attention_gqa_backward_16 -- the fused attention backward on fp16 / bf16 Q, K, V and G over an fp32 handle, with dQ and dK / dV
in fp32 or in that 16-bit type, self-normalising (O = L = NULL) or driven by the final O and L (include/spmv_hip.h).

There is no tolerance anywhere: widening a 16-bit element to fp32 is exact, so the oracle is api.attention_gqa_backward / lse_cases.bwd_lse_host on
the .float() copies.  An fp32 output and dB must have its bits; a 16-bit output must be it rounded once (is_rounded: torch.Tensor.to(dtype)).

1. bits   2. the rounds   3. need masks   4. layout   5. special values   6. head by head, goldens, argument rules, the timer"""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden
from gqa_cases import (BIASES, CANARY, COMBOS, COMBO_IDS, DEV, E_ARG, E_NOSTATE, GOLDENS, METHODS, OPTION, bias_of, gqa_bwd_host, handle, operands, out_shapes, pattern_a,
                       pattern_b, plane, same_bits)
from lse_cases import bwd_lse_host, lse_host
from spmv_amd import api, build, synth
from test_gpu_attention_16 import SHAPES, TYPE_IDS, TYPES, bits16, is_rounded

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = (True, True, True, True)
FORMS = ["self", "lse"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def ops16(csr, heads, kv, k, dv, dt, seed=0):
    """Q, K, V and G of gqa_cases.operands rounded to dt by torch (host tensors)"""
    return tuple(torch.from_numpy(a).to(dt) for a in operands(csr, heads, kv, k, dv, seed))


def widened(ops):
    return tuple(t.float().numpy() for t in ops)


def call16(h, csr, heads, kv, ops, B, scale, dq_dt, dkv_dt, OL=None, need=ALL, pad=3):
    """spmv_hip_attention_gqa_backward_16 through host pointers into canary-filled outputs of the types asked for, `pad` elements behind every row /
    plane and a row behind the last (an odd pad gives a 16-bit output an odd leading dimension); -> (dQ, dK, dV, dB) as tensors or None"""
    Q, K, V, G = ops
    shp = out_shapes(csr, heads, Q, K, V)
    dts = (dq_dt, dkv_dt, dkv_dt, torch.float32)
    bufs = [torch.full((rows + 1, w + pad), CANARY, dtype=d) if want else None for want, (rows, w), d in zip(need, shp, dts)]
    views = [None if b is None else b[:rows, :w] for b, (rows, w) in zip(bufs, shp)]
    O, L = (None, None) if OL is None else OL
    api.attention_gqa_backward_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, B, G, O, L, *views, scale=scale)
    for b, v in zip(bufs, views):
        if b is not None:
            assert bool((b[:, v.shape[1]:] == CANARY).all()) and bool((b[v.shape[0]] == CANARY).all()), "written outside an output's elements"
    return tuple(None if v is None else v.clone().contiguous() for v in views)


def oracle(h, csr, heads, kv, ops, B, scale, form, need=ALL):
    """-> ((dQ, dK, dV, dB) of the fp32 call on the .float() copies, (O, L) for the LSE-driven form or None)"""
    w = widened(ops)
    if form == "self":
        return gqa_bwd_host(h, csr, heads, kv, *w[:3], B, w[3], scale, need=need), None
    O, L = lse_host(h, csr, heads, kv, *w[:3], B, scale)
    return bwd_lse_host(h, csr, heads, kv, *w[:3], B, w[3], O, L, scale, need=need), (O, L)


def matches(got, want, dt):
    """every output: fp32 -> the same bits, 16-bit -> rounded once; None where None"""
    for g, w in zip(got, want):
        if (g is None) != (w is None):
            return False
        if g is None:
            continue
        if g.dtype == torch.float32:
            if not same_bits(g.numpy(), w):
                return False
        elif not is_rounded(g, w, dt):
            return False
    return True


def same16(a, b):
    return all((x is None and y is None) or (x.dtype == y.dtype and np.array_equal(x.view(torch.int16).numpy() if x.dtype != torch.float32 else x.numpy().view(np.int32),
                                                                                   y.view(torch.int16).numpy() if y.dtype != torch.float32 else y.numpy().view(np.int32)))
               for x, y in zip(a, b))


# ----------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_gradients_have_the_fp32_calls_bits(dt, combo):
    """{fp16, bf16} x COMBOS x BIASES x SHAPES on pattern A (rows of every length) and pattern B (columns of every length: the long-column kernel), both
    forms: fp32 outputs have the fp32 call's bits, 16-bit outputs are rounded once, dB is bit-equal in every mode, and the mixed modes (dQ fp32 with
    dK / dV 16-bit and the reverse) agree with the pure ones"""
    heads, kv = combo
    f32 = torch.float32
    for pat in (pattern_a, pattern_b):
        csr = pat(F32)
        with handle(csr) as h:
            for k, dv in SHAPES:
                ops = ops16(csr, heads, kv, k, dv, dt)
                scale = float(F32(1.0 / np.sqrt(k)))
                for kind in BIASES:
                    B = bias_of(csr, heads, kind)
                    for form in FORMS:
                        what = (pat.__name__, k, dv, kind, form)
                        want, OL = oracle(h, csr, heads, kv, ops, B, scale, form)
                        wide = call16(h, csr, heads, kv, ops, B, scale, f32, f32, OL)
                        assert matches(wide, want, dt), what
                        half = call16(h, csr, heads, kv, ops, B, scale, dt, dt, OL)
                        assert half[0].dtype == dt and half[1].dtype == dt and half[2].dtype == dt and matches(half, want, dt), what
                        a = call16(h, csr, heads, kv, ops, B, scale, f32, dt, OL)
                        b = call16(h, csr, heads, kv, ops, B, scale, dt, f32, OL)
                        assert same16(a, (wide[0], half[1], half[2], wide[3])) and same16(b, (half[0], wide[1], wide[2], wide[3])), what


# ----------------------------------------------------------------------------- 2. the rounds
@pytest.mark.parametrize("combo", [(6, 2), (4, 1)], ids=["6over2", "4over1"])
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_rounds_that_end_inside_a_group_round_once(dt, combo):
    """option attention_backward_heads in {1, 2, heads} on pattern B: rounds start and end inside a group, on short and on long columns.  The 16-bit dK
    and dV have the bits of the unbounded call and are the fp32 sums rounded once -- a read-back of a 16-bit partial sum fails here"""
    heads, kv = combo
    csr = pattern_b(F32)
    k, dv = 5, 4
    ops = ops16(csr, heads, kv, k, dv, dt)
    B = bias_of(csr, heads, "planes")
    with handle(csr) as h:
        want, OL = oracle(h, csr, heads, kv, ops, B, 0.5, "lse")
        want_self, _ = oracle(h, csr, heads, kv, ops, B, 0.5, "self")
        free = call16(h, csr, heads, kv, ops, B, 0.5, dt, dt, OL)
        free_self = call16(h, csr, heads, kv, ops, B, 0.5, dt, dt)
        assert matches(free, want, dt) and matches(free_self, want_self, dt)
    for limit in (1, 2, heads):
        with handle(csr, **{OPTION: limit}) as h:
            assert h.option(OPTION) == limit
            got = call16(h, csr, heads, kv, ops, B, 0.5, dt, dt, OL)
            assert same16(got, free) and matches(got, want, dt), limit
            assert same16(call16(h, csr, heads, kv, ops, B, 0.5, dt, dt), free_self), limit
            assert matches(call16(h, csr, heads, kv, ops, B, 0.5, torch.float32, torch.float32, OL), want, dt), limit


# ----------------------------------------------------------------------------- 3. need masks
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_every_subset_of_the_outputs(dt):
    """every subset of (dQ, dK, dV, dB): the wanted ones have the full call's bits, call16's canaries hold the writes, and the unwanted ones are not
    passed at all; with only dB wanted no transpose is built (device_bytes)"""
    heads, kv, k, dv = 4, 2, 5, 4
    csr = pattern_a(F32)
    ops = ops16(csr, heads, kv, k, dv, dt)
    B = bias_of(csr, heads, "planes")
    with handle(csr) as h:
        dev = [t.to(DEV) for t in ops]
        Bd = torch.from_numpy(B).to(DEV)
        h.attention_gqa_lse_16(*dev[:3], heads, kv, Bd, 0.5)   # spmm's tables
        torch.cuda.synchronize()
        b0 = h.info()["device_bytes"]
        only_db = h.attention_gqa_backward_16(*dev[:3], Bd, dev[3], heads, kv, 0.5, need=(False, False, False, True))
        torch.cuda.synchronize()
        b1 = h.info()["device_bytes"]
        assert only_db[:3] == (None, None, None) and b1 - b0 == 2 * 4 * csr.nnz * heads, "only dB: the two plane arrays and nothing else"
        full, OL = oracle(h, csr, heads, kv, ops, B, 0.5, "lse")
        assert same_bits(only_db[3].cpu().numpy(), oracle(h, csr, heads, kv, ops, B, 0.5, "self")[0][3])
        for need in itertools.product((False, True), repeat=4):
            for OLx in (None, OL):
                got = call16(h, csr, heads, kv, ops, B, 0.5, dt, dt, OLx, need=need)
                want = full if OLx is not None else oracle(h, csr, heads, kv, ops, B, 0.5, "self")[0]
                assert matches(got, tuple(w if n else None for w, n in zip(want, need)), dt), need
        # device outputs that are not wanted keep their canaries
        keep = [torch.full(s, CANARY, dtype=d, device=DEV) for s, d in zip(out_shapes(csr, heads, *ops[:3]), (dt, dt, dt, torch.float32))]
        api.attention_gqa_backward_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *dev[:3], Bd, dev[3], None, None, keep[0], None, keep[2], None, scale=0.5)
        torch.cuda.synchronize()
        assert bool((keep[1] == CANARY).all()) and bool((keep[3] == CANARY).all())


# ----------------------------------------------------------------------------- 4. layout
def _wide(ops, pad, off):
    wide = [torch.full((t.shape[0], t.shape[1] + pad + off), float("nan"), dtype=t.dtype) for t in ops]
    for wd, t in zip(wide, ops):
        wd[:, off:off + t.shape[1]] = t
    return wide, [wd[:, off:off + t.shape[1]] for wd, t in zip(wide, ops)]


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_pointer_kind_layout_method_and_stream_change_no_bit(dt):
    """k * 2 and dv * 2 multiples of 8 (k = 12, dv = 8, heads 6 over 2): aligned operands take the 8-byte form; column offsets of 0 .. 3 elements and
    odd leading dimensions take it or the element form, for the inputs and for 16-bit outputs.  Host and device pointers, each operand on its own
    side, every method, a non-default stream with async; canaries behind every row and a row behind the last"""
    csr = pattern_b(F32)
    heads, kv, k, dv = 6, 2, 12, 8
    ops = ops16(csr, heads, kv, k, dv, dt)
    B = bias_of(csr, heads, "planes")
    scale = 0.125
    f32 = torch.float32
    shp = out_shapes(csr, heads, *ops[:3])
    with handle(csr) as h:
        want, OL = oracle(h, csr, heads, kv, ops, B, scale, "lse")
        want_self, _ = oracle(h, csr, heads, kv, ops, B, scale, "self")
        Bd = torch.from_numpy(B).to(DEV)
        OLd = tuple(torch.from_numpy(x).to(DEV) for x in OL)
        for pad, off in ((0, 0), (4, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 2)):
            wide, views = _wide(ops, pad, off)
            for odt in (f32, dt):                                       # host pointers: staged and packed
                assert matches(call16(h, csr, heads, kv, views, B, scale, odt, odt, OL, pad=pad + off), want, dt), (pad, off, odt)
            assert matches(call16(h, csr, heads, kv, views, B, scale, dt, dt, pad=pad + off), want_self, dt), (pad, off)
            dev = [wd.to(DEV)[:, off:off + v.shape[1]] for wd, v in zip(wide, views)]
            for odt in (f32, dt):                                       # device pointers: used where they are, at this alignment and ld
                bufs = [torch.full((rows + 1, w + pad + off), CANARY, dtype=d, device=DEV) for (rows, w), d in zip(shp, (odt, odt, odt, f32))]
                outs = [b[:rows, off:off + w] for b, (rows, w) in zip(bufs[:3], shp)] + [bufs[3][:heads, :csr.nnz]]
                api.attention_gqa_backward_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *dev[:3], Bd, dev[3], *OLd, *outs, scale=scale)
                torch.cuda.synchronize()
                host = [b.cpu() for b in bufs]
                got = [hb[:rows, off:off + w] for hb, (rows, w) in zip(host[:3], shp)] + [host[3][:heads, :csr.nnz]]
                assert matches([g.clone().contiguous() for g in got], want, dt), (pad, off, odt)
                for g in got:
                    g.fill_(CANARY)
                assert all(bool((hb == CANARY).all()) for hb in host), "written outside the outputs' elements"
        dev = [t.to(DEV) for t in ops]
        for i in range(4):                                              # each operand on its own side
            mix = [dev[j] if j == i else ops[j] for j in range(4)]
            assert matches(call16(h, csr, heads, kv, mix, B, scale, dt, f32, OL), want, dt), i
        assert matches(call16(h, csr, heads, kv, ops, B, scale, dt, dt, OLd), want, dt)             # device O and L with host inputs
        st = torch.cuda.Stream()                                        # a non-default stream with async
        h.attach_stream(st.cuda_stream, async_=True)
        with torch.cuda.stream(st):
            g16 = h.attention_gqa_backward_16(*dev[:3], Bd, dev[3], heads, kv, scale, O=OLd[0], L=OLd[1])
            g32 = h.attention_gqa_backward_16(*dev[:3], Bd, dev[3], heads, kv, scale, O=OLd[0], L=OLd[1], dq_dtype=f32, dkv_dtype=f32)
            gs16 = h.attention_gqa_backward_16(*dev[:3], Bd, dev[3], heads, kv, scale)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert matches([g.cpu() for g in g16], want, dt) and matches([g.cpu() for g in g32], want, dt) and matches([g.cpu() for g in gs16], want_self, dt)
        assert matches(call16(h, csr, heads, kv, ops, B, scale, dt, dt, OL), want, dt)              # host operands on an asynchronous handle
    for method in METHODS:
        with handle(csr, method) as h:
            assert matches(call16(h, csr, heads, kv, ops, B, scale, dt, dt, OL), want, dt), method
            assert matches(call16(h, csr, heads, kv, ops, B, scale, f32, f32), want_self, dt), method


# ----------------------------------------------------------------------------- 5. special values
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_masks_and_nan_sit_where_the_fp32_call_puts_them(dt):
    """-inf bias entries, a fully masked row included (its softmax is NaN), behave as the fp32 call on the widened copies does: NaN in the same places
    (is_rounded and same_bits compare them), in both forms"""
    csr = pattern_a(F32)
    heads, kv, k, dv = 4, 2, 5, 4
    ops = ops16(csr, heads, kv, k, dv, dt)
    lens = np.diff(csr.rowptr)
    B = bias_of(csr, heads, "planes")
    two, three = int(np.flatnonzero(lens == 2)[0]), int(np.flatnonzero(lens == 3)[0])
    B[:, csr.rowptr[two]] = -np.inf                                       # one of two entries masked, for every head
    B[1, csr.rowptr[three]:csr.rowptr[three + 1]] = -np.inf               # a fully masked row of head 1
    with handle(csr) as h:
        for form in FORMS:
            want, OL = oracle(h, csr, heads, kv, ops, B, 1.0, form)
            assert np.isnan(want[0][three, k:2 * k]).all() and not np.isnan(want[0][two]).any() and np.isnan(want[1]).any()
            assert matches(call16(h, csr, heads, kv, ops, B, 1.0, torch.float32, torch.float32, OL), want, dt), form
            assert matches(call16(h, csr, heads, kv, ops, B, 1.0, dt, dt, OL), want, dt), form


def test_fp16_subnormals_in_k_v_and_g_are_not_flushed():
    dt = torch.float16
    csr = pattern_a(F32)
    heads, kv, k, dv = 4, 2, 5, 4
    Q, K, V, G = ops16(csr, heads, kv, k, dv, dt)
    rng = np.random.default_rng(4)
    sub = lambda shape: torch.from_numpy(rng.integers(1, 1024, shape).astype(np.int16)).view(torch.float16)   # the bit patterns 0x0001 .. 0x03ff
    K, V, G = sub(tuple(K.shape)), sub(tuple(V.shape)), sub(tuple(G.shape))
    ops = (Q, K, V, G)
    with handle(csr) as h:
        for form in FORMS:
            want, OL = oracle(h, csr, heads, kv, ops, None, 1.0, form)
            assert (want[2] != 0).any() and (want[0] != 0).any()          # the products with the subnormals are there: a flush would give zeros
            assert matches(call16(h, csr, heads, kv, ops, None, 1.0, torch.float32, torch.float32, OL), want, dt), form
            assert matches(call16(h, csr, heads, kv, ops, None, 1.0, dt, dt, OL), want, dt), form


def test_fp16_overflow_at_the_store_gives_inf():
    """Unlike the forward's O, a dV element is a sum over a COLUMN: two one-entry rows (P = 1 exactly) that share column 0, with G = 60000 on both, give
    an fp32 dV of 120000.  The fp16 dV is +inf exactly where the fp32 result is >= 65520 and finite elsewhere; bf16 stays finite"""
    m, n, heads, kv, k, dv = 6, 4, 2, 2, 4, 4
    rp = np.array([0, 1, 2, 4, 5, 5, 6], dtype=np.int32)
    ci = np.array([0, 0, 1, 2, 3, 1], dtype=np.int32)
    csr = synth.CSR(m, n, rp, ci, np.ones(6, dtype=F32))
    Gv = np.full((m, heads * dv), 0.5, dtype=F32)
    Gv[0], Gv[1] = 60000.0, 60000.0
    Gv[3, 0] = 65504.0                                                    # a one-entry row alone on column 3: dV = 65504, the largest fp16, stays finite
    # the CPU check: rows 0 and 1 have one entry, P = 1, so dV[0, c] = 1 * 60000 + 1 * 60000 = 120000 in fp32 (exact): >= 65520
    assert F32(F32(1.0) * F32(60000.0)) + F32(60000.0) == F32(120000.0) and 120000.0 >= 65520.0
    with handle(csr) as h:
        for dt in TYPES:
            base = ops16(csr, heads, kv, k, dv, dt)
            ops = (*base[:3], torch.from_numpy(Gv).to(dt))
            assert bool(torch.isfinite(ops[3]).all())
            for form in FORMS:
                want, OL = oracle(h, csr, heads, kv, ops, None, 0.5, form)
                dV32 = want[2]
                assert np.isfinite(dV32).all() and (dV32[0] == (120000.0 if dt == torch.float16 else float(ops[3][0, 0]) * 2)).all() and (dV32 >= 65520.0).any()
                got = call16(h, csr, heads, kv, ops, None, 0.5, dt, dt, OL)
                assert matches(got, want, dt), (dt, form)
                if dt == torch.float16:
                    assert bool(torch.isposinf(got[2]).eq(torch.from_numpy(dV32 >= 65520.0)).all()) and bool(torch.isposinf(got[2][0]).all())
                    assert bool(torch.isfinite(got[2][3]).all()) and float(got[2][3, 0]) == 65504.0
                else:
                    assert bool(torch.isfinite(got[2]).all())


# ----------------------------------------------------------------------------- 6. head by head, goldens, argument rules, the timer
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_every_head_is_the_one_head_call_on_its_slices(dt):
    """dQ and dB of head h of a 6-over-2 call equal the one-head _16 call on its slices, in both output types (16-bit outputs compared as integers)"""
    heads, kv = 6, 2
    gs = heads // kv
    csr = pattern_a(F32)
    with handle(csr) as h:
        for k, dv in SHAPES[1:]:
            Q, K, V, G = ops16(csr, heads, kv, k, dv, dt)
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                for odt in (torch.float32, dt):
                    dQ, _, _, dB = call16(h, csr, heads, kv, (Q, K, V, G), B, 0.5, odt, odt)
                    for hd in range(heads):
                        g = hd // gs
                        one = (Q[:, hd * k:(hd + 1) * k], K[:, g * k:(g + 1) * k], V[:, g * dv:(g + 1) * dv], G[:, hd * dv:(hd + 1) * dv])
                        q1, _, _, b1 = call16(h, csr, 1, 1, one, plane(B, hd), 0.5, odt, odt)
                        assert same16((q1, b1[0]), (dQ[:, hd * k:(hd + 1) * k].contiguous(), dB[hd].contiguous())), (k, dv, kind, odt, hd)


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", GOLDENS)
def test_golden_patterns(name, dt):
    csr = load_golden(f"{name}_f32_uniform")[0]
    heads, kv, k, dv = 6, 2, 3, 2
    ops = ops16(csr, heads, kv, k, dv, dt)
    with handle(csr) as h:
        for kind in ("none", "planes"):
            B = bias_of(csr, heads, kind)
            for form in FORMS:
                want, OL = oracle(h, csr, heads, kv, ops, B, 0.5, form)
                assert matches(call16(h, csr, heads, kv, ops, B, 0.5, torch.float32, torch.float32, OL), want, dt), (kind, form)
                got = call16(h, csr, heads, kv, ops, B, 0.5, dt, dt, OL)
                assert matches(got, want, dt), (kind, form)
                if csr.nnz == 0:
                    assert all((bits16(g) == 0).all() for g in got[:3])


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_m0_writes_zeros_to_dk_and_dv_and_nothing_else(dt):
    n, heads, kv, k, dv = 70, 4, 2, 3, 5
    csr = synth.CSR(0, n, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=F32))
    ops = (torch.zeros((0, heads * k), dtype=dt), torch.ones((n, kv * k), dtype=dt), torch.ones((n, kv * dv), dtype=dt), torch.zeros((0, heads * dv), dtype=dt))
    with handle(csr) as h:
        want = gqa_bwd_host(h, csr, heads, kv, *widened(ops[:3]), None, widened(ops)[3], 1.0)
        for odt in (torch.float32, dt):
            assert matches(call16(h, csr, heads, kv, ops, None, 1.0, odt, odt), want, dt), odt


def _untouched(outs):
    return all(bool((o == CANARY).all()) for o in outs)


def test_argument_and_handle_rules():
    lib = api.load()
    dt = torch.bfloat16
    heads, kv, k, dv = 4, 2, 3, 2
    for name, want in (("banded_f64_uniform", E_ARG), ("banded_f32_uniform", 0)):
        csr = load_golden(name)[0]
        ops = tuple(torch.from_numpy(a.astype(F32)).to(dt) for a in operands(csr, heads, kv, k, dv))
        outs = [torch.full(s, CANARY, dtype=d) for s, d in zip(out_shapes(csr, heads, *ops[:3]), (dt, dt, dt, torch.float32))]
        with handle(csr) as h:                                              # an fp64 handle is refused; the fp32 one of the same pattern works
            if want:                                                        # the wrapper raises before the library is asked; the symbol itself answers E_ARG
                with pytest.raises(TypeError):
                    api.attention_gqa_backward_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *ops[:3], None, ops[3], None, None, *outs)
                rc = lib.spmv_hip_attention_gqa_backward_16(h.h, csr.m, None, None, None, heads, kv, k, dv, 1.0, api.T_BF16, ops[0].data_ptr(), heads * k, ops[1].data_ptr(),
                                                            kv * k, ops[2].data_ptr(), kv * dv, None, 0, ops[3].data_ptr(), heads * dv, None, heads * dv, None, 0, api.T_BF16,
                                                            outs[0].data_ptr(), heads * k, api.T_BF16, outs[1].data_ptr(), kv * k, outs[2].data_ptr(), kv * dv,
                                                            outs[3].data_ptr(), csr.nnz)
            else:
                rc = api.attention_gqa_backward_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *ops[:3], None, ops[3], None, None, *outs, check=False)
            assert rc == want
            lib.spmv_hip_clear_error()
            assert _untouched(outs) == (want != 0)
    csr = load_golden("banded_f32_uniform")[0]
    ops = ops16(csr, heads, kv, k, dv, dt)
    outs = [torch.full(s, CANARY, dtype=d) for s, d in zip(out_shapes(csr, heads, *ops[:3]), (dt, dt, dt, torch.float32))]
    O, L = torch.zeros((csr.m, heads * dv)), torch.zeros((heads, csr.m))
    head = [csr.m, None, None, None, heads, kv, k, dv, 1.0]
    ins = [ops[0].data_ptr(), heads * k, ops[1].data_ptr(), kv * k, ops[2].data_ptr(), kv * dv, None, 0, ops[3].data_ptr(), heads * dv]
    ol = [O.data_ptr(), heads * dv, L.data_ptr(), csr.m]

    def raw(io=api.T_BF16, dq=api.T_BF16, dkv=api.T_BF16, ol=ol):
        """the symbol itself, for what the wrapper would refuse first: every rule asked here is answered before the CSR arguments are looked at"""
        rc = lib.spmv_hip_attention_gqa_backward_16(h.h, *head, io, *ins, *ol, dq, outs[0].data_ptr(), heads * k, dkv, outs[1].data_ptr(), kv * k, outs[2].data_ptr(), kv * dv,
                                                    outs[3].data_ptr(), csr.nnz)
        err = lib.spmv_hip_last_error()
        lib.spmv_hip_clear_error()
        return rc, err

    with handle(csr) as h:
        for io, dq, dkv in ((0, 0, 0), (3, 0, 0), (api.T_BF16, api.T_F16, 0), (api.T_BF16, 0, api.T_F16), (api.T_BF16, 3, 0), (api.T_F16, api.T_F16, api.T_BF16)):
            assert raw(io, dq, dkv) == (E_ARG, E_ARG), (io, dq, dkv)         # a bad type on a live handle
        assert raw(ol=[O.data_ptr(), heads * dv, None, csr.m]) == (E_ARG, E_ARG)       # exactly one of O and L
        assert raw(ol=[None, heads * dv, L.data_ptr(), csr.m]) == (E_ARG, E_ARG)
        assert raw(ol=[O.data_ptr(), heads * dv - 1, L.data_ptr(), csr.m]) == (E_ARG, E_ARG)   # ldo, ldl as in _backward_lse
        assert raw(ol=[O.data_ptr(), heads * dv, L.data_ptr(), csr.m - 1]) == (E_ARG, E_ARG)
        # found once the handle is looked at: a dB plane stride below nnz -- nothing written
        assert api.attention_gqa_backward_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *ops[:3], None, ops[3], None, None, *outs, check=False,
                                             lddb=csr.nnz - 1) == E_ARG
        lib.spmv_hip_clear_error()
        assert _untouched(outs)
        with pytest.raises(ValueError):
            api.attention_gqa_backward_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *ops[:3], None, ops[3], O, None, *outs)
        # nothing wanted: no work, and good arguments work
        assert api.attention_gqa_backward_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *ops[:3], None, ops[3]) == 0
        want, OL = oracle(h, csr, heads, kv, ops, None, 0.5, "lse")
        assert matches(call16(h, csr, heads, kv, ops, None, 0.5, dt, dt, OL), want, dt)
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert api.attention_gqa_backward_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *ops[:3], None, ops[3], None, None, *outs, check=False) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert _untouched(outs)
    h.close()


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_timer_runs_on_device_operands_and_leaves_the_calls_bits(dt):
    lib = api.load()
    csr = pattern_a(F32)
    heads, kv = 4, 2
    ops = ops16(csr, heads, kv, 8, 8, dt)
    B = bias_of(csr, heads, "planes")
    scale = float(1.0 / np.sqrt(8))
    dev = [t.to(DEV) for t in ops]
    Bd = torch.from_numpy(B).to(DEV)
    with handle(csr) as h:
        want, OL = oracle(h, csr, heads, kv, ops, B, scale, "lse")
        OLd = [torch.from_numpy(x).to(DEV) for x in OL]
        for odt in (dt, torch.float32):
            outs = [torch.empty(s, dtype=d, device=DEV) for s, d in zip(out_shapes(csr, heads, *ops[:3]), (odt, odt, odt, torch.float32))]
            mean, ms = api.time_attention_gqa_backward_16_launches(h.h, heads, kv, *dev[:3], Bd, dev[3], *OLd, *outs, scale=scale, warmup=1, iters=3)
            assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
            assert matches([o.cpu() for o in outs], want, dt)
        with pytest.raises(api.SpmvError):
            api.time_attention_gqa_backward_16_launches(h.h, heads, kv, ops[0], *dev[1:3], Bd, dev[3], *OLd, *outs, scale=scale, warmup=1, iters=1)   # a host Q
        lib.spmv_hip_clear_error()
