"""GPU: spmv_hip_attention_gqa_lse_16 -- the fused attention forward on fp16 / bf16 Q, K and V over an fp32 handle, with O in fp32 or in that 16-bit
type (include/spmv_hip.h).

There is no tolerance anywhere: widening a 16-bit element to fp32 is exact, so the oracle is spmv_hip_attention_gqa_lse itself on the .float()
copies.  An fp32 O and L must have its bits; a 16-bit O must be its O rounded once, which is what torch.Tensor.to(dtype) does.  All operands are
gqa_cases.operands rounded to the 16-bit type by torch.

1. the fp32 call's bits   2. what changes no bit, the writes   3. head by head   4. special values   5. goldens, m = 0   6. handle rules, the timer"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gqa_cases import BIASES, CANARY, COMBOS, COMBO_IDS, DEV, E_ARG, E_NOSTATE, METHODS, M, bias_of, handle, operands, pattern_a, plane, same_bits
from lse_cases import lse_host
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

TYPES = [torch.float16, torch.bfloat16]
TYPE_IDS = ["f16", "bf16"]
SHAPES = [(1, 1), (5, 4), (33, 33), (32, 2)]   # width 1; an odd k: element access; a head wider than a panel in both roles; k a multiple of 32
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def ops16(csr, heads, kv, k, dv, dt, seed=0):
    """Q, K, V of gqa_cases.operands rounded to dt by torch (host tensors)"""
    return tuple(torch.from_numpy(a).to(dt) for a in operands(csr, heads, kv, k, dv, seed)[:3])


def widened(ops):
    """the .float() copies, as the numpy arrays the fp32 call takes"""
    return tuple(t.float().numpy() for t in ops)


def bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def call16(h, csr, heads, kv, Q, K, V, B, scale, out_dtype, pad=3, want_l=True):
    """spmv_hip_attention_gqa_lse_16 into canary-filled host buffers: O (of out_dtype) with `pad` elements behind every row and a row behind the last
    -- an odd pad gives a 16-bit O an odd ldo --, L with `pad` elements behind every plane and a plane behind the last; -> (O, L) as tensors"""
    w = heads * (V.shape[1] // kv)
    ob = torch.full((csr.m + 1, w + pad), CANARY, dtype=out_dtype)   # -7.25 is a value of fp16 and of bf16
    lb = torch.full((heads + 1, csr.m + pad), CANARY, dtype=torch.float32)
    api.attention_gqa_lse_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, B, ob[:csr.m, :w], lb[:heads, :csr.m] if want_l else None, scale=scale)
    assert bool((ob[:, w:] == CANARY).all()) and bool((ob[csr.m] == CANARY).all()), "written outside O's elements"
    assert bool((lb[:, csr.m:] == CANARY).all()) and bool((lb[heads] == CANARY).all()), "written outside L's elements"
    if not want_l:
        assert bool((lb == CANARY).all())
    return ob[:csr.m, :w].clone().contiguous(), (lb[:heads, :csr.m].clone().contiguous() if want_l else None)


def is_rounded(O16, O32, dt):
    """O16's bit pattern is O32.to(dt) wherever O32 is not NaN, and O16 is NaN exactly where O32 is"""
    O32 = torch.from_numpy(np.ascontiguousarray(O32)) if isinstance(O32, np.ndarray) else O32.cpu()
    O16 = O16.cpu()
    want, nan = O32.to(dt), torch.isnan(O32)
    return O16.dtype == dt and O16.shape == want.shape and torch.equal(torch.isnan(O16), nan) and np.array_equal(bits16(O16)[~nan.numpy()], bits16(want)[~nan.numpy()])


def check_both_modes(h, csr, heads, kv, ops, B, scale, dt, what):
    """-> (O32, L32), the fp32 call's results on the .float() copies, after holding both modes of the 16-bit call against them"""
    want_o, want_l = lse_host(h, csr, heads, kv, *widened(ops), B, scale)
    O, L = call16(h, csr, heads, kv, *ops, B, scale, torch.float32)
    assert same_bits(O.numpy(), want_o) and same_bits(L.numpy(), want_l), what
    Oh, Lh = call16(h, csr, heads, kv, *ops, B, scale, dt)
    assert is_rounded(Oh, want_o, dt) and same_bits(Lh.numpy(), want_l), what
    return want_o, want_l


# ----------------------------------------------------------------------------- 1. the fp32 call's bits
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_o_and_l_have_the_fp32_calls_bits(dt, combo):
    """{fp16, bf16} x COMBOS x BIASES x SHAPES on pattern A: with fp32 O, O and L are same_bits with api.attention_gqa_lse on the .float() copies; the
    16-bit O is that O rounded once; L has the same bits in both modes; L = None gives the same O"""
    heads, kv = combo
    csr = pattern_a(F32)
    with handle(csr) as h:
        for k, dv in SHAPES:
            ops = ops16(csr, heads, kv, k, dv, dt)
            scale = float(F32(1.0 / np.sqrt(k)))
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                want_o, _ = check_both_modes(h, csr, heads, kv, ops, B, scale, dt, (heads, kv, k, dv, kind))
                O, none = call16(h, csr, heads, kv, *ops, B, scale, torch.float32, want_l=False)
                assert none is None and same_bits(O.numpy(), want_o), (k, dv, kind)
                Oh, none = call16(h, csr, heads, kv, *ops, B, scale, dt, want_l=False)
                assert none is None and is_rounded(Oh, want_o, dt), (k, dv, kind)


# ----------------------------------------------------------------------------- 2. what changes no bit, the writes
def _wide(ops, pad, off):
    """every operand inside a wider NaN-filled tensor, `off` elements in and `pad` behind: -> (the wide tensors, the views)"""
    wide = [torch.full((t.shape[0], t.shape[1] + pad + off), float("nan"), dtype=t.dtype) for t in ops]
    for wd, t in zip(wide, ops):
        wd[:, off:off + t.shape[1]] = t
    return wide, [wd[:, off:off + t.shape[1]] for wd, t in zip(wide, ops)]


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_pointer_kind_layout_method_and_stream_change_no_bit(dt):
    """k * 2 and dv * 2 multiples of 8 (k = 12, dv = 8, heads 6 over 2): aligned device operands take the 8-byte form; row padding and column offsets
    of 0 .. 3 16-bit elements take it or the element form, for the inputs and for a 16-bit O.  Host and device pointers, each operand on its own
    side, every method, a non-default stream with async.  Canaries around O and L prove the exact writes, a 16-bit O with an odd ldo included"""
    csr = pattern_a(F32)
    heads, kv, k, dv = 6, 2, 12, 8
    w = heads * dv
    ops = ops16(csr, heads, kv, k, dv, dt)
    B = bias_of(csr, heads, "planes")
    scale = 0.125
    with handle(csr) as h:
        O0, L0 = check_both_modes(h, csr, heads, kv, ops, B, scale, dt, "packed")
        Bd = torch.from_numpy(B).to(DEV)
        for pad, off in ((0, 0), (4, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 2)):
            wide, views = _wide(ops, pad, off)
            for odt in (torch.float32, dt):                         # host pointers: staged and packed
                O, L = call16(h, csr, heads, kv, *views, B, scale, odt, pad=pad + off)
                assert (same_bits(O.numpy(), O0) if odt == torch.float32 else is_rounded(O, O0, dt)) and same_bits(L.numpy(), L0), (pad, off, odt)
            dev = [wd.to(DEV)[:, off:off + v.shape[1]] for wd, v in zip(wide, views)]
            for odt in (torch.float32, dt):                         # device pointers: used where they are, at this alignment and ld
                Od = torch.full((csr.m + 1, w + pad + off), CANARY, dtype=odt, device=DEV)
                Ld = torch.full((heads + 1, csr.m + pad + off), CANARY, dtype=torch.float32, device=DEV)
                api.attention_gqa_lse_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *dev, Bd, Od[:csr.m, off:off + w], Ld[:heads, off:off + csr.m], scale=scale)
                torch.cuda.synchronize()
                oh, lh = Od.cpu(), Ld.cpu()
                got = oh[:csr.m, off:off + w]
                assert (same_bits(got.numpy(), O0) if odt == torch.float32 else is_rounded(got, O0, dt)), (pad, off, odt)
                assert same_bits(lh[:heads, off:off + csr.m].numpy(), L0), (pad, off, odt)
                oh[:csr.m, off:off + w] = CANARY
                lh[:heads, off:off + csr.m] = CANARY
                assert bool((oh == CANARY).all()) and bool((lh == CANARY).all()), "written outside the outputs' elements"
        dev = [t.to(DEV) for t in ops]
        for mix in ((dev[0], ops[1], ops[2]), (ops[0], dev[1], ops[2]), (ops[0], ops[1], dev[2])):   # each operand on its own side
            O, L = call16(h, csr, heads, kv, *mix, B, scale, torch.float32)
            assert same_bits(O.numpy(), O0) and same_bits(L.numpy(), L0)
        Od = torch.full((csr.m, w), CANARY, dtype=dt, device=DEV)                                     # a device O with host inputs, a host L
        Lh = torch.full((heads, csr.m), CANARY, dtype=torch.float32)
        api.attention_gqa_lse_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *ops, B, Od, Lh, scale=scale)
        assert is_rounded(Od, O0, dt) and same_bits(Lh.numpy(), L0)
        st = torch.cuda.Stream()                                                                      # a non-default stream with async
        h.attach_stream(st.cuda_stream, async_=True)
        with torch.cuda.stream(st):
            O16, L16 = h.attention_gqa_lse_16(*dev, heads, kv, Bd, scale)
            O32, L32 = h.attention_gqa_lse_16(*dev, heads, kv, Bd, scale, out_dtype=torch.float32)
            On, none = h.attention_gqa_lse_16(*dev, heads, kv, Bd, scale, want_l=False)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert none is None and O16.dtype == dt and O32.dtype == torch.float32 and tuple(L16.shape) == (heads, csr.m) and L16.dtype == torch.float32
        assert is_rounded(O16, O0, dt) and is_rounded(On, O0, dt) and same_bits(O32.cpu().numpy(), O0)
        assert same_bits(L16.cpu().numpy(), L0) and same_bits(L32.cpu().numpy(), L0)
        O, L = call16(h, csr, heads, kv, *ops, B, scale, torch.float32)                               # host operands on an asynchronous handle
        assert same_bits(O.numpy(), O0) and same_bits(L.numpy(), L0)
    for method in METHODS:
        with handle(csr, method) as h:
            O, L = call16(h, csr, heads, kv, *ops, B, scale, torch.float32)
            assert same_bits(O.numpy(), O0) and same_bits(L.numpy(), L0), method
            assert is_rounded(call16(h, csr, heads, kv, *ops, B, scale, dt)[0], O0, dt), method


# ----------------------------------------------------------------------------- 3. head by head
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_every_head_is_the_one_head_call_on_its_slices(dt):
    """head h of a 6-over-2 call equals the one-head _16 call on its slices, in both O modes (bit patterns: a 16-bit O is compared as integers)"""
    heads, kv = 6, 2
    gs = heads // kv
    csr = pattern_a(F32)
    with handle(csr) as h:
        for k, dv in SHAPES[1:]:
            Q, K, V = ops16(csr, heads, kv, k, dv, dt)
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                for odt in (torch.float32, dt):
                    O, L = call16(h, csr, heads, kv, Q, K, V, B, 0.5, odt)
                    for hd in range(heads):
                        g = hd // gs
                        O1, L1 = call16(h, csr, 1, 1, Q[:, hd * k:(hd + 1) * k], K[:, g * k:(g + 1) * k], V[:, g * dv:(g + 1) * dv], plane(B, hd), 0.5, odt)
                        assert same_bits(L1[0].numpy(), L[hd].numpy()), (k, dv, kind, odt, hd)
                        assert same_bits(O1.view(torch.int16).numpy(), O[:, hd * dv:(hd + 1) * dv].contiguous().view(torch.int16).numpy()), (k, dv, kind, odt, hd)


# ----------------------------------------------------------------------------- 4. special values
def test_fp16_subnormals_in_k_and_v_are_not_flushed():
    """K and V made of fp16 subnormals (n * 2^-24, n = 1 .. 1023): the conversion keeps their values, so O and L have the bits of the fp32 call on
    the .float() copies -- and those bits differ from the call with the subnormals replaced by zeros, so a flush would show"""
    dt = torch.float16
    csr = pattern_a(F32)
    heads, kv, k, dv = 4, 2, 5, 4
    Q, K, V = ops16(csr, heads, kv, k, dv, dt)
    rng = np.random.default_rng(4)
    sub = lambda shape: torch.from_numpy(rng.integers(1, 1024, shape).astype(np.int16)).view(torch.float16)   # the bit patterns 0x0001 .. 0x03ff
    K, V = sub(tuple(K.shape)), sub(tuple(V.shape))
    assert bool((K.float() > 0).all()) and bool((K.float() < 2.0 ** -14).all())
    with handle(csr) as h:
        want_o, want_l = check_both_modes(h, csr, heads, kv, (Q, K, V), None, 1.0, dt, "subnormals")
        flushed_o, flushed_l = lse_host(h, csr, heads, kv, Q.float().numpy(), np.zeros(tuple(K.shape), F32), np.zeros(tuple(V.shape), F32), None, 1.0)
    lens = np.diff(csr.rowptr)
    assert (want_o[lens > 0] > 0).all() and (flushed_o == 0).all()          # the products with V's subnormals are there
    assert (want_l[:, lens > 1] != flushed_l[:, lens > 1]).any()            # and so are the scores from K's


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_nan_inf_and_masked_entries(dt):
    """a NaN and a +inf in ONE K row make exactly the rows that reach that column NaN (both heads of its group, O and L); a -inf bias entry is an exact
    +0 weight: a row of two entries with one of them masked returns the other's V row unchanged"""
    csr = pattern_a(F32)
    heads, kv, k, dv = 2, 1, 5, 4
    Q, K, V = ops16(csr, heads, kv, k, dv, dt)
    lens = np.diff(csr.rowptr)
    j0 = 17
    K[j0, 0], K[j0, 1] = float("nan"), float("inf")
    reach = np.array([j0 in csr.colidx[csr.rowptr[i]:csr.rowptr[i + 1]] for i in range(csr.m)])
    assert reach.any() and (~reach & (lens > 0)).any()
    B = bias_of(csr, heads, "planes")
    two = int(np.flatnonzero((lens == 2) & ~reach)[0])
    B[:, csr.rowptr[two]] = -np.inf                                        # the first of its two entries, for both heads
    with handle(csr) as h:
        want_o, want_l = check_both_modes(h, csr, heads, kv, (Q, K, V), B, 1.0, dt, "special")
        Oh, _ = call16(h, csr, heads, kv, Q, K, V, B, 1.0, dt)
    assert np.array_equal(np.isnan(want_o).all(axis=1), reach) and np.array_equal(np.isnan(want_o).any(axis=1), reach)
    assert np.array_equal(np.isnan(want_l), np.broadcast_to(reach, want_l.shape))
    kept = int(csr.colidx[csr.rowptr[two] + 1])
    for hd in range(heads):
        assert np.array_equal(bits16(Oh[two, hd * dv:(hd + 1) * dv]), bits16(V[kept])), hd


def test_fp16_o_rounds_to_nearest_even_at_the_top_of_the_range():
    """fp32 -> fp16 at the store: O32 >= 65520 has to become +inf, anything below it the finite neighbour.  Checked on the CPU first:
    a row's weights are a convex combination (they sum to 1 up to rounding), so with V = 60000 the fp32 sum stays at 60000 and
    even with V = 65504, the largest fp16, it stays within a few ulp of 65504 -- 65520 is not reachable with finite fp16 inputs (see the figures the
    test prints).  What is held instead, for both columns and rows of equal scores (Q = 0) of every length: O32 is finite, the 16-bit O is
    O32.to(float16) bit for bit, +inf wherever O32 >= 65520 (nowhere) -- and a V entry that IS +inf gives +inf in both modes on the rows that reach
    it with a nonzero weight"""
    dt = torch.float16
    csr = pattern_a(F32)
    heads, kv, k, dv = 2, 2, 4, 4
    lens = np.diff(csr.rowptr)
    Q = torch.zeros((csr.m, heads * k), dtype=dt)                          # equal scores: every weight is 1 / len
    K = ops16(csr, heads, kv, k, dv, dt)[1]
    V = torch.empty((csr.n, kv * dv), dtype=dt)
    V[:, :dv], V[:, dv:] = 60000.0, 65504.0
    # the CPU check: len * fl(1 / len) * v in fp32, the chain restated, never gets near 65520
    worst = 0.0
    for n in sorted(set(lens[lens > 0].tolist())):
        p = F32(1.0) / F32(n)
        acc = F32(0.0)
        for _ in range(n):
            acc = F32(np.float64(p) * 65504.0 + np.float64(acc))           # one fma: exact product and sum in double, rounded once
        worst = max(worst, float(acc))
    print(f"CPU: the largest fp32 sum of len weights 1/len times 65504 over pattern A's lengths = {worst!r}; the overflow threshold is 65520")
    assert worst < 65520.0
    with handle(csr) as h:
        want_o, _ = check_both_modes(h, csr, heads, kv, (Q, K, V), None, 1.0, dt, "top of the range")
        Oh, _ = call16(h, csr, heads, kv, Q, K, V, None, 1.0, dt)
        assert np.isfinite(want_o).all() and (want_o[lens > 0] > 59999.0).all()
        print(f"GPU: the largest fp32 O = {float(want_o.max())!r}")
        assert bool(torch.isinf(Oh).eq(torch.from_numpy(want_o >= 65520.0)).all())
        j0 = 23
        V[j0, 0] = float("inf")
        reach = np.array([j0 in csr.colidx[csr.rowptr[i]:csr.rowptr[i + 1]] for i in range(csr.m)])
        want_o, _ = check_both_modes(h, csr, heads, kv, (Q, K, V), None, 1.0, dt, "inf in V")
        Oh, _ = call16(h, csr, heads, kv, Q, K, V, None, 1.0, dt)
        assert reach.any() and bool(torch.isposinf(Oh[:, 0]).eq(torch.from_numpy(reach)).all()) and np.array_equal(np.isposinf(want_o[:, 0]), reach)


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_a_row_of_one_entry_returns_vs_value_unchanged(dt):
    """P is exactly 1 on a row of one entry: the 16-bit O holds V's 16-bit values bit for bit -- subnormals of the 16-bit type, the largest and the
    smallest normal values included (V's row at that column is made of them)"""
    csr = pattern_a(F32)
    heads, kv, k, dv = 4, 2, 5, 6
    Q, K, V = ops16(csr, heads, kv, k, dv, dt)
    lens = np.diff(csr.rowptr)
    rows = np.flatnonzero(lens == 1)
    assert rows.size
    pats = np.array([0x0001, 0x0002, 0x007f, 0x0080, 0x03ff, 0x0400, 0x7bff if dt == torch.float16 else 0x7f7f, 0x8001, 0x83ff, 0xfbff if dt == torch.float16 else 0xff7f,
                     0x3c00, 0x0000], dtype=np.uint16).view(np.int16)
    for i in rows:
        V[int(csr.colidx[csr.rowptr[i]])] = torch.from_numpy(pats.copy()).view(dt)
    with handle(csr) as h:
        check_both_modes(h, csr, heads, kv, (Q, K, V), None, 0.5, dt, "one entry")
        Oh, _ = call16(h, csr, heads, kv, Q, K, V, None, 0.5, dt)
    gs = heads // kv
    for i in rows:
        j = int(csr.colidx[csr.rowptr[i]])
        for hd in range(heads):
            g = hd // gs
            assert np.array_equal(bits16(Oh[i, hd * dv:(hd + 1) * dv]), bits16(V[j, g * dv:(g + 1) * dv])), (i, hd)


# ----------------------------------------------------------------------------- 5. goldens, m = 0
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["nnz0", "empty_mix", "tiny"])
def test_golden_patterns(name, dt):
    """the goldens as patterns only, against the same fp32 oracle; rows without entries get +0 and L = -inf"""
    csr = load_golden(f"{name}_f32_uniform")[0]
    heads, kv, k, dv = 6, 2, 3, 2
    ops = ops16(csr, heads, kv, k, dv, dt)
    lens = np.diff(csr.rowptr)
    with handle(csr) as h:
        for kind in ("none", "planes"):
            B = bias_of(csr, heads, kind)
            want_o, want_l = check_both_modes(h, csr, heads, kv, ops, B, 0.5, dt, (name, kind))
            Oh, _ = call16(h, csr, heads, kv, *ops, B, 0.5, dt)
            assert (bits16(Oh)[lens == 0] == 0).all() and (want_l[:, lens == 0] == -np.inf).all()
            if csr.nnz == 0:
                assert (bits16(Oh) == 0).all()


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_m0_is_no_work(dt):
    n, heads, kv, k, dv = 70, 4, 2, 3, 5
    csr = synth.CSR(0, n, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=F32))
    Q = torch.zeros((0, heads * k), dtype=dt)
    K, V = torch.ones((n, kv * k), dtype=dt), torch.ones((n, kv * dv), dtype=dt)
    with handle(csr) as h:
        for odt in (torch.float32, dt):
            O, L = call16(h, csr, heads, kv, Q, K, V, None, 1.0, odt)   # the canaries: nothing is written
            assert tuple(O.shape) == (0, heads * dv) and tuple(L.shape) == (heads, 0)


# ----------------------------------------------------------------------------- 6. handle rules, the timer
def _untouched(O, L):
    return bool((O == CANARY).all()) and bool((L == CANARY).all())


def test_handle_rules():
    lib = api.load()
    dt = torch.bfloat16
    heads, kv, k, dv = 4, 2, 3, 2
    for name, want in (("banded_f64_uniform", E_ARG), ("banded_f32_uniform", 0)):
        csr = load_golden(name)[0]
        Q, K, V = ops16(csr, heads, kv, k, dv, dt)
        O, L = torch.full((csr.m, heads * dv), CANARY, dtype=dt), torch.full((heads, csr.m), CANARY)
        with handle(csr) as h:                                              # an fp64 handle is refused; the fp32 one of the same pattern works
            assert api.attention_gqa_lse_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, O, L, check=False) == want
            lib.spmv_hip_clear_error()
            assert _untouched(O, L) == (want != 0)
    csr = load_golden("banded_f32_uniform")[0]
    Q, K, V = ops16(csr, heads, kv, k, dv, dt)
    O, L = torch.full((csr.m, heads * dv), CANARY, dtype=dt), torch.full((heads, csr.m), CANARY)
    args = [csr.m, None, None, None, heads, kv, k, dv, 1.0]
    ptrs = [Q.data_ptr(), heads * k, K.data_ptr(), kv * k, V.data_ptr(), kv * dv, None, 0, O.data_ptr(), heads * dv]
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, csr.n).astype(F32)
    with handle(csr) as h:
        y0 = h.spmv(x, np.full(csr.m, np.nan, dtype=F32))
        for io, ot in ((0, 0), (3, 0), (api.T_BF16, api.T_F16), (api.T_BF16, 3)):   # a bad type on a live handle
            assert lib.spmv_hip_attention_gqa_lse_16(h.h, *args, io, *ptrs, ot, L.data_ptr(), csr.m) == E_ARG, (io, ot)
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
        # found before the handle is looked at: planes closer than m; found once it is: a bias plane stride below nnz -- outputs untouched
        assert api.attention_gqa_lse_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, O, L, check=False, ldl=csr.m - 1) == E_ARG
        lib.spmv_hip_clear_error()
        assert api.attention_gqa_lse_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, np.zeros(heads * csr.nnz, dtype=F32), O, L, check=False,
                                        ldb=csr.nnz - 1) == E_ARG
        lib.spmv_hip_clear_error()
        assert _untouched(O, L)
        check_both_modes(h, csr, heads, kv, (Q, K, V), None, 0.5, dt, "banded")
        assert same_bits(h.spmv(x, np.full(csr.m, np.nan, dtype=F32)), y0)   # the resident values are not touched
        # device operands: device_bytes is attention_gqa_lse's
        dev = [t.to(DEV) for t in (Q, K, V)]
        h.attention_gqa_lse(*[t.float() for t in dev], heads, kv, None, 0.5)
        torch.cuda.synchronize()
        b1 = h.info()["device_bytes"]
        h.attention_gqa_lse_16(*dev, heads, kv, None, 0.5)
        h.attention_gqa_lse_16(*dev, heads, kv, None, 0.5, out_dtype=torch.float32)
        torch.cuda.synchronize()
        assert h.info()["device_bytes"] == b1
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            assert api.attention_gqa_lse_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, O, L, check=False) == E_ARG, key
            lib.spmv_hip_clear_error()
            assert _untouched(O, L)
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert api.attention_gqa_lse_16(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, O, L, check=False) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert _untouched(O, L)
    h.close()


def test_reorder_handle_is_an_argument_error():
    lib = api.load()
    m, n, rp, ci, va = synth.banded_holes_device(100_000, 100_000, 24, 0.25, "eighths", torch.float32, DEV, 7)
    api.set_thread_option("reorder", 1)
    try:
        h = api.Handle(m, n, rp, ci, va, M.Method_Parallel)
    finally:
        api.clear_thread_options()
    with h:
        assert h.index is not None
        Q = torch.ones((m, 8), dtype=torch.float16, device=DEV)
        KV = torch.ones((n, 4), dtype=torch.float16, device=DEV)
        O = torch.full((m, 8), CANARY, dtype=torch.float16, device=DEV)
        L = torch.full((4, m), CANARY, dtype=torch.float32, device=DEV)
        lib.spmv_hip_clear_error()
        assert api.attention_gqa_lse_16(h.h, m, rp, ci, va, 4, 2, Q, KV, KV, None, O, L, check=False) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert _untouched(O, L)


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_timer_runs_on_device_operands_and_leaves_the_calls_bits(dt):
    lib = api.load()
    csr = pattern_a(F32)
    heads, kv = 4, 2
    ops = ops16(csr, heads, kv, 8, 8, dt)
    B = bias_of(csr, heads, "planes")
    dev = [t.to(DEV) for t in ops] + [torch.from_numpy(B).to(DEV)]
    scale = float(1.0 / np.sqrt(8))
    with handle(csr) as h:
        want_o, want_l = lse_host(h, csr, heads, kv, *widened(ops), B, scale)
        for odt in (dt, torch.float32):
            O = torch.empty((csr.m, heads * 8), dtype=odt, device=DEV)
            L = torch.empty((heads, csr.m), dtype=torch.float32, device=DEV)
            mean, ms = api.time_attention_gqa_lse_16_launches(h.h, heads, kv, *dev, O, L, warmup=1, iters=3)
            assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
            assert (same_bits(O.cpu().numpy(), want_o) if odt == torch.float32 else is_rounded(O, want_o, dt)) and same_bits(L.cpu().numpy(), want_l)
        with pytest.raises(api.SpmvError):
            api.time_attention_gqa_lse_16_launches(h.h, heads, kv, ops[0], *dev[1:], O, L, warmup=1, iters=1)   # a host Q
        lib.spmv_hip_clear_error()
        with pytest.raises(api.SpmvError):
            api.time_attention_gqa_lse_16_launches(h.h, heads, kv, *dev, O, torch.empty((heads, csr.m)), warmup=1, iters=1)   # a host L
        lib.spmv_hip_clear_error()
