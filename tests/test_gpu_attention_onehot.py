"""GPU: the fused sparse attention family on one-hot and tie rows -- scores 4096 (or 8192 * scale) apart, where a wrong maximum, a term dropped
from the maximum but not from the sum, or a stale M or Z of another head changes the result by orders of magnitude instead of by a rounding.

There is no tolerance (except the two roundings of a tie's L = log 2): with one entry per (row, head) dominant by more than 800 every other
weight is an exact 0 in fp32 and in fp64, Z is exactly 1 and every addition of a +-0 term is exact (edge_cases.py), so
  O[i, head block] == V[j*, its K / V block]          bit for bit; a 16-bit O has the 16-bit V's bits
  L[hd, i]         == t*                              the dominant entry's score: api.sddmm, * scale, + B (lse_cases.scores)
  dQ == 0, dK == 0, dB == 0                           as values: the sign of a zero is free
  dV[j]            == the sum of G[i, head block] over the rows and heads where j is dominant, in the contract's order (edge_cases.onehot_dv)
The dominant entry sits at every position class of edge_cases.position_classes, one head per position.

1. bias entry points, forward   2. the 16-bit call   3. bias entry points, backward   4. the staircase: attention, heads and their backwards
5. ties   6. the merge"""
import math

import numpy as np
import pytest
import torch

import edge_cases as ec
import lse_cases as lc
from gqa_cases import CANARY, DTYPES, IDS, PATTERNS, gqa_bwd_host, gqa_host, handle, operands, pattern_a, same_bits
from test_gpu_attention_16 import TYPES, TYPE_IDS, bits16, call16, ops16, widened
from spmv_amd import api, build

pytestmark = pytest.mark.gpu

F32 = np.float32
# (heads, kv_heads, shift): every position in one call with a plane per head; then the groupings, their heads on positions further down the list
CONFIGS = [(ec.NPOS, ec.NPOS, 0), (2, 1, 0), (2, 1, 9), (6, 2, 3), (6, 2, 12)]
CONFIG_IDS = [f"{h}over{g}+{s}" for h, g, s in CONFIGS]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def widths(dtype):
    """(k, dv): a head wider than a panel, and a narrow one"""
    W, KP = (2, 16) if np.dtype(dtype) == np.float64 else (4, 32)
    return [(3, KP + 1), (W + 1, 2)]


def nonzero_v(ops):
    assert (ops[2] != 0).all(), "V without zeros: no signed-zero case"
    return ops


def assert_gaps(csr, heads, kv, Q, K, B, scale, doms):
    """every head's dominant entries lead their rows by more than GAP, from wide-precision scores; doms: one table, or the two of a tie"""
    gs, k = heads // kv, Q.shape[1] // heads
    wide = lc.hp(csr.val.dtype)
    for hd in range(heads):
        Bh = None if B is None else B[hd].copy()
        for dom in doms[1:]:   # a tie: the second dominant entry is not one of "the others"
            Bh[dom[hd][dom[hd] > doms[0][hd]]] = -np.inf   # (a row of one entry has b == a)
        gap = ec.wide_gap(csr, Q[:, hd * k:(hd + 1) * k], K[:, (hd // gs) * k:(hd // gs + 1) * k], Bh, scale, doms[0][hd], wide)
        assert gap > ec.GAP, (hd, gap)


def dominant_scores(h, csr, heads, kv, Q, K, B, scale, dom):
    """(heads, m): t* in the handle's dtype from api.sddmm, * scale, + B; -inf on a row without entries"""
    gs, k = heads // kv, Q.shape[1] // heads
    out = np.full((heads, csr.m), -np.inf, dtype=csr.val.dtype)
    for hd in range(heads):
        t = lc.scores(h, csr, Q[:, hd * k:(hd + 1) * k], K[:, (hd // gs) * k:(hd // gs + 1) * k], B[hd], scale)
        has = dom[hd] >= 0
        out[hd, has] = t[dom[hd][has]]
    return out


def bias_host(h, csr, heads, Q, K, V, B, scale, pad=3):
    """spmv_hip_attention_bias through host pointers into a canary-filled O"""
    w = V.shape[1]
    buf = np.full((csr.m + 1, w + pad), CANARY, dtype=csr.val.dtype)
    api.attention_bias(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, B, buf[:csr.m, :w], scale=scale)
    assert (buf[:, w:] == CANARY).all() and (buf[csr.m] == CANARY).all(), "written outside O's elements"
    return buf[:csr.m, :w].copy()


def canaries(shapes, dtype, need, pad=3):
    bufs = [np.full((r + 1, w + pad), CANARY, dtype=dtype) if want else None for want, (r, w) in zip(need, shapes)]
    return bufs, [None if b is None else b[:r, :w] for b, (r, w) in zip(bufs, shapes)]


def untouched_around(bufs, views):
    return all(b is None or ((b[:, v.shape[1]:] == CANARY).all() and (b[v.shape[0]] == CANARY).all()) for b, v in zip(bufs, views))


def check_backward(got, csr, want_dv, need, what):
    """dQ, dK, dB zero as values; dV the restated sums (values: the bits wherever the sum is not zero)"""
    for name, g, want in zip(("dQ", "dK", "dV", "dB"), got, need):
        assert (g is not None) == want, (what, name)
        if g is None:
            continue
        if name == "dV":
            assert g.dtype == want_dv.dtype and np.array_equal(g, want_dv), (what, name, int((g != want_dv).sum()))
        else:
            assert (g == 0).all(), (what, name, int((g != 0).sum()))


# ----------------------------------------------------------------------------- 1. bias entry points, forward
@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("which", list(PATTERNS))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bias_onehot_forward(dtype, which, config):
    """attention_bias (kv = heads), attention_gqa and attention_gqa_lse: O is V's row at the dominant column, L the dominant score, bit for bit"""
    heads, kv, shift = config
    csr = PATTERNS[which](dtype)
    dom = ec.dominant(csr, heads, shift)
    B = ec.onehot_bias(csr, dom)
    with handle(csr) as h:
        for k, dv in widths(dtype):
            Q, K, V, _ = nonzero_v(operands(csr, heads, kv, k, dv))
            scale = float(dtype(1.0 / np.sqrt(k)))
            assert_gaps(csr, heads, kv, Q, K, B, scale, [dom])
            want_o = ec.onehot_o(csr, V, dom, kv, dv)
            want_l = dominant_scores(h, csr, heads, kv, Q, K, B, scale, dom)
            if kv == heads:
                assert same_bits(bias_host(h, csr, heads, Q, K, V, B, scale), want_o), ("bias", k, dv)
            assert same_bits(gqa_host(h, csr, heads, kv, Q, K, V, B, scale), want_o), ("gqa", k, dv)
            O, L = lc.lse_host(h, csr, heads, kv, Q, K, V, B, scale)
            assert same_bits(O, want_o) and same_bits(L, want_l), ("gqa_lse", k, dv, int((L != want_l).sum()))


# ----------------------------------------------------------------------------- 2. the 16-bit call
@pytest.mark.parametrize("config", CONFIGS[:1] + CONFIGS[3:4], ids=CONFIG_IDS[:1] + CONFIG_IDS[3:4])
@pytest.mark.parametrize("which", list(PATTERNS))
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_bias_onehot_16(dt, which, config):
    """attention_gqa_lse_16: an fp32 O holds V.float()'s bits, a 16-bit O the 16-bit V's own bits, L the dominant score of the widened operands"""
    heads, kv, shift = config
    gs = heads // kv
    csr = PATTERNS[which](F32)
    dom = ec.dominant(csr, heads, shift)
    B = ec.onehot_bias(csr, dom)
    with handle(csr) as h:
        for k, dv in widths(F32):
            ops = ops16(csr, heads, kv, k, dv, dt)
            Q, K, V = widened(ops)
            assert (V != 0).all()
            scale = float(F32(1.0 / np.sqrt(k)))
            assert_gaps(csr, heads, kv, Q, K, B, scale, [dom])
            want_l = dominant_scores(h, csr, heads, kv, Q, K, B, scale, dom)
            O, L = call16(h, csr, heads, kv, *ops, B, scale, torch.float32)
            assert same_bits(O.numpy(), ec.onehot_o(csr, V, dom, kv, dv)) and same_bits(L.numpy(), want_l), (k, dv)
            Oh, Lh = call16(h, csr, heads, kv, *ops, B, scale, dt)
            assert same_bits(Lh.numpy(), want_l), (k, dv)
            vb, ob = bits16(ops[2]), bits16(Oh)
            for hd in range(heads):
                has = dom[hd] >= 0
                assert np.array_equal(ob[has, hd * dv:(hd + 1) * dv], vb[csr.colidx[dom[hd][has]], (hd // gs) * dv:(hd // gs + 1) * dv]), (k, dv, hd)
                assert (ob[~has, hd * dv:(hd + 1) * dv] == 0).all()


# ----------------------------------------------------------------------------- 3. bias entry points, backward
@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("which", list(PATTERNS))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bias_onehot_backward(dtype, which, config):
    """attention_bias_backward (kv = heads), attention_gqa_backward and attention_gqa_backward_lse on the forward's own O and L; all outputs
    wanted, and dV alone"""
    heads, kv, shift = config
    csr = PATTERNS[which](dtype)
    dom = ec.dominant(csr, heads, shift)
    B = ec.onehot_bias(csr, dom)
    with handle(csr) as h:
        for k, dv in widths(dtype):
            Q, K, V, G = nonzero_v(operands(csr, heads, kv, k, dv))
            scale = float(dtype(1.0 / np.sqrt(k)))
            assert_gaps(csr, heads, kv, Q, K, B, scale, [dom])
            O, L = lc.lse_host(h, csr, heads, kv, Q, K, V, B, scale)
            want_dv = None
            for need in ((True, True, True, True), (False, False, True, False)):
                got = gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, scale, need)
                if want_dv is None:   # the transpose exists once a backward has run
                    rp_t, perm = api.transpose_map(h.h, csr.n, csr.nnz)
                    want_dv = ec.onehot_dv(csr, rp_t, perm, dom, G, kv, dv)
                check_backward(got, csr, want_dv, need, ("gqa_backward", k, dv))
                check_backward(lc.bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, scale, need), csr, want_dv, need, ("gqa_backward_lse", k, dv))
                if kv == heads:
                    bufs, views = canaries(((csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv), (heads, csr.nnz)), dtype, need)
                    api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, B, G, *views, scale=scale)
                    assert untouched_around(bufs, views)
                    check_backward(views, csr, want_dv, need, ("bias_backward", k, dv))


# ----------------------------------------------------------------------------- 4. the staircase
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_staircase_onehot_without_a_bias(dtype):
    """attention_heads and attention_heads_backward with NPOS heads, attention and attention_backward head by head: the dominance comes from one
    extra column of Q (1) and K (0 at the dominant column, -8192 elsewhere); every column lies in one row, so dV[j] is G's row of the row that
    owns j in the heads where j is dominant, and 0 elsewhere"""
    csr = ec.staircase(dtype)
    heads, k, dv, scale = ec.NPOS, 3, 2, 0.125
    k1 = k + 1
    dom = ec.dominant(csr, heads)
    Q, K, V, G = nonzero_v(ec.staircase_operands(csr, heads, k, dv, dom))
    assert ec.KDROP * scale < -ec.GAP
    assert_gaps(csr, heads, heads, Q, K, None, scale, [dom])
    want_o = ec.onehot_o(csr, V, dom, heads, dv)
    want_dv = np.zeros((csr.n, heads * dv), dtype=dtype)
    for hd in range(heads):
        has = dom[hd] >= 0
        want_dv[csr.colidx[dom[hd][has]], hd * dv:(hd + 1) * dv] = G[has, hd * dv:(hd + 1) * dv]
    shapes = ((csr.m, heads * k1), (csr.n, heads * k1), (csr.n, heads * dv))
    with handle(csr) as h:
        buf = np.full((csr.m + 1, heads * dv + 3), CANARY, dtype=dtype)
        api.attention_heads(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, buf[:csr.m, :heads * dv], scale=scale)
        assert (buf[:, heads * dv:] == CANARY).all() and (buf[csr.m] == CANARY).all()
        assert same_bits(buf[:csr.m, :heads * dv], want_o)
        for need in ((True, True, True), (False, False, True)):
            bufs, views = canaries(shapes, dtype, need)
            api.attention_heads_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, G, *views, scale=scale)
            assert untouched_around(bufs, views)
            check_backward((*views, None), csr, want_dv, (*need, False), "heads_backward")
        for hd in range(heads):
            qs, vs = slice(hd * k1, (hd + 1) * k1), slice(hd * dv, (hd + 1) * dv)
            O = np.full((csr.m, dv), CANARY, dtype=dtype)
            api.attention(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q[:, qs], K[:, qs], V[:, vs], O, scale)
            assert same_bits(O, want_o[:, vs]), hd
            for need in ((True, True, True), (False, False, True)):
                bufs, views = canaries(((csr.m, k1), (csr.n, k1), (csr.n, dv)), dtype, need)
                api.attention_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q[:, qs], K[:, qs], V[:, vs], G[:, vs], *views, scale=scale)
                assert untouched_around(bufs, views)
                check_backward((*views, None), csr, np.ascontiguousarray(want_dv[:, vs]), (*need, False), ("backward", hd))


# ----------------------------------------------------------------------------- 5. ties
def half_sum(Va, Vb):
    """fl(0.5 * Va + 0.5 * Vb) in the operands' dtype, rounded once: the halves are exact, the sum is math.fsum's"""
    out = np.array([math.fsum((0.5 * float(x), 0.5 * float(y))) for x, y in zip(Va.ravel(), Vb.ravel())], dtype=np.float64).reshape(Va.shape)
    return out.astype(Va.dtype)   # fp32: the exact sum of two fp32 values of these sizes is a double


def tie_o(csr, V, a, b, kv, dv):
    heads = a.shape[0]
    gs = heads // kv
    O = np.zeros((csr.m, heads * dv), dtype=V.dtype)
    for hd in range(heads):
        has = a[hd] >= 0
        c = slice((hd // gs) * dv, (hd // gs + 1) * dv)
        O[has, hd * dv:(hd + 1) * dv] = half_sum(V[csr.colidx[a[hd][has]], c], V[csr.colidx[b[hd][has]], c])
    return O


def check_tie_l(L, a, b, dtype):
    """two entries: L = 0 + log 2 within the library's bound on log 2 plus the addition's half ulp (test_gpu_attention_merge.py's two roundings);
    one entry: 0; none: -inf"""
    want = np.log(np.longdouble(2))
    bound = lc.LOG_ULP * np.spacing(dtype(np.log(2))) + np.spacing(dtype(want)) / 2
    two, one, none = (a >= 0) & (b > a), (a >= 0) & (b == a), a < 0
    assert two.any() and float(np.abs(L[two].astype(np.longdouble) - want).max()) <= bound
    assert (L[one] == 0).all() and (L[none] == -np.inf).all()


@pytest.mark.parametrize("kv", [None, 3], ids=["ungrouped", "over3"])
@pytest.mark.parametrize("which", list(PATTERNS))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ties_forward(dtype, which, kv):
    """Q = 0 and two dominant entries a < b across the class boundaries: P = 1/2, 1/2 exactly, O == fl(0.5 V_a + 0.5 V_b) bit for bit"""
    heads = ec.NPOS - 1 - (ec.NPOS - 1) % 3   # the adjacent pairs of the longest position list; a multiple of 3
    kv = heads if kv is None else kv
    csr = PATTERNS[which](dtype)
    a, b = ec.tie_pairs(csr, heads)
    B = ec.onehot_bias(csr, a, b)
    with handle(csr) as h:
        for k, dv in widths(dtype):
            _, K, V, _ = nonzero_v(operands(csr, heads, kv, k, dv))
            Q = np.zeros((csr.m, heads * k), dtype=dtype)
            assert_gaps(csr, heads, kv, Q, K, B, 0.5, [a, b])
            want_o = tie_o(csr, V, a, b, kv, dv)
            if kv == heads:
                assert same_bits(bias_host(h, csr, heads, Q, K, V, B, 0.5), want_o), (k, dv)
            assert same_bits(gqa_host(h, csr, heads, kv, Q, K, V, B, 0.5), want_o), (k, dv)
            O, L = lc.lse_host(h, csr, heads, kv, Q, K, V, B, 0.5)
            assert same_bits(O, want_o), (k, dv)
            check_tie_l(L, a, b, dtype)


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_ties_16(dt):
    csr = pattern_a(F32)
    heads, kv = ec.NPOS - 1 - (ec.NPOS - 1) % 3, 3
    a, b = ec.tie_pairs(csr, heads)
    B = ec.onehot_bias(csr, a, b)
    with handle(csr) as h:
        for k, dv in widths(F32):
            _, K, V = ops16(csr, heads, kv, k, dv, dt)
            Q = torch.zeros((csr.m, heads * k), dtype=dt)
            assert_gaps(csr, heads, kv, Q.float().numpy(), K.float().numpy(), B, 0.5, [a, b])
            want_o = tie_o(csr, V.float().numpy(), a, b, kv, dv)
            O, L = call16(h, csr, heads, kv, Q, K, V, B, 0.5, torch.float32)
            assert same_bits(O.numpy(), want_o), (k, dv)
            check_tie_l(L.numpy(), a, b, F32)
            Oh, _ = call16(h, csr, heads, kv, Q, K, V, B, 0.5, dt)
            assert np.array_equal(bits16(Oh), bits16(torch.from_numpy(want_o).to(dt))), (k, dv)


# ----------------------------------------------------------------------------- 6. the merge
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_merge_takes_the_larger_part_unchanged(dtype):
    """L1 - L2 = +-4096 with |L| up to 2^20 (fp32) / 2^40 (fp64): the smaller part's weight is an exact 0 and W exactly 1, so O has the bits of the
    larger part's O and L the larger L's bits"""
    csr = pattern_a(dtype)
    m, heads = csr.m, 3
    top = 20 if dtype == np.float32 else 40
    rng = np.random.default_rng(3)
    KP = 16 if dtype == np.float64 else 32
    with handle(csr) as h:
        for dv in (1, 5, KP, KP + 1):
            O1, O2 = (rng.uniform(0.25, 1, (m, heads * dv)).astype(dtype) * rng.choice([-1, 1], (m, heads * dv)).astype(dtype) for _ in range(2))
            L1 = (rng.choice([-1.0, 1.0], (heads, m)) * 2.0 ** rng.uniform(-2, top, (heads, m))).astype(dtype)
            L1[0, :4] = dtype(2.0 ** top), dtype(-2.0 ** top), dtype(0), dtype(ec.G0)
            first = rng.random((heads, m)) < 0.5               # where part 1 is the larger
            L2 = np.where(first, L1 - dtype(ec.G0), L1 + dtype(ec.G0)).astype(dtype)
            assert (np.abs(L1.astype(np.longdouble) - L2.astype(np.longdouble)) > ec.GAP).all() and first.any() and (~first).any()
            O, L = lc.merge_host(h, m, heads, O1, L1, O2, L2)
            assert same_bits(L, np.where(first, L1, L2))
            want = np.where(np.repeat(first.T, dv, axis=1), O1, O2)   # (m, heads * dv): head hd's block follows first[hd]
            assert same_bits(O, want), dv
