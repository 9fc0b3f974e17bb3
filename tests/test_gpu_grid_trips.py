"""GPU: the second trip through a capped grid.  attention_long_kernel (and its 16-bit instantiations), attention_bwd_long_kernel,
attention_bwd_cols_long_kernel, spmm_long_kernel (also under spmm_transpose, through A^T) and row_reduce_long_kernel are launched with
min(nlong, 8 * CUs) workgroups and loop `for (i = blockIdx.x; i < nlong; i += gridDim.x)`; attention_merge_kernel is capped at 8 * CUs workgroups
of 256 / CW lane groups.  edge_cases.grid_pattern has more than 8 * CUs long rows and long columns, so the loops' second iteration runs: it
reuses part, s_slot, s_max / s_sum and the barriers, takes a later row's parking offset and restarts the grouped-head counters.

The oracles need no tolerance: a row's (column's) result is a function of that row (column) alone, so the call on the whole pattern must have
the bits of the same call on row slices (column parts) of at most 1024 rows (columns) -- handles that take one trip only.

So that the whole call and the slices cannot be wrong together, a sample is also held against the wide reference under the derived bars of
spread_cases.py: 32 long rows (half of them with an index in the long-row list >= 8 * CUs), every row of another length with its neighbours, and
64 columns (half of them beyond column 8 * CUs) with every row that reaches them.

1. the pattern takes the second trip   2. row side   3. column side   4. the merge   5. the sample against the wide reference"""
import numpy as np
import pytest
import torch

import edge_cases as ec
import lse_cases as lc
import spread_cases as sp
from gqa_cases import CANARY, DTYPES, IDS, bias_of, gqa_bwd_host, handle, operands, same_bits
from test_gpu_attention_16 import TYPES, TYPE_IDS, bits16, call16
from test_gpu_attention_merge import restated
from spmv_amd import api, build

pytestmark = pytest.mark.gpu

HEADS, KV, K = 2, 1, 5
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def grid(dtype):
    """the pattern, after asserting that it takes the second trip on this device"""
    csr = ec.grid_pattern(dtype, cus())
    rows, cols = ec.long_counts(csr)
    assert csr.m == csr.n == 8 * cus() + 67 and rows > 8 * cus() and cols > 8 * cus(), (csr.m, rows, cols, cus())
    return csr


def dvs(dtype):
    return [3, (16 if np.dtype(dtype) == np.float64 else 32) + 1]


_FWD = {}


def forward(dtype, dv):
    """operands, bias and the whole pattern's O and L, computed once per (dtype, dv) and shared"""
    key = (np.dtype(dtype), dv)
    if key not in _FWD:
        csr = grid(dtype)
        Q, K_, V, G = operands(csr, HEADS, KV, K, dv)
        B = bias_of(csr, HEADS, "planes")
        scale = float(dtype(1.0 / np.sqrt(K)))
        with handle(csr) as h:
            O, L = lc.lse_host(h, csr, HEADS, KV, Q, K_, V, B, scale)
        _FWD[key] = (csr, Q, K_, V, G, B, scale, O, L)
    return _FWD[key]


# ----------------------------------------------------------------------------- 1. the pattern
def test_the_pattern_takes_the_second_trip():
    csr = grid(F32)
    lens = np.diff(csr.rowptr)
    assert set(ec.IRREGULAR) <= set(lens.tolist()) and (lens == ec.GRID_LEN).sum() > 8 * cus()
    assert all(s.m <= 1024 for s, *_ in ec.row_slices(csr)) and all(p.n <= 1024 for p, _ in lc.split(csr, ec.cuts(csr.n)))


# ----------------------------------------------------------------------------- 2. row side
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_spmm_and_row_softmax_have_the_row_slices_bits(dtype):
    """spmm's Y, row_softmax forward and backward: spmm_long_kernel and row_reduce_long_kernel past their grids"""
    csr = grid(dtype)
    rng = np.random.default_rng(2)
    X = rng.uniform(-1, 1, (csr.n, 3)).astype(dtype)
    S, Gp = rng.uniform(-4, 4, csr.nnz).astype(dtype), rng.uniform(-1, 1, csr.nnz).astype(dtype)
    with handle(csr) as h:
        Y = np.full((csr.m, 5), CANARY, dtype=dtype)
        api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, X, Y[:, :3])
        assert (Y[:, 3:] == CANARY).all()
        P = h.row_softmax(S)
        dS = h.row_softmax_backward(P, Gp)
    for s, r0, r1, e0, e1 in ec.row_slices(csr):
        with handle(s) as hs:
            Ys = np.full((s.m, 5), CANARY, dtype=dtype)
            api.spmm(hs.h, s.m, s.rowptr, s.colidx, s.val, X, Ys[:, :3])
            assert same_bits(Ys, Y[r0:r1]), ("spmm", r0)
            Ps = hs.row_softmax(S[e0:e1].copy())
            assert same_bits(Ps, P[e0:e1]), ("row_softmax", r0)
            assert same_bits(hs.row_softmax_backward(Ps, Gp[e0:e1].copy()), dS[e0:e1]), ("row_softmax_backward", r0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_rows_have_the_row_slices_bits(dtype):
    """attention_gqa_lse's O and L; dQ and dB of attention_gqa_backward and of attention_gqa_backward_lse: 2 heads over 1, a bias, k = 5"""
    for dv in dvs(dtype):
        csr, Q, K_, V, G, B, scale, O, L = forward(dtype, dv)
        need = (True, False, False, True)
        with handle(csr) as h:
            dQ, _, _, dB = gqa_bwd_host(h, csr, HEADS, KV, Q, K_, V, B, G, scale, need)
            dQl, _, _, dBl = lc.bwd_lse_host(h, csr, HEADS, KV, Q, K_, V, B, G, O, L, scale, need)
        for s, r0, r1, e0, e1 in ec.row_slices(csr):
            Bs = np.ascontiguousarray(B[:, e0:e1])
            with handle(s) as hs:
                Os, Ls = lc.lse_host(hs, s, HEADS, KV, Q[r0:r1], K_, V, Bs, scale)
                assert same_bits(Os, O[r0:r1]) and same_bits(Ls, L[:, r0:r1]), ("gqa_lse", dv, r0)
                a, _, _, b = gqa_bwd_host(hs, s, HEADS, KV, Q[r0:r1], K_, V, Bs, G[r0:r1], scale, need)
                assert same_bits(a, dQ[r0:r1]) and same_bits(b, dB[:, e0:e1]), ("gqa_backward", dv, r0)
                a, _, _, b = lc.bwd_lse_host(hs, s, HEADS, KV, Q[r0:r1], K_, V, Bs, G[r0:r1], Os, Ls, scale, need)
                assert same_bits(a, dQl[r0:r1]) and same_bits(b, dBl[:, e0:e1]), ("gqa_backward_lse", dv, r0)


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_attention_16_rows_have_the_row_slices_bits(dt):
    """attention_gqa_lse_16's O (fp32 and 16-bit) and L"""
    for dv in dvs(F32):
        csr, Q, K_, V, _, B, scale, _, _ = forward(F32, dv)
        Q, K_, V = (torch.from_numpy(a).to(dt) for a in (Q, K_, V))
        with handle(csr) as h:
            O, L = call16(h, csr, HEADS, KV, Q, K_, V, B, scale, torch.float32)
            Oh, Lh = call16(h, csr, HEADS, KV, Q, K_, V, B, scale, dt)
        assert same_bits(L.numpy(), Lh.numpy())
        for s, r0, r1, e0, e1 in ec.row_slices(csr):
            Bs = np.ascontiguousarray(B[:, e0:e1])
            with handle(s) as hs:
                Os, Ls = call16(hs, s, HEADS, KV, Q[r0:r1], K_, V, Bs, scale, torch.float32)
                assert same_bits(Os.numpy(), O[r0:r1].numpy()) and same_bits(Ls.numpy(), L[:, r0:r1].numpy()), (dv, r0)
                Os, Ls = call16(hs, s, HEADS, KV, Q[r0:r1], K_, V, Bs, scale, dt)
                assert np.array_equal(bits16(Os), bits16(Oh[r0:r1])) and same_bits(Ls.numpy(), L[:, r0:r1].numpy()), (dv, r0)


# ----------------------------------------------------------------------------- 3. column side
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_columns_have_the_column_parts_bits(dtype):
    """spmm_transpose's rows and dK, dV of attention_gqa_backward_lse, given the whole pattern's O and L: spmm_long_kernel on A^T and
    attention_bwd_cols_long_kernel past their grids.  A part holds the columns [c0, c1) of every row, the rows' order kept"""
    dv = dvs(dtype)[1]
    csr, Q, K_, V, G, B, scale, O, L = forward(dtype, dv)
    X = np.random.default_rng(4).uniform(-1, 1, (csr.m, 3)).astype(dtype)
    need = (False, True, True, False)
    with handle(csr) as h:
        Y = np.full((csr.n, 5), CANARY, dtype=dtype)
        api.spmm_transpose(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, X, Y[:, :3])
        assert (Y[:, 3:] == CANARY).all()
        _, dK, dV, _ = lc.bwd_lse_host(h, csr, HEADS, KV, Q, K_, V, B, G, O, L, scale, need)
    bounds = ec.cuts(csr.n)
    for r, (p, idx) in enumerate(lc.split(csr, bounds)):
        c0, c1 = (0 if r == 0 else bounds[r - 1]), bounds[r]
        with handle(p) as hp:
            Yp = np.full((p.n, 5), CANARY, dtype=dtype)
            api.spmm_transpose(hp.h, p.m, p.rowptr, p.colidx, p.val, X, Yp[:, :3])
            assert same_bits(Yp, Y[c0:c1]), ("spmm_transpose", c0)
            _, a, b, _ = lc.bwd_lse_host(hp, p, HEADS, KV, Q, lc.rows_of(K_, bounds, r), lc.rows_of(V, bounds, r), lc.part_bias(B, idx), G, O, L, scale, need)
            assert same_bits(a, dK[c0:c1]) and same_bits(b, dV[c0:c1]), ("gqa_backward_lse", c0)


# ----------------------------------------------------------------------------- 4. the merge
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_merge_past_its_grid(dtype):
    """heads = 32 with dv = KP + 1 and heads = 256 with dv = 1 on this m: more (row, head) lane groups than 8 * CUs workgroups hold.  Against the
    contract's formula restated (test_gpu_attention_merge.py's bar, scaled by the sizes of O and L) and, bit for bit, against the call on row slices"""
    csr = grid(dtype)
    m = csr.m
    eps = np.finfo(dtype).eps
    V4 = 16 // np.dtype(dtype).itemsize
    KP = 16 if np.dtype(dtype) == np.float64 else 32
    with handle(csr) as h:
        for heads, dv in ((32, KP + 1), (256, 1)):
            cw = 1 if dv <= V4 else (2 if dv <= 2 * V4 else (4 if dv <= 4 * V4 else 8))   # kernels/dispatch.hpp: panel_group_width
            assert m * heads > 8 * cus() * (256 // cw), (heads, dv)
            rng = np.random.default_rng(heads + dv)
            O1, L1, O2, L2 = (rng.uniform(lo, hi, shape).astype(dtype) for lo, hi, shape in
                              ((-1, 1, (m, heads * dv)), (-3, 6, (heads, m)), (-1, 1, (m, heads * dv)), (-3, 6, (heads, m))))
            O, L = lc.merge_host(h, m, heads, O1, L1, O2, L2)
            Or, Lr = restated(O1, L1, O2, L2, heads)
            assert np.abs(O - Or).max() <= 32 * eps and np.abs(L - Lr).max() <= 128 * eps, (heads, dv)   # |O| <= 1, |L| <= 7
            for s, r0, r1, _, _ in ec.row_slices(csr):
                with handle(s) as hs:
                    Os, Ls = lc.merge_host(hs, s.m, heads, O1[r0:r1], np.ascontiguousarray(L1[:, r0:r1]), O2[r0:r1], np.ascontiguousarray(L2[:, r0:r1]))
                assert same_bits(Os, O[r0:r1]) and same_bits(Ls, L[:, r0:r1]), (heads, dv, r0)


# ----------------------------------------------------------------------------- 5. the sample against the wide reference
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_sample_stays_within_the_derived_bars(dtype):
    """O, L, dQ and dB on the sampled rows, dK and dV on the sampled columns, for attention_gqa_backward and attention_gqa_backward_lse: the reference
    and the bars are those of the pattern with every other row emptied, which changes nothing on the kept rows and on columns only kept rows reach"""
    dv = dvs(dtype)[0]
    csr, Q, K_, V, G, B, scale, O, L = forward(dtype, dv)
    cols, kept, picked = ec.grid_sample(csr, cus())
    lens = np.diff(csr.rowptr)
    longs = np.flatnonzero(lens > ec.LONG)
    assert picked.size == 32 and (np.searchsorted(longs, picked) >= 8 * cus()).sum() == 16 and np.isin(picked, kept).all() and (lens[picked] > ec.LONG).all()
    assert np.isin(np.flatnonzero(lens != ec.GRID_LEN), kept).all() and (cols >= 8 * cus()).sum() == 32
    sub, idx = ec.keep_rows(csr, kept)
    assert np.array_equal(np.bincount(sub.colidx, minlength=csr.n)[cols], np.bincount(csr.colidx, minlength=csr.n)[cols])   # the columns are complete
    Bs = np.ascontiguousarray(B[:, idx])
    ref = lc.reference(sub, HEADS, KV, Q, K_, V, Bs, scale, G)
    b = sp.bars(sub, HEADS, KV, Q, K_, V, Bs, scale, G)
    with handle(csr) as h:
        grads = gqa_bwd_host(h, csr, HEADS, KV, Q, K_, V, B, G, scale)
        grads_l = lc.bwd_lse_host(h, csr, HEADS, KV, Q, K_, V, B, G, O, L, scale)
    got = {"O": sp.ratio(O[kept], ref[0][kept], b.O[kept]), "L": sp.ratio(L[:, kept], ref[1][:, kept], b.errL[:, kept])}
    for tag, (dQ, dK, dV, dB), (bq, bk, bv, bb) in (("", grads, (b.dQ, b.dK, b.dV, b.dB)), (" by L", grads_l, (b.dQl, b.dKl, b.dVl, b.dBl))):
        got["dQ" + tag] = sp.ratio(dQ[kept], ref[2][kept], bq[kept])
        got["dK" + tag] = sp.ratio(dK[cols], ref[3][cols], bk[cols])
        got["dV" + tag] = sp.ratio(dV[cols], ref[4][cols], bv[cols])
        got["dB" + tag] = sp.ratio(dB[:, idx], ref[5], bb)
    print(f"{np.dtype(dtype).name} grid sample: max err / bar " + ", ".join(f"{n} {v:.3f}" for n, v in got.items()))
    for n, v in got.items():
        assert v <= 1, (n, v)
