"""CPU: the constructions of the one-hot / tie tests and of the second-grid-trip tests (edge_cases.py) do what the GPU tests rely on."""
import numpy as np
import pytest

import edge_cases as ec
import gqa_cases as gc
import lse_cases as lc


def test_the_position_table_covers_every_class_for_every_length():
    """every class that exists in a row of n entries -- first, second, last; 63 / 64 / 65; 64 * u, u = 2 .. 7; 255 / 256; 511 / 512; the first
    entry of the last partial stride of 256; seg - 1, seg, 63 * seg with seg = ceil(n / 64) -- is in the row's position list, stated here
    independently of edge_cases.position_classes"""
    assert ec.NPOS == len(ec.position_list(5000)) == 19
    for n in gc.LENGTHS:
        pl = ec.position_list(n)
        assert pl == sorted(set(pl)) and all(0 <= p < n for p in pl) and (len(pl) > 0) == (n > 0)
        want = [0, 1, n - 1, 63, 64, 65, 255, 256, 511, 512] + [64 * u for u in range(2, 8)]
        if n > 256:
            tail = max(p for p in range(0, n, 256))
            assert n - 256 <= tail < n
            want.append(tail)
        if n > 512:
            seg = (n + 63) // 64
            want += [seg - 1, seg, 63 * seg]
        assert set(pl) == {p for p in want if 0 <= p < n}, n
    # a head per position: every position of every row of pattern A is some head's dominant entry, and ties pair neighbours of the list
    csr = gc.pattern_a(np.float32)
    dom = ec.dominant(csr, ec.NPOS)
    a, b = ec.tie_pairs(csr, ec.NPOS - 1)
    for i, n in enumerate(np.diff(csr.rowptr).tolist()):
        pl = ec.position_list(n)
        if n == 0:
            assert (dom[:, i] == -1).all() and (a[:, i] == -1).all() and (b[:, i] == -1).all()
            continue
        assert sorted(set((dom[:, i] - csr.rowptr[i]).tolist())) == pl, i
        if n >= 2:
            pairs = set(zip((a[:, i] - csr.rowptr[i]).tolist(), (b[:, i] - csr.rowptr[i]).tolist()))
            assert pairs == set(zip(pl[:-1], pl[1:])), i


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=gc.IDS)
def test_a_gap_of_g0_makes_numpys_softmax_one_hot(dtype):
    """the premise, in the handle's type on the host: with the one-hot bias the row softmax of pattern A's scores is exactly 1 at the dominant
    entry and exactly 0 elsewhere, and the row's log-sum-exp is the dominant score itself"""
    csr = gc.pattern_a(dtype)
    heads, k = 4, 3
    dom = ec.dominant(csr, heads, 7)
    B = ec.onehot_bias(csr, dom)
    Q, K, _, _ = gc.operands(csr, heads, heads, k, 2)
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    for hd in range(heads):
        Qh, Kh = Q[:, hd * k:(hd + 1) * k], K[:, hd * k:(hd + 1) * k]
        assert ec.wide_gap(csr, Qh, Kh, B[hd], 0.5, dom[hd], lc.hp(dtype)) > ec.GAP
        t = (Qh[rows] * Kh[csr.colidx]).sum(1) * dtype(0.5) + B[hd]
        assert t.dtype == dtype
        for i in np.flatnonzero(dom[hd] >= 0):
            r = t[csr.rowptr[i]:csr.rowptr[i + 1]]
            e = np.exp(r - r.max())
            p = e / e.sum()
            assert p[dom[hd, i] - csr.rowptr[i]] == 1 and p.sum() == 1 and r.max() + np.log(e.sum()) == t[dom[hd, i]]


def test_onehot_dv_is_the_plain_sum_where_no_column_is_long():
    """edge_cases.onehot_dv against np.add.at on small integers (exact in any order), with A^T's order from a stable sort by column"""
    csr = gc.pattern_a(np.float64)
    heads, kv, dv = 4, 2, 3
    dom = ec.dominant(csr, heads, 2)
    G = np.random.default_rng(0).integers(1, 9, (csr.m, heads * dv)).astype(np.float64)
    perm = np.argsort(csr.colidx, kind="stable")
    rp_t = np.zeros(csr.n + 1, dtype=np.int64)
    np.cumsum(np.bincount(csr.colidx, minlength=csr.n), out=rp_t[1:])
    want = np.zeros((csr.n, kv * dv))
    for hd in range(heads):
        has = dom[hd] >= 0
        g = hd // (heads // kv)
        np.add.at(want[:, g * dv:(g + 1) * dv], csr.colidx[dom[hd][has]], G[has, hd * dv:(hd + 1) * dv])
    assert np.array_equal(ec.onehot_dv(csr, rp_t, perm, dom, G, kv, dv), want)


def test_the_staircase_gives_every_column_to_one_row():
    csr = ec.staircase(np.float32)
    assert np.diff(csr.rowptr).tolist() == gc.LENGTHS and csr.n == csr.nnz and np.array_equal(csr.colidx, np.arange(csr.nnz))
    dom = ec.dominant(csr, 3)
    Q, K, V, G = ec.staircase_operands(csr, 3, 2, 2, dom)
    assert Q.shape == (csr.m, 9) and K.shape == (csr.n, 9) and (Q[:, 2::3] == 1).all()
    for hd in range(3):
        assert np.array_equal(np.flatnonzero(K[:, hd * 3 + 2] == 0), np.sort(dom[hd][dom[hd] >= 0])) and (K[:, hd * 3 + 2] <= 0).all()
    import torch
    for dt in (torch.float16, torch.bfloat16):   # -8192 and -4096 are exact in both 16-bit types
        assert torch.tensor([ec.KDROP, -ec.G0], dtype=torch.float64).to(dt).double().tolist() == [ec.KDROP, -ec.G0]


def test_the_grid_pattern_takes_a_second_trip_at_256_cus():
    """m = n = 8 * 256 + 67; more than 2048 rows and more than 2048 columns are longer than 512; every irregular length is there; the slices and
    parts the GPU tests compare with stay below the cap; the merge's two shapes exceed 8 * CUs workgroups of 256 / CW lane groups"""
    cus = 256
    csr = ec.grid_pattern(np.float32, cus)
    lens = np.diff(csr.rowptr)
    assert csr.m == csr.n == 2115 and 1_200_000 < csr.nnz < 1_400_000
    odd = np.flatnonzero(lens != ec.GRID_LEN)
    assert (np.diff(odd) == ec.GRID_EVERY).all() and set(lens[odd].tolist()) == set(ec.IRREGULAR)
    for i in (0, 96, 2114):
        assert np.array_equal(csr.colidx[csr.rowptr[i]:csr.rowptr[i + 1]], (i + np.arange(lens[i])) % csr.n)
    rows, cols = ec.long_counts(csr)
    assert rows > 8 * cus and cols > 8 * cus
    assert ec.cuts(2115) == [705, 1410, 2115]
    for s, r0, r1, e0, e1 in ec.row_slices(csr):
        assert s.m == r1 - r0 <= 1024 and s.nnz == e1 - e0 and np.array_equal(s.colidx, csr.colidx[e0:e1])
    parts = lc.split(csr, ec.cuts(csr.n))
    assert all(p.n <= 1024 and ec.long_counts(p)[0] <= 8 * cus for p, _ in parts)
    for heads, cw in ((32, 8), (256, 1)):
        assert csr.m * heads > 8 * cus * (256 // cw)
