"""CPU: the derived bars of spread_cases.py can be met.  The formulas of the bias entry points restated in the handle's type with numpy (its exp,
log and sums in place of the device's), on the very inputs of test_gpu_attention_spread.py, stay within the same bars against the same wide
reference -- forward, backward, the L-driven backward and the merge of the two-part split.  A bar that the arithmetic itself cannot meet shows
up here without a device."""
import numpy as np
import pytest

import gqa_cases as gc
import lse_cases as lc
import spread_cases as sp
from test_gpu_attention_merge import restated as merge_restated

NAMES = ("dQ", "dK", "dV", "dB")


def inputs(dtype, which, S):
    csr = gc.PATTERNS[which](dtype)
    Q, K, V, G = gc.operands(csr, sp.HEADS, sp.KV, sp.K, sp.DV)
    return csr, Q, K, V, G, sp.spread_bias(csr, sp.HEADS, S), float(dtype(1.0 / np.sqrt(sp.K)))


def test_the_bias_fills_the_spread_below_a_row_constant():
    for dtype in gc.DTYPES:
        for S in sp.SPREADS[np.dtype(dtype)]:
            csr, Q, K, V, G, B, scale = inputs(dtype, "rows", S)
            _, L = lc.reference(csr, sp.HEADS, sp.KV, Q, K, V, B, scale)
            lens = np.diff(csr.rowptr)
            assert np.isfinite(L[:, lens > 0]).all() and float(np.abs(L[:, lens > 0]).max()) > 4000   # |L| near 2^12: the u |L| term is there
            for i in np.flatnonzero(lens > 1):
                r = B[0, csr.rowptr[i]:csr.rowptr[i + 1]].astype(np.float64)
                assert r[0] == sp.CONSTANTS[i % 3] and abs((r[0] - r[-1]) - S) <= 4096 * np.finfo(dtype).eps and (r <= r[0]).all() and (r >= r[-1]).all()


@pytest.mark.parametrize("which", list(gc.PATTERNS))
@pytest.mark.parametrize("dtype", gc.DTYPES, ids=gc.IDS)
def test_the_formulas_in_the_handles_type_stay_within_the_bars(dtype, which):
    worst = {}
    for S in sp.SPREADS[np.dtype(dtype)]:
        csr, Q, K, V, G, B, scale = inputs(dtype, which, S)
        ref = lc.reference(csr, sp.HEADS, sp.KV, Q, K, V, B, scale, G)
        b = sp.bars(csr, sp.HEADS, sp.KV, Q, K, V, B, scale, G)
        assert all(np.isfinite(r).all() for r in (ref[0], *ref[2:])), "the reference is finite: no element is left out"
        O, L, grads, grads_l = sp.restated(csr, sp.HEADS, sp.KV, Q, K, V, B, scale, G)
        got = {"O": sp.ratio(O, ref[0], b.O), "L": sp.ratio(L, ref[1], b.errL)}
        for name, g, gl, r, bar, barl in zip(NAMES, grads, grads_l, ref[2:], (b.dQ, b.dK, b.dV, b.dB), (b.dQl, b.dKl, b.dVl, b.dBl)):
            got[name], got[name + " by L"] = sp.ratio(g, r, bar), sp.ratio(gl, r, barl)
        print(f"{np.dtype(dtype).name} {which} S={S}: " + ", ".join(f"{n} {v:.3f}" for n, v in got.items()))
        for n, v in got.items():
            assert v <= 1, (S, n, v)
            worst[n] = max(worst.get(n, 0.0), v)
    assert all(v > 0 for v in worst.values())   # the restatement rounds: the reference is not compared with itself


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=gc.IDS)
def test_the_merge_formula_in_the_handles_type_stays_within_its_bars(dtype):
    for S in sp.SPREADS[np.dtype(dtype)]:
        csr, Q, K, V, G, B, scale = inputs(dtype, "rows", S)
        _, parts, bounds = lc.parts_a(dtype, 2)
        ref = lc.reference(csr, sp.HEADS, sp.KV, Q, K, V, B, scale)
        pb, po = [], []
        for r, (p, idx) in enumerate(parts):
            Kr, Vr, Br = lc.rows_of(K, bounds, r), lc.rows_of(V, bounds, r), lc.part_bias(B, idx)
            pb.append(sp.bars(p, sp.HEADS, sp.KV, Q, Kr, Vr, Br, scale, G))
            po += list(sp.restated(p, sp.HEADS, sp.KV, Q, Kr, Vr, Br, scale, G)[:2])
        barO, barL = sp.merge_bars(pb, sp.HEADS, dtype)
        with np.errstate(invalid="ignore", divide="ignore"):
            O, L = merge_restated(*po, sp.HEADS)
        none = np.isneginf(ref[1])   # no entry in either part: the kernel answers +0 and -inf where the bare formula has 0 / 0
        assert np.array_equal(np.isnan(L), none)
        L[none] = -np.inf
        O[np.repeat(none.T, sp.DV, axis=1)] = 0
        ro, rl = sp.ratio(O, ref[0], barO), sp.ratio(L, ref[1], barL)
        print(f"{np.dtype(dtype).name} S={S}: merged O {ro:.3f}, L {rl:.3f}")
        assert 0 < ro <= 1 and 0 < rl <= 1, (S, ro, rl)
