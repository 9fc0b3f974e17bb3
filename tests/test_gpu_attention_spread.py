"""GPU: the bias entry points of the fused sparse attention at wide finite score spreads -- a per-row constant C_i in {0, +-2^12} plus a spread that
fills [-S, 0] with S on both sides of exp's denormal and zero thresholds (30, 95, 120 in fp32; 30, 730, 800 in fp64) -- against the wide reference
lse_cases.reference under the DERIVED bars of spread_cases.py (its docstring holds the derivation; test_attention_spread_host.py shows on the CPU
that the bars can be met).  Inside [-35, 35], where every other attention test lives, exp cannot overflow or underflow and a wrong maximum that
stays near the true one changes nothing; here it does.

Forward (attention_gqa, attention_gqa_lse, attention_gqa_lse_16), backward (attention_gqa_backward), the L-driven backward
(attention_gqa_backward_lse on the forward's own O and L) and the merge of pattern A's two-part split.  No element is left out of a comparison
(spread_cases.ratio asserts it).  Each case prints max err / bar per output; DESIGN.md 3.24 has the table."""
import numpy as np
import pytest
import torch

import lse_cases as lc
import spread_cases as sp
from gqa_cases import DTYPES, IDS, PATTERNS, gqa_bwd_host, gqa_host, handle, operands, same_bits
from test_gpu_attention_16 import TYPES, TYPE_IDS, call16
from spmv_amd import api, build

pytestmark = pytest.mark.gpu

F32 = np.float32
NAMES = ("dQ", "dK", "dV", "dB")
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def report(what, got):
    print(f"{what}: max err / bar " + ", ".join(f"{n} {v:.3f}" for n, v in got.items()))
    for n, v in got.items():
        assert v <= 1, (what, n, v)


@pytest.mark.parametrize("which", list(PATTERNS))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_forward_and_both_backwards_stay_within_the_derived_bars(dtype, which):
    csr = PATTERNS[which](dtype)
    Q, K, V, G = operands(csr, sp.HEADS, sp.KV, sp.K, sp.DV)
    scale = float(dtype(1.0 / np.sqrt(sp.K)))
    with handle(csr) as h:
        for S in sp.SPREADS[np.dtype(dtype)]:
            B = sp.spread_bias(csr, sp.HEADS, S)
            ref = lc.reference(csr, sp.HEADS, sp.KV, Q, K, V, B, scale, G)
            assert all(np.isfinite(r).all() for r in (ref[0], *ref[2:])), "the reference is finite: no element is left out"
            b = sp.bars(csr, sp.HEADS, sp.KV, Q, K, V, B, scale, G)
            O, L = lc.lse_host(h, csr, sp.HEADS, sp.KV, Q, K, V, B, scale)
            assert same_bits(gqa_host(h, csr, sp.HEADS, sp.KV, Q, K, V, B, scale), O)
            got = {"O": sp.ratio(O, ref[0], b.O), "L": sp.ratio(L, ref[1], b.errL)}
            grads = gqa_bwd_host(h, csr, sp.HEADS, sp.KV, Q, K, V, B, G, scale)
            grads_l = lc.bwd_lse_host(h, csr, sp.HEADS, sp.KV, Q, K, V, B, G, O, L, scale)
            for name, g, gl, r, bar, barl in zip(NAMES, grads, grads_l, ref[2:], (b.dQ, b.dK, b.dV, b.dB), (b.dQl, b.dKl, b.dVl, b.dBl)):
                got[name], got[name + " by L"] = sp.ratio(g, r, bar), sp.ratio(gl, r, barl)
            report(f"{np.dtype(dtype).name} {which} S={S}", got)


@pytest.mark.parametrize("which", list(PATTERNS))
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_the_16_bit_call_stays_within_the_derived_bars(dt, which):
    """the reference and the bars are taken from the 16-bit operands widened (the operands as the kernel receives them); a 16-bit O adds its one
    rounding: u16 (|O_ref| + bar) and half the type's smallest subnormal"""
    csr = PATTERNS[which](F32)
    ops = tuple(torch.from_numpy(a).to(dt) for a in operands(csr, sp.HEADS, sp.KV, sp.K, sp.DV)[:3])
    Q, K, V = (t.float().numpy() for t in ops)
    G = np.zeros((csr.m, sp.HEADS * sp.DV), dtype=F32)
    scale = float(F32(1.0 / np.sqrt(sp.K)))
    sub = 2.0 ** -25 if dt == torch.float16 else 2.0 ** -134
    with handle(csr) as h:
        for S in sp.SPREADS[np.dtype(F32)]:
            B = sp.spread_bias(csr, sp.HEADS, S)
            Oref, Lref = lc.reference(csr, sp.HEADS, sp.KV, Q, K, V, B, scale)
            b = sp.bars(csr, sp.HEADS, sp.KV, Q, K, V, B, scale, G)
            O, L = call16(h, csr, sp.HEADS, sp.KV, *ops, B, scale, torch.float32)
            Oh, Lh = call16(h, csr, sp.HEADS, sp.KV, *ops, B, scale, dt)
            assert same_bits(L.numpy(), Lh.numpy())
            lens = np.diff(csr.rowptr)
            bar16 = b.O + np.where(lens > 0, 1, 0)[:, None] * (U16[dt] * (np.abs(Oref) + b.O) + sub)
            report(f"{dt} {which} S={S}", {"O": sp.ratio(O.numpy(), Oref, b.O), "L": sp.ratio(L.numpy(), Lref, b.errL),
                                          "O16": sp.ratio(Oh.float().numpy(), Oref, bar16)})


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_two_part_merge_stays_within_the_derived_bars(dtype):
    """pattern A cut at column 150: one attention_gqa_lse per part, merged; the weights exp(L_r - Lm) carry the parts' L errors, u |L| among them"""
    csr, parts, bounds = lc.parts_a(dtype, 2)
    Q, K, V, G = operands(csr, sp.HEADS, sp.KV, sp.K, sp.DV)
    scale = float(dtype(1.0 / np.sqrt(sp.K)))
    hs = [handle(p) for p, _ in parts]
    try:
        for S in sp.SPREADS[np.dtype(dtype)]:
            B = sp.spread_bias(csr, sp.HEADS, S)
            Oref, Lref = lc.reference(csr, sp.HEADS, sp.KV, Q, K, V, B, scale)
            pb = [sp.bars(p, sp.HEADS, sp.KV, Q, lc.rows_of(K, bounds, r), lc.rows_of(V, bounds, r), lc.part_bias(B, idx), scale, G) for r, (p, idx) in enumerate(parts)]
            barO, barL = sp.merge_bars(pb, sp.HEADS, dtype)
            O, L = lc.fold(hs, parts, bounds, sp.HEADS, sp.KV, Q, K, V, B, scale)
            report(f"{np.dtype(dtype).name} merge S={S}", {"O": sp.ratio(O, Oref, barO), "L": sp.ratio(L, Lref, barL)})
    finally:
        for x in hs:
            x.close()
