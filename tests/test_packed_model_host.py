"""CPU: the host model of the PACKED tiles (tests/packed_cases.py) and what tests/test_gpu_packed_forms.py assumes about its fixtures.

The GPU tests compare the packed planes with the host's value array through `probe_readback`, and the gate's counts with `model_packed`.  Both
rest on host code, which is checked here without a GPU: the slot permutation, the integer encode / decode (on the values that sit at the edges of
the 24-bit and 32-bit fields), the spans of the edge-value fixtures (54 packs, 55 does not), the distinct-columns condition of every probed matrix,
and the per-tile flags the model gives for every structural fixture.
"""
import numpy as np
import pytest

import packed_cases as pc


@pytest.mark.parametrize("L", [L for L in range(1, 65) if L & (L - 1) == 0])
def test_pack_slot_is_a_bijection_matching_lane4(L):
    """pack_slot maps every aligned block of 4L positions onto itself, and the entry Lane4 hands lane l as its k-th -- chunk-local position
    (k / 2) * 2L + 2l + k % 2 -- lands at slot 4l + k.  Every L in 1 .. 64 that lanes_per_row accepts: the powers of two (pack_slot finds the
    block with a mask)."""
    C = 4 * L
    for base in (0, C, 7 * C, (1 << 31) - C):
        slots = [pc.pack_slot_model(base + q, L) for q in range(C)]
        assert sorted(slots) == list(range(base, base + C))
        for l in range(L):
            for k in range(4):
                assert pc.pack_slot_model(base + (k // 2) * 2 * L + 2 * l + k % 2, L) == base + 4 * l + k


def _fields(v, e=pc.EDGE_E):
    lo, hi = pc.encode(v, e)
    return lo, hi


def test_edge_patterns_hit_the_field_edges():
    fixed = [p for p in pc.EDGE_PATTERNS if p is not None]
    los = {_fields(p)[0] for p in fixed}
    his = {_fields(p)[1] for p in fixed}
    assert {0x7FFFFF, 0x800000, 0xFFFFFF, 0} <= his, sorted(map(hex, his))
    assert {0, 0xFFFFFFFF, 8, 0xFFFFFFF8} <= los, sorted(map(hex, los))
    assert _fields(2.0 ** 15 - 2.0 ** -37) == (0xFFFFFFF8, 0x7FFFFF)          # k = 2^55 - 8
    assert _fields(-(2.0 ** 15 - 2.0 ** -37)) == (8, 0x800000)               # hi = -2^23, the field's minimum
    assert _fields(-2.0 ** -40) == (0xFFFFFFFF, 0xFFFFFF)                    # k = -1
    assert _fields(2.0 ** -8) == (0, 1) and _fields(-2.0 ** -8) == (0, 0xFFFFFF)
    assert _fields(2.0 ** -8 - 2.0 ** -40) == (0xFFFFFFFF, 0)
    assert _fields(0.0) == (0, 0)


def test_decode_inverts_encode_on_every_edge_value():
    """every value of the edge fixture (fixed patterns and the random 53-bit ones), of the DBL_MAX tile and of the subnormal tile, under its
    tile's exponent; and through the three-word layout of four 24-bit fields with the value at each of the four positions"""
    m, rp, ci, va = pc._edges()
    sets = [(np.unique(va), pc.EDGE_E), (np.unique(pc.dblmax_values(8192)), 971), (np.unique(pc.subnormal_values(8192)), -1074)]
    for vals, e in sets:
        span = pc.bit_span(vals)
        assert span[1] == e and span[0] - span[1] <= 54
        for v in vals[:: max(1, vals.size // 3000)].tolist() + [vals[0], vals[-1]]:
            lo, hi = pc.encode(v, e)
            back = pc.decode(lo, hi, e)
            assert np.float64(back).view(np.uint64) == np.float64(v).view(np.uint64), (v, lo, hi, back)
    fixed = [p for p in pc.EDGE_PATTERNS if p is not None]
    for i, v in enumerate(fixed):
        for k in range(4):
            quad = [fixed[(i + 1 + j) % len(fixed)] for j in range(4)]
            quad[k] = v
            enc = [pc.encode(q, pc.EDGE_E) for q in quad]
            h = pc.unpack_hi_words(pc.pack_hi_words([hi for _, hi in enc]))
            for j in range(4):
                assert h[j] == pc._sext24(enc[j][1])
                assert pc.decode(enc[j][0], h[j] & 0xFFFFFF, pc.EDGE_E) == quad[j]


def test_edge_fixture_spans_and_positions():
    """span exactly 54 in every tile of the packing fixture; exactly 55 in tile 2 of its twin (and 54 elsewhere); every fixed pattern at each of
    the four positions of a lane quad (slot % 4 after the permutation, L = 8) in every tile"""
    c = pc.fixture("edges")
    assert pc.tile_spans(c.rp, c.va) == [54] * 5
    t = pc.fixture("edges_twin")
    assert pc.tile_spans(t.rp, t.va) == [54, 54, 55, 54, 54]
    x = pc.fixture("exotic")
    assert pc.tile_spans(x.rp, x.va)[:4] == [54, 52, 54, None]
    slot = np.array([pc.pack_slot_model(p, 8) for p in range(int(c.rp[pc.TILE]))]) % 4
    v0 = c.va[:int(c.rp[pc.TILE])]
    for p in pc.EDGE_PATTERNS:
        if p is not None:
            assert set(slot[v0 == p].tolist()) == {0, 1, 2, 3}, p
    row = np.repeat(np.arange(c.m), np.diff(c.rp))
    idx = (np.arange(c.va.size) + row) % len(pc.EDGE_PATTERNS)
    for tile in range(5):
        assert set(idx[c.rp[tile * pc.TILE]:c.rp[(tile + 1) * pc.TILE]].tolist()) == set(range(len(pc.EDGE_PATTERNS)))


def _all_cases():
    for name in pc.FIXTURES:
        yield name, pc.fixture(name)
    for L, chunks in pc.FORM_CASES:
        yield f"form-L{L}-x{chunks}", pc.form_case(L, chunks)


def test_probed_matrices_have_distinct_columns_modulo_their_stride():
    for name, c in _all_cases():
        assert c.rp[-1] == c.ci.size == c.va.size and c.ci.min() >= 0 and c.ci.max() < c.n, name
        assert pc.distinct_mod(c.rp, c.ci, c.stride), name
    c = pc.form_case(8, 1)               # the transpose case probes A^T of this one
    t = pc.transpose_csr(c.m, c.n, c.rp, c.ci, c.va)
    assert pc.distinct_mod(t[2], t[3], c.stride) and (np.diff(t[2]) == 32).all()
    assert not pc.distinct_mod(c.rp, c.ci, c.stride // 2)                      # the check can fail


def test_model_flags_of_the_structural_fixtures():
    for name, c in _all_cases():
        total, flags = pc.model_packed(c.rp, c.va, c.lanes)
        assert flags == c.flags, (name, flags)
        assert total == sum(int(c.rp[min(c.m, (t + 1) * pc.TILE)] - c.rp[t * pc.TILE]) for t, f in enumerate(flags) if f), name
    # the long-row term alone: the same pattern with the row at the threshold packs everywhere
    lens = np.full(1280, 32)
    lens[300] = 512
    m, n, rp, ci, va = pc.open_band(lens)
    assert all(pc.model_packed(rp, va, 8)[1])
    # an all-zero tile and a tile without entries pack; a -0.0 does not
    c = pc.fixture("exotic")
    assert (c.va[c.rp[3 * pc.TILE]:c.rp[4 * pc.TILE]] == 0).all()
    e = pc.fixture("empty_tile")
    assert e.rp[512] == e.rp[768] and pc.model_packed(e.rp, e.va, 8)[0] == e.va.size
    va = c.va.copy()
    va[c.rp[3 * pc.TILE] + 9] = -0.0
    assert pc.model_packed(c.rp, va, 8)[1] == [True, True, True, False, True]


def test_hp_check_and_probe_model_on_the_host():
    """hp_check accepts a sequential double sum and refuses one entry's sign flipped; probe_readback's arithmetic on a host multiply"""
    c = pc.fixture("exotic")
    x = pc.x_of(c.n)

    def host_mul(v):
        y = np.zeros(c.m)
        np.add.at(y, np.repeat(np.arange(c.m), np.diff(c.rp)), c.va * v[c.ci])
        return y
    y = host_mul(x)
    pc.hp_check(y, c.rp, c.ci, c.va, x)
    wrong = y.copy()
    wrong[700] = -wrong[700] if wrong[700] else 1.0
    with pytest.raises(AssertionError):
        pc.hp_check(wrong, c.rp, c.ci, c.va, x)
    pc.probe_readback(None, c.m, c.n, c.rp, c.ci, c.va, c.stride, mul=host_mul)
    swapped = c.va.copy()
    swapped[[40, 41]] = swapped[[41, 40]]
    with pytest.raises(AssertionError):
        pc.probe_readback(None, c.m, c.n, c.rp, c.ci, swapped, c.stride, mul=host_mul)
