"""GPU: PACKED tiles of the fp64 CSR-vector tile kernel (option pack_values; kernels/csr_vector_tile.hpp).

Every case is a 1000 .. 2304-row banded matrix (row i holds len_i consecutive columns around the diagonal, wrapping at the edges) with
full-precision x.  Unless stated otherwise a case multiplies through a pack_values = 1 handle and through a pack_values = 0 handle and compares y
BIT FOR BIT, and it compares spmv_hip_info.packed_nnz with a host model of the gate (`model_packed`, tests/packed_cases.py): a 256-row tile packs iff every row of it
starts at a multiple of C = 4L and is a whole number of C-blocks long, every value is finite and not -0.0, and the non-zero values' bit
positions span at most 55 (largest leading-bit position - smallest lowest-set-bit position <= 54).  L is read from the handle's info.

Two notes on the expected counts:
  * the gate does not look at columns, so a tile with wrap-around rows (not a RUN tile; it reads its 16-bit slot stream) packs like any other:
    with uniform values and aligned rows packed_nnz is every entry of the matrix;
  * 512 rows of 32, 256 rows of 24, 512 rows of 32: 256 * 24 = 6144 = 192 * 32, so the last block starts ON a multiple of 32 (and of 64 and 128)
    and its tiles do pack; only the tile of 24-entry rows does not (24 % C != 0).  `test_rows_off_the_block_boundary` therefore also runs the
    variant the case is after -- one row of the middle block 36 long, the block 6156 = 192 * 32 + 12 entries -- where every row of the last block
    starts off a C boundary and none of its tiles packs.
"""
import numpy as np
import pytest

from spmv_amd import api
from packed_cases import METHOD, TILE, Pair, banded, x_of

pytestmark = pytest.mark.gpu


def run_case(lens, edit=None, lanes=0, seed=1):
    m, rp, ci, va = banded(lens, seed)
    if edit is not None:
        edit(rp, va)
    p = Pair(m, rp, ci, va, lanes)
    try:
        want, flags = p.check(va, x_of(m))
        return p.L, want, flags, int(rp[-1])
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("m", [1024, 1000])
def test_uniform_values_k32(m):
    """L = 8; m = 1000: the last tile is partial and the rows past m are in play.  Every tile packs, the two with wrap-around rows included."""
    L, want, flags, nnz = run_case(np.full(m, 32))
    assert L == 8 and all(flags) and want == nnz == 32 * m


@pytest.mark.parametrize("k,lanes", [(4, 0), (16, 0), (64, 0), (128, 0), (64, 8), (128, 8), (128, 2)])
def test_other_lane_counts_and_rows_of_several_chunks(k, lanes):
    """The permutation at other L; with lanes_per_row forced below k / 4 a row is several chunks (the continuation loop)."""
    m = 1280 if k <= 16 else 1024
    L, want, flags, nnz = run_case(np.full(m, k), lanes=lanes)
    assert L >= 1 and k % (4 * L) == 0, (k, L)       # the planner's L (or the forced one) divides these row lengths into whole chunks
    if lanes:
        assert L == lanes and k > 4 * L              # several chunks per row
    assert all(flags) and want == nnz


SPOILERS = {
    "nan": lambda v, p: v.__setitem__(p, np.nan),
    "inf": lambda v, p: v.__setitem__(p, np.inf),
    "negative_zero": lambda v, p: v.__setitem__(p, -0.0),
    "sixty_binades_below": lambda v, p: v.__setitem__(p, 2.0 ** -62),     # the tile's largest values are in [0.5, 1)
    "third_beside_2_40": lambda v, p: (v.__setitem__(p, 1.0 / 3.0), v.__setitem__(p + 1, 2.0 ** 40)),
}


@pytest.mark.parametrize("what", sorted(SPOILERS))
def test_one_tile_spoiled_by_one_entry(what):
    m, k, bad_tile = 1280, 32, 2
    m, rp, ci, va = banded(np.full(m, k))
    SPOILERS[what](va, int(rp[bad_tile * TILE + 100]) + 5)
    p = Pair(m, rp, ci, va)
    try:
        want, flags = p.check(va, x_of(m))
        assert flags == [t != bad_tile for t in range(5)] and want == (m - TILE) * k
        if what == "negative_zero":      # x = 0: the signs of the zeros in y are the 8-byte path's
            y = p.same_bits(np.zeros(m))
            assert (y == 0).all()
    finally:
        p.close()


def test_per_tile_exponent():
    """Tiles scaled by 2^300, 2^-300 and into the subnormals (2^-1040: the products round onto the subnormal grid), another scale per tile: all pack."""
    m, k = 1280, 32
    scales = [1.0, 2.0 ** 300, 2.0 ** -300, 2.0 ** -1040, 2.0 ** -1000]

    def edit(rp, va):
        for t, s in enumerate(scales):
            va[rp[t * TILE]:rp[(t + 1) * TILE]] *= s
        sub = va[rp[3 * TILE]:rp[4 * TILE]]
        assert (np.abs(sub[sub != 0]) < 2.0 ** -1022).all() and (sub != 0).any()
    L, want, flags, nnz = run_case(np.full(m, k), edit=edit)
    assert all(flags) and want == nnz


def test_rows_of_31_pack_nothing():
    L, want, flags, nnz = run_case(np.full(1024, 31))
    assert want == 0 and not any(flags)


def test_rows_off_the_block_boundary():
    # 512 x 32, 256 x 24, 512 x 32: only the tile of 24-entry rows fails (module docstring)
    lens = np.concatenate([np.full(512, 32), np.full(256, 24), np.full(512, 32)])
    L, want, flags, nnz = run_case(lens)
    assert 24 % (4 * L) != 0
    assert flags[:3] == [True, True, False] and want == sum(int(lens[t * TILE:(t + 1) * TILE].sum()) for t in range(5) if flags[t])
    if 4 * L in (32, 64, 128):
        assert flags[3:] == [True, True]
    # one row of the middle block 36 long: the last block starts 12 entries off a multiple of 32 and none of its tiles packs
    lens[700] = 36
    L, want, flags, nnz = run_case(lens)
    assert (4 * L) % 8 == 0, L
    assert flags == [True, True, False, False, False] and want == 512 * 32


def test_update_values():
    m, k = 1280, 32
    m, rp, ci, va = banded(np.full(m, k))
    x = x_of(m)
    p = Pair(m, rp, ci, va)
    try:
        p.check(va, x)
        other = np.random.default_rng(5).uniform(-1.0, 1.0, size=va.size)
        misfit = other.copy()
        misfit[rp[3 * TILE + 17] + 3] = 2.0 ** -70               # tile 3 no longer fits one exponent
        for new, packs in ((other, [True] * 5), (misfit, [True, True, True, False, True]), (other, [True] * 5), (va, [True] * 5)):
            for h in p.h.values():
                h.update_values(new.copy())
            want, flags = p.check(new, x)
            assert flags == packs and want == sum(packs) * TILE * k
    finally:
        p.close()


def test_default_allocates_nothing_at_small_sizes():
    m, rp, ci, va = banded(np.full(2304, 32))
    info = {}
    for pack in (2, 0):
        api.set_thread_option("pack_values", pack)
        try:
            with api.Handle(m, m, rp, ci, va, METHOD) as h:
                info[pack] = h.info()
        finally:
            api.clear_thread_options()
    assert info[2]["packed_nnz"] == 0 and info[2]["pack_ms"] == [0.0, 0.0]
    assert info[2]["device_bytes"] == info[0]["device_bytes"]
