"""GPU: PACKED tiles in every compiled kernel form, every tile mode, at |k| up to 2^55 - 8, and through the handle's state changes.

tests/test_gpu_packed_values.py runs the default form (four steps in flight, step 0 issued before the barrier) on RUN tiles with values in [-1, 1)
and compares with the 8-byte path alone.  Here every case builds the matrix under pack_values = 1 and 0 (`Pair`), asserts the tile kernel and
packed_nnz == the host model of the gate, and then checks the packed handle three ways (`three_checks`):
  * y bit-equal to the pack_values = 0 handle on full-precision x;
  * `probe_readback`: `stride` multiplies by 0 / 1 vectors read every stored entry back from the packed planes and compare it with the host's
    value array bit for bit -- exact whatever the order of the additions, and independent of the other GPU path;
  * `hp_check`: y against np.longdouble sums within the textbook bound 2 len 2^-53 sum |a x|.
Matrices, values, model and references are in tests/packed_cases.py; tests/test_packed_model_host.py checks them on the CPU.

Sizes: 1056 .. 1280 rows -- four whole 256-row tiles and a partial one (a whole number of tiles only where the wrap-around band of 256-entry rows
needs m % 256 == 0).  Every tile mode is reached at these sizes; the info counts each case asserts say so.  The one large case is the timed
default (pack_values = 2), which starts at nnz = 2^24.
"""
import functools

import numpy as np
import pytest

import packed_cases as pc
from packed_cases import TILE, TILE_KERNEL, Pair, hp_check, model_packed, probe_readback, x_of
from spmv_amd import api

pytestmark = pytest.mark.gpu

FORMS = [10, 11, 5, 12]            # four / two steps in flight, with / without step 0 issued before the barrier: the four packed kernels


@functools.lru_cache(maxsize=None)
def case(name):
    """a fixture of packed_cases, or ("form", L, chunks); built once and never written to (Pair copies the values)"""
    c = pc.form_case(*name[1:]) if isinstance(name, tuple) else pc.fixture(name)
    for a in (c.rp, c.ci, c.va):
        a.setflags(write=False)
    return c


def pair_of(c, options=None, kernel=TILE_KERNEL, va=None):
    return Pair(c.m, c.rp, c.ci, c.va if va is None else va, c.lanes, options, n=c.n, kernel=kernel)


def spmv(h, m, x):
    return h.spmv(x, np.full(m, np.nan))


def three_checks(p, c, va=None, flags=None):
    """-> the packed handle's info"""
    va = c.va if va is None else va
    x = x_of(c.n)
    assert p.L == c.lanes
    want, got = p.check(va, x)                                   # bit equality, packed_nnz == model
    assert got == (c.flags if flags is None else flags), got
    probe_readback(p, c.m, c.n, c.rp, c.ci, va, c.stride)
    hp_check(spmv(p.h[1], c.m, x), c.rp, c.ci, va, x)
    return p.h[1].info()


def counts(info):
    return {k: info[k] for k in ("nnz", "packed_nnz", "run_nnz", "byte_nnz", "tmpl_nnz", "x_groups", "x_groups_staged")}


# ------------------------------------------------------------------------------------------------ kernel forms
@pytest.mark.parametrize("L,chunks", pc.FORM_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("form", FORMS)
def test_every_packed_kernel_form(form, L, chunks):
    """vector_form 10 / 11 / 5 / 12 x every lanes_per_row, rows of one aligned chunk; L = 2 and 8 also with three chunks (the continuation loop)"""
    c = case(("form", L, chunks))
    with pair_of(c, {"vector_form": form}) as p:
        info = three_checks(p, c)
        assert info["packed_nnz"] == info["nnz"] == c.va.size
        print(f"form {form} L {L} chunks {chunks}: {counts(info)}")


@pytest.mark.parametrize("form,kernel", [(6, TILE_KERNEL), (4, "csr_vector_pipe_kernel")])
def test_forms_without_a_packed_kernel_keep_the_8_byte_stream(form, kernel):
    """eight steps in flight and the pipe kernel: no planes are built, packed_nnz = 0, same bits and memory as pack_values = 0"""
    c = case(("form", 8, 1))
    with pair_of(c, {"vector_form": form}, kernel=kernel) as p:
        x = x_of(c.n)
        y = p.same_bits(x)
        i1, i0 = p.h[1].info(), p.h[0].info()
        assert i1["packed_nnz"] == 0 and i1["device_bytes"] == i0["device_bytes"] and i1["stream_bytes"] == i0["stream_bytes"]
        hp_check(y, c.rp, c.ci, c.va, x)


# ------------------------------------------------------------------------------------------------ tile modes
def _is_run(i):
    return i["run_nnz"] == i["nnz"] and i["x_groups_staged"] == i["x_groups"]


def _is_slots16(i):
    return i["run_nnz"] == i["byte_nnz"] == i["tmpl_nnz"] == 0 and i["x_groups_staged"] == i["x_groups"] > 0


def _is_global(i):
    return i["x_groups_staged"] == 0 and i["run_nnz"] == i["byte_nnz"] == i["tmpl_nnz"] == 0


def _is_byte(i):
    return i["byte_nnz"] >= 0.9 * i["nnz"] and i["tmpl_nnz"] == 0


def _is_tmpl(i):
    return i["tmpl_nnz"] >= 0.9 * i["nnz"] and i["byte_nnz"] == 0


# mode: (fixture, options, the info fields that prove the mode was reached, forms)
MODES = {
    "run": ("run", {}, _is_run, (0, 12)),                                   # MODE 2
    "slots16": ("run3", {"run_tiles": 0}, _is_slots16, (0, 12)),            # MODE 1 over the whole matrix, three chunks per row
    "global": ("scatter3", {}, _is_global, (10, 12)),                       # MODE 0 (unstaged), three chunks per row: see below
    "byte32": ("byte32", {}, _is_byte, (0, 12)),                            # MODE 3
    "byte64": ("byte64", {}, _is_byte, (0, 12)),                            # MODE 3, two chunks per row
    "tmpl32": ("tmpl32", {}, _is_tmpl, (0, 12)),                            # MODE 4
    "tmpl64": ("tmpl64", {}, _is_tmpl, (0, 12)),                            # MODE 4, two chunks per row, the longest list
}


@pytest.mark.parametrize("mode,second", [(m, s) for m in MODES for s in (0, 1)])
def test_every_tile_mode_reads_packed_values(mode, second):
    """The unstaged mode is reached through the matrix, not through option x_windows: CSR-vector's tile inspector does not read that option (it
    switches the SELL and CSR5 windows), so x_windows = 0 leaves a band's tiles staged.  Rows of 96 bands 1024 columns apart need more windows
    than a tile may hold: no tile stages (x_groups_staged == 0) and the tile kernel runs only because vector_form forces it, hence forms 10 and
    12 there instead of the default and 12."""
    name, options, reached, forms = MODES[mode]
    c = case(name)
    with pair_of(c, dict(options, vector_form=forms[second])) as p:
        info = three_checks(p, c)
        assert reached(info), counts(info)
        assert info["packed_nnz"] == info["nnz"]
        print(f"mode {mode} form {forms[second]}: {counts(info)}")


# ------------------------------------------------------------------------------------------------ values at the edges of the fields
@pytest.mark.parametrize("form", [0, 12])
def test_edge_values_pack_in_every_tile(form):
    """|k| up to 2^55 - 8, hi = 0x7fffff / -2^23 / -1, lo = 0 / 0xffffffff, at every position of a lane quad; and the signs of zeros: x = 0, x = -1"""
    c = case("edges")
    with pair_of(c, {"vector_form": form}) as p:
        info = three_checks(p, c)
        assert info["packed_nnz"] == info["nnz"]
        y = p.same_bits(np.zeros(c.n))
        assert (y == 0).all()
        p.same_bits(np.full(c.n, -1.0))


def test_one_more_binade_keeps_the_tile_unpacked():
    """the twin: one 2^15 in tile 2 makes its span 55 -- exactly that tile keeps its 8-byte stream"""
    c = case("edges_twin")
    with pair_of(c) as p:
        info = three_checks(p, c)
        assert info["packed_nnz"] == info["nnz"] - TILE * 32


def test_dbl_max_subnormal_and_all_zero_tiles():
    """tile 1: DBL_MAX and odd multiples of 2^971 (e = 971); tile 2: the subnormal grid from 5e-324 to 2^-1020 (e = -1074, span 54); tile 3: zeros"""
    c = case("exotic")
    with pair_of(c) as p:
        info = three_checks(p, c)
        assert info["packed_nnz"] == info["nnz"]
        y = spmv(p.h[1], c.m, x_of(c.n))
        assert (y[3 * TILE:4 * TILE] == 0).all() and not np.signbit(y[3 * TILE:4 * TILE]).any()


# ------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("name", ["empty_rows", "empty_tile"])
def test_empty_rows_and_an_empty_tile(name):
    c = case(name)
    with pair_of(c) as p:
        info = three_checks(p, c)
        assert info["packed_nnz"] == info["nnz"] and info["empty_rows"] == int((np.diff(c.rp) == 0).sum()) > 0
        y = spmv(p.h[1], c.m, x_of(c.n))
        assert (y[np.diff(c.rp) == 0] == 0).all()


def test_a_long_row_keeps_its_tile_unpacked():
    """544 entries > long_thr = 512: tile 1 alone does not pack, the row's sum comes from the long-row path; the same through update_values"""
    c = case("long_row")
    with pair_of(c) as p:
        info = three_checks(p, c)
        assert info["max_row_len"] == 544 and len(info["launch_kernels"]) > 1, info["launch_kernels"]     # the long-row path is in the launch
        assert info["packed_nnz"] == info["nnz"] - (255 * 32 + 544)
        other = np.random.default_rng(5).uniform(-1.0, 1.0, size=c.va.size)
        p.update(other)
        three_checks(p, c, va=other)
        edges = pc.edge_values(c.va.size, c.rp)
        p.update(edges)
        three_checks(p, c, va=edges)


# ------------------------------------------------------------------------------------------------ state
def test_transposed_schedule_packs_and_repacks():
    """A^T of the constant-length band has the same aligned rows: the child handle packs at its build and again after the parent's update_values"""
    c = case(("form", 8, 1))
    nnz = c.va.size
    x = x_of(c.m, seed=9)
    with pair_of(c) as p:
        def mul_t(h):
            return lambda v: h.spmv_transpose(v, np.full(c.n, np.nan))

        def check(va, drop=0):
            tm, tn, trp, tci, tva = pc.transpose_csr(c.m, c.n, c.rp, c.ci, va)
            y1, y0 = mul_t(p.h[1])(x), mul_t(p.h[0])(x)
            assert y1.tobytes() == y0.tobytes()
            ti = api.get_transpose_info(p.h[1].h)
            want, flags = model_packed(trp, tva, ti["lanes_per_row"])
            assert ti["kernel_name"] == TILE_KERNEL and ti["packed_nnz"] == want == nnz - drop, (ti["packed_nnz"], want, flags)
            assert api.get_transpose_info(p.h[0].h)["packed_nnz"] == 0
            probe_readback(p, tm, tn, trp, tci, tva, c.stride, mul=mul_t(p.h[1]))
            hp_check(y1, trp, tci, tva, x)
        check(c.va)
        edges = pc.edge_values(nnz, c.rp)
        p.update(edges)
        check(edges)
        wide = edges.copy()
        wide[c.rp[300] + 16] = 2.0 ** 15          # row 300, column 300: row 300 of A^T, its tile 1 -- span 55 there
        assert c.ci[c.rp[300] + 16] == 300
        p.update(wide)
        check(wide, drop=TILE * 32)
        p.same_bits(x_of(c.n))                    # and the parent itself


@pytest.mark.parametrize("name,form", [("edges", 0), ("scatter3", 10)])
def test_update_values_sequence_and_accounting(name, form):
    """packable -> every tile spoiled -> packable: packed_nnz follows, y stays bit-equal, stream_bytes equals a freshly created handle's at
    every step, and the planes cost 7 B per entry (+ an exponent per tile and the streams' padding).  Staged tiles at the default form, and
    unstaged tiles under a forced tile form (the traffic model's other branch)."""
    c = case(name)
    nnz, tiles = c.va.size, len(c.flags)
    x = x_of(c.n)
    spoiled = np.random.default_rng(5).uniform(-1.0, 1.0, size=nnz)
    for t in range(tiles):
        spoiled[c.rp[t * TILE + 17] + 3] = 2.0 ** -70               # no tile fits one exponent
    uniform = np.random.default_rng(6).uniform(-1.0, 1.0, size=nnz)
    with pair_of(c, {"vector_form": form}) as p:
        extra = p.h[1].info()["device_bytes"] - p.h[0].info()["device_bytes"]
        assert 7 * nnz <= extra < 8 * nnz, (extra, nnz)
        steps = [(None, nnz), (spoiled, 0), (uniform, nnz), (spoiled, 0), (np.asarray(c.va), nnz)]
        for step, (va, packed) in enumerate(steps):
            if va is not None:
                p.update(va)
            va = c.va if va is None else va
            want, flags = p.check(va, x)
            assert want == packed
            for pack in (1, 0):
                with p.create(va, pack) as fresh:
                    fi, hi = fresh.info(), p.h[pack].info()
                    assert fi["packed_nnz"] == hi["packed_nnz"] and fi["stream_bytes"] == hi["stream_bytes"], (step, pack, packed, fi["stream_bytes"], hi["stream_bytes"])
            assert p.h[0].info()["stream_bytes"] - p.h[1].info()["stream_bytes"] == (packed - 4 * tiles if packed else 0)
        assert p.h[1].info()["device_bytes"] - p.h[0].info()["device_bytes"] == extra
        probe_readback(p, c.m, c.n, c.rp, c.ci, c.va, c.stride)


# ------------------------------------------------------------------------------------------------ the timed default
def test_timed_default_at_the_smallest_size_that_times():
    """pack_values = 2 (default options) at nnz = 2^24, autotune_vector's threshold: 2^19 banded rows of 32.  Which side wins is the machine's
    business; what is asserted is that the decision follows the measured times, that a loser leaves nothing behind, and that y is the 8-byte
    path's whichever side was kept."""
    m, rp, ci, va = pc.banded(np.full(1 << 19, 32))
    nnz = va.size
    assert nnz == 1 << 24
    x = x_of(m)
    api.set_thread_option("pack_values", 0)
    try:
        h0 = api.Handle(m, m, rp, ci, va.copy(), pc.METHOD)
    finally:
        api.clear_thread_options()
    with h0, api.Handle(m, m, rp, ci, va.copy(), pc.METHOD) as h2:
        i2, i0 = h2.info(), h0.info()
        print(f"timed default: kernel {i2['kernel_name']} pack_ms {i2['pack_ms']} packed_nnz {i2['packed_nnz']} tuned_choice {i2['tuned_choice']}")
        assert i0["packed_nnz"] == 0 and i0["pack_ms"] == [0.0, 0.0]
        if i2["kernel_name"] == TILE_KERNEL:
            plain, packed = np.float32(i2["pack_ms"][0]), np.float32(i2["pack_ms"][1])
            assert plain > 0 and packed > 0
            if packed < np.float32(0.95) * plain:
                assert i2["packed_nnz"] == nnz
            else:
                assert i2["packed_nnz"] == 0 and i2["device_bytes"] == i0["device_bytes"]
        y2, y0 = spmv(h2, m, x), spmv(h0, m, x)
        assert y2.tobytes() == y0.tobytes()
        hp_check(y2, rp, ci, va, x)
        misfit = va.copy()
        misfit[rp[3 * TILE + 17] + 3] = 2.0 ** -70
        h2.update_values(misfit.copy())
        h0.update_values(misfit.copy())
        assert spmv(h2, m, x).tobytes() == spmv(h0, m, x).tobytes()
        if i2["packed_nnz"]:
            assert h2.info()["packed_nnz"] == nnz - TILE * 32
