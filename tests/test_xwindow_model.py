"""CPU: the matrices of tests/test_gpu_lds_edges.py hit the x windows they are aimed at.

synth.span_rows promises that every tile of a matrix, however a schedule cuts it, references the same known column set.  Here a numpy
restatement of build_windows (kernels/xwindows.hpp: the plain span -> one window, else runs of touched 64-column segments, at most 16
runs, 64 x segments <= max_cols, at most 1024 bitmap words, ends clipped at n) is run over the tiles of every case and compared with
what the case's description intends -- for every budget, so that the GPU sweep's expectations (which form stages, with which total)
are checked before any GPU time is spent on them."""
import numpy as np
import pytest

import lds_edges as E
from spmv_amd import synth

CASES = E.all_cases()
_CSR = {}


def _matrix(case):
    if case.name not in _CSR:
        _CSR.clear()                                                          # one matrix at a time: the cases come grouped by name
        _CSR[case.name] = E.matrix(case)
    return _CSR[case.name]


def _row_tiles(csr, rows):
    rp = csr.rowptr.astype(np.int64)
    for r0 in range(0, csr.m, rows):
        yield csr.colidx[rp[r0]:rp[min(r0 + rows, csr.m)]]


def _entry_tiles(csr, entries):
    for b in range(0, csr.nnz, entries):
        yield csr.colidx[b:b + entries]


def test_case_names_are_unique():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)


def test_model_on_hand_made_tiles():
    """The restated rule itself, on tiles small enough to check by eye."""
    mw = E.model_windows
    assert mw([], 100, 10) == (0, 0) and mw([-1, -1], 100, 10) == (0, 0)                     # padding only
    assert mw([7, -1, 16], 100, 10) == (1, 10) and mw([7, 17], 100, 10) == (0, 0)            # span 10 fits, span 11: one run of one segment = 64 > 10
    assert mw([0, 200], 1000, 128) == (2, 128) and mw([0, 200], 1000, 127) == (0, 0)         # two runs of one segment each
    assert mw([0, 64, 200], 1000, 192) == (2, 192)                                           # adjoining segments are one run
    assert mw([0, 990], 1000, 128) == (2, 64 + 40)                                           # the last run is clipped at n
    cols = [i * 128 for i in range(17)]
    assert mw(cols[:16], 10 ** 6, 1100) == (16, 1024) and mw(cols, 10 ** 6, 1100) == (0, 0)  # 16 runs, 17 runs
    assert mw([0, 32767 * 64], 1 << 22, 200) == (2, 128) and mw([0, 32768 * 64], 1 << 22, 200) == (0, 0)  # 1024 / 1025 bitmap words
    assert mw([63, 32768 * 64], 1 << 22, 200) == (0, 0) and mw([64, 32768 * 64], 1 << 22, 200) == (2, 128)  # counted from the first segment


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_tile_has_the_intended_windows(case):
    csr = _matrix(case)
    lens = np.diff(csr.rowptr)
    assert csr.m >= 2 * E.SIGMA and csr.nnz <= 400_000 and csr.nnz < (1 << 21), (csr.m, csr.nnz)   # small; under the blocked executor's size
    assert lens.max() >= 8 and csr.nnz / csr.m >= 8 or case.empty_every, "rows under 8 entries are handed to the nnz-split executor"
    for budget in E.BUDGETS:
        max_cols = E.cap(budget, case.dt)
        want = E.intended_windows(case, max_cols)
        for rows in (256, 1024):                                              # CSR-vector's tiles and blocks, Balanced's row blocks, a sigma window
            got = {E.model_windows(t, case.n, max_cols) for t in _row_tiles(csr, rows)}
            assert got == {want}, (case.name, budget, rows, got, want)
        groups = list(_entry_tiles(csr, 4096))                                # CSR5's smallest group: 16 tiles of 256 entries, cut anywhere in a row
        got = {E.model_windows(t, case.n, max_cols) for t in groups[:-1]}
        assert got == {want}, (case.name, budget, "entry ranges", got, want)
        tail = E.model_windows(groups[-1], case.n, max_cols)                  # a short last group may see less, never more
        assert tail[1] <= want[1] or want == (0, 0), (case.name, budget, tail, want)


@pytest.mark.parametrize("case", [c for c in CASES if c.name.endswith("-over")], ids=lambda c: c.name)
def test_over_budget_spans_touch_too_many_segments(case):
    """Variant b: one column past a budget, and the rows of every 256-row tile together touch more 64-column segments than the budget
    holds -- the several-window path cannot rescue the tile."""
    csr = _matrix(case)
    budget = int(case.name.split("-")[1][:-1]) * E.KIB
    max_cols = E.cap(budget, case.dt)
    assert case.bands[0][1] == max_cols + 1
    for t in _row_tiles(csr, 256):
        assert np.unique(t >> 6).size * E.SEG > max_cols
        assert E.model_windows(t, case.n, max_cols) == (0, 0)


@pytest.mark.parametrize("case", [c for c in CASES if "bands" in c.name or "seg" in c.name or "clipped" in c.name], ids=lambda c: c.name)
def test_band_cases_have_their_run_count(case):
    csr = _matrix(case)
    nwin, total = E.model_windows(csr.colidx[:256 * case.k], case.n, E.cap(E.CSR5, case.dt))
    if case.name.endswith("17bands") or case.name.endswith("32769seg"):
        assert (nwin, total) == (0, 0)
    else:
        assert nwin == len(case.bands) and total == sum(min(((a + w - 1) // 64 + 1) * 64, case.n) - a // 64 * 64 for a, w in case.bands)
    if case.name.endswith("clipped"):
        assert case.n % 64 and total % 64 == case.n % 64


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_dyadic_bit_budget_holds(case):
    """Operands as wide as the plan allows, rows (and for the transpose check: columns) as long as the cases have them: every value keeps
    at least one bit and every row sum stays below 2^p, so exact_ref's integers are the expected bits."""
    csr = _matrix(case)
    lens = np.diff(csr.rowptr.astype(np.int64))
    for which, max_len in (("rows", int(lens.max())), ("columns", max(int(lens.max()), int(np.bincount(csr.colidx).max())))):
        for kind in (0, 1):
            plan = synth.dyadic_plan(max_len, E.DTYPES[case.dt], kind, 7)
            bits = synth.dyadic_row_bits(np.array([max_len]), plan)
            assert plan.xbits >= 1 and int(bits.min()) >= 1, (which, plan)
            assert plan.xbits + int(bits.max()) + int(max_len).bit_length() <= plan.p, (which, plan)


def test_line_cases_aim_at_every_kib():
    """The 64 KiB sweep: the windows' request (+ one sigma window's row sums for SELL) is the target, a whole number of KiB."""
    seen = {}
    for case, family, target in E.line_cases():
        S = case.bands[0][1]
        want = E.xbytes(S, case.dt) + (E.size_of(case.dt) * E.SIGMA if family == "sell" else 0)
        assert want == target and (S + 1) * E.size_of(case.dt) % E.KIB == 0, (case.name, want, target)
        assert family == "sell" or S > E.cap(E.NARROW, case.dt), "the wide rows form runs only where the narrow one does not stage"
        seen.setdefault((case.dt, family), set()).add(target // E.KIB)
    assert all(v == set(range(56, 69)) for v in seen.values()) and len(seen) == 4, seen
    # SELL's groups stay at one sigma window while the windows cost at most 15 % of the window's stream (build_sell)
    for case, family, _ in E.line_cases():
        if family == "sell":
            s = E.size_of(case.dt)
            assert case.bands[0][1] * s <= 0.15 * E.SIGMA * case.k * (s + 2), case.name
