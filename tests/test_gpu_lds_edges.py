"""GPU: every staged x-window kernel at its LDS capacity boundaries, compared bit for bit with an exact integer evaluation.

The launchers size their dynamic LDS request at run time from the widest staged window of the matrix.  synth.span_rows builds matrices
whose every tile references a known column set (tests/test_xwindow_model.py checks that on the CPU), so the request can be put where the
arithmetic is at its limit: on a budget (max_cols - 1, max_cols, max_cols + 1), on every KiB around the 64 KiB default of dynamic LDS
(the attribute has to be raised above it, and the kernels' static LDS comes on top), on the largest request a kernel can make, and on
the limits of the several-window path (16 windows, the budget in whole segments, the clip at n, 32768 bitmap segments).
spmv_hip_info.x_span_max / lds_bytes prove that a case reached the byte it aimed at.

Operands are synth's signed full-precision dyadic draws, the reference is tests/exact_ref.py: finite and infinite rows bit for bit, NaN
rows by isnan.  No tolerance anywhere.  A rejected launch comes back through spmv_hip_last_error and fails the case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_ref
import lds_edges as E
from spmv_amd import api, build, synth
from test_gpu_exact_operands import _check, _check_device, _options

pytestmark = pytest.mark.gpu
M = api.SPMV_METHODS
DEV = "cuda:0"
KIB = E.KIB
STAGED_KERNELS = ("csr_vector_rows_kernel", "sell_window_kernel", "csr5_group_kernel", "csr5_group_pipe_kernel", "nat_group_kernel")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    api.load()


def _no_error(where):
    code, text = api.last_error()
    assert code == 0, (where, code, text)


def _operands(case, seed, transpose=False):
    """-> (csr with dyadic values, x, plan); the wide operand alternates with the seed."""
    csr = E.matrix(case)
    lens = np.diff(csr.rowptr.astype(np.int64))
    max_len = int(lens.max())
    if transpose:
        max_len = max(max_len, int(np.bincount(csr.colidx, minlength=csr.n).max()))
    plan = synth.dyadic_plan(max_len, E.DTYPES[case.dt], seed, seed)
    csr.val = synth.dyadic_values(csr.rowptr, plan, seed + 1, **(dict(colidx=csr.colidx, n=csr.n) if transpose else {}))
    return csr, synth.dyadic_x(csr.m if transpose else csr.n, plan, seed + 2), plan


def _to_dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _assert_form(info, want, case, method):
    """The schedule create() settled on is the one the case aims at, with the windows it aims at."""
    what = (case.name, method.name, want, {k: info[k] for k in ("kernel_name", "x_groups", "x_groups_staged", "x_span_max", "lds_bytes", "cache_blocked")})
    assert info["cache_blocked"] == 0 and info["far_nnz"] == 0, what
    assert info["kernel_name"] == want["kernel"], what
    assert info["x_span_max"] == want["span"], what
    if want["staged"]:
        assert info["x_groups"] > 0 and info["x_groups_staged"] == info["x_groups"], what
        extra = info["lds_bytes"] - want["xbytes"]                             # SELL: the row sums of 1, 2, 4 or 8 sigma windows
        s = E.size_of(case.dt)
        maps = [4 * stride * 4 for stride in (64, 5 * 64, 9 * 64, 17 * 64)] if case.empty_every else [0]   # CSR5 / nnz-split with empty rows: the waves' row maps
        assert extra in ([s * E.SIGMA * g for g in (1, 2, 4, 8)] if method == M.Method_SellCSigma else maps), what
    else:
        assert info["x_groups_staged"] == 0, what


def _run_case(case, seed, methods=E.METHODS, edge=False, reached=None):
    """Every method on the case: the form, exact y, no error on the channel.  edge: also the window's neighbours in x set to NaN, a values
    refresh, and x / y handed over 0..3 elements past an aligned address."""
    csr, x, plan = _operands(case, seed)
    want = exact_ref.spmv_csr(csr, x, plan)
    rp, ci, va, xd = _to_dev(csr.rowptr, csr.colidx, csr.val, x)
    for method in methods:
        exp = E.expected(method, case, csr.nnz)
        api.load().spmv_hip_clear_error()
        with api.Handle(csr.m, csr.n, rp, ci, va, method) as h:
            _no_error((case.name, method.name, "create"))
            info = h.info()
            _assert_form(info, exp, case, method)
            if reached is not None and exp["staged"]:
                reached.setdefault(info["kernel_name"], set()).add(info["lds_bytes"])
            y = torch.full((csr.m,), float("nan"), dtype=va.dtype, device=DEV)
            h.spmv(xd, y)
            _no_error((case.name, method.name, "spmv"))
            torch.cuda.synchronize()
            _check(y.cpu().numpy(), want, case.name, method.name, info["kernel_name"], info["lds_bytes"], plan)
            if not edge:
                continue
            lo, hi = case.bands[0][0], case.bands[-1][0] + case.bands[-1][1] - 1
            assert lo >= 1 and hi + 1 < csr.n
            xn = xd.clone()
            xn[lo - 1] = xn[hi + 1] = float("nan")                            # the staged window's neighbours: referenced by no row
            y.fill_(float("nan"))
            h.spmv(xn, y)
            torch.cuda.synchronize()
            _check(y.cpu().numpy(), want, case.name, method.name, info["kernel_name"], "NaN beside the window")
            xbig = torch.zeros(csr.n + 8, dtype=va.dtype, device=DEV)
            ybig = torch.empty(csr.m + 8, dtype=va.dtype, device=DEV)
            wd = torch.from_numpy(want).to(DEV)
            for off in (0, 1, 2, 3):
                xs, ys = xbig[off: off + csr.n], ybig[off: off + csr.m]
                xs.copy_(xd)
                ys.fill_(float("nan"))
                h.spmv(xs, ys)
                _check_device(ys, wd, case.name, method.name, info["kernel_name"], "element offset", off)
            v2 = synth.dyadic_values(csr.rowptr, plan, seed + 3)               # freshly drawn values behind the same pattern
            want2 = exact_ref.spmv(csr.rowptr, csr.colidx, v2, x, plan.ev, plan.ex)
            h.update_values(torch.from_numpy(v2).to(DEV))
            y.fill_(float("nan"))
            h.spmv(xd, y)
            _no_error((case.name, method.name, "update_values + spmv"))
            torch.cuda.synchronize()
            _check(y.cpu().numpy(), want2, case.name, method.name, info["kernel_name"], "update_values")


# ----------------------------------------------------------------------------- a budget's last column, and one past it
EDGE = E.budget_edge_cases()


@pytest.mark.parametrize("case", EDGE, ids=[c.name for c in EDGE])
def test_budget_edge(case):
    """S = max_cols - 1 and max_cols: every form of that budget stages the span (x_span_max = S, the staged kernel runs); at max_cols:
    also NaN in x[off - 1] and x[off + S], x at element offsets 0..3, update_values.  S = max_cols + 1 with every segment touched: the
    form is turned down -- CSR-vector narrow -> wide -> unstaged, the others -> their global-column kernel -- and y is still exact."""
    _run_case(case, 3 + EDGE.index(case), edge=case.name.endswith("-at"))


def test_budget_edge_reaches_every_form():
    """What test_budget_edge relies on, from the expectations alone: at each budget's cap the forms of that budget are staged with
    x_span_max = max_cols, one past it they are not."""
    for dt in E.DTYPES:
        for method, budget, name in ((M.Method_Parallel, E.NARROW, "csr_vector_tile_kernel"), (M.Method_Parallel, E.WIDE, "csr_vector_rows_kernel"),
                                     (M.Method_Balanced, E.NARROW, "csr_vector_rows_kernel"), (M.Method_Balanced2, E.WIDE, "csr_vector_rows_kernel"),
                                     (M.Method_SellCSigma, E.SELL, "sell_window_kernel"), (M.Method_CSR5SPMV, E.CSR5, E._c5_kernel(dt)),
                                     (M.Method_Balanced_Yid, E.NAT, "nat_group_kernel")):
            by = {c.name: c for c in EDGE}
            at, over = by[f"{dt}-{budget // KIB}K-at"], by[f"{dt}-{budget // KIB}K-over"]
            e_at, e_over = E.expected(method, at, at.m * at.k), E.expected(method, over, over.m * over.k)
            assert (e_at["kernel"], e_at["budget"], e_at["span"]) == (name, budget, E.cap(budget, dt)), (dt, method, e_at)
            assert e_over["budget"] != budget or e_over["kernel"] != name, (dt, method, e_over)


# ----------------------------------------------------------------------------- every KiB around the 64 KiB default of dynamic LDS
LINE = E.line_cases()
_LINE_REACHED = {}


def _run_line(i):
    if i not in _LINE_REACHED:
        case, family, target = LINE[i]
        reached = {}
        methods = [M.Method_SellCSigma] if family == "sell" else [m for m in E.METHODS if m != M.Method_SellCSigma]
        _run_case(case, 40 + i, methods, reached=reached)
        assert reached and all(v == {target} for v in reached.values()), (case.name, target, reached)   # the KiB aimed at, on every staged kernel
        _LINE_REACHED[i] = reached
    return _LINE_REACHED[i]


@pytest.mark.parametrize("i", range(len(LINE)), ids=[c.name for c, _, _ in LINE])
def test_request_on_every_kib_around_64k(i):
    """lds_bytes = 56 .. 68 KiB for the wide rows form, SELL, CSR5 and the nnz-split groups: the rounding and zero-slot arithmetic of the
    request on either side of the line, create and spmv without an error, exact y.  By the time these run, earlier cases of this process
    have raised the kernels' LDS attribute to 96 KiB and more: what the DEFAULT attribute does with the band is
    test_band_under_the_default_attribute's to see."""
    _run_line(i)


BAND_KIB = range(59, 65)


def test_band_under_the_default_attribute():
    """59 .. 64 KiB of dynamic LDS + the kernels' 1-5 KiB of static LDS: above 64 KiB in all, while ensure_lds (told of no static bytes
    by these launchers) leaves hipFuncAttributeMaxDynamicSharedMemorySize alone.  In a fresh process (tests/lds_band_child.py), requests
    ascending, nothing larger launched before: no error on the channel, exact y, for the wide rows form, SELL, both CSR5 group kernels
    and the nnz-split groups in both value types."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lds_band_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    reached = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(reached) == set(STAGED_KERNELS), reached
    for k, v in reached.items():
        assert v == [t * KIB for t in BAND_KIB], (k, v)


def test_line_coverage():
    """The sweep must keep straddling the line when a budget is retuned: each kernel with a case in 59..64 KiB and one above 64 KiB."""
    reached = {}
    for i in range(len(LINE)):
        for k, v in _run_line(i).items():
            reached.setdefault(k, set()).update(v)
    assert set(reached) == set(STAGED_KERNELS), reached
    for k, v in reached.items():
        assert any(59 * KIB <= b <= 64 * KIB for b in v) and any(b > 64 * KIB for b in v), (k, sorted(v))


# ----------------------------------------------------------------------------- nnz-split groups either side of their buffer switch
@pytest.mark.parametrize("dt", list(E.DTYPES))
def test_nat_group_either_side_of_the_half_switch(dt):
    """launch_csr5_form hands the tiles over in halves (half-size static buffers) once windows + row maps + the full-size buffers exceed
    76 KiB.  At the automatic tile size of these matrices (64 x 4 entries: tile_nnz = 256) that is from 62 KiB of windows on in fp64 and
    from 66 KiB in fp32: the last request of the full form and the first of the half form, each exact, and both inside the KiB sweep."""
    first_half = E.nat_half_from_kib(dt)
    assert first_half - 1 in E.LINE_KIB and first_half in E.LINE_KIB, (dt, first_half, "the 56..68 KiB sweep no longer straddles the switch")
    assert first_half == {"f64": 62, "f32": 66}[dt]
    for t, half in ((first_half - 1, False), (first_half, True)):
        case = next(c for c, family, target in LINE if family == "x" and c.dt == dt and target == t * KIB)
        reached = {}
        _run_case(case, 70 + t, [M.Method_Balanced_Yid], reached=reached)
        assert reached == {"nat_group_kernel": {t * KIB}}, reached
        assert (t * KIB + E.nat_tile_buffers(dt) > E.NAT_SWITCH) == half
        csr = E.matrix(case)
        with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Balanced_Yid) as h:
            assert h.info()["tile_nnz"] == 64 * E.NAT_SIGMA, h.info()         # the tile size the switch point was computed for


# ----------------------------------------------------------------------------- the largest requests
UPPER = E.upper_end_cases()


@pytest.mark.parametrize("case", UPPER, ids=[c.name for c in UPPER])
def test_upper_end(case):
    s = E.size_of(case.dt)
    if "csr5-mapped" in case.name:
        # 128 KiB of windows + the four waves' row maps: at sigma = 16 a tile of 16-entry rows holds 64 row starts -> stride 17 x 64 ints
        with _options({"csr5_sigma": 16}):
            reached = {}
            _run_case(case, 81, [M.Method_CSR5SPMV], reached=reached)
        assert reached == {E._c5_kernel(case.dt): {128 * KIB + 4 * 17 * 64 * 4}}, reached
        _run_case(case, 82, [M.Method_CSR5SPMV, M.Method_Balanced_Yid])         # the automatic tile size; nnz-split: over its budget, global columns
    elif "nat-mapped" in case.name:
        # 96 KiB of windows + the waves' row maps (64 row starts per 256-entry tile: stride 5 x 64 ints), handed over in halves
        reached = {}
        _run_case(case, 85, [M.Method_Balanced_Yid], reached=reached)
        assert reached == {"nat_group_kernel": {E.NAT + 4 * 5 * 64 * 4}}, reached
        assert E.NAT // KIB >= E.nat_half_from_kib(case.dt, 4 * 5 * 64 * 4)
    else:
        # 8-entry rows: staging 96 KiB costs far more than 15 % of a window's stream, the groups grow while lds_fits allows --
        # fp64: 4 sigma windows (8 would need 96 + 64 KiB), fp32: 8.  Either way 96 + 32 KiB.
        reached = {}
        _run_case(case, 83, [M.Method_SellCSigma], reached=reached)
        assert reached == {"sell_window_kernel": {E.SELL + s * E.SIGMA * (4 if s == 8 else 8)}}, reached
        _run_case(case, 84, [m for m in E.METHODS if m != M.Method_SellCSigma])


# ----------------------------------------------------------------------------- the several-window path at its limits
MULTI = E.multi_window_cases()


@pytest.mark.parametrize("case", MULTI, ids=[c.name for c in MULTI])
def test_multi_window_limits(case):
    """15 / 16 / 17 bands (staged, staged, not); total = max_cols in whole segments and 64 more; a last band clipped at n (n not a
    multiple of 64); a tile span of 32768 segments (analysed) and 32769 (not).  Which form takes each is lds_edges.expected's chain."""
    if case.name.endswith("bands"):
        w = len(case.bands)
        for method in E.METHODS:
            exp = E.expected(method, case, case.m * case.k)
            assert exp["staged"] == (w <= 16) and exp["nwin"] == (w if w <= 16 else 0), (case.name, method, exp)
    _run_case(case, 100 + MULTI.index(case))


# ----------------------------------------------------------------------------- spmm and the transpose build their own schedules from the same budgets
@pytest.mark.parametrize("dt", list(E.DTYPES))
def test_spmm_and_transpose_at_a_cap(dt):
    case = next(c for c in EDGE if c.name == f"{dt}-96K-at")
    csr, _, plan = _operands(case, 9, transpose=True)
    X = np.ascontiguousarray(np.stack([synth.dyadic_x(csr.n, plan, 500 + c) for c in range(3)], axis=1))
    xt = synth.dyadic_x(csr.m, plan, 510)
    rt, ct, vt = exact_ref.transpose(csr.rowptr, csr.colidx, csr.val, csr.n)
    want_t = exact_ref.spmv(rt, ct, vt, xt, plan.ev, plan.ex)
    for method in (M.Method_Parallel, M.Method_SellCSigma, M.Method_CSR5SPMV):
        api.load().spmv_hip_clear_error()
        with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method) as h:
            info = h.info()
            assert info["x_span_max"] == E.cap(E.WIDE, dt), (method.name, info)
            Y = h.spmm(X, np.full((csr.m, 3), np.nan, dtype=E.DTYPES[dt]))
            _no_error((method.name, "spmm"))
            for c in range(3):
                _check(np.ascontiguousarray(Y[:, c]), exact_ref.spmv(csr.rowptr, csr.colidx, csr.val, X[:, c], plan.ev, plan.ex), method.name, "spmm", c, plan)
            y = h.spmv_transpose(xt, np.full(csr.n, np.nan, dtype=E.DTYPES[dt]))
            _no_error((method.name, "spmv_transpose"))
            _check(y, want_t, method.name, "transpose", plan)
            _assert_transpose_info(api.get_transpose_info(h.h), dt, csr.m)
    # the at-cap matrix's transpose (12 303 rows, one of them 2048 long) need not stage anything; a band's transpose is a band and must:
    # x_span_max and lds_bytes of the TRANSPOSED schedule are filled from it, by the same expressions
    band = synth.banded(4096, 4096, 20, 20, "eighths", E.DTYPES[dt], seed=5)   # 41-entry rows: one step of a lane group, no long-row path
    plan = synth.dyadic_plan(41, E.DTYPES[dt], 4, 4)
    band.val = synth.dyadic_values(band.rowptr, plan, 6, colidx=band.colidx, n=band.n)
    xt = synth.dyadic_x(band.m, plan, 7)
    rt, ct, vt = exact_ref.transpose(band.rowptr, band.colidx, band.val, band.n)
    want_t = exact_ref.spmv(rt, ct, vt, xt, plan.ev, plan.ex)
    for method in (M.Method_Parallel, M.Method_SellCSigma, M.Method_CSR5SPMV):
        with api.Handle(band.m, band.n, band.rowptr, band.colidx, band.val, method) as h:
            _check(h.spmv_transpose(xt, np.full(band.n, np.nan, dtype=E.DTYPES[dt])), want_t, method.name, "band transpose", plan)
            tinfo = api.get_transpose_info(h.h)
            assert tinfo["x_groups_staged"] == tinfo["x_groups"] > 0 and tinfo["x_span_max"] > 0, tinfo
            _assert_transpose_info(tinfo, dt, band.m)


def _assert_transpose_info(tinfo, dt, cols):
    """x_span_max and lds_bytes of a transposed schedule agree with its kernel: a staged total and the request for it, or nothing staged."""
    staged = tinfo["x_groups_staged"] > 0 and tinfo["kernel_name"] != "csr_vector_pipe_kernel" and not tinfo["cache_blocked"]
    assert (tinfo["x_span_max"] > 0) == staged and tinfo["x_span_max"] <= cols, tinfo
    if staged:
        s = E.size_of(dt)
        extra = tinfo["lds_bytes"] - E.xbytes(tinfo["x_span_max"], dt)
        allowed = [s * E.SIGMA * g for g in (1, 2, 4, 8)] if tinfo["kernel_name"] == "sell_window_kernel" else [0] + [4 * st * 4 for st in (64, 5 * 64, 9 * 64, 17 * 64)]
        assert extra in allowed, (extra, tinfo)
