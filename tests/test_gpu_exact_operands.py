"""GPU: every schedule on full-precision signed operands and on non-finite inputs, compared with an exact integer evaluation.

The "eighths" data of the other exact tests proves the indexing, but its operands are exact in fp16 and never negative.  Here values and
x are signed dyadic numbers that use the whole significand of one operand (synth.dyadic_*: fp64 30-bit values or x, scales up to
2^+-300, a subnormal draw), yet every partial sum stays exact, so every schedule must still give the bits of tests/exact_ref.py: an fp64
operand rounded through fp32 anywhere (value stream, LDS x windows, split halves, spmm staging), an fp64 row accumulated in fp32 or a
lost sign shows.  Non-finite x and values check that masked and padding slots never multiply x and that no NaN / Inf leaks into a row
that does not reference it; all -0.0 rows check that accumulators start at +0.0 as the reference's do.

Comparison: finite and infinite rows bit for bit (+0.0 is not -0.0), NaN rows by isnan.
SPMV_EXACT_FIRST / SPMV_EXACT_SEEDS widen the option fuzz."""
import contextlib
import os

import numpy as np
import pytest
import torch

import exact_ref
from spmv_amd import api, build, synth
from test_gpu_bigfuzz import CASES as BIG_CASES, _matrix as big_matrix
from test_gpu_fuzz import METHODS, OPTIONS, _case
from test_gpu_routing import ROWS as SPLIT_ROWS, _mixed as split_matrix

pytestmark = pytest.mark.gpu
M = api.SPMV_METHODS
DEV = "cuda:0"
_FIRST, _COUNT = int(os.environ.get("SPMV_EXACT_FIRST", "0")), int(os.environ.get("SPMV_EXACT_SEEDS", "32"))
SEEDS = range(_FIRST, _FIRST + _COUNT)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    api.load()


@contextlib.contextmanager
def _options(chosen):
    defaults = {k: api.get_option(k) for k in chosen}
    try:
        for k, v in chosen.items():
            api.set_option(k, v)
        yield
    finally:
        for k, v in defaults.items():
            api.set_option(k, v)


def _report(bad, y, want, what):
    rows = ", ".join(f"y[{r}] = {float(y[r])!r} want {float(want[r])!r}" for r in bad[:4])
    return f"{len(bad)} rows differ: {rows}; {what}"


def _check(y, want, *what):
    bad = exact_ref.mismatches(y, want)
    assert bad.size == 0, _report(bad.tolist(), y, want, what)


def _check_device(y, want, *what):
    torch.cuda.synchronize()
    bad = exact_ref.mismatches_device(y, want)
    assert bad.numel() == 0, _report(bad[:4].tolist(), y, want, (what, f"{bad.numel()} rows in all"))


def _fuzz_case(seed, subnormal=False):
    """test_gpu_fuzz's shape and options for this seed, with dyadic values and x (wide operand alternating with the seed)."""
    csr, _, rng = _case(seed)
    chosen = {k: int(rng.choice(v)) for k, v in OPTIONS.items()}
    plan = synth.dyadic_plan(int(np.diff(csr.rowptr).max(initial=0)), csr.val.dtype, seed, seed, subnormal)
    csr.val = synth.dyadic_values(csr.rowptr, plan, 10 * seed + 1)
    return csr, synth.dyadic_x(csr.n, plan, 10 * seed + 2), plan, chosen


def _note(seen, info):
    seen["kernels"].add(info["kernel_name"])
    seen["schedules"].add(info["schedule_name"])
    for k in ("run_nnz", "byte_nnz", "tmpl_nnz", "far_nnz"):
        seen[k] = max(seen.get(k, 0), int(info[k]))


def _new_seen():
    return {"kernels": set(), "schedules": set()}


# ----------------------------------------------------------------------------- option fuzz: all methods, random options, update_values
_FUZZ_SEEN = {}


def _run_fuzz(seed):
    if seed in _FUZZ_SEEN:
        return _FUZZ_SEEN[seed]
    csr, x, plan, chosen = _fuzz_case(seed)
    seen = _new_seen()
    want = exact_ref.spmv_csr(csr, x, plan)
    v2 = synth.dyadic_values(csr.rowptr, plan, 10 * seed + 3)              # freshly drawn signed values behind the same pattern
    want2 = exact_ref.spmv(csr.rowptr, csr.colidx, v2, x, plan.ev, plan.ex)
    with _options(chosen):
        for method in METHODS:
            with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val.copy(), method) as h:
                y = h.spmv(x, np.full(csr.m, np.nan, dtype=csr.val.dtype))
                info = h.info()
                _note(seen, info)
                _check(y, want, seed, method.name, info["kernel_name"], plan, chosen)
                h.update_values(v2)
                y = h.spmv(x, np.full(csr.m, np.nan, dtype=csr.val.dtype))
                _check(y, want2, seed, method.name, info["kernel_name"], plan, chosen, "update_values")
    _FUZZ_SEEN[seed] = seen
    return seen


@pytest.mark.parametrize("seed", SEEDS)
def test_option_fuzz_every_schedule_is_exact(seed):
    _run_fuzz(seed)


@pytest.mark.parametrize("seed", range(8))
def test_subnormal_rows_are_exact(seed):
    """Products on the smallest subnormal's grid, row sums below the smallest normal, each operand normal: nothing may flush to zero."""
    csr, x, plan, chosen = _fuzz_case(seed, subnormal=True)
    want = exact_ref.spmv_csr(csr, x, plan)
    assert (want[np.diff(csr.rowptr) > 0] != 0).any() or csr.nnz == 0 or not x.any()
    with _options(chosen):
        for method in METHODS:
            with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method) as h:
                y = h.spmv(x, np.full(csr.m, np.nan, dtype=csr.val.dtype))
                _check(y, want, seed, method.name, h.info()["kernel_name"], plan, chosen)


# ----------------------------------------------------------------------------- non-finite x and values, signed zero
@pytest.mark.parametrize("seed", SEEDS)
def test_nonfinite_inputs_stay_in_their_rows(seed):
    """NaN / +-Inf in about 0.3 % of x (always the first and last column) and in a few values, some of them where x = 0.  Rows that
    reference no non-finite product must come out finite and exact: masked and padding slots never multiply x."""
    _nonfinite_sweep(seed, METHODS)


@pytest.mark.parametrize("seed", [1, 17])
def test_nonfinite_regression_nnz_split_forward_and_long_rows(seed):
    """Found by this sweep: the nnz-split tiles with forward completion (csr5.hpp) added 0 * x[0] for the lanes beyond a row cut by a
    tile boundary, and a row longer than a tile (nat_long_row) 0 * x[0] for the slots past its end -- a NaN / Inf in x[0] reached
    rows that never reference it, and turned +-Inf rows into NaN.  Seeds 1 and 17 under Method_Balanced (nat_kernel)."""
    _nonfinite_sweep(seed, [M.Method_Balanced])


def _nonfinite_sweep(seed, methods):
    csr, x, plan, chosen = _fuzz_case(seed)
    val, xn = exact_ref.sprinkle_nonfinite(csr.colidx, csr.val, x, seed)
    val2, _ = exact_ref.sprinkle_nonfinite(csr.colidx, synth.dyadic_values(csr.rowptr, plan, 10 * seed + 3), x, seed + 1)
    want = exact_ref.spmv(csr.rowptr, csr.colidx, val, xn, plan.ev, plan.ex)
    want2 = exact_ref.spmv(csr.rowptr, csr.colidx, val2, xn, plan.ev, plan.ex)
    with _options(chosen):
        for method in methods:
            with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, val.copy(), method) as h:
                y = h.spmv(xn, np.full(csr.m, np.nan, dtype=csr.val.dtype))
                _check(y, want, seed, method.name, h.info()["kernel_name"], plan, chosen)
                h.update_values(val2)
                y = h.spmv(xn, np.full(csr.m, np.nan, dtype=csr.val.dtype))
                _check(y, want2, seed, method.name, h.info()["kernel_name"], plan, chosen, "update_values")


@pytest.mark.parametrize("seed", range(12))
def test_rows_of_negative_zero_products_give_plus_zero(seed):
    csr, x, plan, chosen = _fuzz_case(seed)
    csr.val, x, zrows = exact_ref.signed_zero_rows(csr, x, seed)
    want = exact_ref.spmv_csr(csr, x, plan)
    assert zrows.size and not np.signbit(want[zrows]).any()
    with _options(chosen):
        for method in METHODS:
            with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method) as h:
                y = h.spmv(x, np.full(csr.m, np.nan, dtype=csr.val.dtype))
                _check(y, want, seed, method.name, h.info()["kernel_name"], plan, chosen)


# ----------------------------------------------------------------------------- directed device matrices: BYTE / TEMPLATE tiles, the near / far split
def _device_dyadic(rp, n, dt, case, seed):
    lens = rp[1:].long() - rp[:-1].long()
    plan = synth.dyadic_plan(int(lens.max()), np.float64 if dt == torch.float64 else np.float32, case, seed)
    return synth.dyadic_values_device(rp, plan, seed + 1), synth.dyadic_x_device(n, plan, seed + 2, DEV), plan


def _device_nonfinite_x(x, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    n = x.numel()
    xn = x.clone()
    cols = torch.cat([torch.tensor([0, n - 1], device=DEV), torch.randint(0, n, (max(1, n * 3 // 1000),), generator=g, device=DEV)])
    special = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=x.dtype, device=DEV)
    xn[cols] = special[torch.randint(0, 3, (cols.numel(),), generator=g, device=DEV)]
    return xn


def _device_run(rp, ci, va, x, plan, methods, seen, what):
    m, n = rp.numel() - 1, x.numel()
    xn = _device_nonfinite_x(x, 5)
    want = exact_ref.spmv_device(rp, ci, va, x, plan.ev, plan.ex)
    want_n = exact_ref.spmv_device(rp, ci, va, xn, plan.ev, plan.ex)
    for method in methods:
        y = torch.full((m,), float("nan"), dtype=va.dtype, device=DEV)
        with api.Handle(m, n, rp, ci, va, method) as h:
            info = h.info()
            _note(seen, info)
            h.spmv(x, y)
            _check_device(y, want, what, method.name, info["kernel_name"], info["far_nnz"], plan)
            h.spmv(xn, y)
            _check_device(y, want_n, what, method.name, info["kernel_name"], info["far_nnz"], plan, "non-finite x")
    return seen


_DIRECTED_SEEN = {}


def _run_directed(name):
    if name in _DIRECTED_SEEN:
        return _DIRECTED_SEEN[name]
    seen = _new_seen()
    if name == "banded_holes":
        for k, dt, case in ((32, torch.float64, 0), (24, torch.float32, 1)):
            _, _, rp, ci, _ = synth.banded_holes_device(200_000, 200_000, k, 0.25, "eighths", dt, DEV, seed=3)
            va, x, plan = _device_dyadic(rp, 200_000, dt, case, 11 + case)
            _device_run(rp, ci, va, x, plan, METHODS, seen, name)
    elif name == "stencil27":
        for nx, dt, case in ((48, torch.float64, 1), (40, torch.float32, 0)):
            _, _, rp, ci, _ = synth.stencil27_device(nx, "eighths", dt, DEV, seed=4)
            va, x, plan = _device_dyadic(rp, nx ** 3, dt, case, 21 + case)
            _device_run(rp, ci, va, x, plan, METHODS, seen, name)
    elif name == "blocked_forms":                                              # the row-block x column-slab executor, narrow and wide forms
        for waves, det, dt, case in ((1, 1, torch.float64, 1), (4, 1, torch.float64, 0), (8, 0, torch.float32, 1)):
            _, _, rp, ci, _ = synth.from_row_lengths_device(synth.powerlaw_lengths_device(300_000, 6.0, 3000, 1.6, DEV, seed=7), 300_000,
                                                            "eighths", dt, DEV, seed=8)
            va, x, plan = _device_dyadic(rp, 300_000, dt, case, 31 + case)
            with _options({"cache_block": 2, "blk_waves": waves, "deterministic": det}):
                _device_run(rp, ci, va, x, plan, [M.Method_Parallel, M.Method_Balanced2, M.Method_CSR5SPMV], seen, (name, waves, det))
    elif name in ("split_tail10", "split_every10"):                           # test_gpu_routing's partly local shapes: A_near + A_far
        rp, ci, _ = split_matrix(name.split("_")[1])
        va, x, plan = _device_dyadic(rp, SPLIT_ROWS, torch.float64, 0 if name == "split_tail10" else 1, 41)
        _device_run(rp, ci, va, x, plan, [M.Method_Parallel, M.Method_CSR5SPMV, M.Method_SellCSigma], seen, name)
        del rp, ci, va, x
        torch.cuda.empty_cache()
    _DIRECTED_SEEN[name] = seen
    return seen


DIRECTED = ["banded_holes", "stencil27", "blocked_forms", "split_tail10", "split_every10"]


@pytest.mark.parametrize("name", DIRECTED)
def test_directed_forms_are_exact(name):
    _run_directed(name)


# ----------------------------------------------------------------------------- at size: hot cells, super slabs, long-row sub-matrices, autotune
BIG = [0, 3, 6, 7, 9]     # wide windows, no locality, web split, R-MAT fp32 hot cells, runs
_BIG_SEEN = {}


def _run_big(case):
    if case in _BIG_SEEN:
        return _BIG_SEEN[case]
    m, n, _, _, dt = BIG_CASES[case]
    rp, ci, _, _ = big_matrix(case)
    va, x, plan = _device_dyadic(rp, n, dt, BIG.index(case), 500 + case)
    seen = _device_run(rp, ci, va, x, plan, [M.Method_Parallel, M.Method_Balanced, M.Method_Balanced2, M.Method_Balanced_Yid,
                                             M.Method_SellCSigma, M.Method_CSR5SPMV], _new_seen(), ("big", case))
    del rp, ci, va, x
    torch.cuda.empty_cache()
    _BIG_SEEN[case] = seen
    return seen


@pytest.mark.parametrize("case", BIG)
def test_big_shapes_are_exact(case):
    _run_big(case)


def test_form_coverage():
    """The sweep above must keep reaching every form: RUN / BYTE / TEMPLATE tiles, the split, both blocked executors, SELL and CSR5."""
    seen = _new_seen()
    for s in [_run_fuzz(seed) for seed in SEEDS] + [_run_directed(nm) for nm in DIRECTED] + [_run_big(c) for c in BIG]:
        seen["kernels"] |= s["kernels"]
        seen["schedules"] |= s["schedules"]
        for k in ("run_nnz", "byte_nnz", "tmpl_nnz", "far_nnz"):
            seen[k] = max(seen.get(k, 0), s.get(k, 0))
    for k in ("run_nnz", "byte_nnz", "tmpl_nnz", "far_nnz"):
        assert seen[k] > 0, (k, seen)
    assert {"blk_kernel", "blk_wide_kernel"} <= seen["kernels"], seen
    assert {"sell-c-sigma", "csr5"} <= seen["schedules"], seen


# ----------------------------------------------------------------------------- spmm, transpose, sharded handles
def _small_matrix(dt, seed, transpose=False):
    rng = np.random.default_rng(seed)
    m, n = 2500, 2100
    lens = rng.integers(0, 40, m)
    lens[rng.integers(0, m, 4)] = 0
    lens[7] = 600                                                           # a row over 512 entries
    lens[m - 3] = 1100
    csr = synth.from_row_lengths(lens, n, "eighths", dt, seed)
    max_len = int(lens.max())
    if transpose:
        max_len = max(max_len, int(np.bincount(csr.colidx, minlength=n).max()))
    plan = synth.dyadic_plan(max_len, dt, seed, seed)
    csr.val = synth.dyadic_values(csr.rowptr, plan, seed + 1, **(dict(colidx=csr.colidx, n=n) if transpose else {}))
    return csr, plan


@pytest.mark.parametrize("kind", ["dyadic", "nonfinite"])
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", [0, 1])
def test_spmm_columns_are_exact(case, dt, kind):
    """k across both panel boundaries (16 fp64 / 32 fp32 columns) and a row of more than 512 entries."""
    csr, plan = _small_matrix(dt, 60 + case)
    val = csr.val
    for method in METHODS:
        for k in (1, 2, 5, 16, 17, 33):
            X = np.stack([synth.dyadic_x(csr.n, plan, 1000 * k + c) for c in range(k)], axis=1)
            if kind == "nonfinite":
                cols = [exact_ref.sprinkle_nonfinite(csr.colidx, csr.val, X[:, c], 77 + c) for c in range(k)]
                val = cols[0][0]
                X = np.ascontiguousarray(np.stack([c[1] for c in cols], axis=1))
            with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, val, method) as h:
                Y = h.spmm(X, np.full((csr.m, k), np.nan, dtype=dt))
                for c in range(k):
                    want = exact_ref.spmv(csr.rowptr, csr.colidx, val, X[:, c], plan.ev, plan.ex)
                    _check(np.ascontiguousarray(Y[:, c]), want, method.name, k, c, plan, kind)


@pytest.mark.parametrize("kind", ["dyadic", "nonfinite"])
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", [0, 1])
def test_transpose_is_exact(case, dt, kind):
    csr, plan = _small_matrix(dt, 70 + case, transpose=True)
    xt = synth.dyadic_x(csr.m, plan, 71 + case)
    val = csr.val
    if kind == "nonfinite":
        row_of = np.repeat(np.arange(csr.m), np.diff(csr.rowptr.astype(np.int64)))
        val, xt = exact_ref.sprinkle_nonfinite(row_of, csr.val, xt, 72 + case)
    rt, ct, vt = exact_ref.transpose(csr.rowptr, csr.colidx, val, csr.n)
    want = exact_ref.spmv(rt, ct, vt, xt, plan.ev, plan.ex)
    for method in METHODS:
        with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, val, method) as h:
            y = h.spmv_transpose(xt, np.full(csr.n, np.nan, dtype=dt))
            _check(y, want, method.name, plan, kind)


@pytest.mark.parametrize("gpus,xchg", [(2, 0), (3, 2), (3, 1)])
@pytest.mark.parametrize("seed", [1, 17, 25])
def test_sharded_handles_are_exact(monkeypatch, seed, gpus, xchg):
    monkeypatch.setenv("SPMV_HIP_GPUS_VIRTUAL", "1")
    csr, x, plan, _ = _fuzz_case(seed)
    val_n, x_n = exact_ref.sprinkle_nonfinite(csr.colidx, csr.val, x, seed)
    for kind, val, xx in (("dyadic", csr.val, x), ("nonfinite", val_n, x_n)):
        want = exact_ref.spmv(csr.rowptr, csr.colidx, val, xx, plan.ev, plan.ex)
        for method in METHODS:
            api.set_thread_option("gpus", gpus)
            api.set_thread_option("x_exchange", xchg)
            try:
                h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, val, method)
            finally:
                api.clear_thread_options()
            with h:
                y = h.spmv(xx, np.full(csr.m, np.nan, dtype=csr.val.dtype))
                _check(y, want, seed, gpus, xchg, method.name, plan, kind)
