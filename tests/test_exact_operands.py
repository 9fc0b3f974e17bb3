"""Host checks of the full-precision signed dyadic operands (synth.dyadic_*) and of their exact reference (tests/exact_ref.py).

The GPU module test_gpu_exact_operands.py compares every schedule with exact_ref bit for bit; that is only sound if the generator keeps
its bit budget, really uses the precision it claims, and if exact_ref says what the reference's Method_Serial says -- +0.0 rows,
subnormal rows and non-finite rows included.  No GPU needed."""
import numpy as np
import pytest

import exact_ref
import oracle
from spmv_amd import synth
from test_gpu_fuzz import _case


def _draw(seed, case, subnormal=False, colidx_budget=False):
    csr, _, _ = _case(seed)
    lens = np.diff(csr.rowptr.astype(np.int64))
    max_len = int(lens.max(initial=0))
    if colidx_budget:
        max_len = max(max_len, int(np.bincount(csr.colidx, minlength=csr.n).max(initial=0)))
    plan = synth.dyadic_plan(max_len, csr.val.dtype, case, seed, subnormal)
    kw = dict(colidx=csr.colidx, n=csr.n) if colidx_budget else {}
    csr.val = synth.dyadic_values(csr.rowptr, plan, seed + 1, **kw)
    return csr, synth.dyadic_x(csr.n, plan, seed + 2), plan


def _int_bits(a, e):
    return synth.bit_length(np.ldexp(a.astype(np.float64), -e).astype(np.int64))


SEEDS = range(24)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("subnormal", [False, True])
def test_bit_budget_holds_on_every_row(seed, subnormal):
    for case in (0, 1):
        csr, x, plan = _draw(seed, case, subnormal)
        rp = csr.rowptr.astype(np.int64)
        lens = np.diff(rp)
        vb = _int_bits(csr.val, plan.ev)
        xb = int(_int_bits(x, plan.ex).max(initial=0))
        assert xb <= plan.xbits
        row_vb = np.zeros(csr.m, dtype=np.int64)
        np.maximum.at(row_vb, np.repeat(np.arange(csr.m), lens), vb)
        used = np.where(lens > 0, row_vb + xb + synth.bit_length(lens), 0)
        assert int(used.max(initial=0)) <= plan.p, (seed, case, plan, int(used.max()))
        # every row sum then stays below 2^p on the product grid: in the subnormal draw below the smallest normal
        y = exact_ref.spmv_csr(csr, x, plan)
        assert np.isfinite(y).all()
        if subnormal:
            assert (np.abs(y) < np.finfo(csr.val.dtype).tiny).all()
            assert (np.abs(csr.val[csr.val != 0]) >= np.finfo(csr.val.dtype).tiny).all() and (np.abs(x[x != 0]) >= np.finfo(x.dtype).tiny).all()
            assert (y != 0).any()


def test_wide_operands_are_not_exact_in_the_narrower_type():
    wide64, total64 = 0, 0
    for seed in SEEDS:
        for case in (0, 1):
            csr, x, plan = _draw(seed, case)
            ints = np.ldexp((csr.val if plan.wide_values else x).astype(np.float64), -(plan.ev if plan.wide_values else plan.ex))
            ints = ints[ints != 0]
            if plan.dtype == np.float64:
                total64 += ints.size
                wide64 += int((ints.astype(np.float32).astype(np.float64) != ints).sum())
            elif plan.wide_values:
                lens = np.diff(csr.rowptr.astype(np.int64))
                budget = np.repeat(synth.dyadic_row_bits(lens, plan), lens)
                sel = ints[budget[csr.val != 0] >= 12] if csr.val.size else ints
                with np.errstate(over="ignore"):
                    assert (sel.astype(np.float16).astype(np.float64) != sel).all(), (seed, plan)
            else:
                assert plan.xbits < 12 or (ints.astype(np.float16).astype(np.float64) != ints).all(), (seed, plan)
    assert total64 > 0 and wide64 >= 0.9 * total64, (wide64, total64)


def test_scales_include_the_huge_ones():
    for dt, big in ((np.float64, 300), (np.float32, 40)):
        seen = {e for seed in range(64) for p in [synth.dyadic_plan(100, dt, seed, seed)] for e in (p.ev, p.ex)}
        assert {big, -big} <= seen, (dt, sorted(seen))
        p = synth.dyadic_plan(100, dt, 0, 0, subnormal=True)
        assert np.ldexp(1.0, p.ev + p.ex) == {np.float64: 2.0**-1074, np.float32: 2.0**-149}[dt]


def _assert_same(y, want, what):
    bad = exact_ref.mismatches(y, want)
    assert bad.size == 0, (what, int(bad[0]), float(y[bad[0]]), float(want[bad[0]]))


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_equals_the_oracle_bit_for_bit(seed):
    for case in (0, 1):
        for kind in ("dyadic", "subnormal", "nonfinite", "signed_zero"):
            csr, x, plan = _draw(seed, case, kind == "subnormal")
            if kind == "nonfinite":
                csr.val, x = exact_ref.sprinkle_nonfinite(csr.colidx, csr.val, x, seed)
            if kind == "signed_zero":
                csr.val, x, zrows = exact_ref.signed_zero_rows(csr, x, seed)
            want = exact_ref.spmv_csr(csr, x, plan)
            if kind == "signed_zero" and csr.nnz:
                assert zrows.size and (want[zrows] == 0).all() and not np.signbit(want[want == 0]).any()
            _assert_same(oracle.spmv_serial(csr, x), want, ("serial", seed, case, kind))
            _assert_same(oracle.spmv_omp(csr, x), want, ("omp", seed, case, kind))


@pytest.mark.skipif(not oracle.have_ref(), reason="the reference build (oracle/_ref) is not present")
@pytest.mark.parametrize("seed", range(8))
def test_reference_equals_the_real_reference(seed):
    for case in (0, 1):
        for kind in ("dyadic", "subnormal", "nonfinite"):
            csr, x, plan = _draw(seed, case, kind == "subnormal")
            if kind == "nonfinite":
                csr.val, x = exact_ref.sprinkle_nonfinite(csr.colidx, csr.val, x, seed)
            want = exact_ref.spmv_csr(csr, x, plan)
            for method in (0, 1):
                y, _ = oracle.ref_spmv(csr, x, method)
                _assert_same(y, want, ("ref", method, seed, case, kind))


@pytest.mark.parametrize("seed", range(8))
def test_transpose_budget_and_reference(seed):
    """With the column budget the draw is exact for A^T x too: exact_ref.transpose + spmv equals the oracle on the explicit A^T."""
    for case in (0, 1):
        csr, _, plan = _draw(seed, case, colidx_budget=True)
        xt = synth.dyadic_x(csr.m, plan, seed + 5)
        rt, ct, vt = exact_ref.transpose(csr.rowptr, csr.colidx, csr.val, csr.n)
        at = synth.CSR(csr.n, csr.m, rt.astype(np.int32), ct.astype(np.int32), vt)
        want = exact_ref.spmv(rt, ct, vt, xt, plan.ev, plan.ex)
        _assert_same(oracle.spmv_serial(at, xt), want, ("transpose", seed, case))


def test_int64_prefix_sums_stay_exact_past_2_to_the_64():
    """Every row sum fits in 53 bits, the running sum over the matrix does not: 5000 rows near 2^52 wrap the int64 prefix sums (a float64
    cumsum would round there); the differences at RowPtr are still exact."""
    m = 5000
    rp = np.arange(m + 1, dtype=np.int32)
    ci = np.zeros(m, dtype=np.int32)
    val = 2.0**45 - 1 - np.arange(m, dtype=np.float64) * 2**20
    x = np.array([127.0])
    want = exact_ref.spmv(rp, ci, val, x, 0, 0)
    assert np.array_equal(want, val * 127.0)
    _assert_same(oracle.spmv_serial(synth.CSR(m, 1, rp, ci, val), x), want, "int64 prefix sums")
