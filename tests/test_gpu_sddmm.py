"""GPU: spmv_hip_sddmm, Out[p] = sum_c U[row(p), c] V[col(p), c] over the handle's pattern (include/spmv_hip.h).

Reference: every entry's sum in float64 (fp32 handles) or np.longdouble (fp64 handles).  Bars: random inputs ->
|err| <= (k + 1) u sum_c |U[i, c] V[j, c]| with u = 2^-53 / 2^-24, the standard gamma_k bound of a length-k inner product, which holds for
any summation order with or without fma (derived, not measured); "eighths" inputs -> BIT-EXACT (the reference is checked to be
representable first); k = 1 -> the bits of U[i] * V[j] for any operands.  Bits do not depend on ld, alignment, the pointers' kind, the
stream or the handle's method."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from spmv_amd import api, build

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    NAMES = sorted(json.load(_f)["cases"].keys())
ALL_METHODS = [M.Method_Serial, M.Method_Parallel, M.Method_Balanced, M.Method_Balanced2,
               M.Method_Balanced_Yid, M.Method_SellCSigma, M.Method_CSR5SPMV]
UNIT = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
WIDE = {np.dtype(np.float64): np.longdouble, np.dtype(np.float32): np.float64}
E_ARG, E_NOSTATE = 3, 5
DEV = "cuda:0"
# 16 / 17 and 32 / 33 straddle the kernel's column chunk (8 lanes x 16 bytes: 16 fp64 / 32 fp32 columns)
KS = (1, 2, 3, 8, 16, 17, 32, 33, 65)
GUARD = -7.25


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


_CASES = {}


def case(name):
    """(csr, row of every entry): loaded once, shared, never changed"""
    if name not in _CASES:
        csr = load_golden(name)[0]
        _CASES[name] = (csr, np.repeat(np.arange(csr.m), np.diff(csr.rowptr)))
    return _CASES[name]


def operands(csr, k, kind, seed=5):
    rng = np.random.default_rng(seed + k)
    if kind == "eighths":   # signed multiples of 1/8 in [-1, 1]: products are multiples of 1/64, sums of 65 of them need 14 bits
        U, V = (rng.integers(-8, 9, (r, k)) * 0.125 for r in (csr.m, csr.n))
    else:
        U, V = (rng.uniform(-1, 1, (r, k)) for r in (csr.m, csr.n))
    return U.astype(csr.val.dtype), V.astype(csr.val.dtype)


def reference(csr, rows, U, V):
    """(sum, sum of magnitudes) per entry, accumulated in the wider type"""
    wide = WIDE[U.dtype]
    ref, mag = np.zeros(csr.nnz, dtype=wide), np.zeros(csr.nnz, dtype=wide)
    for a in range(0, csr.nnz, 8192):
        prod = U[rows[a:a + 8192]].astype(wide) * V[csr.colidx[a:a + 8192]].astype(wide)
        ref[a:a + 8192] = prod.sum(1)
        # numpy's reduction starts from +0; an IEEE sum in any order is -0 exactly when every term is -0
        ref[a:a + 8192][((prod == 0) & np.signbit(prod)).all(1)] = -0.0
        mag[a:a + 8192] = np.abs(prod).sum(1)
    return ref, mag


def check(out, csr, rows, U, V, exact):
    assert out.shape == (csr.nnz,) and out.dtype == U.dtype
    assert not np.isnan(out).any(), f"{int(np.isnan(out).sum())} entries left unwritten"
    ref, mag = reference(csr, rows, U, V)
    k = U.shape[1]
    if exact:
        want = ref.astype(out.dtype)
        assert np.array_equal(want.astype(ref.dtype), ref), "the reference itself must be representable for the bit-exact bar"
        assert np.array_equal(out.view(np.uint8), want.view(np.uint8))
        return
    err = np.abs(out.astype(ref.dtype) - ref)
    bar = (k + 1) * UNIT[out.dtype] * mag
    worst = float((err / np.maximum(bar, 1e-300)).max(initial=0))
    print(f"k = {k}: max err / bar = {worst:.3f}")
    assert (err <= bar).all(), (k, worst)


def handle(csr, method=M.Method_Parallel, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method)
    finally:
        api.clear_thread_options()


def sddmm_host(h, csr, U, V):
    """through host pointers, into a NaN-prefilled Out with a guard element behind its end"""
    buf = np.full(csr.nnz + 1, np.nan, dtype=csr.val.dtype)
    buf[-1] = GUARD
    api.sddmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, U, V, buf[:csr.nnz])
    assert buf[-1] == GUARD, "written past the end of Out"
    return buf[:csr.nnz].copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ----------------------------------------------------------------------------- 1. every golden case, both dtypes
@pytest.mark.parametrize("name", NAMES)
def test_golden(name):
    csr, rows = case(name)
    exact = name.endswith("eighths")
    with handle(csr) as h:
        for k in KS:
            U, V = operands(csr, k, "eighths" if exact else "uniform")
            check(sddmm_host(h, csr, U, V), csr, rows, U, V, exact)


# ----------------------------------------------------------------------------- 2. the handle's method and kind change no bit
@pytest.mark.parametrize("method", ALL_METHODS, ids=lambda m: m.name)
@pytest.mark.parametrize("name", ["skewed_f64_uniform", "powerlaw_f32_uniform", "banded_f64_uniform", "empty_mix_f32_uniform"])
def test_methods_give_the_same_bits(name, method):
    csr, rows = case(name)
    with handle(csr) as base:
        want = {k: sddmm_host(base, csr, *operands(csr, k, "uniform")) for k in (3, 17, 33)}
    for opts in ({}, {"keep_columns": 1}, {"cache_block": 2}):   # released columns restored / kept; the blocked executor where it can be built
        with handle(csr, method, **opts) as h:
            y = np.full(csr.m, np.nan, dtype=csr.val.dtype)
            x = np.ones(csr.n, dtype=csr.val.dtype)
            h.spmv(x, y)
            for k in (3, 17, 33):
                U, V = operands(csr, k, "uniform")
                out = sddmm_host(h, csr, U, V)
                assert same_bits(out, want[k]), (opts, k)
            y2 = np.full(csr.m, np.nan, dtype=csr.val.dtype)
            h.spmv(x, y2)
            assert same_bits(y, y2)                                  # spmv() computes what it did before
    check(want[17], csr, rows, *operands(csr, 17, "uniform"), False)


# ----------------------------------------------------------------------------- 3. k = 1: the correctly rounded product, any operands
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_k1_is_the_single_product(dtype):
    csr, rows = case("skewed_f64_uniform" if dtype == np.float64 else "skewed_f32_uniform")
    rng = np.random.default_rng(3)
    fi = np.finfo(dtype)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal * 3, fi.max, -fi.max,
                        fi.eps, 1.0, -1.0], dtype=dtype)

    def draw(r):
        v = (rng.standard_normal(r) * np.exp2(rng.integers(-60, 60, r))).astype(dtype)
        pick = rng.random(r) < 0.3
        v[pick] = rng.choice(special, int(pick.sum()))
        return v.reshape(-1, 1)

    U, V = draw(csr.m), draw(csr.n)
    with np.errstate(all="ignore"):
        want = (U[rows, 0] * V[csr.colidx, 0]).astype(dtype)
    with handle(csr) as h:
        out = sddmm_host(h, csr, U, V)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan)                       # NaN where IEEE 754 gives one (payloads are not compared)
    assert same_bits(out[~nan], want[~nan])                         # signed zeros, subnormals, infinities: bit for bit
    assert np.isinf(want).any() and (want == 0).any() and nan.any()


# ----------------------------------------------------------------------------- 4. ld, alignment, pointers' kind, stream: identical bits
@pytest.mark.parametrize("name", ["skewed_f64_uniform", "powerlaw_f32_uniform", "single_long_f64_uniform", "dense_row0_f32_uniform"])
def test_layout_and_pointer_kind_change_no_bit(name):
    import torch
    csr, rows = case(name)
    with handle(csr) as h:
        for k in (1, 5, 17, 33):
            U, V = operands(csr, k, "uniform")
            base = sddmm_host(h, csr, U, V)
            check(base, csr, rows, U, V, False)
            for ld, off in ((k, 0), (k + 1, 0), (k + 3, 0), (k + 1, 1), (k + 3, 1)):   # off = 1: a view one element (8 / 4 bytes) into the row
                Uo = np.full((csr.m, ld + off), np.nan, dtype=U.dtype)   # NaN in the padding of U / V never reaches Out
                Vo = np.full((csr.n, ld + off), np.nan, dtype=U.dtype)
                Uo[:, off:off + k], Vo[:, off:off + k] = U, V
                assert same_bits(sddmm_host(h, csr, Uo[:, off:off + k], Vo[:, off:off + k]), base), (k, ld, off)
                Ud, Vd = torch.from_numpy(Uo).to(DEV), torch.from_numpy(Vo).to(DEV)
                Od = torch.full((csr.nnz + 1,), float("nan"), dtype=Ud.dtype, device=DEV)
                Od[-1] = GUARD
                api.sddmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Ud[:, off:off + k], Vd[:, off:off + k], Od[:csr.nnz])
                torch.cuda.synchronize()
                assert float(Od[-1]) == GUARD
                assert same_bits(Od[:csr.nnz].cpu().numpy(), base), (k, ld, off)
            # each of U, V and Out on its own side
            Ud, Vd = torch.from_numpy(U).to(DEV), torch.from_numpy(V).to(DEV)
            for uu, vv, dev_out in ((Ud, V, False), (U, Vd, False), (U, V, True), (Ud, Vd, False), (Ud, V, True)):
                if dev_out:
                    o = torch.full((csr.nnz,), float("nan"), dtype=Ud.dtype, device=DEV)
                    api.sddmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, uu, vv, o)
                    torch.cuda.synchronize()
                    o = o.cpu().numpy()
                else:
                    o = sddmm_host(h, csr, uu, vv)
                assert same_bits(o, base), k
        # an attached stream with async
        s = torch.cuda.Stream()
        h.attach_stream(s.cuda_stream, async_=True)
        o = torch.full((csr.nnz,), float("nan"), dtype=Ud.dtype, device=DEV)
        with torch.cuda.stream(s):
            api.sddmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Ud, Vd, o)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert same_bits(o.cpu().numpy(), base)
        with torch.cuda.stream(s):
            o2 = h.sddmm(Ud, Vd)                                     # Handle.sddmm allocates Out like U
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert same_bits(o2.cpu().numpy(), base)


# ----------------------------------------------------------------------------- 5. device CSR arrays
def test_device_csr_arrays():
    import torch
    csr, rows = case("empty_mix_f64_eighths")
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    U, V = operands(csr, 8, "eighths")
    with api.Handle(csr.m, csr.n, rp, ci, va, M.Method_CSR5SPMV) as h:
        out = h.sddmm(torch.from_numpy(U).to(DEV), torch.from_numpy(V).to(DEV))
        torch.cuda.synchronize()
        assert out.device.type == "cuda" and tuple(out.shape) == (csr.nnz,)
        check(out.cpu().numpy(), csr, rows, U, V, True)
        check(h.sddmm(U, V), csr, rows, U, V, True)


# ----------------------------------------------------------------------------- 6. errors and degenerate shapes
def test_reorder_handle_is_an_argument_error():
    import torch
    from spmv_amd import synth
    lib = api.load()
    m, n, rp, ci, va = synth.banded_holes_device(100_000, 100_000, 24, 0.25, "eighths", torch.float64, DEV, 7)
    api.set_thread_option("reorder", 1)
    try:
        h = api.Handle(m, n, rp, ci, va, M.Method_Parallel)
    finally:
        api.clear_thread_options()
    with h:
        assert h.index is not None
        U = torch.ones((m, 3), dtype=torch.float64, device=DEV)
        out = torch.full((int(rp[-1].item()),), GUARD, dtype=torch.float64, device=DEV)
        lib.spmv_hip_clear_error()
        assert api.sddmm(h.h, m, rp, ci, va, U, U, out, check=False) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())


def test_errors_leave_out_untouched():
    lib = api.load()
    csr, _ = case("banded_f64_uniform")
    U, V = operands(csr, 4, "uniform")
    with handle(csr) as h:
        def call(k, pu, ldu, pv, ldv, po):
            lib.spmv_hip_clear_error()
            return lib.spmv_hip_sddmm(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, k, pu, ldu, pv, ldv, po)
        out = np.full(csr.nnz, GUARD)
        u, v, o = U.ctypes.data, V.ctypes.data, out.ctypes.data
        for args in ((0, u, 4, v, 4, o), (4, u, 3, v, 4, o), (4, u, 4, v, 3, o), (4, None, 4, v, 4, o), (4, u, 4, None, 4, o), (4, u, 4, v, 4, None)):
            assert call(*args) == E_ARG, args
            assert lib.spmv_hip_last_error() == E_ARG
            assert (out == GUARD).all()
        lib.spmv_hip_clear_error()
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            out = np.full(csr.nnz, GUARD)
            assert api.sddmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, U, V, out, check=False) == E_ARG, key
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
            assert (out == GUARD).all()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    out = np.full(csr.nnz, GUARD)
    assert api.sddmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, U, V, out, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert (out == GUARD).all()
    h.close()


def test_empty_matrix_writes_nothing():
    lib = api.load()
    csr, _ = case("nnz0_f64_uniform")
    U, V = operands(csr, 5, "uniform")
    with handle(csr) as h:
        guard = np.full(3, GUARD)
        lib.spmv_hip_clear_error()
        assert api.sddmm(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, U, V, guard[:0]) == 0
        assert lib.spmv_hip_sddmm(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, 5, U.ctypes.data, 5, V.ctypes.data, 5, None) == 0
        assert lib.spmv_hip_last_error() == 0
        assert (guard == GUARD).all()
        assert h.sddmm(U, V).shape == (0,)


def test_destroy_returns_the_memory():
    import torch
    csr, _ = case("skewed_f64_eighths")
    U, V = operands(csr, 9, "eighths")

    def cycle():
        for method in ALL_METHODS:
            h = handle(csr, method)
            sddmm_host(h, csr, U, V)          # three staging buffers, restored columns
            if method == M.Method_CSR5SPMV:
                api.spmv_clear_handle(h.h)
            h.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    first = cycle()
    for _ in range(2):
        last = cycle()
    assert last >= first - (1 << 20), (first, last)
