"""GPU: spmv_hip_attention -- O = softmax_rows(scale * Q K^T on A's pattern) V in one pass (include/spmv_hip.h).

1. Bits.  The call promises the composition's result step by step, so it is compared BIT FOR BIT with the composition through the library's
   own calls: Handle.sddmm, a numpy `* dtype(scale)`, Handle.row_softmax, and Handle.spmm on a second handle whose values are P (its Y has
   ldy > dv, so that dv = 1 does not take the spmv schedule).  Rows whose scores hold a NaN, a +inf or only -inf are NaN in both.
2. Accuracy against a wide reference -- float64 (fp32 handles) or np.longdouble (fp64 handles).  The bar is derived, not measured.  With u the
   unit roundoff, d_p = reference score minus the row maximum, E = 2 ulp for exp (HIP's math documentation states 1), tiny the smallest normal:
     delta_p  = (k + 2) u |scale| sum_c |Q_ic K_jc|       the dot's gamma_k bound (any order, fma or not) plus the scaling's rounding: the
                                                           absolute error of t_p, hence a relative error of exp(t_p - M)
     barP_p   = 2 ref_p (u (|d_p| + sum_q ref_q |d_q| + 4 E + len) + delta_p + sum_q ref_q delta_q) + tiny
                                                           test_gpu_row_softmax.py's forward bar with the scores' own error added: once
                                                           for the entry, once -- weighted by the shares ref_q -- through Z
     barO_ic  = sum_p barP_p |V_pc| + (len + 1) u sum_p ref_p |V_pc| + tiny
                                                           P's error carried through the product, plus the length-len chain's gamma bound
   Q, K and V are uniform in [-1, 1].
3. Invariance: host and device pointers, padded ld with NaN in every padding element, misaligned base pointers, every method, stream and
   async settings, K and V the same pointer, repeated calls -- identical bits.
4. Memory rules: canaries, inputs, spmv() before and after, device_bytes, keep_columns = 0.
5. Golden patterns through 1 and 2.   6. Handle rules."""
import numpy as np
import pytest

from conftest import load_golden
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
METHODS = [M.Method_Parallel, M.Method_Balanced, M.Method_Balanced_Yid, M.Method_CSR5SPMV, M.Method_SellCSigma]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
UNIT = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
WIDE = {np.dtype(np.float64): np.longdouble, np.dtype(np.float32): np.float64}
E_ULP = 2
E_ARG, E_NOSTATE = 3, 5
DEV = "cuda:0"
CANARY = -7.25
N = 300
STREAM_PAD = 4 * 64 + 8   # elements behind the resident ColIdx (kernels/csr_vector4.hpp)
# both sides of: the lane groups (1 .. 64), the register chain (64 per step), the long-row threshold and the LDS chunk (512), the chunk's
# packing of several rows (575 .. 577 beside their neighbours), the 2048 batch and the 64-segment split (ceil(len / 64) changes at 4097)
LENGTHS = [0, 1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64, 65, 511, 512, 513, 575, 576, 577, 1025, 2047, 2048, 2049, 4097, 5000]
GOLDENS = ["rowlen_sweep", "single_long", "powerlaw", "empty_mix", "nnz0", "tiny"]


def shapes(dtype):
    """(k, dv, scale) triples: every k, dv and scale of the issue at least once; the largest k with the largest dv"""
    W, KP = (2, 16) if np.dtype(dtype) == np.float64 else (4, 32)
    ks = [1, W, W + 1, 4 * W + 1, 8 * W, 8 * W + 1, 33]
    dvs = [1, 16 // np.dtype(dtype).itemsize, KP - 1, KP, KP + 1, 2 * KP + 3, 2 * KP + 3]
    scales = [1.0, 0.125, None, 1.0, 0.125, None, None]   # None: 1 / sqrt(k) rounded to dtype
    return [(k, dv, float(dtype(1.0 / np.sqrt(k))) if s is None else s) for k, dv, s in zip(ks, dvs, scales)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


_PAT = {}


def pattern(dtype):
    """the rows LENGTHS in a shuffled order, with runs of empty rows at the start, in the middle and at the end; columns in [0, N).  Built
    once per dtype, shared, never changed."""
    key = np.dtype(dtype)
    if key not in _PAT:
        rng = np.random.default_rng(11)
        order = rng.permutation(len(LENGTHS))
        lens = [0] * 5
        for pos, i in enumerate(order):
            if pos == len(order) // 2:
                lens += [0] * 70   # more empty rows than a wave looks at in one step
            lens.append(LENGTHS[i])
        lens += [0] * 6
        rp = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(lens, out=rp[1:])
        nnz = int(rp[-1])
        ci = rng.integers(0, N, nnz).astype(np.int32)
        _PAT[key] = synth.CSR(len(lens), N, rp, ci, rng.uniform(-1, 1, nnz).astype(dtype))
        assert set(np.diff(rp).tolist()) == set(LENGTHS)
    return _PAT[key]


def operands(csr, k, dv, seed=0):
    rng = np.random.default_rng(100 * k + dv + seed)
    dt = csr.val.dtype
    return rng.uniform(-1, 1, (csr.m, k)).astype(dt), rng.uniform(-1, 1, (csr.n, k)).astype(dt), rng.uniform(-1, 1, (csr.n, dv)).astype(dt)


def handle(csr, method=M.Method_Parallel, val=None, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val if val is None else val, method)
    finally:
        api.clear_thread_options()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def fused_host(h, csr, Q, K, V, scale, pad=3):
    """through host pointers, into a canary-filled O with `pad` extra elements behind every row and a row behind the last"""
    dv = V.shape[1]
    buf = np.full((csr.m + 1, dv + pad), CANARY, dtype=csr.val.dtype)
    api.attention(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q, K, V, buf[:csr.m, :dv], scale)
    assert (buf[:, dv:] == CANARY).all() and (buf[csr.m] == CANARY).all(), "written outside O's m x dv elements"
    return buf[:csr.m, :dv].copy()


def composition(h, csr, Q, K, V, scale):
    """the three calls the fused one replaces, on the library's kernels; P lives on a second handle"""
    dt, dv = Q.dtype.type, V.shape[1]
    if csr.nnz == 0:
        return np.zeros((csr.m, dv), dtype=dt)
    S = h.sddmm(Q, K)
    with np.errstate(all="ignore"):
        T = S * dt(scale)
    P = h.row_softmax(T)
    Y = np.full((csr.m, dv + 2), CANARY, dtype=dt)
    with handle(csr, val=P) as hp:
        api.spmm(hp.h, csr.m, csr.rowptr, csr.colidx, P, V, Y[:, :dv])
    return Y[:, :dv].copy()


def check_bits(out, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan)
    assert same_bits(out[~nan], want[~nan])


def check_accuracy(out, csr, Q, K, V, scale):
    dt = np.dtype(Q.dtype)
    wide, u, tiny = WIDE[dt], UNIT[dt], np.finfo(dt).tiny
    k = Q.shape[1]
    Qw, Kw, Vw = Q.astype(wide), K.astype(wide), V.astype(wide)
    sc = wide(dt.type(scale))
    worst = 0.0
    for i in range(csr.m):
        a, b = int(csr.rowptr[i]), int(csr.rowptr[i + 1])
        if a == b:
            assert (out[i] == 0).all() and not np.signbit(out[i]).any(), i
            continue
        cols = csr.colidx[a:b]
        t = (Qw[i] * Kw[cols]).sum(1) * sc
        delta = (k + 2) * u * abs(sc) * (np.abs(Qw[i]) * np.abs(Kw[cols])).sum(1)
        d = t - t.max()
        e = np.exp(d)
        ref = e / e.sum()
        barP = 2 * ref * (u * (np.abs(d) + (ref * np.abs(d)).sum() + 4 * E_ULP + (b - a)) + delta + (ref * delta).sum()) + tiny
        aV = np.abs(Vw[cols])
        barO = (barP[:, None] * aV).sum(0) + (b - a + 1) * u * (ref[:, None] * aV).sum(0) + tiny
        err = np.abs(out[i].astype(wide) - (ref[:, None] * Vw[cols]).sum(0))
        worst = max(worst, float((err / barO).max()))
        assert (err <= barO).all(), (i, b - a, float((err / barO).max()))
    print(f"attention {dt} k={k} dv={V.shape[1]} scale={scale:.4g}: max err / bar = {worst:.3f}")


# ----------------------------------------------------------------------------- 1 + 2. the composition's bits; the derived bar
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_equal_the_composition_and_accuracy(dtype):
    csr = pattern(dtype)
    with handle(csr) as h:
        for k, dv, scale in shapes(dtype):
            Q, K, V = operands(csr, k, dv)
            out = fused_host(h, csr, Q, K, V, scale)
            assert same_bits(out, composition(h, csr, Q, K, V, scale)), (k, dv, scale)
            check_accuracy(out, csr, Q, K, V, scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_scores(dtype):
    """k = 1, Q > 0: a NaN in Q[i] makes row i's scores NaN, +inf in Q[i] makes them +inf (or -inf), K[j*] = -inf puts a -inf beside finite scores
    in every row that holds column j* and makes a row that holds nothing else all -inf"""
    base = pattern(dtype)
    rng = np.random.default_rng(5)
    jstar = 17
    lens = np.diff(base.rowptr)
    rows = [int(np.flatnonzero(lens == n)[0]) for n in (1, 3, 65, 513, 5000)]
    ci = base.colidx.copy()
    ci[base.rowptr[rows[0]]] = jstar          # the row of length 1: only -inf
    ci[base.rowptr[rows[2]] + 40] = jstar     # -inf beside finite scores, short and long rows
    ci[base.rowptr[rows[4]] + 4000] = jstar
    csr = synth.CSR(base.m, base.n, base.rowptr, ci, base.val)
    dv = 5
    Q = rng.uniform(0.5, 1, (csr.m, 1)).astype(dtype)
    K = rng.uniform(0.5, 1, (csr.n, 1)).astype(dtype)
    V = rng.uniform(-1, 1, (csr.n, dv)).astype(dtype)
    K[jstar] = -np.inf
    Q[rows[1]] = np.nan
    Q[rows[3]] = np.inf
    with handle(csr) as h:
        out = fused_host(h, csr, Q, K, V, 1.0)
        want = composition(h, csr, Q, K, V, 1.0)
    check_bits(out, want)
    nan_rows = np.isnan(out).any(1)
    assert np.isnan(out[[rows[0], rows[1], rows[3]]]).all()                         # all -inf, NaN, +inf: the whole row
    assert not nan_rows[rows[2]] and not nan_rows[rows[4]]                          # -inf beside finite scores: an exact +0 weight
    has_j = np.array([jstar in ci[csr.rowptr[i]:csr.rowptr[i + 1]] for i in range(csr.m)])
    expect = np.zeros(csr.m, dtype=bool)
    expect[[rows[0], rows[1], rows[3]]] = True
    expect |= has_j & (lens == 1)
    assert np.array_equal(nan_rows, expect)                                         # and only those rows


# ----------------------------------------------------------------------------- 3. invariance
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layout_pointer_kind_method_and_stream_change_no_bit(dtype):
    import torch
    csr = pattern(dtype)
    KP = 16 if dtype == np.float64 else 32
    k = dv = KP + 1
    Q, K, V = operands(csr, k, dv)
    scale = 0.125
    with handle(csr) as h:
        base = fused_host(h, csr, Q, K, V, scale)
        assert same_bits(fused_host(h, csr, Q, K, V, scale), base)                  # repeated
        for pad, off in ((0, 0), (1, 0), (3, 0), (4, 0), (1, 1), (2, 2), (3, 3)):   # off: a view that many elements into the row
            wide = [np.full((a.shape[0], a.shape[1] + pad + off), np.nan, dtype=dtype) for a in (Q, K, V)]   # NaN in every padding element
            views = []
            for wd, a in zip(wide, (Q, K, V)):
                wd[:, off:off + a.shape[1]] = a
                views.append(wd[:, off:off + a.shape[1]])
            assert same_bits(fused_host(h, csr, *views, scale, pad=pad + off), base), (pad, off)
            dev = [torch.from_numpy(wd).to(DEV) for wd in wide]
            Od = torch.full((csr.m + 1, dv + pad + off), CANARY, dtype=dev[0].dtype, device=DEV)
            api.attention(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, *(d[:, off:off + a.shape[1]] for d, a in zip(dev, (Q, K, V))), Od[:csr.m, off:off + dv], scale)
            torch.cuda.synchronize()
            Oh = Od.cpu().numpy()
            assert same_bits(Oh[:csr.m, off:off + dv], base), (pad, off)
            Oh[:csr.m, off:off + dv] = CANARY
            assert (Oh == CANARY).all(), "written outside O's m x dv elements"
        # each operand on its own side
        Qd, Kd, Vd = (torch.from_numpy(a).to(DEV) for a in (Q, K, V))
        for q, kk, v in ((Qd, K, V), (Q, Kd, V), (Q, K, Vd), (Qd, Kd, V)):
            assert same_bits(fused_host(h, csr, q, kk, v, scale), base)
        # K and V the same pointer (k == dv)
        assert same_bits(fused_host(h, csr, Q, K, K, scale), fused_host(h, csr, Q, K, K.copy(), scale))
        od = h.attention(Qd, Kd, Kd, scale)
        torch.cuda.synchronize()
        assert same_bits(od.cpu().numpy(), fused_host(h, csr, Q, K, K.copy(), scale))
        # an attached stream with async
        s = torch.cuda.Stream()
        h.attach_stream(s.cuda_stream, async_=True)
        with torch.cuda.stream(s):
            o = h.attention(Qd, Kd, Vd, scale)                                      # Handle.attention allocates O like Q
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert tuple(o.shape) == (csr.m, dv) and same_bits(o.cpu().numpy(), base)
        assert same_bits(fused_host(h, csr, Q, K, V, scale), base)                  # host operands on an asynchronous handle
        want_default = fused_host(h, csr, Q, K, V, None)
    for method in METHODS:
        with handle(csr, method) as h:
            assert same_bits(fused_host(h, csr, Q, K, V, scale), base), method
            assert same_bits(h.attention(Q, K, V), want_default), method            # scale=None: 1 / sqrt(k)
    assert same_bits(want_default, _default_scale(csr, Q, K, V))


def _default_scale(csr, Q, K, V):
    with handle(csr) as h:
        return fused_host(h, csr, Q, K, V, 1.0 / np.sqrt(Q.shape[1]))


# ----------------------------------------------------------------------------- 4. memory rules
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_memory_rules(dtype):
    import torch
    csr = pattern(dtype)
    s = np.dtype(dtype).itemsize
    k, dv = 9, 7
    Q, K, V = operands(csr, k, dv)
    lens = np.diff(csr.rowptr)
    nlong, long_sum = int((lens > 512).sum()), int(lens[lens > 512].sum())
    nb = -(-csr.nnz // 2048)
    tables = 4 * (nb + 1) + 4 * nlong + 4 * (nlong + 1) + s * long_sum   # spmm's batch table and long-row list, the parked rows' offsets and space
    staging = s * (csr.m * k + csr.n * k + csr.n * dv + csr.m * dv)
    x = np.random.default_rng(1).uniform(-1, 1, csr.n).astype(dtype)
    for method in (M.Method_Parallel, M.Method_CSR5SPMV):
        for opts in ({"keep_columns": 1}, {"keep_columns": 0}):
            with handle(csr, method, **opts) as h:
                y0 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
                b0 = h.info()["device_bytes"]
                Qd, Kd, Vd = (torch.from_numpy(a).to(DEV) for a in (Q, K, V))
                od = h.attention(Qd, Kd, Vd, 0.5)
                torch.cuda.synchronize()
                b1 = h.info()["device_bytes"]
                restored = 4 * (csr.nnz + STREAM_PAD)
                assert b1 - b0 in ((tables,) if opts["keep_columns"] else (tables, tables + restored)), (method, opts, b1 - b0, tables)
                bits = [a.tobytes() for a in (Q, K, V, csr.rowptr, csr.colidx, csr.val)]
                out = fused_host(h, csr, Q, K, V, 0.5)
                assert h.info()["device_bytes"] - b1 == staging, (method, opts)
                assert [a.tobytes() for a in (Q, K, V, csr.rowptr, csr.colidx, csr.val)] == bits   # the inputs keep their bits
                assert same_bits(out, od.cpu().numpy())
                assert same_bits(fused_host(h, csr, Q, K, V, 0.5), out) and h.info()["device_bytes"] - b1 == staging   # nothing grows with use
                y1 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
                assert same_bits(y0, y1), "spmv() after the call must multiply the handle's own values"
    with handle(csr) as h:
        assert same_bits(out, fused_host(h, csr, Q, K, V, 0.5))


# ----------------------------------------------------------------------------- 5. golden patterns
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", GOLDENS)
def test_golden_patterns(name, dtype):
    csr = load_golden(f"{name}_{'f64' if dtype == np.float64 else 'f32'}_uniform")[0]
    KP = 16 if dtype == np.float64 else 32
    with handle(csr) as h:
        for k, dv, scale in ((33, 2 * KP + 3, float(dtype(1 / np.sqrt(33)))), (3, 5, 1.0)):
            Q, K, V = operands(csr, k, dv)
            out = fused_host(h, csr, Q, K, V, scale)
            assert same_bits(out, composition(h, csr, Q, K, V, scale)), (k, dv)
            check_accuracy(out, csr, Q, K, V, scale)
            if csr.nnz == 0:
                assert (out == 0).all() and not np.signbit(out).any()


# ----------------------------------------------------------------------------- 6. handle rules
def test_reorder_handle_is_an_argument_error():
    import torch
    lib = api.load()
    m, n, rp, ci, va = synth.banded_holes_device(100_000, 100_000, 24, 0.25, "eighths", torch.float64, DEV, 7)
    api.set_thread_option("reorder", 1)
    try:
        h = api.Handle(m, n, rp, ci, va, M.Method_Parallel)
    finally:
        api.clear_thread_options()
    with h:
        assert h.index is not None
        Q = torch.ones((m, 3), dtype=torch.float64, device=DEV)
        out = torch.full((m, 3), CANARY, dtype=torch.float64, device=DEV)
        lib.spmv_hip_clear_error()
        assert api.attention(h.h, m, rp, ci, va, Q, Q, Q, out, check=False) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all())


def test_errors_leave_o_untouched():
    lib = api.load()
    csr = load_golden("banded_f64_uniform")[0]
    Q, K, V = operands(csr, 4, 3)
    with handle(csr) as h:
        O = np.full((csr.m, 3), CANARY)
        q, kk, v, o = Q.ctypes.data, K.ctypes.data, V.ctypes.data, O.ctypes.data

        def call(k, dv, pq, ldq, pk, ldk, pv, ldv, po, ldo):
            lib.spmv_hip_clear_error()
            return lib.spmv_hip_attention(h.h, csr.m, csr.rowptr.ctypes.data, csr.colidx.ctypes.data, csr.val.ctypes.data, k, dv, 1.0, pq, ldq, pk, ldk, pv, ldv, po, ldo)
        for args in ((0, 3, q, 4, kk, 4, v, 3, o, 3), (4, 0, q, 4, kk, 4, v, 3, o, 3), (4, 3, q, 3, kk, 4, v, 3, o, 3), (4, 3, q, 4, kk, 3, v, 3, o, 3),
                     (4, 3, q, 4, kk, 4, v, 2, o, 3), (4, 3, q, 4, kk, 4, v, 3, o, 2), (4, 3, None, 4, kk, 4, v, 3, o, 3), (4, 3, q, 4, None, 4, v, 3, o, 3),
                     (4, 3, q, 4, kk, 4, None, 3, o, 3), (4, 3, q, 4, kk, 4, v, 3, None, 3)):
            assert call(*args) == E_ARG, args
            assert lib.spmv_hip_last_error() == E_ARG
            assert (O == CANARY).all()
        lib.spmv_hip_clear_error()
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            O = np.full((csr.m, 3), CANARY)
            assert api.attention(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q, K, V, O, check=False) == E_ARG, key
            assert lib.spmv_hip_last_error() == E_ARG
            lib.spmv_hip_clear_error()
            assert (O == CANARY).all()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    O = np.full((csr.m, 3), CANARY)
    assert api.attention(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, Q, K, V, O, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert (O == CANARY).all()
    h.close()


def test_timer_runs_on_device_operands():
    import torch
    csr = pattern(np.float32)
    Q, K, V = (torch.from_numpy(a).to(DEV) for a in operands(csr, 8, 8))
    with handle(csr) as h:
        O = torch.empty((csr.m, 8), dtype=torch.float32, device=DEV)
        mean, ms = api.time_attention_launches(h.h, Q, K, V, O, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        assert same_bits(O.cpu().numpy(), fused_host(h, csr, Q.cpu().numpy(), K.cpu().numpy(), V.cpu().numpy(), 1.0 / np.sqrt(8)))
