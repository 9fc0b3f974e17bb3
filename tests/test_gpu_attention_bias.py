"""GPU: spmv_hip_attention_bias -- spmv_hip_attention_heads with an additive bias per head and stored entry, t = (s * scale) + B
(include/spmv_hip.h).  Everything is exact: no tolerance anywhere.

1. B = None: the bits of api.attention_heads.
2. The composition oracle, per head: api.sddmm -> numpy `s * scale`, then `+ B[h]` as two separately rounded numpy operations ->
   api.row_softmax -> spmm with values P (update_values, ld = dv + 2 so that width 1 does not take the spmv schedule; the handle's own values
   are put back afterwards).  Bias uniform in [-2, 2].
3. A shared plane (ldb = 0) equals `heads` copies of it.
4. ldb = nnz + 5 with NaN between the planes, base pointers one element in, host and device B, every method, an attached stream, the same
   call twice: the same bits.
5. Masks: -inf on a third of the entries against the composition; one row fully masked in one head is NaN there and nowhere else.
6. Memory and side effects.   7. Errors."""
import numpy as np
import pytest

from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
METHODS = [M.Method_Parallel, M.Method_Balanced, M.Method_Balanced_Yid, M.Method_CSR5SPMV, M.Method_SellCSigma]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
HEADS = [1, 2, 3]
E_ARG = 3
DEV = "cuda:0"
CANARY = -7.25
N = 300
# both sides of: the lane groups (1 .. 64), the register chain (64 per step), the long-row threshold and the LDS chunk (512), the chunk's
# packing of several rows (575 .. 577 beside their neighbours), the 2048 batch and the 64-segment split (ceil(len / 64) changes at 4097)
LENGTHS = [0, 1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64, 65, 511, 512, 513, 575, 576, 577, 1025, 2047, 2048, 2049, 4097, 5000]


def widths(dtype):
    """(k, dv) of ONE head: width 1; the 16-byte unit; one element more (head bases misaligned); more than a chunk of columns and two panels"""
    W, KP = (2, 16) if np.dtype(dtype) == np.float64 else (4, 32)
    return [(1, 1), (W, 16 // np.dtype(dtype).itemsize), (W + 1, KP + 1), (8 * W + 1, 2 * KP + 3)]


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


def operands(csr, heads, k, dv, seed=0):
    """Q (m x heads*k), K (n x heads*k), V (n x heads*dv) uniform in [-1, 1]; B (heads, nnz) uniform in [-2, 2]"""
    rng = np.random.default_rng(1000 * heads + 100 * k + dv + seed)
    dt = csr.val.dtype
    return (rng.uniform(-1, 1, (csr.m, heads * k)).astype(dt), rng.uniform(-1, 1, (csr.n, heads * k)).astype(dt),
            rng.uniform(-1, 1, (csr.n, heads * dv)).astype(dt), rng.uniform(-2, 2, (heads, csr.nnz)).astype(dt))


def handle(csr, method=M.Method_Parallel, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method)
    finally:
        api.clear_thread_options()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_bits(out, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan)
    assert same_bits(out[~nan], want[~nan])


def bias_host(h, csr, heads, Q, K, V, B, scale, pad=3, **kw):
    """the bias call through host pointers (B may be anything api.attention_bias takes), into a canary-filled O with `pad` extra elements
    behind every row and a row behind the last"""
    w = V.shape[1]
    buf = np.full((csr.m + 1, w + pad), CANARY, dtype=csr.val.dtype)
    api.attention_bias(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, B, buf[:csr.m, :w], scale, **kw)
    assert (buf[:, w:] == CANARY).all() and (buf[csr.m] == CANARY).all(), "written outside O's m x heads*dv elements"
    return buf[:csr.m, :w].copy()


def composition(h, csr, heads, Q, K, V, B, scale):
    """the calls the fused one replaces, head by head on the library's kernels, the bias added in numpy after the scaling: two roundings.  P
    becomes the handle's values for the product; the handle's own values come back afterwards."""
    dt = Q.dtype.type
    k, dv = Q.shape[1] // heads, V.shape[1] // heads
    out = np.zeros((csr.m, heads * dv), dtype=dt)
    if csr.nnz == 0:
        return out
    try:
        for hd in range(heads):
            ck, cv = slice(hd * k, (hd + 1) * k), slice(hd * dv, (hd + 1) * dv)
            S = h.sddmm(Q[:, ck], K[:, ck])
            with np.errstate(all="ignore"):
                T = S * dt(scale)
                T = T + B[hd]
            P = h.row_softmax(T)
            Y = np.full((csr.m, dv + 2), CANARY, dtype=dt)   # ld = dv + 2: width 1 does not take the spmv schedule
            h.update_values(P)
            api.spmm(h.h, csr.m, csr.rowptr, csr.colidx, P, V[:, cv], Y[:, :dv])
            out[:, cv] = Y[:, :dv]
    finally:
        h.update_values(csr.val)
    return out


# ----------------------------------------------------------------------------- 1. no bias
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_bias_is_the_heads_call(dtype, heads):
    import torch
    csr = pattern(dtype)
    with handle(csr) as h:
        for k, dv in widths(dtype):
            Q, K, V, _ = operands(csr, heads, k, dv)
            for scale in (0.125, None):
                want = np.full((csr.m, heads * dv), CANARY, dtype=dtype)
                api.attention_heads(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, want, scale)
                assert same_bits(bias_host(h, csr, heads, Q, K, V, None, scale), want), (k, dv, scale)
                assert same_bits(bias_host(h, csr, heads, Q, K, V, None, scale, ldb=12345), want), (k, dv, scale)   # ldb is ignored
            Qd, Kd, Vd = (torch.from_numpy(a).to(DEV) for a in (Q, K, V))
            od = h.attention_bias(Qd, Kd, Vd, heads, None)
            torch.cuda.synchronize()
            assert same_bits(od.cpu().numpy(), want), (k, dv)


# ----------------------------------------------------------------------------- 2. the composition
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_equal_the_composition(dtype, heads):
    csr = pattern(dtype)
    lens = np.diff(csr.rowptr)
    with handle(csr) as h:
        for k, dv in widths(dtype):
            Q, K, V, B = operands(csr, heads, k, dv)
            for scale in (0.125, float(dtype(1.0 / np.sqrt(k)))):
                want = composition(h, csr, heads, Q, K, V, B, scale)
                assert not np.isnan(want).any()
                out = bias_host(h, csr, heads, Q, K, V, B, scale)
                assert same_bits(out, want), (k, dv, scale)
                assert (out[lens == 0] == 0).all() and not np.signbit(out[lens == 0]).any()   # empty rows: +0 in every head
            nobias = bias_host(h, csr, heads, Q, K, V, None, 0.125)
            assert not same_bits(nobias, bias_host(h, csr, heads, Q, K, V, B, 0.125))         # the bias is not ignored


# ----------------------------------------------------------------------------- 3. a shared plane
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shared_plane_equals_copies(dtype):
    import torch
    csr = pattern(dtype)
    with handle(csr) as h:
        for heads in (2, 3):
            for k, dv in widths(dtype)[1:3]:
                Q, K, V, B = operands(csr, heads, k, dv)
                want = bias_host(h, csr, heads, Q, K, V, np.tile(B[0], (heads, 1)), 0.25)
                assert same_bits(bias_host(h, csr, heads, Q, K, V, B[0].copy(), 0.25), want), (heads, k, dv)
                Qd, Kd, Vd, bd = (torch.from_numpy(a).to(DEV) for a in (Q, K, V, B[0].copy()))
                od = h.attention_bias(Qd, Kd, Vd, heads, bd, 0.25)
                torch.cuda.synchronize()
                assert same_bits(od.cpu().numpy(), want), (heads, k, dv)
        # the handle's own values as the bias (edge weights): only read
        Q, K, V, _ = operands(csr, 2, 3, 3)
        val = csr.val.copy()
        want = bias_host(h, csr, 2, Q, K, V, val, 0.5)
        assert same_bits(bias_host(h, csr, 2, Q, K, V, csr.val, 0.5), want) and same_bits(csr.val, val)


# ----------------------------------------------------------------------------- 4. layout, pointer kinds, settings
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_plane_stride_pointer_kind_method_and_stream_change_no_bit(dtype):
    import torch
    csr = pattern(dtype)
    heads, nnz = 3, csr.nnz
    k, dv = widths(dtype)[2]
    Q, K, V, B = operands(csr, heads, k, dv)
    scale = 0.125
    with handle(csr) as h:
        base = bias_host(h, csr, heads, Q, K, V, B, scale)
        assert same_bits(base, composition(h, csr, heads, Q, K, V, B, scale))
        assert same_bits(bias_host(h, csr, heads, Q, K, V, B, scale), base)                  # the same call twice
        for off in (0, 1):   # ldb = nnz + 5 with NaN between the planes; off: the first plane that many elements into the buffer
            flat = np.full(off + heads * (nnz + 5), np.nan, dtype=dtype)
            planes = flat[off:].reshape(heads, nnz + 5)[:, :nnz]
            planes[:] = B
            assert same_bits(bias_host(h, csr, heads, Q, K, V, planes, scale), base), off    # host B
            fd = torch.from_numpy(flat).to(DEV)
            pd = fd[off:].view(heads, nnz + 5)[:, :nnz]
            assert same_bits(bias_host(h, csr, heads, Q, K, V, pd, scale), base), off        # device B, host Q, K, V, O
            Qd, Kd, Vd = (torch.from_numpy(a).to(DEV) for a in (Q, K, V))
            od = h.attention_bias(Qd, Kd, Vd, heads, pd, scale)                              # all on the device
            od2 = h.attention_bias(Qd, Kd, Vd, heads, torch.from_numpy(B).to(DEV), scale)
            od3 = h.attention_bias(Qd, Kd, Vd, heads, planes, scale)                         # host B beside device operands
            torch.cuda.synchronize()
            assert same_bits(od.cpu().numpy(), base) and same_bits(od2.cpu().numpy(), base) and same_bits(od3.cpu().numpy(), base), off
            assert np.isnan(flat).sum() == off + heads * 5 and same_bits(planes, B)          # B is only read
        s = torch.cuda.Stream()
        h.attach_stream(s.cuda_stream, async_=True)
        with torch.cuda.stream(s):
            o = h.attention_bias(Qd, Kd, Vd, heads, pd, scale)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert same_bits(o.cpu().numpy(), base)
        assert same_bits(bias_host(h, csr, heads, Q, K, V, B, scale), base)                  # host operands on an asynchronous handle
    for method in METHODS:
        with handle(csr, method) as h:
            assert same_bits(bias_host(h, csr, heads, Q, K, V, B, scale), base), method


# ----------------------------------------------------------------------------- 5. masks
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masked_entries_weigh_nothing(dtype):
    """-inf on a random third of the entries of every row longer than 1, never all of a row"""
    csr = pattern(dtype)
    rng = np.random.default_rng(9)
    heads = 2
    k, dv = widths(dtype)[2]
    Q, K, V, B = operands(csr, heads, k, dv)
    for hd in range(heads):
        for i in np.flatnonzero(np.diff(csr.rowptr) > 1):
            s, e = csr.rowptr[i], csr.rowptr[i + 1]
            mask = rng.random(e - s) < 1 / 3
            mask[rng.integers(0, e - s)] = False
            B[hd, s:e][mask] = -np.inf
    with handle(csr) as h:
        want = composition(h, csr, heads, Q, K, V, B, 0.25)
        assert not np.isnan(want).any()
        assert same_bits(bias_host(h, csr, heads, Q, K, V, B, 0.25), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_fully_masked_row_is_nan_in_its_head_only(dtype):
    csr = pattern(dtype)
    lens = np.diff(csr.rowptr)
    heads, dv = 3, 5
    Q, K, V, B = operands(csr, heads, 3, dv)
    with handle(csr) as h:
        clean = bias_host(h, csr, heads, Q, K, V, B, 0.5)
        for n in (1, 65, 513, 5000):   # a row of each kind of pass, short and long
            r = int(np.flatnonzero(lens == n)[0])
            Bm = B.copy()
            Bm[1, csr.rowptr[r]:csr.rowptr[r + 1]] = -np.inf
            out = bias_host(h, csr, heads, Q, K, V, Bm, 0.5)
            nan = np.zeros_like(out, dtype=bool)
            nan[r, dv:2 * dv] = True
            assert np.array_equal(np.isnan(out), nan), n
            assert same_bits(out[~nan], clean[~nan]), n
        for bad in (np.nan, np.inf):   # a NaN or +inf bias: the same rule
            r = int(np.flatnonzero(lens == 577)[0])
            Bm = B.copy()
            Bm[2, csr.rowptr[r] + 300] = bad
            out = bias_host(h, csr, heads, Q, K, V, Bm, 0.5)
            nan = np.zeros_like(out, dtype=bool)
            nan[r, 2 * dv:] = True
            assert np.array_equal(np.isnan(out), nan), bad
            assert same_bits(out[~nan], clean[~nan]), bad


# ----------------------------------------------------------------------------- 6. memory and side effects
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_memory_and_side_effects(dtype):
    import torch
    csr = pattern(dtype)
    heads, k, dv = 3, 4, 8
    Q, K, V, B = operands(csr, heads, k, dv)
    x = np.random.default_rng(1).uniform(-1, 1, csr.n).astype(dtype)
    Qd, Kd, Vd, Bd = (torch.from_numpy(a).to(DEV) for a in (Q, K, V, B))
    for keep in (1, 0):
        grown = {}
        for bias in (Bd, None):
            with handle(csr, keep_columns=keep) as h:
                y0 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
                b0 = h.info()["device_bytes"]
                od = h.attention_bias(Qd, Kd, Vd, heads, bias, 0.5) if bias is not None else h.attention_heads(Qd, Kd, Vd, heads, 0.5)
                torch.cuda.synchronize()
                grown[bias is not None] = h.info()["device_bytes"] - b0
                od2 = h.attention_bias(Qd, Kd, Vd, heads, bias, 0.5)
                torch.cuda.synchronize()
                assert h.info()["device_bytes"] - b0 == grown[bias is not None]   # once: nothing grows with use
                assert same_bits(od.cpu().numpy(), od2.cpu().numpy())
                y1 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
                assert same_bits(y0, y1), "spmv() after the call must multiply the handle's own values"
        assert grown[True] == grown[False], (keep, grown)   # device operands: nothing over the no-bias call
    with handle(csr) as h:   # a host B is staged: its planes, packed, and nothing else
        b0 = h.info()["device_bytes"]
        h.attention_heads(Qd, Kd, Vd, heads, 0.5)
        b1 = h.info()["device_bytes"]
        h.attention_bias(Qd, Kd, Vd, heads, B, 0.5)
        assert h.info()["device_bytes"] - b1 == heads * csr.nnz * np.dtype(dtype).itemsize
        h.attention_bias(Qd, Kd, Vd, heads, B[0].copy(), 0.5)
        assert h.info()["device_bytes"] - b1 == heads * csr.nnz * np.dtype(dtype).itemsize and b1 > b0


# ----------------------------------------------------------------------------- 7. errors
def test_a_plane_stride_below_nnz_is_an_argument_error():
    import torch
    lib = api.load()
    csr = pattern(np.float64)
    heads, k, dv = 2, 4, 3
    Q, K, V, B = operands(csr, heads, k, dv)
    with handle(csr) as h:
        O = np.full((csr.m, heads * dv), CANARY)
        Od = torch.full((csr.m, heads * dv), CANARY, dtype=torch.float64, device=DEV)
        for ldb in (1, csr.nnz - 1):
            for out in (O, Od):
                lib.spmv_hip_clear_error()
                assert api.attention_bias(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, B, out, 1.0, check=False, ldb=ldb) == E_ARG, ldb
                assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
        torch.cuda.synchronize()
        assert (O == CANARY).all() and bool((Od == CANARY).all())
        assert api.attention_bias(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, B, O, 1.0, ldb=csr.nnz) == 0   # nnz itself is fine
        assert not (O == CANARY).any()


def test_timer_runs_on_device_operands():
    import torch
    csr = pattern(np.float32)
    heads, k, dv = 2, 8, 8
    Qh, Kh, Vh, Bh = operands(csr, heads, k, dv)
    Q, K, V, B = (torch.from_numpy(a).to(DEV) for a in (Qh, Kh, Vh, Bh))
    with handle(csr) as h:
        O = torch.empty((csr.m, heads * dv), dtype=torch.float32, device=DEV)
        mean, ms = api.time_attention_bias_launches(h.h, heads, Q, K, V, B, O, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        assert same_bits(O.cpu().numpy(), bias_host(h, csr, heads, Qh, Kh, Vh, Bh, 1.0 / np.sqrt(k)))
        with pytest.raises(api.SpmvError):   # device pointers only
            api.time_attention_bias_launches(h.h, heads, Q, K, V, Bh, O, warmup=0, iters=1)
