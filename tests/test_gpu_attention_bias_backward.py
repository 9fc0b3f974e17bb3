"""GPU: spmv_hip_attention_bias_backward -- dQ, dK, dV and dB of spmv_hip_attention_bias in two passes per group of heads
(include/spmv_hip.h).  Everything is exact: no tolerance anywhere.

1. B = None: dQ, dK and dV have the bits of api.attention_heads_backward.
2. The composition, per head: P = row_softmax(sddmm(Q, K) * scale + B[h]) with the bias added in numpy as a rounding of its own,
   dB = row_softmax_backward(P, sddmm(G, V)), dS = dB * scale, dQ = A_dS K, dK = A_dS^T Q, dV = A_P^T G on second handles holding dS and P
   (outputs with ld = width + 2, so that width 1 does not take the spmv schedule) -- test_gpu_attention_backward.py's composition with the
   bias added to t.
3. Every subset of the four outputs: the same bits, unwanted buffers untouched; only dB wanted builds no transpose.
4. Option "attention_backward_heads" 1 and 2 with three heads: the same bits for all four outputs.
5. lddb = nnz + 3 with canaries between the planes, host and device pointers.
6. -inf entries: dB there is +-0, everything else is the composition's."""
import itertools

import numpy as np
import pytest

from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
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


def small(dtype):
    """a 40-row pattern with an empty row, a row of one entry and rows on both sides of 64; 50 columns"""
    key = ("small", np.dtype(dtype))
    if key not in _PAT:
        rng = np.random.default_rng(4)
        lens = [0, 1, 2, 7, 63, 64, 65, 130] * 5
        rp = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(lens, out=rp[1:])
        ci = rng.integers(0, 50, int(rp[-1])).astype(np.int32)
        _PAT[key] = synth.CSR(len(lens), 50, rp, ci, rng.uniform(-1, 1, int(rp[-1])).astype(dtype))
    return _PAT[key]


def operands(csr, heads, k, dv, seed=0):
    """Q, K (x heads*k), V, G (x heads*dv) uniform in [-1, 1]; B (heads, nnz) uniform in [-2, 2]"""
    rng = np.random.default_rng(1000 * heads + 100 * k + dv + seed)
    dt = csr.val.dtype
    Q, K, V, G = (rng.uniform(-1, 1, shape).astype(dt) for shape in ((csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv), (csr.m, heads * dv)))
    return Q, K, V, G, rng.uniform(-2, 2, (heads, csr.nnz)).astype(dt)


def handle(csr, method=M.Method_Parallel, val=None, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val if val is None else val, method)
    finally:
        api.clear_thread_options()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def all_same(got, want):
    return all((g is None and w is None) or (g is not None and w is not None and same_bits(g, w)) for g, w in zip(got, want))


def bias_bwd_host(h, csr, heads, Q, K, V, B, G, scale, need=(True, True, True, True), pad=3):
    """through host pointers, into canary-filled outputs with `pad` extra elements behind every row / plane and a row / plane behind the last;
    an unwanted output is passed as None; -> (dQ, dK, dV, dB)"""
    dims = ((csr.m, Q.shape[1]), (csr.n, Q.shape[1]), (csr.n, V.shape[1]), (heads, csr.nnz))
    bufs = [np.full((rows + 1, width + pad), CANARY, dtype=csr.val.dtype) if want else None for want, (rows, width) in zip(need, dims)]
    views = [None if b is None else b[:rows, :width] for b, (rows, width) in zip(bufs, dims)]
    api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, B, G, *views, scale=scale)
    for b, v in zip(bufs, views):
        if b is not None:
            assert (b[:, v.shape[1]:] == CANARY).all() and (b[v.shape[0]] == CANARY).all(), "written outside an output's elements"
    return tuple(None if v is None else v.copy() for v in views)


def composition(h, csr, heads, Q, K, V, B, G, scale):
    """the calls the fused one replaces, head by head on the library's kernels; dS and P live on second handles; -> (dQ, dK, dV, dB)"""
    dt = Q.dtype.type
    k, dv = Q.shape[1] // heads, V.shape[1] // heads
    dQ, dK, dV = np.zeros_like(Q), np.zeros_like(K), np.zeros_like(V)
    dB = np.zeros((heads, csr.nnz), dtype=dt)
    for hd in range(heads):
        ck, cv = slice(hd * k, (hd + 1) * k), slice(hd * dv, (hd + 1) * dv)
        with np.errstate(all="ignore"):
            T = h.sddmm(Q[:, ck], K[:, ck]) * dt(scale)
            if B is not None:
                T = T + B[hd]
            P = h.row_softmax(T)
            dB[hd] = h.row_softmax_backward(P, h.sddmm(G[:, cv], V[:, cv]))
            dS = dB[hd] * dt(scale)
        oq, ok, ov = (np.full((rows, w + 2), CANARY, dtype=dt) for rows, w in ((csr.m, k), (csr.n, k), (csr.n, dv)))
        with handle(csr, val=dS) as hs:
            api.spmm(hs.h, csr.m, csr.rowptr, csr.colidx, dS, K[:, ck], oq[:, :k])
            api.spmm_transpose(hs.h, csr.m, csr.rowptr, csr.colidx, dS, Q[:, ck], ok[:, :k])
        with handle(csr, val=P) as hp:
            api.spmm_transpose(hp.h, csr.m, csr.rowptr, csr.colidx, P, G[:, cv], ov[:, :dv])
        dQ[:, ck], dK[:, ck], dV[:, cv] = oq[:, :k], ok[:, :k], ov[:, :dv]
    return dQ, dK, dV, dB


# ----------------------------------------------------------------------------- 1. no bias
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_bias_is_the_heads_backward(dtype, heads):
    csr = pattern(dtype)
    with handle(csr) as h:
        for k, dv in widths(dtype):
            Q, K, V, G, _ = operands(csr, heads, k, dv)
            for scale in (0.125, None):
                want = [np.full_like(a, CANARY) for a in (Q, K, V)]
                api.attention_heads_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, G, *want, scale=scale)
                got = bias_bwd_host(h, csr, heads, Q, K, V, None, G, scale)
                assert all_same(got[:3], want), (k, dv, scale)
                assert all_same(bias_bwd_host(h, csr, heads, Q, K, V, None, G, scale, need=(True, True, True, False)), [*want, None]), (k, dv, scale)
            # dB without a bias is still P (dP - D): the composition's
            assert same_bits(got[3], composition(h, csr, heads, Q, K, V, None, G, float(dtype(1.0 / np.sqrt(k))))[3]), (k, dv)


# ----------------------------------------------------------------------------- 2. the composition
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_equal_the_composition(dtype, heads):
    csr = pattern(dtype)
    with handle(csr) as h:
        for (k, dv), scale in zip(widths(dtype), (1.0, 0.125, 0.5, None)):
            scale = float(dtype(1.0 / np.sqrt(k))) if scale is None else scale
            Q, K, V, G, B = operands(csr, heads, k, dv)
            want = composition(h, csr, heads, Q, K, V, B, G, scale)
            assert not any(np.isnan(w).any() for w in want)
            got = bias_bwd_host(h, csr, heads, Q, K, V, B, G, scale)
            for name, g, w in zip(("dQ", "dK", "dV", "dB"), got, want):
                assert same_bits(g, w), (name, k, dv, scale)
            shared = bias_bwd_host(h, csr, heads, Q, K, V, B[0].copy(), G, scale)   # one plane for all heads: `heads` copies of it
            assert all_same(shared, bias_bwd_host(h, csr, heads, Q, K, V, np.tile(B[0], (heads, 1)), G, scale)), (k, dv)


# ----------------------------------------------------------------------------- 3. every subset of the outputs
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_subset_of_the_outputs(dtype):
    import torch
    csr = small(dtype)
    heads = 2
    k, dv = widths(dtype)[2]
    Q, K, V, G, B = operands(csr, heads, k, dv)
    with handle(csr) as h:
        base = bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.25)
        assert all_same(base, composition(h, csr, heads, Q, K, V, B, G, 0.25))
        dev = [torch.from_numpy(a).to(DEV) for a in (Q, K, V, B, G)]
        for need in itertools.product((True, False), repeat=4):
            assert all_same(bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.25, need=need), [b if n else None for b, n in zip(base, need)]), need
            # device operands; the unwanted outputs' buffers exist, are not passed, and keep their canaries
            outs = [torch.full(b.shape, CANARY, dtype=dev[0].dtype, device=DEV) for b in base]
            api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, dev[0], dev[1], dev[2], dev[3], dev[4],
                                        *(o if n else None for o, n in zip(outs, need)), scale=0.25)
            torch.cuda.synchronize()
            for o, b, n in zip(outs, base, need):
                assert same_bits(o.cpu().numpy(), b) if n else bool((o == CANARY).all()), need
    with handle(csr) as h:   # a fresh handle, only dB wanted: the row pass alone, no transpose
        got = bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.25, need=(False, False, False, True))
        assert same_bits(got[3], base[3])
        with pytest.raises(api.SpmvError):
            api.get_transpose_info(h.h)
        api.load().spmv_hip_clear_error()
        got = bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.25, need=(True, False, False, True))   # dQ as well: still none
        assert all_same(got, [base[0], None, None, base[3]])
        with pytest.raises(api.SpmvError):
            api.get_transpose_info(h.h)
        api.load().spmv_hip_clear_error()
        bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.25, need=(False, True, False, False))
        assert api.get_transpose_info(h.h)["m"] == csr.n


# ----------------------------------------------------------------------------- 4. rounds of heads
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rounds_of_heads_change_no_bit(dtype):
    import torch
    csr = pattern(dtype)
    heads = 3
    k, dv = widths(dtype)[2]
    Q, K, V, G, B = operands(csr, heads, k, dv)
    with handle(csr) as h:
        base = bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.25)
        b_all = h.info()["device_bytes"]
    dev = [torch.from_numpy(a).to(DEV) for a in (Q, K, V, B, G)]
    for hg in (1, 2):
        with handle(csr, attention_backward_heads=hg) as h:
            assert all_same(bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.25), base), hg
            assert all_same(bias_bwd_host(h, csr, heads, Q, K, V, B[1].copy(), G, 0.25),
                            bias_bwd_host(h, csr, heads, Q, K, V, np.tile(B[1], (heads, 1)), G, 0.25)), hg   # a shared plane in every round
            got = h.attention_bias_backward(dev[0], dev[1], dev[2], dev[3], dev[4], heads, 0.25)
            torch.cuda.synchronize()
            assert all_same([g.cpu().numpy() for g in got], base), hg
        with handle(csr, attention_backward_heads=hg) as h, handle(csr, attention_backward_heads=hg) as h0:   # device operands: the no-bias call's memory
            h.attention_bias_backward(dev[0], dev[1], dev[2], dev[3], dev[4], heads, 0.25)
            h0.attention_heads_backward(dev[0], dev[1], dev[2], dev[4], heads, 0.25)
            torch.cuda.synchronize()
            assert h.info()["device_bytes"] == h0.info()["device_bytes"] < b_all, hg


# ----------------------------------------------------------------------------- 5. plane strides and pointer kinds
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_plane_strides_and_pointer_kinds_change_no_bit(dtype):
    import torch
    csr = pattern(dtype)
    heads, nnz = 3, csr.nnz
    k, dv = widths(dtype)[1]
    Q, K, V, G, B = operands(csr, heads, k, dv)
    x = np.random.default_rng(1).uniform(-1, 1, csr.n).astype(dtype)
    with handle(csr) as h:
        y0 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
        base = bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.5)
        assert all_same(bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.5), base)   # the same call twice
        for off in (0, 1):
            # B: ldb = nnz + 5, NaN between the planes; dB: lddb = nnz + 3, canaries between the planes; off: one element into the buffers
            bflat = np.full(off + heads * (nnz + 5), np.nan, dtype=dtype)
            bp = bflat[off:].reshape(heads, nnz + 5)[:, :nnz]
            bp[:] = B
            dflat = np.full(off + (heads + 1) * (nnz + 3), CANARY, dtype=dtype)
            dp = dflat[off:].reshape(heads + 1, nnz + 3)[:heads, :nnz]
            outs = [np.full_like(a, CANARY) for a in (Q, K, V)]
            api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, bp, G, *outs, dp, scale=0.5)
            assert all_same([*outs, dp], base), off
            keep = dp.copy()
            dp[:] = CANARY
            assert (dflat == CANARY).all(), "written outside dB's planes"
            dp[:] = keep
            # the same on the device
            dev = [torch.from_numpy(a).to(DEV) for a in (Q, K, V, G)]
            bd = torch.from_numpy(bflat).to(DEV)
            dd = torch.full((off + (heads + 1) * (nnz + 3),), CANARY, dtype=bd.dtype, device=DEV)
            douts = [torch.full(a.shape, CANARY, dtype=bd.dtype, device=DEV) for a in (Q, K, V)]
            api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, dev[0], dev[1], dev[2],
                                        bd[off:].view(heads, nnz + 5)[:, :nnz], dev[3], *douts, dd[off:].view(heads + 1, nnz + 3)[:heads, :nnz], scale=0.5)
            torch.cuda.synchronize()
            dh = dd.cpu().numpy()
            assert all_same([o.cpu().numpy() for o in douts] + [dh[off:].reshape(heads + 1, nnz + 3)[:heads, :nnz]], base), off
            assert same_bits(dh, dflat), off   # canaries and all
            # host B and dB beside device operands
            dp2 = np.full((heads, nnz), CANARY, dtype=dtype)
            api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, dev[0], dev[1], dev[2], bp, dev[3], dB=dp2, scale=0.5)
            assert same_bits(dp2, base[3]), off
        y1 = h.spmv(x, np.full(csr.m, np.nan, dtype=dtype))
        assert same_bits(y0, y1), "spmv() after the calls must multiply the handle's own values"
        lib = api.load()
        outs = [np.full_like(a, CANARY) for a in (Q, K, V)]
        dB = np.full((heads, nnz), CANARY, dtype=dtype)
        for kw in (dict(ldb=nnz - 1), dict(lddb=nnz - 1), dict(ldb=1)):   # a plane stride below nnz: E_ARG once nnz is known, nothing written
            lib.spmv_hip_clear_error()
            assert api.attention_bias_backward(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, Q, K, V, B, G, *outs, dB, scale=0.5, check=False,
                                               **{"ldb": nnz, "lddb": nnz, **kw}) == E_ARG, kw
            assert lib.spmv_hip_last_error() == E_ARG
            assert all((o == CANARY).all() for o in [*outs, dB]), kw
        lib.spmv_hip_clear_error()


# ----------------------------------------------------------------------------- 6. masks
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masked_entries_have_a_zero_gradient(dtype):
    """-inf on a random third of the entries of every row longer than 1, never all of a row"""
    csr = pattern(dtype)
    rng = np.random.default_rng(9)
    heads = 2
    k, dv = widths(dtype)[2]
    Q, K, V, G, B = operands(csr, heads, k, dv)
    for hd in range(heads):
        for i in np.flatnonzero(np.diff(csr.rowptr) > 1):
            s, e = csr.rowptr[i], csr.rowptr[i + 1]
            mask = rng.random(e - s) < 1 / 3
            mask[rng.integers(0, e - s)] = False
            B[hd, s:e][mask] = -np.inf
    with handle(csr) as h:
        want = composition(h, csr, heads, Q, K, V, B, G, 0.25)
        assert not any(np.isnan(w).any() for w in want)
        got = bias_bwd_host(h, csr, heads, Q, K, V, B, G, 0.25)
    assert (got[3][np.isinf(B)] == 0).all()          # +-0 exactly where the entry is masked
    assert (got[3][~np.isinf(B)] != 0).any()
    for name, g, w in zip(("dQ", "dK", "dV", "dB"), got, want):
        assert same_bits(g, w), name


def test_timer_runs_on_device_operands():
    import torch
    csr = pattern(np.float32)
    heads, k, dv = 2, 8, 8
    host = operands(csr, heads, k, dv)
    Q, K, V, G, B = (torch.from_numpy(a).to(DEV) for a in host)
    with handle(csr) as h:
        outs = [torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V), torch.empty_like(B)]
        mean, ms = api.time_attention_bias_backward_launches(h.h, heads, Q, K, V, B, G, *outs, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        want = bias_bwd_host(h, csr, heads, *host[:3], host[4], host[3], 1.0 / np.sqrt(k))
        assert all_same([o.cpu().numpy() for o in outs], want)
        with pytest.raises(api.SpmvError):   # device pointers only
            api.time_attention_bias_backward_launches(h.h, heads, Q, K, V, host[4], G, *outs, warmup=0, iters=1)
