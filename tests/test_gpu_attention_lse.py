"""GPU: spmv_hip_attention_gqa_lse -- the forward pass that also returns the rows' log-sum-exps L = M + log Z (include/spmv_hip.h).

O has no tolerance: it is spmv_hip_attention_gqa's, to the bit.  L's bits are compared across everything that must not change them; its VALUE
is compared with a log-sum-exp in np.longdouble of the very scores the kernel holds, under the bound derived in lse_cases.py (l_bound).

1. O's bits, L = None, the writes   2. what changes no bit of L   3. special values   4. goldens, m = 0   5. the value of L   6. handle rules, the timer"""
import numpy as np
import pytest

from conftest import load_golden
from gqa_cases import (BIASES, CANARY, COMBOS, COMBO_IDS, DEV, DTYPES, E_ARG, E_NOSTATE, IDS, METHODS, M, bias_of, device_ops, gqa_host, handle, operands, pattern_a, plane,
                       same_bits, shapes)
from lse_cases import l_bound, l_reference, lse_host, lse_restated, scores
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


# ----------------------------------------------------------------------------- 1. O's bits, L = None, the writes
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_o_has_the_gqa_calls_bits_and_l_is_written_exactly(dtype, combo):
    """over COMBOS x BIASES x shapes x dtypes: O bit-equal to attention_gqa; L = None is attention_gqa; exactly m elements per plane are written
    with a padded ldl (lse_host's canaries); rows without entries get -inf and every other row a finite value"""
    heads, kv = combo
    csr = pattern_a(dtype)
    empty = np.diff(csr.rowptr) == 0
    with handle(csr) as h:
        for k, dv in shapes(dtype):
            Q, K, V, _ = operands(csr, heads, kv, k, dv)
            scale = float(dtype(1.0 / np.sqrt(k)))
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                want = gqa_host(h, csr, heads, kv, Q, K, V, B, scale)
                O, L = lse_host(h, csr, heads, kv, Q, K, V, B, scale)
                assert same_bits(O, want), (heads, kv, k, dv, kind)
                assert (L[:, empty] == -np.inf).all() and np.isfinite(L[:, ~empty]).all()
                O2, none = lse_host(h, csr, heads, kv, Q, K, V, B, scale, want_l=False)
                assert none is None and same_bits(O2, want)


# ----------------------------------------------------------------------------- 2. what changes no bit of L
def _wide(arrays, dtype, pad, off):
    wide, views = [], []
    for a in arrays:
        wd = np.full((a.shape[0], a.shape[1] + pad + off), np.nan, dtype=dtype)
        wd[:, off:off + a.shape[1]] = a
        wide.append(wd)
        views.append(wd[:, off:off + a.shape[1]])
    return wide, views


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pointer_kind_layout_method_and_stream_change_no_bit_of_l(dtype):
    import torch
    csr = pattern_a(dtype)
    s = np.dtype(dtype).itemsize
    heads, kv, k, dv = 6, 2, 3 * (16 // s), 2 * (16 // s)   # k * s and dv * s multiples of 16: aligned operands take the 16-byte form
    Q, K, V, _ = operands(csr, heads, kv, k, dv)
    B = bias_of(csr, heads, "planes")
    scale = 0.125
    with handle(csr) as h:
        O0, L0 = lse_host(h, csr, heads, kv, Q, K, V, B, scale, pad=0)
        assert same_bits(O0, gqa_host(h, csr, heads, kv, Q, K, V, B, scale))
        for pad, off in ((4, 0), (1, 0), (3, 0), (0, 1), (1, 1), (2, 2)):   # padded and unaligned ld: the 16-byte and the element form
            wide, views = _wide((Q, K, V), dtype, pad, off)
            O, L = lse_host(h, csr, heads, kv, *views, B, scale, pad=pad + off)
            assert same_bits(O, O0) and same_bits(L, L0), (pad, off)
            dev = [torch.from_numpy(wd).to(DEV)[:, off:off + v.shape[1]] for wd, v in zip(wide, views)]
            Od = torch.full((csr.m + 1, heads * dv + pad + off), CANARY, dtype=dev[0].dtype, device=DEV)
            Ld = torch.full((heads + 1, csr.m + pad + off), CANARY, dtype=dev[0].dtype, device=DEV)
            api.attention_gqa_lse(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, *dev, torch.from_numpy(B).to(DEV), Od[:csr.m, off:off + heads * dv],
                                  Ld[:heads, off:off + csr.m], scale=scale)
            torch.cuda.synchronize()
            lh, oh = Ld.cpu().numpy(), Od.cpu().numpy()
            assert same_bits(lh[:heads, off:off + csr.m], L0) and same_bits(oh[:csr.m, off:off + heads * dv], O0), (pad, off)
            lh[:heads, off:off + csr.m] = CANARY
            oh[:csr.m, off:off + heads * dv] = CANARY
            assert (lh == CANARY).all() and (oh == CANARY).all(), "written outside the outputs' elements"
        ops = device_ops((Q, K, V))
        for mix in ((ops[0], K, V), (Q, ops[1], V), (Q, K, ops[2])):   # each operand on its own side
            assert same_bits(lse_host(h, csr, heads, kv, *mix, B, scale)[1], L0)
        st = torch.cuda.Stream()                                       # a non-default stream with async
        h.attach_stream(st.cuda_stream, async_=True)
        with torch.cuda.stream(st):
            Od, Ld = h.attention_gqa_lse(*ops, heads, kv, torch.from_numpy(B).to(DEV), scale)
        assert api.load().spmv_hip_synchronize(h.h) == 0
        assert tuple(Ld.shape) == (heads, csr.m) and same_bits(Ld.cpu().numpy(), L0) and same_bits(Od.cpu().numpy(), O0)
        assert same_bits(lse_host(h, csr, heads, kv, Q, K, V, B, scale)[1], L0)   # host operands on an asynchronous handle
    for method in METHODS:
        with handle(csr, method) as h:
            assert same_bits(lse_host(h, csr, heads, kv, Q, K, V, B, scale)[1], L0), method


@pytest.mark.parametrize("combo", [(4, 2), (6, 2), (3, 3)], ids=["4over2", "6over2", "3over3"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_head_has_the_one_head_calls_l(dtype, combo):
    """head h of an H-head call versus the one-head call on its slices: the same bits of L (and of O)"""
    heads, kv = combo
    gs = heads // kv
    csr = pattern_a(dtype)
    with handle(csr) as h:
        for k, dv in shapes(dtype)[1:]:
            Q, K, V, _ = operands(csr, heads, kv, k, dv)
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                O, L = lse_host(h, csr, heads, kv, Q, K, V, B, 0.5)
                for hd in range(heads):
                    g = hd // gs
                    O1, L1 = lse_host(h, csr, 1, 1, Q[:, hd * k:(hd + 1) * k], K[:, g * k:(g + 1) * k], V[:, g * dv:(g + 1) * dv], plane(B, hd), 0.5)
                    assert same_bits(L1[0], L[hd]) and same_bits(O1, O[:, hd * dv:(hd + 1) * dv]), (k, dv, kind, hd)


# ----------------------------------------------------------------------------- 3. special values
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values_give_nan_in_l_for_their_row_and_head_only(dtype):
    """heads = 4 over 2: a NaN in Q of head 1 on a short and a long row; head 2's bias all -inf on every row; a +inf bias on one entry of a short
    and of a long row of head 3.  L is NaN exactly where O's row is, and head 0 is finite throughout"""
    csr = pattern_a(dtype)
    heads, kv, k, dv = 4, 2, 3, 5
    Q, K, V, _ = operands(csr, heads, kv, k, dv)
    B = bias_of(csr, heads, "planes")
    lens = np.diff(csr.rowptr)
    rows = [int(np.flatnonzero(lens == n)[0]) for n in (3, 1025)]   # a short row and a long one
    inf_rows = [int(np.flatnonzero(lens == n)[0]) for n in (17, 2049)]
    Q[rows, 1 * k] = np.nan
    B[2] = -np.inf
    for r in inf_rows:
        B[3, csr.rowptr[r] + 1] = np.inf
    with handle(csr) as h:
        O, L = lse_host(h, csr, heads, kv, Q, K, V, B, 1.0)
    nan_l = np.isnan(L)
    for hd in range(heads):
        assert np.array_equal(nan_l[hd], np.isnan(O[:, hd * dv:(hd + 1) * dv]).all(axis=1)), hd
        assert np.array_equal(nan_l[hd], np.isnan(O[:, hd * dv:(hd + 1) * dv]).any(axis=1)), hd
    assert not nan_l[0].any()
    assert sorted(np.flatnonzero(nan_l[1]).tolist()) == sorted(rows)
    assert np.array_equal(nan_l[2], lens > 0) and (L[2, lens == 0] == -np.inf).all()
    assert sorted(np.flatnonzero(nan_l[3]).tolist()) == sorted(inf_rows)
    assert np.isfinite(L[:, lens > 0][~nan_l[:, lens > 0]]).all()


# ----------------------------------------------------------------------------- 4. goldens, m = 0
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["nnz0", "tiny"])
def test_golden_patterns(name, dtype):
    csr = load_golden(f"{name}_{'f64' if dtype == np.float64 else 'f32'}_uniform")[0]
    heads, kv, k, dv = 6, 2, 3, 2
    Q, K, V, _ = operands(csr, heads, kv, k, dv)
    with handle(csr) as h:
        for kind in ("none", "planes"):
            B = bias_of(csr, heads, kind)
            O, L = lse_host(h, csr, heads, kv, Q, K, V, B, 0.5)
            assert same_bits(O, gqa_host(h, csr, heads, kv, Q, K, V, B, 0.5))
            lens = np.diff(csr.rowptr)
            assert (L[:, lens == 0] == -np.inf).all() and np.isfinite(L[:, lens > 0]).all()
            if csr.nnz == 0:
                assert (L == -np.inf).all() and (O == 0).all() and not np.signbit(O).any()
            else:
                for hd in range(heads):
                    g = hd // (heads // kv)
                    t = scores(h, csr, Q[:, hd * k:(hd + 1) * k], K[:, g * k:(g + 1) * k], plane(B, hd), 0.5)
                    ref = l_reference(csr, t)
                    for i in np.flatnonzero(lens):
                        assert abs(np.longdouble(L[hd, i]) - ref[i]) <= l_bound(int(lens[i]), ref[i], dtype), (hd, i)


def test_m0_is_no_work():
    n, heads, kv, k, dv = 70, 4, 2, 3, 5
    csr = synth.CSR(0, n, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    rng = np.random.default_rng(3)
    Q = np.zeros((0, heads * k))
    K, V = rng.uniform(-1, 1, (n, kv * k)), rng.uniform(-1, 1, (n, kv * dv))
    with handle(csr) as h:
        O, L = lse_host(h, csr, heads, kv, Q, K, V, None, 1.0)   # the canaries: nothing is written
        assert O.shape == (0, heads * dv) and L.shape == (heads, 0)


# ----------------------------------------------------------------------------- 5. the value of L
@pytest.mark.parametrize("kind", BIASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_l_is_the_log_sum_exp_of_the_kernels_scores(dtype, kind):
    """|L - L_ref| <= (a(len) + c(len)) * eps * max(1, |L_ref|) on every row of pattern A (lengths 1 .. 5000), every shape, grouped heads.  L_ref is
    the log-sum-exp in np.longdouble of t_p = api.sddmm * scale + B, computed in the handle's dtype: by contract the kernel's own bits.  The bound
    is derived, not measured -- the derivation is the comment above lse_cases.l_bound: a(len) additions on the longest path of the documented
    order, c(len) = ln(len) / 2 (the subtraction) + 3 (exp) + 3 max(1, ln len) (log) + 1 / 2 (the addition), exp and log at the OpenCL C
    specification's 3 ulp since the installed ROCm carries no accuracy table of its own."""
    heads, kv = 4, 2
    csr = pattern_a(dtype)
    lens = np.diff(csr.rowptr)
    worst = 0.0
    with handle(csr) as h:
        for k, dv in shapes(dtype):
            Q, K, V, _ = operands(csr, heads, kv, k, dv)
            scale = float(dtype(1.0 / np.sqrt(k)))
            B = bias_of(csr, heads, kind)
            _, L = lse_host(h, csr, heads, kv, Q, K, V, B, scale)
            for hd in range(heads):
                g = hd // (heads // kv)
                t = scores(h, csr, Q[:, hd * k:(hd + 1) * k], K[:, g * k:(g + 1) * k], plane(B, hd), scale)
                ref = l_reference(csr, t)
                for i in np.flatnonzero(lens):
                    e, b = abs(np.longdouble(L[hd, i]) - ref[i]), l_bound(int(lens[i]), ref[i], dtype)
                    worst = max(worst, float(e / b))
                    assert e <= b, (k, dv, hd, i, int(lens[i]), float(e), b)
    print(f"L: worst error / bound = {worst:.3f}")


def test_the_restated_order_gives_the_kernels_bits_up_to_the_library():
    """fp32: the documented order restated in numpy (lse_cases.lse_restated, numpy's exp and log in place of the device's) is within the bound of
    the kernel's L -- twice the bound, each side being within one of the reference"""
    dtype = np.float32
    csr = pattern_a(dtype)
    lens = np.diff(csr.rowptr)
    Q, K, V, _ = operands(csr, 1, 1, 5, 4)
    with handle(csr) as h:
        _, L = lse_host(h, csr, 1, 1, Q, K, V, None, 0.5)
        t = scores(h, csr, Q, K, None, 0.5)
    ref = l_reference(csr, t)
    for i in np.flatnonzero(lens):
        mine = lse_restated(t[csr.rowptr[i]:csr.rowptr[i + 1]])
        b = l_bound(int(lens[i]), ref[i], dtype)
        assert abs(np.longdouble(mine) - ref[i]) <= b and abs(np.float64(mine) - np.float64(L[0, i])) <= 2 * b, i


# ----------------------------------------------------------------------------- 6. handle rules, the timer
def test_handle_rules():
    import torch
    lib = api.load()
    csr = load_golden("banded_f64_uniform")[0]
    heads, kv, k, dv = 4, 2, 3, 2
    Q, K, V, _ = operands(csr, heads, kv, k, dv)
    O, L = np.full((csr.m, heads * dv), CANARY), np.full((heads, csr.m), CANARY)
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, csr.n)
    with handle(csr) as h:
        y0 = h.spmv(x, np.full(csr.m, np.nan))
        # found before the handle is looked at: planes closer than m; found once it is: a bias plane stride below nnz -- outputs untouched
        assert api.attention_gqa_lse(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, O, L, check=False, ldl=csr.m - 1) == E_ARG
        lib.spmv_hip_clear_error()
        assert api.attention_gqa_lse(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, np.zeros(heads * csr.nnz), O, L, check=False, ldb=csr.nnz - 1) == E_ARG
        lib.spmv_hip_clear_error()
        assert (O == CANARY).all() and (L == CANARY).all()
        got, _ = lse_host(h, csr, heads, kv, Q, K, V, None, 0.5)
        assert same_bits(got, gqa_host(h, csr, heads, kv, Q, K, V, None, 0.5))
        assert same_bits(h.spmv(x, np.full(csr.m, np.nan)), y0)          # the resident values are not touched
        # device operands: device_bytes is attention_gqa's
        ops = device_ops((Q, K, V))
        h.attention_gqa(*ops, heads, kv, None, 0.5)
        torch.cuda.synchronize()
        b1 = h.info()["device_bytes"]
        h.attention_gqa_lse(*ops, heads, kv, None, 0.5)
        torch.cuda.synchronize()
        assert h.info()["device_bytes"] == b1
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            assert api.attention_gqa_lse(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, O, L, check=False) == E_ARG, key
            lib.spmv_hip_clear_error()
            assert (O == CANARY).all() and (L == CANARY).all()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert api.attention_gqa_lse(h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, O, L, check=False) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert (O == CANARY).all() and (L == CANARY).all()
    h.close()


def test_timer_runs_on_device_operands_and_leaves_the_calls_bits():
    import torch
    lib = api.load()
    csr = pattern_a(np.float32)
    heads, kv = 4, 2
    Q, K, V, _ = operands(csr, heads, kv, 8, 8)
    B = bias_of(csr, heads, "planes")
    ops = device_ops((Q, K, V, B))
    with handle(csr) as h:
        O = torch.empty((csr.m, heads * 8), dtype=torch.float32, device=DEV)
        L = torch.empty((heads, csr.m), dtype=torch.float32, device=DEV)
        mean, ms = api.time_attention_gqa_lse_launches(h.h, heads, kv, *ops, O, L, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        want = lse_host(h, csr, heads, kv, Q, K, V, B, float(1.0 / np.sqrt(8)))
        assert same_bits(O.cpu().numpy(), want[0]) and same_bits(L.cpu().numpy(), want[1])
        with pytest.raises(api.SpmvError):
            api.time_attention_gqa_lse_launches(h.h, heads, kv, *ops, O, np.empty((heads, csr.m), dtype=np.float32), warmup=1, iters=1)   # a host L
        lib.spmv_hip_clear_error()
