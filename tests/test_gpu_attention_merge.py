"""GPU: spmv_hip_attention_merge -- two partial attention results combined by their row log-sum-exps (include/spmv_hip.h) -- and the forward
partition equivalence built on it: pattern A cut by column into two and three parts (lse_cases.parts_a), one spmv_hip_attention_gqa_lse per
part, folded left to right, against the one-handle call on the unsplit pattern.

1. exact cases   2. in place, L = None, canaries, widths, pointer kinds   3. NaN stays in its row and head   4. the partition equivalence
5. handle rules, the timer"""
import numpy as np
import pytest

from gqa_cases import BIASES, CANARY, COMBOS, COMBO_IDS, DEV, DTYPES, E_ARG, E_NOSTATE, IDS, M, bias_of, gqa_host, handle, operands, pattern_a, same_bits
import lse_cases
from lse_cases import err, fold, lse_host, merge_host, parts_a, reference
from spmv_amd import api, build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def partials(dtype, m, heads, dv, seed=0):
    """two partial results of plausible sizes: O in [-1, 1], L in [-3, 6]"""
    rng = np.random.default_rng(100 * heads + dv + seed)
    return tuple(rng.uniform(lo, hi, shape).astype(dtype) for lo, hi, shape in ((-1, 1, (m, heads * dv)), (-3, 6, (heads, m)), (-1, 1, (m, heads * dv)), (-3, 6, (heads, m))))


def widths(dtype):
    """dv = 1, an odd width, a whole panel and KP + 1"""
    KP = 16 if np.dtype(dtype) == np.float64 else 32
    return [1, 5, KP, KP + 1]


def restated(O1, L1, O2, L2, heads):
    """the contract's formula in the operands' dtype, numpy's exp and log in place of the device's: for the sizes of the results, not their bits"""
    dv = O1.shape[1] // heads
    lm = np.fmax(L1, L2)
    with np.errstate(invalid="ignore"):
        w1, w2 = np.exp(L1 - lm), np.exp(L2 - lm)
    W = w1 + w2
    O = np.empty_like(O1)
    for hd in range(heads):
        c = slice(hd * dv, (hd + 1) * dv)
        O[:, c] = (w2[hd][:, None] * O2[:, c] + w1[hd][:, None] * O1[:, c]) / W[hd][:, None]
    return O, lm + np.log(W)


# ----------------------------------------------------------------------------- 1. exact cases
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases(dtype):
    csr = pattern_a(dtype)
    m, heads = csr.m, 3
    eps = np.finfo(dtype).eps
    with handle(csr) as h:
        for dv in widths(dtype):
            O1, L1, O2, L2 = partials(dtype, m, heads, dv)
            # part 2 empty on some rows of some heads (L2 = -inf, O2 = 0): O == O1 and L has L1's bits there
            gone = np.zeros((heads, m), dtype=bool)
            gone[0, ::3] = gone[2, 5:40] = True
            gone[1] = True
            L2e, O2e = L2.copy(), O2.copy()
            L2e[gone] = -np.inf
            for hd in range(heads):
                O2e[gone[hd], hd * dv:(hd + 1) * dv] = 0
            O, L = merge_host(h, m, heads, O1, L1, O2e, L2e)
            for hd in range(heads):
                c = slice(hd * dv, (hd + 1) * dv)
                assert np.array_equal(O[gone[hd], c], O1[gone[hd], c]) and same_bits(L[hd, gone[hd]], L1[hd, gone[hd]]), (dv, hd)
            # ... and the other way round: part 1 empty gives part 2's
            Ob, Lb = merge_host(h, m, heads, O2e, L2e, O1, L1)
            for hd in range(heads):
                c = slice(hd * dv, (hd + 1) * dv)
                assert np.array_equal(Ob[gone[hd], c], O1[gone[hd], c]) and same_bits(Lb[hd, gone[hd]], L1[hd, gone[hd]]), (dv, hd)
            # both parts empty: +0 and -inf
            L1e, O1e = L1.copy(), O1.copy()
            L1e[gone] = -np.inf
            for hd in range(heads):
                O1e[gone[hd], hd * dv:(hd + 1) * dv] = 0
            O, L = merge_host(h, m, heads, O1e, L1e, O2e, L2e)
            for hd in range(heads):
                blk = O[gone[hd], hd * dv:(hd + 1) * dv]
                assert (blk == 0).all() and not np.signbit(blk).any() and (L[hd, gone[hd]] == -np.inf).all()
            # identical parts: O bit-equal to O1, L within 2 ulp of L1 + log 2.  The contract's L = Lm + log(W) rounds twice in the handle's
            # precision: log 2 to within the library's bound (3 ulp of 0.69.. at the most, lse_cases.LOG_ULP) and the sum to half an ulp of L.
            # Where |L1 + log 2| >= 1 an ulp of L is at least two of log 2, the first rounding at most 3/2 ulp of L: 2 ulp of L is what the formula
            # can promise there, and it is asserted there; where L1 is near -log 2 the sum cancels, an ulp of L is far smaller than the rounding
            # of log 2 itself, and no evaluation of the formula in this precision can be within 2 ulp of L: there the two roundings are
            # asserted as they are, 3 ulp of log 2 plus half an ulp of L.  Every row and head is checked by one of the two.
            O, L = merge_host(h, m, heads, O1, L1, O1.copy(), L1.copy())
            assert same_bits(O, O1)
            want = L1.astype(np.longdouble) + np.log(np.longdouble(2))
            e = np.abs(L.astype(np.longdouble) - want)
            ulp = np.spacing(np.abs(want).astype(dtype)).astype(np.longdouble)
            far = np.abs(want) >= 1
            print(f"{np.dtype(dtype).name} dv {dv}: identical parts, L error in ulp of L: {float((e / ulp)[far].max()):.2f} where |L| >= 1, "
                  f"{float((e / ulp)[~far].max()):.2f} elsewhere ({float((e[~far] / np.spacing(dtype(np.log(2)))).max()):.2f} ulp of log 2)")
            assert far.any() and (~far).any()
            assert (e[far] <= 2 * ulp[far]).all(), dv
            assert (e[~far] <= lse_cases.LOG_ULP * np.spacing(dtype(np.log(2))) + ulp[~far] / 2).all(), dv
            # the general case is the contract's formula up to the library's exp and log
            O, L = merge_host(h, m, heads, O1, L1, O2, L2)
            Or, Lr = restated(O1, L1, O2, L2, heads)
            assert np.abs(O - Or).max() <= 32 * eps and np.abs(L - Lr).max() <= 128 * eps   # |O| <= 1, |L| <= 7: a few library ulps each side


# ----------------------------------------------------------------------------- 2. in place, L = None, widths, pointer kinds
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_in_place_no_l_layouts_and_pointer_kinds_change_no_bit(dtype):
    import torch
    csr = pattern_a(dtype)
    m = csr.m
    s = np.dtype(dtype).itemsize
    with handle(csr) as h:
        for heads, dv in [(3, w) for w in widths(dtype)] + [(1, 1), (4, 2 * (16 // s)), (1, 7)]:
            O1, L1, O2, L2 = partials(dtype, m, heads, dv)
            L2[1 % heads, 3] = -np.inf
            O0, L0 = merge_host(h, m, heads, O1, L1, O2, L2, pad=0)   # aligned: the 16-byte form when dv allows it
            On, none = merge_host(h, m, heads, O1, L1, O2, L2, want_l=False)
            assert none is None and same_bits(On, O0)
            # in place on the host: O is O1 and L is L1
            Oa, La = O1.copy(), L1.copy()
            api.attention_merge(h.h, heads, Oa, La, O2, L2, Oa, La)
            assert same_bits(Oa, O0) and same_bits(La, L0), (heads, dv)
            # padded and unaligned operands, host and device; in place on the device
            for pad, off in ((0, 0), (4, 0), (1, 0), (0, 1), (3, 2)):
                w = heads * dv
                big = [np.full((m + 1, w + pad + off), CANARY, dtype=dtype) for _ in range(2)]
                lbig = [np.full((heads + 1, m + pad + off), CANARY, dtype=dtype) for _ in range(2)]
                big[0][:m, off:off + w], big[1][:m, off:off + w] = O1, O2
                lbig[0][:heads, off:off + m], lbig[1][:heads, off:off + m] = L1, L2
                views = [big[0][:m, off:off + w], lbig[0][:heads, off:off + m], big[1][:m, off:off + w], lbig[1][:heads, off:off + m]]
                O, L = merge_host(h, m, heads, *views, pad=pad + off)
                assert same_bits(O, O0) and same_bits(L, L0), (heads, dv, pad, off)
                dO = [torch.from_numpy(b).to(DEV) for b in big]
                dL = [torch.from_numpy(b).to(DEV) for b in lbig]
                acc_o, acc_l = dO[0][:m, off:off + w], dL[0][:heads, off:off + m]
                api.attention_merge(h.h, heads, acc_o, acc_l, dO[1][:m, off:off + w], dL[1][:heads, off:off + m], acc_o, acc_l)   # the running accumulator
                torch.cuda.synchronize()
                oh, lh = dO[0].cpu().numpy(), dL[0].cpu().numpy()
                assert same_bits(oh[:m, off:off + w], O0) and same_bits(lh[:heads, off:off + m], L0), (heads, dv, pad, off)
                oh[:m, off:off + w] = CANARY
                lh[:heads, off:off + m] = CANARY
                assert (oh == CANARY).all() and (lh == CANARY).all(), "written outside the accumulator's elements"
                assert same_bits(dO[1].cpu().numpy(), big[1]) and same_bits(dL[1].cpu().numpy(), lbig[1])   # the inputs are only read
            # mixed pointer kinds
            d = [torch.from_numpy(a).to(DEV) for a in (O1, L1, O2, L2)]
            for mix in ((d[0], L1, O2, L2), (O1, d[1], O2, d[3]), (d[0], d[1], d[2], L2)):
                O, L = merge_host(h, m, heads, *mix)
                assert same_bits(O, O0) and same_bits(L, L0)
            Od, Ld = h.attention_merge(*d, heads)
            torch.cuda.synchronize()
            assert same_bits(Od.cpu().numpy(), O0) and same_bits(Ld.cpu().numpy(), L0)
            Od, none = h.attention_merge(*d, heads, want_lse=False)
            torch.cuda.synchronize()
            assert none is None and same_bits(Od.cpu().numpy(), O0)


# ----------------------------------------------------------------------------- 3. NaN
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nan_stays_in_its_row_and_head(dtype):
    csr = pattern_a(dtype)
    m, heads, dv = csr.m, 3, 5
    O1, L1, O2, L2 = partials(dtype, m, heads, dv)
    with handle(csr) as h:
        clean = merge_host(h, m, heads, O1, L1, O2, L2)
        L1[1, 7] = np.nan            # a NaN in L1 ...
        L2[2, 9] = np.nan            # ... in L2 ...
        L1[0, 11] = L2[0, 11] = np.nan   # ... in both
        O2[20, 2 * dv + 1] = np.nan  # a NaN element of O stays in its element's row and head
        O, L = merge_host(h, m, heads, O1, L1, O2, L2)
    want_l = np.zeros((heads, m), dtype=bool)
    want_l[1, 7] = want_l[2, 9] = want_l[0, 11] = True
    assert np.array_equal(np.isnan(L), want_l)
    want_o = np.zeros(O.shape, dtype=bool)
    for hd, i in ((1, 7), (2, 9), (0, 11)):
        want_o[i, hd * dv:(hd + 1) * dv] = True
    want_o[20, 2 * dv + 1] = True
    assert np.array_equal(np.isnan(O), want_o)
    assert same_bits(O[~want_o], clean[0][~want_o]) and same_bits(L[~want_l], clean[1][~want_l])


# ----------------------------------------------------------------------------- 4. the partition equivalence (forward)
RATIOS = {}


@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_parts_merged_are_the_unsplit_attention(dtype, combo, nparts):
    """Two-part and three-part splits of pattern A, COMBOS x BIASES: the merged O and L against the one-handle attention_gqa_lse on the unsplit
    pattern, both through a high-precision row-by-row numpy reference (float64 for fp32 handles, np.longdouble for fp64):
        E_parts <= 8 * E_one + 8 * eps * max|ref|,   E = max |result - ref|, for O and for L,
    with E_one the error of the UNCHANGED existing call (attention_gqa) on the same inputs for O, and of the one-handle L for L.  The margin of
    eight (three bits): the merge adds a handful of roundings per element and another summation order; a wrong row, plane, head, scale or weight
    errs by many orders more.  Measured E_parts / E_one: DESIGN.md 3.22."""
    heads, kv = combo
    csr, parts, bounds = parts_a(dtype, nparts)
    eps = float(np.finfo(dtype).eps)
    k, dv = (5, 4) if heads > 1 else (33, 17)
    Q, K, V, _ = operands(csr, heads, kv, k, dv)
    scale = float(dtype(1.0 / np.sqrt(k)))
    hs = [handle(p) for p, _ in parts]
    try:
        with handle(csr) as h:
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                Oref, Lref = reference(csr, heads, kv, Q, K, V, B, scale)
                e_one = err(gqa_host(h, csr, heads, kv, Q, K, V, B, scale), Oref)
                O1, L1 = lse_host(h, csr, heads, kv, Q, K, V, B, scale)
                el_one = err(L1, Lref)
                O, L = fold(hs, parts, bounds, heads, kv, Q, K, V, B, scale)
                e_parts, el_parts = err(O, Oref), err(L, Lref)
                print(f"{np.dtype(dtype).name} {heads}over{kv} {nparts} parts {kind}: O {e_parts / eps:.2f} eps vs {e_one / eps:.2f}, L {el_parts / eps:.2f} eps vs {el_one / eps:.2f}")
                fin = np.isfinite(Lref)
                assert e_parts <= 8 * e_one + 8 * eps * float(np.abs(Oref).max()), (kind, e_parts, e_one)
                assert el_parts <= 8 * el_one + 8 * eps * float(np.abs(Lref[fin]).max()), (kind, el_parts, el_one)
                assert np.array_equal(np.isneginf(L), ~fin)
                # rows without entries in every part: +0 and -inf, as in the unsplit call
                none = np.diff(csr.rowptr) == 0
                assert (O[none] == 0).all() and not np.signbit(O[none]).any() and (L[:, none] == -np.inf).all()
    finally:
        for x in hs:
            x.close()


# ----------------------------------------------------------------------------- 5. handle rules, the timer
def test_handle_rules():
    lib = api.load()
    csr = pattern_a(np.float64)
    m, heads, dv = csr.m, 2, 3
    O1, L1, O2, L2 = partials(np.float64, m, heads, dv)
    O, L = np.full_like(O1, CANARY), np.full_like(L1, CANARY)
    with handle(csr) as h:
        # found once m is known: planes closer than m, a NULL operand -- outputs untouched
        for ldl in ((m - 1, m, m), (m, m - 1, m), (m, m, m - 1)):
            assert api.attention_merge(h.h, heads, O1, L1, O2, L2, O, L, check=False, ldl=ldl) == E_ARG
            lib.spmv_hip_clear_error()
        assert lib.spmv_hip_attention_merge(h.h, heads, dv, O1.ctypes.data, heads * dv, None, m, O2.ctypes.data, heads * dv, L2.ctypes.data, m, O.ctypes.data, heads * dv,
                                            L.ctypes.data, m) == E_ARG
        lib.spmv_hip_clear_error()
        assert (O == CANARY).all() and (L == CANARY).all()
        b0 = h.info()["device_bytes"]
        import torch
        d = [torch.from_numpy(a).to(DEV) for a in (O1, L1, O2, L2)]
        h.attention_merge(*d, heads)
        torch.cuda.synchronize()
        assert h.info()["device_bytes"] == b0           # device operands: nothing is allocated
        merge_host(h, m, heads, O1, L1, O2, L2)
        assert h.info()["device_bytes"] > b0            # host operands: the staging buffers, counted
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            assert api.attention_merge(h.h, heads, O1, L1, O2, L2, O, L, check=False) == E_ARG, key
            lib.spmv_hip_clear_error()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert api.attention_merge(h.h, heads, O1, L1, O2, L2, O, L, check=False) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert (O == CANARY).all() and (L == CANARY).all()
    h.close()


def test_timer_runs_on_device_operands_and_leaves_the_calls_bits():
    import torch
    lib = api.load()
    csr = pattern_a(np.float32)
    m, heads, dv = csr.m, 4, 8
    ops = partials(np.float32, m, heads, dv)
    d = [torch.from_numpy(a).to(DEV) for a in ops]
    with handle(csr) as h:
        O = torch.empty((m, heads * dv), dtype=torch.float32, device=DEV)
        L = torch.empty((heads, m), dtype=torch.float32, device=DEV)
        mean, ms = api.time_attention_merge_launches(h.h, heads, *d, O, L, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        want = merge_host(h, m, heads, *ops)
        assert same_bits(O.cpu().numpy(), want[0]) and same_bits(L.cpu().numpy(), want[1])
        with pytest.raises(api.SpmvError):
            api.time_attention_merge_launches(h.h, heads, ops[0], *d[1:], O, L, warmup=1, iters=1)   # a host O1
        lib.spmv_hip_clear_error()
