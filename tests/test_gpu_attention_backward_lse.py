"""GPU: spmv_hip_attention_gqa_backward_lse -- the gradients of one part of an attention, driven by the FINAL output O and row log-sum-exp L
(include/spmv_hip.h): P = exp(t - L), D = <G row, O row>, everything after that spmv_hip_attention_gqa_backward's.

1. exact structure: dQ and dK are spmm / spmm_transpose over dB * scale   2. what changes no bit   3. values, one handle and two parts, against the
unchanged spmv_hip_attention_gqa_backward through a high-precision reference   4. outputs and special values   5. handle rules, the timer"""
import itertools

import numpy as np
import pytest

from gqa_cases import (BIASES, CANARY, COMBOS, COMBO_IDS, DEV, DTYPES, E_ARG, E_NOSTATE, IDS, METHODS, OPTION, M, all_same, bias_of, chain, device_ops, gqa_bwd_host, handle,
                       operands, pattern_a, pattern_b, plane, same_bits, shapes)
from lse_cases import bwd_lse_host, err, fold, lse_host, part_bias, parts_a, reference, rows_of
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu
NAMES = ("dQ", "dK", "dV", "dB")
NEEDS = list(itertools.product((True, False), repeat=4))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def sub(base, need):
    return [b if n else None for b, n in zip(base, need)]


# ----------------------------------------------------------------------------- 1. exact structure
@pytest.mark.parametrize("which", ["rows", "cols"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dq_and_dk_are_spmm_over_the_calls_ds(dtype, which):
    """one head, k, dv > 1: with dB from the call, dQ has the bits of api.spmm on a second handle whose values are dB * scale with X = K, and dK
    those of api.spmm_transpose with X = Q"""
    csr = (pattern_a if which == "rows" else pattern_b)(dtype)
    with handle(csr) as h:
        for k, dv in shapes(dtype)[1:]:
            Q, K, V, G = operands(csr, 1, 1, k, dv)
            scale = float(dtype(1.0 / np.sqrt(k)))
            for kind in ("none", "planes"):
                B = bias_of(csr, 1, kind)
                O, L = lse_host(h, csr, 1, 1, Q, K, V, B, scale)
                dQ, dK, dV, dB = bwd_lse_host(h, csr, 1, 1, Q, K, V, B, G, O, L, scale)
                dS = dB[0] * dtype(scale)
                assert dS.dtype == np.dtype(dtype)
                with handle(synth.CSR(csr.m, csr.n, csr.rowptr, csr.colidx, dS)) as h2:
                    assert same_bits(h2.spmm(K), dQ), (k, dv, kind)
                    assert same_bits(h2.spmm_transpose(Q), dK), (k, dv, kind)


# ----------------------------------------------------------------------------- 2. what changes no bit
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_need_pointer_kind_layout_method_and_rounds_change_no_bit(dtype):
    import torch
    csr = pattern_a(dtype)
    s = np.dtype(dtype).itemsize
    heads, kv, k, dv = 6, 2, 3 * (16 // s), 2 * (16 // s)   # k * s and dv * s multiples of 16: aligned operands take the 16-byte form
    Q, K, V, G = host = operands(csr, heads, kv, k, dv)
    B = bias_of(csr, heads, "planes")
    scale = 0.125
    with handle(csr) as h:
        O, L = lse_host(h, csr, heads, kv, Q, K, V, B, scale)
        base = bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, scale, pad=0)
        assert all(np.isfinite(b).all() for b in base)
        # only dB wanted, on a handle that has computed no dK or dV yet: the row pass alone, no transpose is built
        with handle(csr) as h2:
            assert all_same(bwd_lse_host(h2, csr, heads, kv, Q, K, V, B, G, O, L, scale, need=(False, False, False, True)), sub(base, (False, False, False, True)))
            with pytest.raises(api.SpmvError, match=r"\[5\]"):
                api.get_transpose_info(h2.h)
            api.load().spmv_hip_clear_error()
        for need in NEEDS:   # all sixteen subsets of the wanted outputs
            assert all_same(bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, scale, need=need), sub(base, need)), need
        # padded and unaligned operands, O and L among them
        for pad, off in ((4, 0), (1, 0), (0, 1), (3, 2)):
            views = []
            for a in (*host, O):
                wd = np.full((a.shape[0], a.shape[1] + pad + off), np.nan, dtype=dtype)
                wd[:, off:off + a.shape[1]] = a
                views.append(wd[:, off:off + a.shape[1]])
            Lw = np.full((heads, csr.m + pad + off), np.nan, dtype=dtype)
            Lw[:, off:off + csr.m] = L
            assert all_same(bwd_lse_host(h, csr, heads, kv, *views[:3], B, views[3], views[4], Lw[:, off:off + csr.m], scale, pad=pad + off), base), (pad, off)
        # pointer kinds: everything on the device; each of the new operands on its own side
        ops = device_ops((*host, B, O, L))
        got = h.attention_gqa_backward_lse(*ops[:3], ops[4], ops[3], ops[5], ops[6], heads, kv, scale)
        torch.cuda.synchronize()
        assert [tuple(g.shape) for g in got] == [(csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv), (heads, csr.nnz)]
        assert all_same([g.cpu().numpy() for g in got], base)
        assert all_same(bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, ops[5], L, scale), base)
        assert all_same(bwd_lse_host(h, csr, heads, kv, ops[0], K, V, B, ops[3], O, ops[6], scale), base)
    for method in METHODS:
        with handle(csr, method) as h:
            assert all_same(bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, scale), base), method
    for n in (1, 2, heads):   # option attention_backward_heads: rounds that end inside a group of three, at its end, one round
        with handle(csr, **{OPTION: n}) as h:
            assert h.option(OPTION) == n
            assert all_same(bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, scale), base), n


@pytest.mark.parametrize("combo", [(4, 2), (6, 2), (3, 3), (4, 1)], ids=["4over2", "6over2", "3over3", "4over1"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_per_head_and_the_chain_per_group(dtype, combo):
    """head h of the grouped call versus the one-head _lse call on its slices (Q + h*k, K + (h/gs)*k, V + (h/gs)*dv, G + h*dv, O + h*dv, plane h of B
    and of L): dQ and dB are its bits, dK and dV of a group the chain (gqa_cases.chain) of its heads' terms in ascending head"""
    heads, kv = combo
    gs = heads // kv
    csr = pattern_a(dtype)
    with handle(csr) as h:
        for k, dv in shapes(dtype)[1:3]:
            Q, K, V, G = operands(csr, heads, kv, k, dv)
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                O, L = lse_host(h, csr, heads, kv, Q, K, V, B, 0.5)
                dQ, dK, dV, dB = bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, 0.5)
                tK, tV = [], []
                for hd in range(heads):
                    g = hd // gs
                    one = bwd_lse_host(h, csr, 1, 1, Q[:, hd * k:(hd + 1) * k], K[:, g * k:(g + 1) * k], V[:, g * dv:(g + 1) * dv], plane(B, hd), G[:, hd * dv:(hd + 1) * dv],
                                       O[:, hd * dv:(hd + 1) * dv], L[hd:hd + 1], 0.5)
                    assert same_bits(one[0], dQ[:, hd * k:(hd + 1) * k]) and same_bits(one[3][0], dB[hd]), (k, dv, kind, hd)
                    tK.append(one[1])
                    tV.append(one[2])
                for g in range(kv):
                    assert same_bits(chain(tK[g * gs:(g + 1) * gs]), dK[:, g * k:(g + 1) * k]), (k, dv, kind, g)
                    assert same_bits(chain(tV[g * gs:(g + 1) * gs]), dV[:, g * dv:(g + 1) * dv]), (k, dv, kind, g)


# ----------------------------------------------------------------------------- 3. values
def _floor(ref, dtype):
    """eight roundings of the largest element of the exact result: what a different but equally good order may differ by"""
    return 8 * float(np.finfo(dtype).eps) * float(np.abs(ref).max())


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_values_against_the_unchanged_backward_one_handle_and_two_parts(dtype, combo):
    """Both through the high-precision row-by-row reference (lse_cases.reference: float64 for fp32 handles, np.longdouble for fp64), per output:
        E_new <= 8 * E_old + 8 * eps * max|ref|
    E_old: the unchanged spmv_hip_attention_gqa_backward on the unsplit pattern; E_new: (a) the _lse call on the same handle with its own forward's
    O and L, (b) the two-part split with the merged O and L: dQ1 + dQ2, [dK1; dK2], [dV1; dV2] and the parts' dB scattered back to the unsplit
    entry order.  The margin of eight is the forward partition test's (test_gpu_attention_merge.py); the floor is eight roundings of the
    largest exact element, for outputs the old call happens to get almost exactly."""
    heads, kv = combo
    csr, parts, bounds = parts_a(dtype, 2)
    eps = float(np.finfo(dtype).eps)
    k, dv = (5, 4) if heads > 1 else (33, 17)
    Q, K, V, G = operands(csr, heads, kv, k, dv)
    scale = float(dtype(1.0 / np.sqrt(k)))
    hs = [handle(p) for p, _ in parts]
    try:
        with handle(csr) as h:
            for kind in BIASES:
                B = bias_of(csr, heads, kind)
                ref = reference(csr, heads, kv, Q, K, V, B, scale, G)[2:]
                old = gqa_bwd_host(h, csr, heads, kv, Q, K, V, B, G, scale)
                O, L = lse_host(h, csr, heads, kv, Q, K, V, B, scale)
                new = bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, scale)
                Om, Lm = fold(hs, parts, bounds, heads, kv, Q, K, V, B, scale)
                dq, dks, dvs, db = None, [], [], np.full((heads, csr.nnz), CANARY, dtype=dtype)
                for r, ((p, idx), hp) in enumerate(zip(parts, hs)):
                    g = bwd_lse_host(hp, p, heads, kv, Q, rows_of(K, bounds, r), rows_of(V, bounds, r), part_bias(B, idx), G, Om, Lm, scale)
                    dq = g[0] if dq is None else dq + g[0]
                    dks.append(g[1])
                    dvs.append(g[2])
                    db[:, idx] = g[3]
                split = (dq, np.concatenate(dks), np.concatenate(dvs), db)
                for name, o, n, sp, r in zip(NAMES, old, new, split, ref):
                    e_old, e_new, e_split = err(o, r), err(n, r), err(sp, r)
                    print(f"{np.dtype(dtype).name} {heads}over{kv} {kind} {name}: old {e_old / eps:.2f} eps, lse {e_new / eps:.2f}, two parts {e_split / eps:.2f}")
                    assert e_new <= 8 * e_old + _floor(r, dtype), (kind, name, e_new, e_old)
                    assert e_split <= 8 * e_old + _floor(r, dtype), (kind, name, e_split, e_old)
    finally:
        for x in hs:
            x.close()


# ----------------------------------------------------------------------------- 4. outputs and special values
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_rows_and_columns_give_plus_zero(dtype):
    """canaries on every output (bwd_lse_host); rows of A without entries: +0 rows of dQ; columns without entries: +0 rows of dK and dV"""
    heads, kv, k, dv = 4, 2, 3, 5
    for pat in (pattern_a, pattern_b):
        csr = pat(dtype)
        Q, K, V, G = operands(csr, heads, kv, k, dv)
        with handle(csr) as h:
            O, L = lse_host(h, csr, heads, kv, Q, K, V, None, 0.5)
            dQ, dK, dV, dB = bwd_lse_host(h, csr, heads, kv, Q, K, V, None, G, O, L, 0.5)
        norow = np.diff(csr.rowptr) == 0
        nocol = np.bincount(csr.colidx, minlength=csr.n) == 0
        assert norow.any() if pat is pattern_a else nocol.any()   # pattern A has the empty rows, its transpose the empty columns
        assert (dQ[norow] == 0).all() and not np.signbit(dQ[norow]).any()
        for d in (dK, dV):
            assert (d[nocol] == 0).all() and not np.signbit(d[nocol]).any()
        assert all(np.isfinite(d).all() for d in (dQ, dK, dV, dB))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nan_in_l_stays_in_its_head_its_row_and_its_groups_kv_head(dtype):
    """heads = 6 over 2 (groups of three): L of head 1 is NaN on a short and a long row.  dQ and dB are NaN in head 1 on those rows only; dK and dV
    are NaN in K / V head 0 only, on the columns those rows reach; everything else has the clean call's bits.  An L below the row's true
    log-sum-exp gives other values, never a fault"""
    csr = pattern_a(dtype)
    heads, kv, k, dv = 6, 2, 3, 5
    Q, K, V, G = operands(csr, heads, kv, k, dv)
    B = bias_of(csr, heads, "planes")
    lens = np.diff(csr.rowptr)
    rows = [int(np.flatnonzero(lens == n)[0]) for n in (3, 1025)]
    with handle(csr) as h:
        O, L = lse_host(h, csr, heads, kv, Q, K, V, B, 1.0)
        clean = bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, 1.0)
        Ln = L.copy()
        Ln[1, rows] = np.nan
        dQ, dK, dV, dB = got = bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, Ln, 1.0)
        low = bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L - dtype(5), 1.0)   # inconsistent: every P is e^5 too large
        assert all(np.isfinite(x).all() for x in low)
    nq = np.zeros(dQ.shape, dtype=bool)
    nq[rows, k:2 * k] = True
    nb = np.zeros(dB.shape, dtype=bool)
    reached = np.zeros(csr.n, dtype=bool)
    for r in rows:
        nb[1, csr.rowptr[r]:csr.rowptr[r + 1]] = True
        reached[csr.colidx[csr.rowptr[r]:csr.rowptr[r + 1]]] = True
    assert np.array_equal(np.isnan(dQ), nq) and np.array_equal(np.isnan(dB), nb)
    for d, w in ((dK, k), (dV, dv)):
        nan = np.isnan(d)
        assert not nan[:, w:].any() and np.array_equal(nan[:, :w].all(axis=1), reached) and np.array_equal(nan[:, :w].any(axis=1), reached)
    for g, c in zip(got, clean):
        ok = ~np.isnan(g)
        assert same_bits(g[ok], c[ok])


# ----------------------------------------------------------------------------- 5. handle rules, the timer
def test_handle_rules():
    import torch
    lib = api.load()
    csr = pattern_a(np.float64)
    heads, kv, k, dv = 4, 2, 3, 2
    Q, K, V, G = operands(csr, heads, kv, k, dv)
    outs = [np.full(s, CANARY) for s in ((csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv), (heads, csr.nnz))]
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, csr.n)
    with handle(csr) as h:
        y0 = h.spmv(x, np.full(csr.m, np.nan))
        O, L = lse_host(h, csr, heads, kv, Q, K, V, None, 0.5)
        args = (h.h, csr.m, csr.rowptr, csr.colidx, csr.val, heads, kv, Q, K, V, None, G)
        assert api.attention_gqa_backward_lse(*args, O, L, *outs, check=False, ldl=csr.m - 1) == E_ARG
        lib.spmv_hip_clear_error()
        assert api.attention_gqa_backward_lse(*args, O, L, *outs, check=False, lddb=csr.nnz - 1) == E_ARG   # found once nnz is known
        lib.spmv_hip_clear_error()
        assert all((o == CANARY).all() for o in outs)
        old = gqa_bwd_host(h, csr, heads, kv, Q, K, V, None, G, 0.5)
        torch.cuda.synchronize()
        ops = device_ops((Q, K, V, G, O, L))
        h.attention_gqa_backward(*ops[:3], None, ops[3], heads, kv, 0.5)
        torch.cuda.synchronize()
        b1 = h.info()["device_bytes"]
        got = h.attention_gqa_backward_lse(*ops[:3], None, ops[3], ops[4], ops[5], heads, kv, 0.5)   # device operands: nothing more than the GQA backward holds
        torch.cuda.synchronize()
        assert h.info()["device_bytes"] == b1
        for g, o in zip(got, old):
            assert np.allclose(g.cpu().numpy(), o, rtol=1e-9, atol=1e-12)
        assert same_bits(h.spmv(x, np.full(csr.m, np.nan)), y0)   # the resident values are not touched
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        api.set_thread_option(key, 1)
        try:
            h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial, way=way)
        finally:
            api.clear_thread_options()
        with h:
            assert api.attention_gqa_backward_lse(h.h, *args[1:], O, L, *outs, check=False) == E_ARG, key
            lib.spmv_hip_clear_error()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert api.attention_gqa_backward_lse(h.h, *args[1:], O, L, *outs, check=False) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert all((o == CANARY).all() for o in outs)
    h.close()


def test_timer_runs_on_device_operands_and_leaves_the_calls_bits():
    import torch
    lib = api.load()
    csr = pattern_a(np.float32)
    heads, kv = 4, 2
    Q, K, V, G = operands(csr, heads, kv, 8, 8)
    B = bias_of(csr, heads, "planes")
    scale = float(1.0 / np.sqrt(8))
    with handle(csr) as h:
        O, L = lse_host(h, csr, heads, kv, Q, K, V, B, scale)
        want = bwd_lse_host(h, csr, heads, kv, Q, K, V, B, G, O, L, scale)
        ops = device_ops((Q, K, V, B, G, O, L))
        outs = [torch.empty(w.shape, dtype=torch.float32, device=DEV) for w in want]
        mean, ms = api.time_attention_gqa_backward_lse_launches(h.h, heads, kv, *ops, *outs, warmup=1, iters=3)
        assert mean > 0 and ms.shape == (3,) and (ms > 0).all()
        assert all_same([o.cpu().numpy() for o in outs], want)
        with pytest.raises(api.SpmvError):
            api.time_attention_gqa_backward_lse_launches(h.h, heads, kv, *ops[:5], O, ops[6], *outs, warmup=1, iters=1)   # a host O
        lib.spmv_hip_clear_error()
