"""GPU: the kv_heads= keyword of spmv_amd.autograd.attention_heads -- grouped-query attention with K (n, kv_heads * k) and V (n, kv_heads * dv) at
their narrow widths (Handle.attention_gqa / attention_gqa_backward).

Bars: torch.autograd.gradcheck in fp64 with its default tolerances through the real kernels for (heads, kv_heads) = (4, 2) and (3, 1), with and
without a bias, in both backward modes, on a small pattern with an empty row and a long row; both modes give identical bits (the per-head mode
accumulates dK and dV of a group in torch in ascending head, the first head assigned: the fused call's chain); kv_heads=None gives today's
bits; widths that do not divide raise ValueError."""
import numpy as np
import pytest

from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
DEV = "cuda:0"
COMBOS = [(4, 2), (3, 1)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def device_handle(csr, method=M.Method_Parallel):
    import torch
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    return api.Handle(csr.m, csr.n, rp, ci, va, method)


def small_pattern():
    """9 x 10: an empty row, a row of one entry and a LONG row (513 entries, a workgroup's; its columns repeat) among rows of 2 .. 6 entries"""
    rng = np.random.default_rng(4)
    m, n = 9, 10
    lens = rng.integers(2, 7, m)
    lens[2], lens[4], lens[6] = 0, 1, 513
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(n, int(l), replace=l > n)) for l in lens]).astype(np.int32)
    return synth.CSR(m, n, rp, ci, rng.uniform(-1, 1, int(rp[-1])))


def mid_pattern():
    """60 x 80: rows on both sides of 64 and of 512 (a long row), empty rows"""
    rng = np.random.default_rng(6)
    lens = [0, 1, 2, 9, 63, 64, 65, 0, 130, 513] * 6
    rp = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    return synth.CSR(len(lens), 80, rp, rng.integers(0, 80, int(rp[-1])).astype(np.int32), rng.uniform(-1, 1, int(rp[-1])))


def rand(shape, seed, lo=-1.0, hi=1.0):
    import torch
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.rand(shape, generator=g, device=DEV, dtype=torch.float64) * (hi - lo) + lo


def bits(t):
    import torch
    return t.detach().contiguous().view(torch.int64)


def leaves(csr, heads, kv, k, dv, bias_shape=None):
    Q, K, V = (rand(s, i).requires_grad_(True) for i, s in enumerate(((csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv))))
    if bias_shape is None:
        return Q, K, V
    return Q, K, V, rand(bias_shape, 7, -2.0, 2.0).requires_grad_(True)


@pytest.mark.parametrize("backward", ["per_head", "fused"])
@pytest.mark.parametrize("combo", COMBOS, ids=["4over2", "3over1"])
def test_gradcheck(combo, backward):
    import torch
    from spmv_amd import autograd
    heads, kv = combo
    csr = small_pattern()
    with device_handle(csr) as h:
        Q, K, V = leaves(csr, heads, kv, 3, 2)
        assert torch.autograd.gradcheck(lambda q, kk, v: autograd.attention_heads(h, q, kk, v, heads, None, backward, kv_heads=kv), (Q, K, V))   # default eps / atol / rtol
        for shape in ((heads, csr.nnz), (csr.nnz,)):   # a plane per QUERY head; one shared plane
            Q, K, V, B = leaves(csr, heads, kv, 3, 2, shape)
            assert torch.autograd.gradcheck(lambda q, kk, v, b: autograd.attention_heads(h, q, kk, v, heads, 0.6, backward, bias=b, kv_heads=kv), (Q, K, V, B))


def grads(fn, leaves_, G):
    import torch
    out = fn(*leaves_)
    return out, torch.autograd.grad(out, leaves_, G)


@pytest.mark.parametrize("combo", COMBOS + [(6, 2)], ids=["4over2", "3over1", "6over2"])
def test_the_modes_agree_to_the_bit(combo):
    import torch
    from spmv_amd import autograd
    heads, kv = combo
    csr = mid_pattern()
    k, dv = 5, 3
    with device_handle(csr) as h:
        G = rand((csr.m, heads * dv), 9)
        for shape in (None, (heads, csr.nnz)):
            lv = leaves(csr, heads, kv, k, dv, shape)
            fn = {mode: (lambda *a, mode=mode: autograd.attention_heads(h, *a[:3], heads, 0.4, mode, bias=a[3] if len(a) > 3 else None, kv_heads=kv))
                  for mode in ("fused", "per_head")}
            o_f, g_f = grads(fn["fused"], lv, G)
            o_p, g_p = grads(fn["per_head"], lv, G)
            assert torch.equal(bits(o_f), bits(o_p))
            assert [tuple(g.shape) for g in g_f[:3]] == [(csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv)]
            for a, b in zip(g_f, g_p):
                assert not torch.isnan(a).any() and torch.equal(bits(a), bits(b))
        # only V needs a gradient: the others get none, in both modes, and dV keeps its bits
        Q, K, V = leaves(csr, heads, kv, k, dv)
        want = torch.autograd.grad(fn["fused"](Q, K, V), (V,), G)[0]
        Q2, K2 = Q.detach(), K.detach()
        for mode in ("fused", "per_head"):
            got = torch.autograd.grad(fn[mode](Q2, K2, V), (V,), G)[0]
            assert torch.equal(bits(got), bits(want)), mode


def test_saved_tensors_keep_the_narrow_width():
    import torch
    from spmv_amd import autograd
    heads, kv, k, dv = 4, 1, 5, 3
    csr = mid_pattern()
    with device_handle(csr) as h:
        Q, K, V = leaves(csr, heads, kv, k, dv)
        out = autograd.attention_heads(h, Q, K, V, heads, backward="fused", kv_heads=kv)
        saved = [t for t in out.grad_fn.saved_tensors if t is not None]
        assert sorted(tuple(t.shape) for t in saved) == sorted([(csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv)])   # Q, K and V only, nothing nnz-sized


def test_kv_heads_none_is_todays_path_and_kv_heads_equal_to_heads_has_its_bits():
    import torch
    from spmv_amd import autograd
    heads, k, dv = 3, 5, 3
    csr = mid_pattern()
    with device_handle(csr) as h:
        G = rand((csr.m, heads * dv), 9)
        for mode in ("per_head", "fused"):
            lv = leaves(csr, heads, heads, k, dv, (heads, csr.nnz))
            o0, g0 = grads(lambda *a: autograd.attention_heads(h, *a[:3], heads, 0.4, mode, bias=a[3]), lv, G)
            out = autograd.attention_heads(h, *lv[:3], heads, 0.4, mode, bias=lv[3], kv_heads=None)
            assert type(out.grad_fn).__name__.startswith("_AttentionHeads")   # the existing function, untouched
            g1 = torch.autograd.grad(out, lv, G)
            o2, g2 = grads(lambda *a: autograd.attention_heads(h, *a[:3], heads, 0.4, mode, bias=a[3], kv_heads=heads), lv, G)
            assert torch.equal(bits(o0), bits(out)) and torch.equal(bits(o0), bits(o2))
            for a, b, c in zip(g0, g1, g2):
                assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))


def test_widths_that_do_not_divide_raise():
    import torch
    from spmv_amd import autograd
    csr = small_pattern()
    with device_handle(csr) as h:
        Q, K, V = (rand(s, i) for i, s in enumerate(((csr.m, 12), (csr.n, 6), (csr.n, 4))))   # 4 heads of k = 3 over 2 K / V heads, dv = 2
        assert tuple(autograd.attention_heads(h, Q, K, V, 4, kv_heads=2).shape) == (csr.m, 8)
        for heads, kv in ((4, 3), (4, 0), (4, 8), (3, 2)):
            with pytest.raises(ValueError):
                autograd.attention_heads(h, Q, K, V, heads, kv_heads=kv)
        with pytest.raises(ValueError):   # K as wide as Q: not 2 K / V heads of Q's head width
            autograd.attention_heads(h, Q, Q[:csr.m].new_zeros((csr.n, 12)), V, 4, kv_heads=2)
        with pytest.raises(ValueError):   # V's width is no multiple of kv_heads
            autograd.attention_heads(h, Q, K, V[:, :3], 4, kv_heads=2)
        with pytest.raises(ValueError):   # the bias stays per QUERY head
            autograd.attention_heads(h, Q, K, V, 4, kv_heads=2, bias=torch.zeros((2, csr.nnz), dtype=torch.float64, device=DEV))
        with pytest.raises(ValueError):   # without kv_heads K has to be as wide as Q: today's rule
            autograd.attention_heads(h, Q, K, V, 4)
