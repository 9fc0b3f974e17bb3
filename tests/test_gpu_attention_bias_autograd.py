"""GPU: the bias= keyword of spmv_amd.autograd.attention and attention_heads -- a (nnz,) or (heads, nnz) tensor added to the scaled scores, which
receives a gradient (Handle.attention_bias / attention_bias_backward).

Bars: torch.autograd.gradcheck in fp64 with its default tolerances through the real kernels, both modes of both functions, per-head and shared
bias; the two modes of each function give the same bits for k, dv > 1; a shared bias' gradient is the sum of the per-head run's planes
(assert_close at the dtype's default tolerance: the sum is torch's); a bias that needs no gradient gets none computed."""
import numpy as np
import pytest

from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
DEV = "cuda:0"


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
    """12 x 10 with rows of length 0, 1, 3 and 10 (every column) among rows of 2 .. 6 entries"""
    rng = np.random.default_rng(4)
    m, n = 12, 10
    lens = rng.integers(2, 7, m)
    lens[7], lens[3], lens[5], lens[9] = 0, 1, 3, 10
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(n, int(l), replace=False)) for l in lens]).astype(np.int32)
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


def leaves(csr, heads, k, dv, bias_shape):
    Q, K, V = (rand(s, i).requires_grad_(True) for i, s in enumerate(((csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv))))
    return Q, K, V, rand(bias_shape, 7, -2.0, 2.0).requires_grad_(True)


@pytest.mark.parametrize("backward", ["composed", "fused"])
def test_gradcheck_attention(backward):
    import torch
    from spmv_amd import autograd
    csr = small_pattern()
    with device_handle(csr) as h:
        for shape in ((csr.nnz,), (1, csr.nnz)):
            Q, K, V, B = leaves(csr, 1, 3, 2, shape)
            assert torch.autograd.gradcheck(lambda q, kk, v, b: autograd.attention(h, q, kk, v, 0.7, backward, bias=b), (Q, K, V, B))   # default eps / atol / rtol


@pytest.mark.parametrize("backward", ["per_head", "fused"])
def test_gradcheck_attention_heads(backward):
    import torch
    from spmv_amd import autograd
    csr = small_pattern()
    heads = 2
    with device_handle(csr) as h:
        for shape in ((heads, csr.nnz), (csr.nnz,)):   # a plane per head; one shared plane
            Q, K, V, B = leaves(csr, heads, 3, 2, shape)
            assert torch.autograd.gradcheck(lambda q, kk, v, b: autograd.attention_heads(h, q, kk, v, heads, None, backward, bias=b), (Q, K, V, B))


def grads(fn, leaves_, G):
    import torch
    out = fn(*leaves_)
    return out, torch.autograd.grad(out, leaves_, G)


def test_the_modes_agree_to_the_bit_and_the_shared_gradient_is_the_planes_sum():
    import torch
    from spmv_amd import autograd
    csr = mid_pattern()
    heads, k, dv = 3, 5, 3
    with device_handle(csr) as h:
        Q, K, V, B = leaves(csr, heads, k, dv, (heads, csr.nnz))
        G = rand((csr.m, heads * dv), 9)
        o_f, g_f = grads(lambda *a: autograd.attention_heads(h, *a[:3], heads, 0.4, "fused", bias=a[3]), (Q, K, V, B), G)
        o_p, g_p = grads(lambda *a: autograd.attention_heads(h, *a[:3], heads, 0.4, "per_head", bias=a[3]), (Q, K, V, B), G)
        assert torch.equal(bits(o_f), bits(o_p))
        for a, b in zip(g_f, g_p):
            assert torch.equal(bits(a), bits(b))
        assert g_f[3].shape == B.shape and bool((g_f[3] != 0).any())
        # head h of the heads call is attention() on its slices and its plane, in both of ITS modes
        for hd in range(heads):
            ck, cv = slice(hd * k, (hd + 1) * k), slice(hd * dv, (hd + 1) * dv)
            ls = tuple(t.detach().clone().requires_grad_(True) for t in (Q[:, ck], K[:, ck], V[:, cv], B[hd]))
            for mode in ("composed", "fused"):
                o_1, g_1 = grads(lambda *a: autograd.attention(h, *a[:3], 0.4, mode, bias=a[3]), ls, G[:, cv].contiguous())
                assert torch.equal(bits(o_1), bits(o_f[:, cv])), (hd, mode)
                for a, b in zip(g_1, (g_f[0][:, ck], g_f[1][:, ck], g_f[2][:, cv], g_f[3][hd])):
                    assert torch.equal(bits(a), bits(b)), (hd, mode)
        # one shared plane: `heads` copies of it forward; its gradient the sum of the per-head run's planes -- torch's sum
        b1 = B[1].detach().clone().requires_grad_(True)
        bt = B[1].detach().repeat(heads, 1).requires_grad_(True)
        for mode in ("fused", "per_head"):
            o_s, g_s = grads(lambda *a: autograd.attention_heads(h, *a[:3], heads, 0.4, mode, bias=a[3]), (Q, K, V, b1), G)
            o_t, g_t = grads(lambda *a: autograd.attention_heads(h, *a[:3], heads, 0.4, mode, bias=a[3]), (Q, K, V, bt), G)
            assert torch.equal(bits(o_s), bits(o_t)), mode
            for a, b in zip(g_s[:3], g_t[:3]):
                assert torch.equal(bits(a), bits(b)), mode
            assert g_s[3].shape == b1.shape
            torch.testing.assert_close(g_s[3], g_t[3].sum(0))
        # bias=None is the call without the keyword
        o_0, g_0 = grads(lambda *a: autograd.attention_heads(h, *a, heads, 0.4, "fused"), (Q, K, V), G)
        o_n, g_n = grads(lambda *a: autograd.attention_heads(h, *a, heads, 0.4, "fused", bias=None), (Q, K, V), G)
        assert torch.equal(bits(o_0), bits(o_n)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(g_0, g_n))
        assert not torch.equal(bits(o_0), bits(o_f))


def test_a_bias_without_requires_grad_gets_no_gradient_computed(monkeypatch):
    import torch
    from spmv_amd import autograd
    csr = small_pattern()
    heads = 2
    seen = []
    real = api.Handle.attention_bias_backward

    def spy(self, Q, K, V, bias, G, heads, scale=None, need=(True, True, True, True)):
        seen.append(tuple(need))
        return real(self, Q, K, V, bias, G, heads, scale, need)
    monkeypatch.setattr(api.Handle, "attention_bias_backward", spy)
    with device_handle(csr) as h:
        Q, K, V, B = leaves(csr, heads, 3, 2, (heads, csr.nnz))
        autograd.attention_heads(h, Q, K, V, heads, None, "fused", bias=B.detach()).sum().backward()
        assert seen == [(True, True, True, False)] and B.grad is None
        autograd.attention_heads(h, Q.detach(), K, V.detach(), heads, None, "fused", bias=B).sum().backward()
        assert seen[-1] == (False, True, False, True) and B.grad is not None and B.grad.shape == B.shape
        autograd.attention(h, Q[:, :3].detach(), K[:, :3].detach(), V[:, :2].detach(), None, "fused", bias=B[0]).sum().backward()
        assert seen[-1] == (False, False, False, True)
        n = len(seen)
        autograd.attention_heads(h, Q, K, V, heads, None, "fused").sum().backward()   # no bias: the no-bias call, as before
        assert len(seen) == n
