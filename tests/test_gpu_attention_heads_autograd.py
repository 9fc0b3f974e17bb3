"""GPU: spmv_amd.autograd.attention_heads -- Handle.attention_heads forward, one spmv_hip_attention_backward call per head backward.

Bars: torch.autograd.gradcheck in fp64 with its default tolerances through the real kernels; on the row-length pattern of
test_gpu_attention_heads.py every head slice of O, dQ, dK and dV has the BITS of autograd.attention(..., backward="fused") on that head's
slices made contiguous (both are spmv_hip_attention / spmv_hip_attention_backward, whose results do not depend on ld or alignment).  Only the
gradients asked for are computed, no Handle.update_values is made and the handle multiplies the same matrix afterwards."""
import numpy as np
import pytest

from conftest import load_golden
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
DEV = "cuda:0"
N = 300
LENGTHS = [0, 1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64, 65, 511, 512, 513, 575, 576, 577, 1025, 2047, 2048, 2049, 4097, 5000]


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
    """12 x 10 with rows of length 0, 1, 3 and 10 (every column) among rows of 2 .. 6 entries; column 6 only in the full row"""
    rng = np.random.default_rng(4)
    m, n = 12, 10
    cols_ok = np.array([c for c in range(n) if c != 6], dtype=np.int32)
    lens = rng.integers(2, 7, m)
    lens[7], lens[3], lens[5], lens[9] = 0, 1, 3, 10
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([np.arange(n, dtype=np.int32) if l == n else np.sort(rng.choice(cols_ok, int(l), replace=False)) for l in lens]).astype(np.int32)
    return synth.CSR(m, n, rp, ci, rng.uniform(-1, 1, int(rp[-1])))


def big_pattern():
    """test_gpu_attention_heads.py's rows: every length on both sides of the 64 / 512 / 2048 / 4097 boundaries, runs of empty rows"""
    rng = np.random.default_rng(11)
    order = rng.permutation(len(LENGTHS))
    lens = [0] * 5
    for pos, i in enumerate(order):
        if pos == len(order) // 2:
            lens += [0] * 70
        lens.append(LENGTHS[i])
    lens += [0] * 6
    rp = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    nnz = int(rp[-1])
    return synth.CSR(len(lens), N, rp, rng.integers(0, N, nnz).astype(np.int32), rng.uniform(-1, 1, nnz))


def rand(shape, seed):
    import torch
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.rand(shape, generator=g, device=DEV, dtype=torch.float64) * 2 - 1


def bits(t):
    import torch
    return t.detach().contiguous().view(torch.int64)


@pytest.mark.parametrize("scale", [None, 0.7])
def test_gradcheck(scale):
    import torch
    from spmv_amd import autograd
    csr = small_pattern()
    heads, k, dv = 2, 3, 2
    with device_handle(csr) as h:
        Q, K, V = (rand(s, i).requires_grad_(True) for i, s in enumerate(((csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv))))
        assert torch.autograd.gradcheck(lambda q, kk, v: autograd.attention_heads(h, q, kk, v, heads, scale), (Q, K, V))     # default eps / atol / rtol


def test_head_slices_have_the_single_head_bits_and_the_handle_is_left_alone(monkeypatch):
    import torch
    from spmv_amd import autograd
    csr = big_pattern()
    heads, k, dv = 3, 4, 5
    with device_handle(csr) as h:
        x = rand((csr.n,), 1)
        before = h.spmv(x, torch.empty(csr.m, dtype=torch.float64, device=DEV)).clone()
        token, ref, keep = getattr(h, "_values_token", None), getattr(h, "_values_ref", None), h._keep[2]
        Q0, K0, V0, G = rand((csr.m, heads * k), 2), rand((csr.n, heads * k), 3), rand((csr.n, heads * dv), 4), rand((csr.m, heads * dv), 5)
        # the oracle: the single-head function with the fused backward, on each head's slices made contiguous
        want = []
        for hd in range(heads):
            ck, cv = slice(hd * k, (hd + 1) * k), slice(hd * dv, (hd + 1) * dv)
            q, kk, v = (t.contiguous().requires_grad_(True) for t in (Q0[:, ck], K0[:, ck], V0[:, cv]))
            o = autograd.attention(h, q, kk, v, backward="fused")            # scale=None: 1 / sqrt(k) of this head's k
            o.backward(G[:, cv].contiguous())
            want.append((o.detach(), q.grad, kk.grad, v.grad))
        updates, calls = [], []
        real_update, real_bwd = api.Handle.update_values, api.attention_backward
        monkeypatch.setattr(api.Handle, "update_values", lambda self, *a, **kw: (updates.append(1), real_update(self, *a, **kw))[1])
        monkeypatch.setattr(api, "attention_backward", lambda *a, **kw: (calls.append(tuple(t is not None for t in a[9:12])), real_bwd(*a, **kw))[1])
        Q, K, V = (t.clone().requires_grad_(True) for t in (Q0, K0, V0))
        O = autograd.attention_heads(h, Q, K, V, heads)
        O.backward(G)
        torch.cuda.synchronize()
        assert calls == [(True, True, True)] * heads and not updates        # one call per head, no update_values
        for hd in range(heads):
            ck, cv = slice(hd * k, (hd + 1) * k), slice(hd * dv, (hd + 1) * dv)
            for name, got, exp in zip(("O", "dQ", "dK", "dV"), (O[:, cv], Q.grad[:, ck], K.grad[:, ck], V.grad[:, cv]), want[hd]):
                assert torch.equal(bits(got), bits(exp)), (hd, name)
        # needs_input_grad reaches every head's call; the other gradients stay None
        for which in range(3):
            ops = [t.clone().requires_grad_(i == which) for i, t in enumerate((Q0, K0, V0))]
            del calls[:]
            autograd.attention_heads(h, *ops, heads).backward(G)
            assert calls == [tuple(i == which for i in range(3))] * heads and not updates, (which, calls)
            assert torch.equal(bits(ops[which].grad), bits((Q, K, V)[which].grad))
            assert all(t.grad is None for i, t in enumerate(ops) if i != which)
        monkeypatch.undo()
        assert getattr(h, "_values_token", None) is token and getattr(h, "_values_ref", None) is ref and h._keep[2] is keep
        after = h.spmv(x, torch.empty(csr.m, dtype=torch.float64, device=DEV))
        torch.cuda.synchronize()
        assert torch.equal(bits(before), bits(after))


def test_no_stored_entry_gives_zero_gradients():
    import torch
    from spmv_amd import autograd
    csr = load_golden("nnz0_f64_uniform")[0]
    assert csr.nnz == 0 and csr.m > 0
    with api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Parallel) as h:
        Q, K, V = (rand(s, i).requires_grad_(True) for i, s in enumerate(((csr.m, 4), (csr.n, 4), (csr.n, 6))))
        O = autograd.attention_heads(h, Q, K, V, 2)
        O.sum().backward()
        torch.cuda.synchronize()
        assert tuple(O.shape) == (csr.m, 6) and bool((O == 0).all())
        for t in (Q, K, V):
            assert t.grad.shape == t.shape and bool((t.grad == 0).all())


def test_wrong_arguments_raise():
    import torch
    from spmv_amd import autograd
    csr = small_pattern()
    with device_handle(csr) as h:
        Q, K, V = (torch.zeros(s, dtype=torch.float64, device=DEV) for s in ((csr.m, 6), (csr.n, 6), (csr.n, 4)))
        for heads in (0, -2, 3, 4, 5):        # 3 divides only Q's and K's 6 columns, 4 only V's 4
            with pytest.raises(ValueError):
                autograd.attention_heads(h, Q, K, V, heads)
        with pytest.raises(TypeError):
            autograd.attention_heads(h, Q.float(), K, V, 2)
        with pytest.raises(ValueError):
            autograd.attention_heads(h, Q[:-1], K, V, 2)
        assert tuple(autograd.attention_heads(h, Q, K, V, 2).shape) == (csr.m, 4)
