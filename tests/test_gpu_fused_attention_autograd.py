"""GPU: spmv_amd.autograd.attention -- the fused forward pass (Handle.attention) with a backward pass composed of the existing operations.

Bars: torch.autograd.gradcheck in fp64 with its default tolerances through the real kernels; forward and gradients against dense masked torch
attention on the CPU in float64 to 1e-10 relative, the tolerance test_gpu_attention_autograd.py uses for the three-function composition (k <= 8
and rows of <= 8 entries: the error is a few hundred unit roundoffs of 1.1e-16); the forward pass equals the composition bit for bit."""
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
    """(handle on device arrays, values tensor)"""
    import torch
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    return api.Handle(csr.m, csr.n, rp, ci, va, method), va


def random_pattern(m=12, n=10, seed=4):
    """12 x 10 with an empty row (7), a row of length 1 (3) and an empty column (6)"""
    rng = np.random.default_rng(seed)
    cols_ok = np.array([c for c in range(n) if c != 6], dtype=np.int32)
    lens = rng.integers(2, 7, m)
    lens[7], lens[3] = 0, 1
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(cols_ok, int(l), replace=False)) for l in lens]).astype(np.int32)
    return synth.CSR(m, n, rp, ci, rng.uniform(-1, 1, int(rp[-1])))


def rand(shape, seed):
    import torch
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.rand(shape, generator=g, device=DEV, dtype=torch.float64) * 2 - 1


def composition(autograd, h, Q, K, V, scale):
    return autograd.matmul(h, V, values=autograd.row_softmax(h, autograd.sddmm(h, Q, K) * scale))


def bits(t):
    import torch
    return t.detach().contiguous().view(torch.int64)


@pytest.mark.parametrize("scale", [None, 0.7])
def test_gradcheck(scale):
    import torch
    from spmv_amd import autograd
    csr = random_pattern()
    h, _ = device_handle(csr)
    with h:
        Q, K, V = rand((csr.m, 4), 4).requires_grad_(True), rand((csr.n, 4), 5).requires_grad_(True), rand((csr.n, 3), 6).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda q, k, v: autograd.attention(h, q, k, v, scale), (Q, K, V))     # default eps / atol / rtol


def test_against_dense_torch_and_the_composition():
    import torch
    from spmv_amd import autograd
    csr = random_pattern(40, 30)
    k, dv = 8, 6
    scale = 1.0 / np.sqrt(k)
    rng = np.random.default_rng(3)
    Qh, Kh, Vh, Gh = rng.uniform(-1, 1, (csr.m, k)), rng.uniform(-1, 1, (csr.n, k)), rng.uniform(-1, 1, (csr.n, dv)), rng.uniform(-1, 1, (csr.m, dv))
    h, _ = device_handle(csr)
    with h:
        G = torch.from_numpy(Gh).to(DEV)
        Q, K, V = (torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (Qh, Kh, Vh))
        O = autograd.attention(h, Q, K, V)                           # scale=None: 1 / sqrt(k)
        O.backward(G)
        Q2, K2, V2 = (torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (Qh, Kh, Vh))
        O2 = composition(autograd, h, Q2, K2, V2, scale)
        O2.backward(G)
        torch.cuda.synchronize()
        assert torch.equal(bits(O), bits(O2))                        # the forward pass: the composition's bits
        got = [t.detach().cpu() for t in (O, Q.grad, K.grad, V.grad)]
        comp = [t.detach().cpu() for t in (O2, Q2.grad, K2.grad, V2.grad)]
    mask = torch.zeros((csr.m, csr.n), dtype=torch.bool)
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    mask[torch.from_numpy(rows), torch.from_numpy(csr.colidx.astype(np.int64))] = True
    Qc, Kc, Vc = (torch.from_numpy(a).requires_grad_(True) for a in (Qh, Kh, Vh))
    scores = (Qc @ Kc.T * scale).masked_fill(~mask, float("-inf"))
    some = mask.any(1, keepdim=True)
    P = torch.where(some, torch.softmax(torch.where(some, scores, torch.zeros_like(scores)), dim=1), torch.zeros_like(scores))
    P = torch.where(mask, P, torch.zeros_like(P))          # the empty pattern row: zeros
    Oc = P @ Vc
    Oc.backward(torch.from_numpy(Gh))
    for name, a, b, c in zip(("O", "dQ", "dK", "dV"), got, (Oc.detach(), Qc.grad, Kc.grad, Vc.grad), comp):
        ref = float(b.abs().max())
        err, err_c = float((a - b).abs().max()), float((a - c).abs().max())
        print(f"{name}: max err {err:.3e} against dense torch, {err_c:.3e} against the composition, scale {ref:.3e}")
        assert a.shape == b.shape and err <= 1e-10 * ref and err_c <= 1e-10 * ref, name
    assert bool((got[0][7] == 0).all()) and bool((got[1][7] == 0).all()) and bool((got[2][6] == 0).all()) and bool((got[3][6] == 0).all())   # the empty row and column


@pytest.mark.parametrize("held", ["create-time array", "matmul tensor"])
def test_backward_puts_the_values_back(held):
    import torch
    from spmv_amd import autograd
    csr = random_pattern(40, 30)
    h, va = device_handle(csr)
    with h:
        X, x0, x1 = rand((csr.n, 3), 7), rand((csr.n,), 11), rand((csr.m,), 8)
        values = None
        if held == "matmul tensor":
            values = (va * 2 + 1).requires_grad_(True)
            autograd.matmul(h, X, values=values)
        before = autograd.matmul(h, X, values=values).detach().clone()
        before_v = h.spmv(x0, torch.empty(csr.m, dtype=torch.float64, device=DEV)).clone()
        before_t = h.spmv_transpose(x1).clone()
        token, ref, keep = getattr(h, "_values_token", None), getattr(h, "_values_ref", None), h._keep[2]
        Q, K, V = rand((csr.m, 5), 9).requires_grad_(True), rand((csr.n, 5), 10).requires_grad_(True), rand((csr.n, 4), 12).requires_grad_(True)
        O = autograd.attention(h, Q, K, V)
        mid_v = h.spmv(x0, torch.empty(csr.m, dtype=torch.float64, device=DEV)).clone()      # the forward pass does not touch the values
        O.sum().backward()
        assert Q.grad is not None and K.grad is not None and V.grad is not None
        assert getattr(h, "_values_token", None) == token and getattr(h, "_values_ref", None) is ref and h._keep[2] is keep
        after = autograd.matmul(h, X, values=values).detach()
        after_none = autograd.matmul(h, X).detach()
        after_v = h.spmv(x0, torch.empty(csr.m, dtype=torch.float64, device=DEV))
        after_t = h.spmv_transpose(x1)
        torch.cuda.synchronize()
        assert torch.equal(bits(before), bits(after)) and torch.equal(bits(before), bits(after_none))
        assert torch.equal(bits(before_v), bits(mid_v)) and torch.equal(bits(before_v), bits(after_v))
        assert torch.equal(bits(before_t), bits(after_t))


def test_only_the_requested_gradients_are_computed(monkeypatch):
    import torch
    from spmv_amd import autograd
    csr = random_pattern(40, 30)
    h, _ = device_handle(csr)
    with h:
        full = [rand((csr.m, 5), 9).requires_grad_(True), rand((csr.n, 5), 10).requires_grad_(True), rand((csr.n, 4), 12).requires_grad_(True)]
        autograd.attention(h, *full).sum().backward()
        calls = []
        for name in ("spmm", "spmm_transpose", "sddmm", "row_softmax_backward", "update_values"):
            real = getattr(api.Handle, name)
            monkeypatch.setattr(api.Handle, name, (lambda real, name: lambda self, *a, **kw: (calls.append(name), real(self, *a, **kw))[1])(real, name))
        for which, expect in ((0, ["sddmm", "sddmm", "row_softmax_backward", "update_values", "spmm", "update_values"]),
                              (1, ["sddmm", "sddmm", "row_softmax_backward", "update_values", "spmm_transpose", "update_values"]),
                              (2, ["sddmm", "update_values", "spmm_transpose", "update_values"])):
            ops = [t.detach().clone().requires_grad_(i == which) for i, t in enumerate(full)]
            del calls[:]
            autograd.attention(h, *ops).sum().backward()
            assert calls == expect, (which, calls)
            assert torch.equal(ops[which].grad, full[which].grad)
            assert all(t.grad is None for i, t in enumerate(ops) if i != which)
        del calls[:]
        ops = [t.detach().clone().requires_grad_(True) for t in full]
        autograd.attention(h, *ops).sum().backward()
        assert calls.count("update_values") == 3                     # P, dS, and the values put back: what the docstring states


def test_wrong_arguments_raise():
    import torch
    from spmv_amd import autograd
    csr = random_pattern()
    h, _ = device_handle(csr)
    with h:
        Q, K, V = (torch.zeros(s, dtype=torch.float64, device=DEV) for s in ((csr.m, 2), (csr.n, 2), (csr.n, 3)))
        for bad in ((Q.float(), K, V), (Q, K.float(), V), (Q, K, V.float()), (Q.cpu(), K, V), (Q, K.cpu(), V), (Q, K, V.cpu()), (Q.cpu().numpy(), K, V)):
            with pytest.raises(TypeError):
                autograd.attention(h, *bad)
        for bad in ((Q[:-1], K, V), (Q, K[:, :1], V), (Q, K, V[:-1]), (Q[:, 0], K[:, 0], V)):
            with pytest.raises(ValueError):
                autograd.attention(h, *bad)


def test_reorder_and_multi_gpu_handles_raise():
    import torch
    from spmv_amd import autograd
    m, n, rp, ci, va = synth.banded_holes_device(100_000, 100_000, 24, 0.25, "eighths", torch.float64, DEV, 7)
    api.set_thread_option("reorder", 1)
    try:
        h = api.Handle(m, n, rp, ci, va, M.Method_Parallel)
    finally:
        api.clear_thread_options()
    with h:
        assert h.index is not None
        Q = torch.ones((m, 2), dtype=torch.float64, device=DEV)
        with pytest.raises(ValueError):
            autograd.attention(h, Q, Q, Q)
    csr = random_pattern(40, 30)
    api.set_thread_option("gpus", 1)
    try:
        h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial)
    finally:
        api.clear_thread_options()
    with h:
        Q, K = (torch.zeros(s, dtype=torch.float64, device=DEV) for s in ((csr.m, 2), (csr.n, 2)))
        with pytest.raises(ValueError):
            autograd.attention(h, Q, K, K)
