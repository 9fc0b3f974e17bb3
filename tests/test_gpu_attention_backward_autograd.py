"""GPU: spmv_amd.autograd.attention(..., backward="fused") -- the fused forward pass with ONE Handle.attention_backward call as its backward pass.

Bars: torch.autograd.gradcheck in fp64 with its default tolerances through the real kernels; the gradients equal the composed backward's bit
for bit when k > 1 and dv > 1 (at width 1 contiguous tensors send the composition's products down the spmv schedule) and match dense masked
torch attention on the CPU in float64 to 1e-10 of the reference's largest magnitude, the tolerance test_gpu_fused_attention_autograd.py uses.
The fused backward calls none of the composed operations and leaves the handle's value bookkeeping alone."""
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
    """12 x 10 with an empty row (7), a row of length 1 (3) and an empty column (6): test_gpu_fused_attention_autograd.py's"""
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
        assert torch.autograd.gradcheck(lambda q, k, v: autograd.attention(h, q, k, v, scale, backward="fused"), (Q, K, V))     # default eps / atol / rtol


def test_against_the_composed_backward_and_dense_torch():
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
        O = autograd.attention(h, Q, K, V, backward="fused")             # scale=None: 1 / sqrt(k)
        O.backward(G)
        Q2, K2, V2 = (torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (Qh, Kh, Vh))
        O2 = autograd.attention(h, Q2, K2, V2)                           # the default: the composed backward
        O2.backward(G)
        torch.cuda.synchronize()
        for a, b in ((O, O2), (Q.grad, Q2.grad), (K.grad, K2.grad), (V.grad, V2.grad)):
            assert torch.equal(bits(a), bits(b))                         # k > 1 and dv > 1: the composition's bits
        got = [t.detach().cpu() for t in (O, Q.grad, K.grad, V.grad)]
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
    for name, a, b in zip(("O", "dQ", "dK", "dV"), got, (Oc.detach(), Qc.grad, Kc.grad, Vc.grad)):
        ref = float(b.abs().max())
        err = float((a - b).abs().max())
        print(f"{name}: max err {err:.3e} against dense torch, scale {ref:.3e}")
        assert a.shape == b.shape and err <= 1e-10 * ref, name
    assert bool((got[1][7] == 0).all()) and bool((got[2][6] == 0).all()) and bool((got[3][6] == 0).all())   # the empty row and column


def test_width_one_matches_dense_torch():
    """k = dv = 1: the fused call keeps spmm's executor, so only the tolerance is promised against the composed backward"""
    import torch
    from spmv_amd import autograd
    csr = random_pattern(40, 30)
    h, _ = device_handle(csr)
    with h:
        ops = [rand((csr.m, 1), 1), rand((csr.n, 1), 2), rand((csr.n, 1), 3)]
        a = [t.clone().requires_grad_(True) for t in ops]
        b = [t.clone().requires_grad_(True) for t in ops]
        autograd.attention(h, *a, 0.7, backward="fused").sum().backward()
        autograd.attention(h, *b, 0.7).sum().backward()
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            ref = float(y.grad.abs().max())
            assert float((x.grad - y.grad).abs().max()) <= 1e-10 * ref


def test_the_fused_backward_is_one_call_and_leaves_the_values_alone(monkeypatch):
    import torch
    from spmv_amd import autograd
    csr = random_pattern(40, 30)
    h, va = device_handle(csr)
    with h:
        X, x0, x1 = rand((csr.n, 3), 7), rand((csr.n,), 11), rand((csr.m,), 8)
        values = (va * 2 + 1).requires_grad_(True)
        before = autograd.matmul(h, X, values=values).detach().clone()
        before_v = h.spmv(x0, torch.empty(csr.m, dtype=torch.float64, device=DEV)).clone()
        before_t = h.spmv_transpose(x1).clone()
        token, ref, keep = getattr(h, "_values_token", None), getattr(h, "_values_ref", None), h._keep[2]
        calls = []
        for name in ("update_values", "sddmm", "row_softmax", "row_softmax_backward", "spmm", "spmm_transpose", "attention_backward"):
            real = getattr(api.Handle, name)
            monkeypatch.setattr(api.Handle, name, (lambda real, name: lambda self, *a, **kw: (calls.append((name, kw)), real(self, *a, **kw))[1])(real, name))
        full = [rand((csr.m, 5), 9).requires_grad_(True), rand((csr.n, 5), 10).requires_grad_(True), rand((csr.n, 4), 12).requires_grad_(True)]
        autograd.attention(h, *full, backward="fused").sum().backward()
        assert [c[0] for c in calls] == ["attention_backward"] and calls[0][1]["need"] == (True, True, True)
        assert getattr(h, "_values_token", None) is token and getattr(h, "_values_ref", None) is ref and h._keep[2] is keep
        # needs_input_grad reaches `need`; the other gradients stay None
        for which in range(3):
            ops = [t.detach().clone().requires_grad_(i == which) for i, t in enumerate(full)]
            del calls[:]
            autograd.attention(h, *ops, backward="fused").sum().backward()
            assert [c[0] for c in calls] == ["attention_backward"] and calls[0][1]["need"] == tuple(i == which for i in range(3)), (which, calls)
            assert torch.equal(bits(ops[which].grad), bits(full[which].grad))
            assert all(t.grad is None for i, t in enumerate(ops) if i != which)
        monkeypatch.undo()
        after = autograd.matmul(h, X, values=values).detach()
        after_v = h.spmv(x0, torch.empty(csr.m, dtype=torch.float64, device=DEV))
        after_t = h.spmv_transpose(x1)
        torch.cuda.synchronize()
        assert torch.equal(bits(before), bits(after)) and torch.equal(bits(before_v), bits(after_v)) and torch.equal(bits(before_t), bits(after_t))


def test_wrong_arguments_raise():
    import torch
    from spmv_amd import autograd
    csr = random_pattern()
    h, _ = device_handle(csr)
    with h:
        Q, K, V = (torch.zeros(s, dtype=torch.float64, device=DEV) for s in ((csr.m, 2), (csr.n, 2), (csr.n, 3)))
        for bad in ("Fused", "both", "", None):
            with pytest.raises(ValueError):
                autograd.attention(h, Q, K, V, backward=bad)
        with pytest.raises(TypeError):
            autograd.attention(h, Q.float(), K, V, backward="fused")
        with pytest.raises(ValueError):
            autograd.attention(h, Q[:-1], K, V, backward="fused")


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
            autograd.attention(h, Q, Q, Q, backward="fused")
    csr = random_pattern(40, 30)
    api.set_thread_option("gpus", 1)
    try:
        h = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial)
    finally:
        api.clear_thread_options()
    with h:
        Q, K = (torch.zeros(s, dtype=torch.float64, device=DEV) for s in ((csr.m, 2), (csr.n, 2)))
        with pytest.raises(ValueError):
            autograd.attention(h, Q, K, K, backward="fused")
