"""GPU: spmv_amd.autograd.row_softmax and spmv_amd.autograd.sddmm, and with autograd.matmul the sparse attention
softmax_rows(Q K^T on A's pattern) V on the library's kernels, forward and backward.

Bars: torch.autograd.gradcheck in fp64 with its default tolerances through the real kernels; the composition against dense torch on the CPU
in float64 to 1e-10 relative (k <= 8 and rows of <= 8 entries: the error is a few hundred unit roundoffs of 1.1e-16)."""
import numpy as np
import pytest

from conftest import load_golden
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


def random_pattern(m=40, n=30, seed=4):
    """40 x 30 with an empty row (7) and an empty column (11)"""
    rng = np.random.default_rng(seed)
    cols_ok = np.array([c for c in range(n) if c != 11], dtype=np.int32)
    lens = rng.integers(1, 9, m)
    lens[7] = 0
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(cols_ok, int(l), replace=False)) for l in lens]).astype(np.int32)
    csr = synth.CSR(m, n, rp, ci, rng.uniform(-1, 1, int(rp[-1])))
    assert (np.diff(rp) == 0).any() and 11 not in ci
    return csr


def the_case(case):
    return load_golden("tiny_f64_uniform")[0] if case == "tiny" else random_pattern()


def rand(shape, seed):
    import torch
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.rand(shape, generator=g, device=DEV, dtype=torch.float64) * 2 - 1


# ----------------------------------------------------------------------------- 1. gradcheck through the kernels
@pytest.mark.parametrize("case", ["tiny", "random"])
def test_gradcheck_row_softmax(case):
    import torch
    from spmv_amd import autograd
    csr = the_case(case)
    h, _ = device_handle(csr)
    with h:
        S = (rand((csr.nnz,), 1) * 3).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda s: autograd.row_softmax(h, s), (S,))     # default eps / atol / rtol


@pytest.mark.parametrize("wrt", ["U", "V", "both"])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("case", ["tiny", "random"])
def test_gradcheck_sddmm(case, k, wrt):
    import torch
    from spmv_amd import autograd
    csr = the_case(case)
    h, _ = device_handle(csr)
    with h:
        U = rand((csr.m, k), 2).requires_grad_(wrt in ("U", "both"))
        V = rand((csr.n, k), 3).requires_grad_(wrt in ("V", "both"))
        if wrt == "U":
            fn, inputs = (lambda u: autograd.sddmm(h, u, V)), (U,)
        elif wrt == "V":
            fn, inputs = (lambda v: autograd.sddmm(h, U, v)), (V,)
        else:
            fn, inputs = (lambda u, v: autograd.sddmm(h, u, v)), (U, V)
        assert torch.autograd.gradcheck(fn, inputs)


@pytest.mark.parametrize("case", ["tiny", "random"])
def test_gradcheck_attention(case):
    import torch
    from spmv_amd import autograd
    csr = the_case(case)
    h, _ = device_handle(csr)
    with h:
        Q, K, Vf = rand((csr.m, 4), 4).requires_grad_(True), rand((csr.n, 4), 5).requires_grad_(True), rand((csr.n, 3), 6).requires_grad_(True)
        fn = lambda q, k, v: autograd.matmul(h, v, values=autograd.row_softmax(h, autograd.sddmm(h, q, k)))
        assert torch.autograd.gradcheck(fn, (Q, K, Vf))


# ----------------------------------------------------------------------------- 2. the composition against dense torch on the CPU
def test_attention_against_dense_torch():
    import torch
    from spmv_amd import autograd
    csr = random_pattern()
    k, kv = 8, 6
    rng = np.random.default_rng(3)
    Qh, Kh, Vh, Gh = rng.uniform(-1, 1, (csr.m, k)), rng.uniform(-1, 1, (csr.n, k)), rng.uniform(-1, 1, (csr.n, kv)), rng.uniform(-1, 1, (csr.m, kv))
    h, _ = device_handle(csr)
    with h:
        Q, K, Vf = (torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (Qh, Kh, Vh))
        Y = autograd.matmul(h, Vf, values=autograd.row_softmax(h, autograd.sddmm(h, Q, K)))
        Y.backward(torch.from_numpy(Gh).to(DEV))
        torch.cuda.synchronize()
        got = [t.detach().cpu() for t in (Y, Q.grad, K.grad, Vf.grad)]
    mask = torch.zeros((csr.m, csr.n), dtype=torch.bool)
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    mask[torch.from_numpy(rows), torch.from_numpy(csr.colidx.astype(np.int64))] = True
    Qc, Kc, Vc = (torch.from_numpy(a).requires_grad_(True) for a in (Qh, Kh, Vh))
    scores = (Qc @ Kc.T).masked_fill(~mask, float("-inf"))
    some = mask.any(1, keepdim=True)
    P = torch.where(some, torch.softmax(torch.where(some, scores, torch.zeros_like(scores)), dim=1), torch.zeros_like(scores))
    P = torch.where(mask, P, torch.zeros_like(P))          # the empty pattern row: zeros
    Yc = P @ Vc
    Yc.backward(torch.from_numpy(Gh))
    assert bool((Yc[7] == 0).all())
    for name, a, b in zip(("Y", "dQ", "dK", "dV"), got, (Yc.detach(), Qc.grad, Kc.grad, Vc.grad)):
        err = float((a - b).abs().max())
        scale = float(b.abs().max())
        print(f"{name}: max err {err:.3e}, scale {scale:.3e}")
        assert a.shape == b.shape and err <= 1e-10 * scale, name
    assert bool((got[1][7] == 0).all()) and bool((got[2][11] == 0).all()) and bool((got[3][11] == 0).all())   # the empty row and column


# ----------------------------------------------------------------------------- 3. the handle's values survive sddmm's backward
@pytest.mark.parametrize("held", ["create-time array", "matmul tensor"])
def test_sddmm_backward_puts_the_values_back(held):
    import torch
    from spmv_amd import autograd
    csr = random_pattern()
    h, va = device_handle(csr)
    with h:
        X, x1 = rand((csr.n, 3), 7), rand((csr.m,), 8)
        values = None
        if held == "matmul tensor":
            values = (va * 2 + 1).requires_grad_(True)
            autograd.matmul(h, X, values=values)
        before = autograd.matmul(h, X, values=values).detach().clone()
        before_t = h.spmv_transpose(x1).clone()
        token, ref, keep = getattr(h, "_values_token", None), getattr(h, "_values_ref", None), h._keep[2]
        U, V = rand((csr.m, 5), 9).requires_grad_(True), rand((csr.n, 5), 10).requires_grad_(True)
        autograd.sddmm(h, U, V).sum().backward()
        assert U.grad is not None and V.grad is not None
        assert getattr(h, "_values_token", None) == token and getattr(h, "_values_ref", None) is ref and h._keep[2] is keep
        after = autograd.matmul(h, X, values=values).detach()
        after_none = autograd.matmul(h, X).detach()
        after_t = h.spmv_transpose(x1)
        torch.cuda.synchronize()
        assert torch.equal(before.view(torch.int64), after.view(torch.int64))
        assert torch.equal(before.view(torch.int64), after_none.view(torch.int64))
        assert torch.equal(before_t.view(torch.int64), after_t.view(torch.int64))
        # only the gradient asked for is computed
        U2 = rand((csr.m, 5), 9).requires_grad_(True)
        autograd.sddmm(h, U2, V.detach()).sum().backward()
        assert torch.equal(U2.grad, U.grad)


# ----------------------------------------------------------------------------- 4. argument checks
def test_wrong_arguments_raise():
    import torch
    from spmv_amd import autograd
    csr = random_pattern()
    h, _ = device_handle(csr)
    with h:
        S = torch.zeros(csr.nnz, dtype=torch.float64, device=DEV)
        U, V = torch.zeros((csr.m, 2), dtype=torch.float64, device=DEV), torch.zeros((csr.n, 2), dtype=torch.float64, device=DEV)
        with pytest.raises(TypeError):
            autograd.row_softmax(h, S.float())
        with pytest.raises(TypeError):
            autograd.row_softmax(h, S.cpu())
        with pytest.raises(TypeError):
            autograd.row_softmax(h, S.cpu().numpy())
        with pytest.raises(ValueError):
            autograd.row_softmax(h, S[:-1])
        with pytest.raises(TypeError):
            autograd.sddmm(h, U.float(), V)
        with pytest.raises(TypeError):
            autograd.sddmm(h, U, V.cpu())
        with pytest.raises(ValueError):
            autograd.sddmm(h, U[:-1], V)
        with pytest.raises(ValueError):
            autograd.sddmm(h, U, V[:, :1])
        with pytest.raises(ValueError):
            autograd.sddmm(h, U[:, 0], V[:, 0])
