"""GPU: spmv_amd.autograd.matmul, Y = A X as a differentiable torch operation over spmv_hip_spmm (forward), spmv_hip_spmm_transpose
(dL/dX = A^T G) and spmv_hip_sddmm (dL/dvalues[p] = sum_c G[row(p), c] X[col(p), c]).

Bars: torch.autograd.gradcheck in fp64 with its default tolerances through the real kernels; gradients against a dense float64 CPU
computation -- dX with the per-row bars of test_gpu_spmm.check_block applied to A^T, dvalues with the gamma_k bar of test_gpu_sddmm."""
import numpy as np
import pytest

from conftest import load_golden
from spmv_amd import api, build, synth

pytestmark = pytest.mark.gpu

M = api.SPMV_METHODS
TOL = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-3}
SHARP = {np.dtype(np.float64): 64 * 2.3e-16, np.dtype(np.float32): 64 * 1.2e-7}
UNIT = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def device_handle(csr, method=M.Method_Parallel, **opts):
    """(handle on device arrays, values tensor)"""
    import torch
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    for k, v in opts.items():
        api.set_thread_option(k, v)
    try:
        return api.Handle(csr.m, csr.n, rp, ci, va, method), va
    finally:
        api.clear_thread_options()


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


def dense(csr):
    A = np.zeros((csr.m, csr.n))
    rows = np.repeat(np.arange(csr.m), np.diff(csr.rowptr))
    np.add.at(A, (rows, csr.colidx), csr.val.astype(np.float64))
    return A, rows


# ----------------------------------------------------------------------------- 1. gradcheck through the kernels
GRAD_CASES = [("tiny", 3), ("random", 1), ("random", 5), ("random", None)]   # None: a 1-D X


@pytest.mark.parametrize("wrt", ["X", "values", "both"])
@pytest.mark.parametrize("case,k", GRAD_CASES, ids=[f"{c}-k{k}" for c, k in GRAD_CASES])
def test_gradcheck(case, k, wrt):
    import torch
    from spmv_amd import autograd
    csr = load_golden("tiny_f64_uniform")[0] if case == "tiny" else random_pattern()
    h, va = device_handle(csr)
    with h:
        g = torch.Generator(device=DEV); g.manual_seed(1)
        shape = (csr.n,) if k is None else (csr.n, k)
        X = (torch.rand(shape, generator=g, device=DEV, dtype=torch.float64) * 2 - 1).requires_grad_(wrt in ("X", "both"))
        values = va.clone().requires_grad_(wrt in ("values", "both"))
        inputs = {"X": (X,), "values": (values,), "both": (X, values)}[wrt]
        # gradcheck perturbs its inputs through tensor.data, behind the version counter the values token is made of: the values enter
        # through clone(), a new tensor per evaluation (what an optimiser step or any op upstream of matmul produces)
        if wrt == "X":
            fn = lambda x: autograd.matmul(h, x, values)
        elif wrt == "values":
            fn = lambda v: autograd.matmul(h, X, v.clone())
        else:
            fn = lambda x, v: autograd.matmul(h, x, v.clone())
        assert torch.autograd.gradcheck(fn, inputs)     # default eps / atol / rtol


# ----------------------------------------------------------------------------- 2. gradients against a dense float64 computation
@pytest.mark.parametrize("name", ["powerlaw_f32_uniform", "powerlaw_f64_uniform", "banded_wide_f32_uniform", "banded_wide_f64_uniform"])
def test_gradients_against_dense(name):
    import torch
    from spmv_amd import autograd
    csr = load_golden(name)[0]
    dt = csr.val.dtype
    A, rows = dense(csr)
    rng = np.random.default_rng(2)
    k = 6
    Xh, Gh = rng.uniform(-1, 1, (csr.n, k)).astype(dt), rng.uniform(-1, 1, (csr.m, k)).astype(dt)
    h, va = device_handle(csr)
    with h:
        X = torch.from_numpy(Xh).to(DEV).requires_grad_(True)
        values = va.clone().requires_grad_(True)
        Y = autograd.matmul(h, X, values)
        assert Y.shape == (csr.m, k) and Y.requires_grad
        Y.backward(torch.from_numpy(Gh).to(DEV))
        torch.cuda.synchronize()
        dX, dV = X.grad.cpu().numpy(), values.grad.cpu().numpy()
        direct = h.spmm(X.detach())
        torch.cuda.synchronize()
        assert torch.equal(Y.detach().view(torch.int32), direct.view(torch.int32))     # the bits of a direct Handle.spmm
    assert dX.dtype == dt and dV.dtype == dt and dV.shape == (csr.nnz,)
    G64, X64 = Gh.astype(np.float64), Xh.astype(np.float64)
    # dX = A^T G: the per-row bars of check_block, the rows being those of A^T
    want = A.T @ G64
    s = np.abs(A).T @ np.abs(G64)
    cnt = np.maximum(1, np.bincount(csr.colidx, minlength=csr.n))[:, None]
    err = np.abs(dX.astype(np.float64) - want)
    assert (err <= TOL[np.dtype(dt)] * s + 1e-300).all()
    assert (err <= SHARP[np.dtype(dt)] * cnt * s + 1e-300).all()
    # dvalues = (G X^T)[rows, cols]: the gamma_k bar
    prod = G64[rows] * X64[csr.colidx]
    errv = np.abs(dV.astype(np.float64) - prod.sum(1))
    bar = (k + 1) * UNIT[np.dtype(dt)] * np.abs(prod).sum(1)
    print(f"{name}: dvalues max err / bar = {float((errv / np.maximum(bar, 1e-300)).max(initial=0)):.3f}")
    assert (errv <= bar).all()


# ----------------------------------------------------------------------------- 3. the values token
def test_backward_uses_the_forward_pass_values():
    import torch
    from spmv_amd import autograd
    csr = load_golden("powerlaw_f64_eighths")[0]
    A1, rows = dense(csr)
    h, va = device_handle(csr)
    with h:
        g = torch.Generator(device=DEV); g.manual_seed(3)
        X = (torch.randint(-8, 9, (csr.n, 4), generator=g, device=DEV) * 0.125).double().requires_grad_(True)
        G = (torch.randint(-8, 9, (csr.m, 4), generator=g, device=DEV) * 0.125).double()
        v1 = va.clone().requires_grad_(True)
        v2 = (va * 2).requires_grad_(True)
        Y1 = autograd.matmul(h, X, v1)
        Y2 = autograd.matmul(h, X, v2)          # the handle now holds v2
        torch.cuda.synchronize()
        assert torch.equal(Y2, 2 * Y1)
        Y1.backward(G)                           # ... and must multiply by v1's matrix again
        torch.cuda.synchronize()
        want = torch.from_numpy(A1.T).to(DEV) @ G   # eighths: exact in every order
        assert torch.equal(X.grad, want)
        assert v2.grad is None and v1.grad is not None
        # unchanged tensor state: no second upload (same token); an in-place change is seen
        token = h._values_token
        autograd.matmul(h, X, v1)
        assert h._values_token == token
        with torch.no_grad():
            v1.mul_(0.5)
        Y3 = autograd.matmul(h, X.detach(), v1)
        torch.cuda.synchronize()
        assert h._values_token != token
        assert torch.equal(Y3, 0.5 * Y1.detach())


def test_constant_matrix_builds_no_graph_into_it():
    import torch
    from spmv_amd import autograd
    csr = load_golden("banded_f64_eighths")[0]
    A, _ = dense(csr)
    h, va = device_handle(csr)
    with h:
        X = torch.ones((csr.n, 3), dtype=torch.float64, device=DEV)
        assert not autograd.matmul(h, X).requires_grad           # nothing to differentiate
        assert not autograd.matmul(h, X, va).requires_grad
        Xg = X.clone().requires_grad_(True)
        Y = autograd.matmul(h, Xg)
        assert Y.requires_grad
        Y.sum().backward()
        torch.cuda.synchronize()
        assert va.grad is None
        assert torch.equal(Xg.grad, torch.from_numpy(A.T.sum(1, keepdims=True).repeat(3, 1)).to(DEV))


# ----------------------------------------------------------------------------- 4. layouts and streams
def test_strided_and_transposed_operands():
    import torch
    from spmv_amd import autograd
    csr = load_golden("powerlaw_f64_eighths")[0]
    A, _ = dense(csr)
    At = torch.from_numpy(A).to(DEV)
    h, va = device_handle(csr)
    with h:
        g = torch.Generator(device=DEV); g.manual_seed(6)
        wide = (torch.randint(-8, 9, (csr.n, 9), generator=g, device=DEV) * 0.125).double()
        wide[:, 5:] = float("nan")
        Xv = wide[:, :5].detach().requires_grad_(True)                      # row stride 9 > k = 5; NaN in the padding
        leaf = wide.clone().requires_grad_(True)
        Y = autograd.matmul(h, leaf[:, :5])
        assert torch.equal(Y.detach(), At @ wide[:, :5])
        Y.sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(leaf.grad[:, :5], At.T.sum(1, keepdim=True).expand(-1, 5)) and bool((leaf.grad[:, 5:] == 0).all())
        assert torch.equal(autograd.matmul(h, Xv).detach(), Y.detach())
        Xt = (torch.randint(-8, 9, (5, csr.n), generator=g, device=DEV) * 0.125).double().requires_grad_(True)
        Yt = autograd.matmul(h, Xt.t())                                      # column stride != 1: made contiguous
        assert torch.equal(Yt.detach(), At @ Xt.detach().t())
        Yt.sum().backward()
        assert torch.equal(Xt.grad, At.T.sum(1, keepdim=True).expand(-1, 5).t())
        # a side stream: calls run on torch's current stream
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            Ys = autograd.matmul(h, wide[:, :5])
        s.synchronize()
        assert h.attached == (s.cuda_stream, True)
        assert torch.equal(Ys, Y.detach())
        Y0 = autograd.matmul(h, wide[:, :5])
        torch.cuda.synchronize()
        assert h.attached == (torch.cuda.current_stream().cuda_stream, True) and torch.equal(Y0, Ys)


# ----------------------------------------------------------------------------- 5. errors
def test_errors():
    import torch
    from spmv_amd import autograd
    csr = load_golden("banded_f64_uniform")[0]
    h, va = device_handle(csr)
    with h:
        X = torch.ones((csr.n, 2), dtype=torch.float64, device=DEV)
        with pytest.raises(TypeError):
            autograd.matmul(h, X.float())
        with pytest.raises(TypeError):
            autograd.matmul(h, X.cpu())
        with pytest.raises(TypeError):
            autograd.matmul(h, X, va.float())
        with pytest.raises(TypeError):
            autograd.matmul(h, X, va.cpu())
        with pytest.raises(ValueError):
            autograd.matmul(h, X[:-1])
        with pytest.raises(ValueError):
            autograd.matmul(h, X, va[:-1])
    import torch as _t
    m, n, rp, ci, vv = synth.banded_holes_device(100_000, 100_000, 24, 0.25, "eighths", _t.float64, DEV, 7)
    api.set_thread_option("reorder", 1)
    try:
        hr = api.Handle(m, n, rp, ci, vv, M.Method_Parallel)
    finally:
        api.clear_thread_options()
    with hr:
        assert hr.index is not None
        with pytest.raises(ValueError):
            autograd.matmul(hr, torch.ones((n, 2), dtype=torch.float64, device=DEV))
    api.set_thread_option("gpus", 1)
    try:
        hm = api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, M.Method_Serial)
    finally:
        api.clear_thread_options()
    with hm:
        with pytest.raises(ValueError):
            autograd.matmul(hm, torch.ones((csr.n, 2), dtype=torch.float64, device=DEV))
