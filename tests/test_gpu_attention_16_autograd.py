"""GPU: spmv_amd.autograd.attention, attention_heads and attention_parts on torch.float16 / torch.bfloat16 Q, K and V over float32 handles.

The contract has no tolerance: O is fp32_result.to(dtype) and every gradient of Q, K and V is fp32_gradient.to(dtype), where the float32 results are
those of the SAME function on .float() leaves with dL/dO.float(); the bias stays float32 and its gradient has the float32 run's bits.  Compared by
integer views, NaN positions equal."""
import numpy as np
import pytest
import torch

from gqa_cases import DEV, M, pattern_a
from lse_cases import part_bias, parts_a
from spmv_amd import api, build

pytestmark = pytest.mark.gpu

TYPES = [torch.float16, torch.bfloat16]
TYPE_IDS = ["f16", "bf16"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def device_handle(csr, method=M.Method_Parallel):
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    return api.Handle(csr.m, csr.n, rp, ci, va, method)


def rand(shape, seed, lo=-1.0, hi=1.0, dtype=torch.float32):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.rand(shape, generator=g, device=DEV, dtype=torch.float64) * (hi - lo) + lo).to(dtype)


def leaves(tensors, dtype=None):
    return [t.detach().clone().to(dtype or t.dtype).requires_grad_(True) for t in tensors]


def is_rounded(got, want32, dt):
    """got (of dt) has the bit pattern of want32.to(dt) wherever want32 is not NaN, and is NaN exactly where want32 is"""
    want, nan = want32.to(dt), torch.isnan(want32)
    return got.dtype == dt and got.shape == want.shape and torch.equal(torch.isnan(got), nan) and \
        torch.equal(got.detach().contiguous().view(torch.int16)[~nan], want.contiguous().view(torch.int16)[~nan])


def same_bits32(a, b):
    return a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_both(fn, ops16, B, G16, dt):
    """fn(Q, K, V, bias) on the 16-bit leaves with dL/dO = G16 and on their .float() copies with G16.float(): held against each other, -> None"""
    Q, K, V = leaves(ops16)
    Bh = None if B is None else leaves([B])[0]
    O = fn(Q, K, V, Bh)
    grads = torch.autograd.grad(O, [Q, K, V] + ([] if B is None else [Bh]), G16)
    Qf, Kf, Vf = leaves(ops16, torch.float32)
    Bf = None if B is None else leaves([B])[0]
    Of = fn(Qf, Kf, Vf, Bf)
    want = torch.autograd.grad(Of, [Qf, Kf, Vf] + ([] if B is None else [Bf]), G16.float())
    assert Of.dtype == torch.float32 and is_rounded(O, Of.detach(), dt), "O"
    for name, g, w in zip(("dQ", "dK", "dV"), grads, want):
        assert is_rounded(g, w, dt), name
    if B is not None:
        assert same_bits32(grads[3], want[3]), "dB"
        assert bool(grads[3].ne(0).any())


@pytest.mark.parametrize("mode", ["per_head", "fused"])
@pytest.mark.parametrize("kv", [None, 2], ids=["mha", "gqa"])
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_attention_heads(dt, kv, mode):
    """both backward= modes, with and without kv_heads, an fp32 bias that requires grad (a plane per head, then one shared plane)"""
    from spmv_amd import autograd
    csr = pattern_a(np.float32)
    heads, k, dv = 4, 5, 4
    g = heads if kv is None else kv
    ops = [rand(s, i).to(dt) for i, s in enumerate(((csr.m, heads * k), (csr.n, g * k), (csr.n, g * dv)))]
    G = rand((csr.m, heads * dv), 9).to(dt)
    with device_handle(csr) as h:
        for B in (rand((heads, csr.nnz), 7, -2, 2), rand((csr.nnz,), 8, -2, 2), None):
            run_both(lambda Q, K, V, b: autograd.attention_heads(h, Q, K, V, heads, 0.4, mode, bias=b, kv_heads=kv), ops, B, G, dt)


@pytest.mark.parametrize("mode", ["composed", "fused"])
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_attention(dt, mode):
    from spmv_amd import autograd
    csr = pattern_a(np.float32)
    k, dv = 5, 4
    ops = [rand(s, i).to(dt) for i, s in enumerate(((csr.m, k), (csr.n, k), (csr.n, dv)))]
    G = rand((csr.m, dv), 9).to(dt)
    x = rand((csr.n,), 11)
    with device_handle(csr) as h:
        y0 = torch.full((csr.m,), float("nan"), device=DEV)
        h.spmv(x, y0)
        for B in (rand((csr.nnz,), 7, -2, 2), None):
            run_both(lambda Q, K, V, b: autograd.attention(h, Q, K, V, None, mode, bias=b), ops, B, G, dt)
        y1 = torch.full((csr.m,), float("nan"), device=DEV)
        h.spmv(x, y1)
        torch.cuda.synchronize()
        assert same_bits32(y0, y1)   # the composed backward puts the handle's values back


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_attention_parts_over_two_handles(dt):
    """pattern A split by column into two handles (lse_cases.parts_a), 4 query heads over 2, a bias per part: each part is a _16 call with fp32 O and L,
    the fold stays fp32 and the merged O is rounded once -- so O and the gradients are the fp32 function's on .float() leaves, rounded once; L is fp32
    and has its bits"""
    from spmv_amd import autograd
    csr, parts, bounds = parts_a(np.float32, 2)
    heads, kv, k, dv = 4, 2, 5, 3
    Q16 = rand((csr.m, heads * k), 0).to(dt)
    K16, V16 = rand((csr.n, kv * k), 1).to(dt), rand((csr.n, kv * dv), 2).to(dt)
    G = rand((csr.m, heads * dv), 9).to(dt)
    Bfull = rand((heads, csr.nnz), 7, -2, 2).cpu().numpy()
    Bs = [torch.from_numpy(part_bias(Bfull, parts[0][1])).to(DEV), torch.from_numpy(part_bias(Bfull[0], parts[1][1])).to(DEV)]   # planes, then one shared plane
    hs = [device_handle(p) for p, _ in parts]
    try:
        def run(dtype, Gin):
            Q = leaves([Q16], dtype)[0]
            Ks = leaves([K16[:bounds[0]], K16[bounds[0]:]], dtype)
            Vs = leaves([V16[:bounds[0]], V16[bounds[0]:]], dtype)
            bs = leaves(Bs)
            O, L = autograd.attention_parts(hs, Q, Ks, Vs, heads, 0.4, kv_heads=kv, biases=bs, return_lse=True)
            return O, L, torch.autograd.grad(O, [Q, *Ks, *Vs, *bs], Gin)
        O, L, grads = run(None, G)
        Of, Lf, want = run(torch.float32, G.float())
        assert is_rounded(O, Of.detach(), dt) and same_bits32(L, Lf) and not L.requires_grad
        for i, (g, w) in enumerate(zip(grads[:5], want[:5])):
            assert is_rounded(g, w, dt), i
        for g, w in zip(grads[5:], want[5:]):
            assert same_bits32(g, w)
    finally:
        for h in hs:
            h.close()


def test_mixed_dtypes_and_an_fp64_handle_raise():
    from spmv_amd import autograd
    csr = pattern_a(np.float32)
    heads, k, dv = 2, 4, 4
    Q, K, V = (torch.ones(s, device=DEV, dtype=torch.float16) for s in ((csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv)))
    with device_handle(csr) as h:
        for bad in ((Q, K.bfloat16(), V), (Q, K, V.float()), (Q.float(), K, V), (Q.bfloat16(), K, V)):
            with pytest.raises(TypeError, match="the handle holds torch.float32"):
                autograd.attention_heads(h, *bad, heads)
            with pytest.raises(TypeError, match="the handle holds torch.float32"):
                autograd.attention_parts([h], bad[0], [bad[1]], [bad[2]], heads)
        with pytest.raises(TypeError, match="the handle holds torch.float32"):
            autograd.attention(h, Q[:, :k], K[:, :k].bfloat16(), V[:, :dv])
        with pytest.raises(TypeError):   # the bias stays float32
            autograd.attention_heads(h, Q, K, V, heads, bias=torch.zeros((heads, csr.nnz), device=DEV, dtype=torch.float16))
    csr64 = pattern_a(np.float64)
    with device_handle(csr64) as h:
        for dt in TYPES:
            with pytest.raises(TypeError, match="the handle holds torch.float64"):
                autograd.attention_heads(h, Q.to(dt), K.to(dt), V.to(dt), heads)
            with pytest.raises(TypeError, match="the handle holds torch.float64"):
                autograd.attention(h, Q[:, :k].to(dt), K[:, :k].to(dt), V[:, :dv].to(dt))
            with pytest.raises(TypeError, match="the handle holds torch.float64"):
                autograd.attention_parts([h], Q.to(dt), [K.to(dt)], [V.to(dt)], heads)
