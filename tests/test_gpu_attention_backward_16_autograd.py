"""GPU: the backward of spmv_amd.autograd.attention, attention_heads and attention_parts on torch.float16 / torch.bfloat16 tensors goes through
Handle.attention_gqa_backward_16 -- no float32 copy of Q, K, V or dL/dO, no float32 backward entry point of the handle -- and keeps the contract to
the bit: every gradient of Q, K and V is fp32_gradient.to(dtype), the float32 gradients being those of the SAME function on .float() leaves with
dL/dO.float(); the bias gradient stays float32 and has the float32 run's bits.  Compared by integer views, NaN positions equal."""
import numpy as np
import pytest
import torch

from gqa_cases import DEV, pattern_a
from lse_cases import part_bias, parts_a
from spmv_amd import api, build
from test_gpu_attention_16_autograd import device_handle, is_rounded, leaves, rand, same_bits32

pytestmark = pytest.mark.gpu

TYPES = [torch.float16, torch.bfloat16]
TYPE_IDS = ["f16", "bf16"]
FP32_BACKWARDS = ["attention_backward", "attention_heads_backward", "attention_bias_backward", "attention_gqa_backward", "attention_gqa_backward_lse"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


class Counting:
    """for the duration: counting wrappers around Handle.attention_gqa_backward_16, around the module's attention_gqa_backward_16 (which the Handle method
    and the per-head loop both call) and around every float32 backward entry point of the handle; all restored on the way out"""

    def __enter__(self):
        self.n = {"handle16": 0, "call16": 0, "fp32": 0}
        self.dtypes = []
        self.kept = {name: getattr(api.Handle, name) for name in ["attention_gqa_backward_16"] + FP32_BACKWARDS}
        self.kept_fn = api.attention_gqa_backward_16

        def count16(h, *a, **kw):
            self.n["handle16"] += 1
            out = self.kept["attention_gqa_backward_16"](h, *a, **kw)
            self.dtypes.append(tuple(None if g is None else g.dtype for g in out))
            return out

        def call16(*a, **kw):
            self.n["call16"] += 1
            return self.kept_fn(*a, **kw)

        def fp32(name):
            def f(h, *a, **kw):
                self.n["fp32"] += 1
                return self.kept[name](h, *a, **kw)
            return f

        api.Handle.attention_gqa_backward_16 = count16
        api.attention_gqa_backward_16 = call16
        for name in FP32_BACKWARDS:
            setattr(api.Handle, name, fp32(name))
        return self

    def __exit__(self, *exc):
        for name, f in self.kept.items():
            setattr(api.Handle, name, f)
        api.attention_gqa_backward_16 = self.kept_fn


def run_both(fn, ops16, B, G16, dt):
    """fn(Q, K, V, bias) on the 16-bit leaves with dL/dO = G16 (under the counting wrappers) and on their .float() copies with G16.float(): the gradients
    held against each other; -> the counts of the 16-bit run"""
    Q, K, V = leaves(ops16)
    Bh = None if B is None else leaves([B])[0]
    O = fn(Q, K, V, Bh)
    with Counting() as c:
        grads = torch.autograd.grad(O, [Q, K, V] + ([] if B is None else [Bh]), G16)
    assert api.Handle.attention_gqa_backward_16 is c.kept["attention_gqa_backward_16"] and api.attention_gqa_backward_16 is c.kept_fn
    Qf, Kf, Vf = leaves(ops16, torch.float32)
    Bf = None if B is None else leaves([B])[0]
    Of = fn(Qf, Kf, Vf, Bf)
    want = torch.autograd.grad(Of, [Qf, Kf, Vf] + ([] if B is None else [Bf]), G16.float())
    for name, g, w in zip(("dQ", "dK", "dV"), grads, want):
        assert is_rounded(g, w, dt), name
    if B is not None:
        assert same_bits32(grads[3], want[3]) and bool(grads[3].ne(0).any()), "dB"
    return c


@pytest.mark.parametrize("mode", ["per_head", "fused"])
@pytest.mark.parametrize("kv", [None, 2], ids=["mha", "gqa"])
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_attention_heads(dt, kv, mode):
    """both backward= modes, with and without kv_heads, an fp32 bias that requires grad (a plane per head, one shared plane, none): fused is ONE
    Handle.attention_gqa_backward_16 call with 16-bit gradients, per_head one attention_gqa_backward_16 call per head; no float32 backward either way"""
    from spmv_amd import autograd
    csr = pattern_a(np.float32)
    heads, k, dv = 4, 5, 4
    g = heads if kv is None else kv
    ops = [rand(s, i).to(dt) for i, s in enumerate(((csr.m, heads * k), (csr.n, g * k), (csr.n, g * dv)))]
    G = rand((csr.m, heads * dv), 9).to(dt)
    with device_handle(csr) as h:
        for B in (rand((heads, csr.nnz), 7, -2, 2), rand((csr.nnz,), 8, -2, 2), None):
            c = run_both(lambda Q, K, V, b: autograd.attention_heads(h, Q, K, V, heads, 0.4, mode, bias=b, kv_heads=kv), ops, B, G, dt)
            assert c.n["fp32"] == 0
            if mode == "fused":
                assert c.n["handle16"] == 1 and c.n["call16"] == 1 and c.dtypes[0][:3] == (dt, dt, dt)
            else:
                assert c.n["handle16"] == 0 and c.n["call16"] == heads


@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_attention_fused(dt):
    from spmv_amd import autograd
    csr = pattern_a(np.float32)
    k, dv = 5, 4
    ops = [rand(s, i).to(dt) for i, s in enumerate(((csr.m, k), (csr.n, k), (csr.n, dv)))]
    G = rand((csr.m, dv), 9).to(dt)
    with device_handle(csr) as h:
        for B in (rand((csr.nnz,), 7, -2, 2), None):
            c = run_both(lambda Q, K, V, b: autograd.attention(h, Q, K, V, None, "fused", bias=b), ops, B, G, dt)
            assert c.n == {"handle16": 1, "call16": 1, "fp32": 0}


@pytest.mark.parametrize("nparts", [1, 2])
@pytest.mark.parametrize("dt", TYPES, ids=TYPE_IDS)
def test_attention_parts(dt, nparts):
    """one part (pattern A whole) and two (lse_cases.parts_a), 4 query heads over 2, a bias per part: one Handle.attention_gqa_backward_16 per part with
    the saved fp32 O and L; dK and dV 16-bit; dQ 16-bit with one part, fp32 per part -- summed in part order, rounded once -- with two"""
    from spmv_amd import autograd
    heads, kv, k, dv = 4, 2, 5, 3
    if nparts == 1:
        csr = pattern_a(np.float32)
        parts, bounds = [(csr, np.arange(csr.nnz))], [csr.n]
    else:
        csr, parts, bounds = parts_a(np.float32, 2)
    Q16 = rand((csr.m, heads * k), 0).to(dt)
    K16, V16 = rand((csr.n, kv * k), 1).to(dt), rand((csr.n, kv * dv), 2).to(dt)
    G = rand((csr.m, heads * dv), 9).to(dt)
    Bfull = rand((heads, csr.nnz), 7, -2, 2).cpu().numpy()
    Bs = [torch.from_numpy(part_bias(Bfull if r == 0 else Bfull[0], idx)).to(DEV) for r, (_, idx) in enumerate(parts)]   # planes, then one shared plane
    cuts = [0] + list(bounds)
    hs = [device_handle(p) for p, _ in parts]
    try:
        def run(dtype, Gin, counted):
            Q = leaves([Q16], dtype)[0]
            Ks = leaves([K16[cuts[r]:cuts[r + 1]] for r in range(nparts)], dtype)
            Vs = leaves([V16[cuts[r]:cuts[r + 1]] for r in range(nparts)], dtype)
            bs = leaves(Bs)
            O = autograd.attention_parts(hs, Q, Ks, Vs, heads, 0.4, kv_heads=kv, biases=bs)
            if not counted:
                return torch.autograd.grad(O, [Q, *Ks, *Vs, *bs], Gin), None
            with Counting() as c:
                return torch.autograd.grad(O, [Q, *Ks, *Vs, *bs], Gin), c
        grads, c = run(None, G, True)
        want, _ = run(torch.float32, G.float(), False)
        assert c.n == {"handle16": nparts, "call16": nparts, "fp32": 0}
        assert all(d[:3] == ((dt if nparts == 1 else torch.float32), dt, dt) for d in c.dtypes), c.dtypes
        nb = 1 + 2 * nparts
        for i, (g, w) in enumerate(zip(grads[:nb], want[:nb])):
            assert is_rounded(g, w, dt), i
        for g, w in zip(grads[nb:], want[nb:]):
            assert same_bits32(g, w)
    finally:
        for h in hs:
            h.close()
