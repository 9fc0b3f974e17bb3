"""GPU: spmv_amd.autograd.attention_parts -- attention over a key / value set cut into parts, one handle per part: one Handle.attention_gqa_lse per
part folded with Handle.attention_merge, and one Handle.attention_gqa_backward_lse per part with the merged O and L.

Bars: with one handle the forward has attention_heads' bits and the gradients its values (the value scheme of test_gpu_attention_backward_lse.py);
two and three parts give the unsplit handle's values, with kv_heads and per-part biases; torch.autograd.gradcheck in fp64 with its default
tolerances on the `tiny` golden split in two; a part without entries changes nothing; gradients that are not needed are not computed; the
handles' values are untouched."""
import numpy as np
import pytest

from conftest import load_golden
from gqa_cases import DEV, M, pattern_a
from lse_cases import err, part_bias, parts_a, reference, split
from spmv_amd import api, build

pytestmark = pytest.mark.gpu


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


def rand(shape, seed, lo=-1.0, hi=1.0, dtype=None):
    import torch
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.rand(shape, generator=g, device=DEV, dtype=torch.float64) * (hi - lo) + lo).to(dtype or torch.float64)


def spmv(h, x):
    import torch
    y = torch.full((h.m,), float("nan"), dtype=x.dtype, device=x.device)
    h.spmv(x, y)
    torch.cuda.synchronize()
    return y


def bits(t):
    import torch
    return t.detach().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def cut(K, V, bounds):
    """leaves for the parts: the rows of K and V between the bounds"""
    Ks, Vs, lo = [], [], 0
    for hi in bounds:
        Ks.append(K.detach()[lo:hi].clone().requires_grad_(True))
        Vs.append(V.detach()[lo:hi].clone().requires_grad_(True))
        lo = hi
    return Ks, Vs


FLOOR = 8   # roundings of the largest exact element: test_gpu_attention_backward_lse.py's floor


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_handle_is_attention_heads_with_the_lse_driven_backward(dt):
    import torch
    from spmv_amd import autograd
    dtype, tdt = (np.float64, torch.float64) if dt == "f64" else (np.float32, torch.float32)
    eps = float(np.finfo(dtype).eps)
    csr = pattern_a(dtype)
    heads, k, dv = 3, 5, 4
    with device_handle(csr) as h:
        Q, K, V = (rand(s, i, dtype=tdt).requires_grad_(True) for i, s in enumerate(((csr.m, heads * k), (csr.n, heads * k), (csr.n, heads * dv))))
        B = rand((heads, csr.nnz), 7, -2, 2, tdt).requires_grad_(True)
        G = rand((csr.m, heads * dv), 9, dtype=tdt)
        x = rand((csr.n,), 11, dtype=tdt)
        y0 = spmv(h, x)
        want = autograd.attention_heads(h, Q, K, V, heads, 0.4, "fused", bias=B)
        g_old = torch.autograd.grad(want, (Q, K, V, B), G)
        got = autograd.attention_parts([h], Q, [K], [V], heads, 0.4, biases=[B])
        assert torch.equal(bits(got), bits(want))              # the forward: bit-equal
        g_new = torch.autograd.grad(got, (Q, K, V, B), G)
        assert torch.equal(bits(spmv(h, x)), bits(y0))          # the handle's values: untouched
        ref = reference(csr, heads, heads, *(t.detach().cpu().numpy() for t in (Q, K, V, B)), 0.4, G.cpu().numpy())[2:]
        for name, o, n, r in zip(("dQ", "dK", "dV", "dB"), g_old, g_new, ref):
            e_old, e_new = err(o.cpu().numpy(), r), err(n.cpu().numpy(), r)
            assert e_new <= 8 * e_old + FLOOR * eps * float(np.abs(r).max()), (name, e_new, e_old)
        # (O, L) on request; L gets no gradient and is -inf on rows without entries
        O2, L = autograd.attention_parts([h], Q, [K], [V], heads, 0.4, biases=[B], return_lse=True)
        assert torch.equal(bits(O2), bits(want)) and tuple(L.shape) == (heads, csr.m) and not L.requires_grad
        assert torch.equal(torch.isneginf(L[0]).cpu(), torch.from_numpy(np.diff(csr.rowptr) == 0))


@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("combo", [(4, 2), (3, 1), (2, 2)], ids=["4over2", "3over1", "2over2"])
def test_parts_give_the_unsplit_handles_values(combo, nparts):
    """fp64, with kv_heads and a bias per part (a plane per head for the first part, one shared plane for the second, none for a third)"""
    import torch
    from spmv_amd import autograd
    heads, kv = combo
    dtype = np.float64
    eps = float(np.finfo(dtype).eps)
    csr, parts, bounds = parts_a(dtype, nparts)
    k, dv = 5, 3
    hs = [device_handle(p) for p, _ in parts]
    try:
        with device_handle(csr) as h:
            Q, K, V = (rand(s, i).requires_grad_(True) for i, s in enumerate(((csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv))))
            G = rand((csr.m, heads * dv), 9)
            # the unsplit bias that the parts' biases are pieces of
            Bfull = np.zeros((heads, csr.nnz))
            Bs = []
            for r, (p, idx) in enumerate(parts):
                if r == 0:
                    b = rand((heads, p.nnz), 20, -2, 2)
                    Bfull[:, idx] = b.cpu().numpy()
                elif r == 1:
                    b = rand((p.nnz,), 21, -2, 2)
                    Bfull[:, idx] = b.cpu().numpy()[None, :]
                else:
                    b = None
                Bs.append(None if b is None else b.requires_grad_(True))
            Bf = torch.from_numpy(Bfull).to(DEV).requires_grad_(True)
            x = [rand((p.n,), 30 + r) for r, (p, _) in enumerate(parts)]
            y0 = [spmv(hp, xr) for hp, xr in zip(hs, x)]
            want = autograd.attention_heads(h, Q, K, V, heads, None, "fused", bias=Bf, kv_heads=kv)
            g_old = torch.autograd.grad(want, (Q, K, V, Bf), G)
            Ks, Vs = cut(K, V, bounds)
            got = autograd.attention_parts(hs, Q, Ks, Vs, heads, kv_heads=kv, biases=Bs)
            leaves = [Q, *Ks, *Vs, *[b for b in Bs if b is not None]]
            g = torch.autograd.grad(got, leaves, G)
            for hp, xr, y in zip(hs, x, y0):
                assert torch.equal(bits(spmv(hp, xr)), bits(y))   # the handles' values: untouched
            n = len(parts)
            dQ, dK, dV = g[0], torch.cat(g[1:1 + n]), torch.cat(g[1 + n:1 + 2 * n])
            dB = np.zeros((heads, csr.nnz))
            gb = list(g[1 + 2 * n:])
            dB[:, parts[0][1]] = gb[0].cpu().numpy()
            shared = gb[1].cpu().numpy()   # a shared plane's gradient: the sum over the heads
            ref = reference(csr, heads, kv, *(t.detach().cpu().numpy() for t in (Q, K, V)), Bfull, 1.0 / np.sqrt(k), G.cpu().numpy())
            assert err(got.detach().cpu().numpy(), ref[0]) <= 8 * err(want.detach().cpu().numpy(), ref[0]) + FLOOR * eps * float(np.abs(ref[0]).max())
            for name, o, nw, r in zip(("dQ", "dK", "dV"), g_old, (dQ, dK, dV), ref[2:5]):
                e_old, e_new = err(o.cpu().numpy(), r), err(nw.cpu().numpy(), r)
                assert e_new <= 8 * e_old + FLOOR * eps * float(np.abs(r).max()), (name, e_new, e_old)
            rb, ob = ref[5], g_old[3].cpu().numpy()
            i0, i1 = parts[0][1], parts[1][1]
            assert err(dB[:, i0], rb[:, i0]) <= 8 * err(ob[:, i0], rb[:, i0]) + FLOOR * eps * float(np.abs(rb).max())
            assert err(shared, rb[:, i1].sum(0)) <= 8 * err(ob[:, i1].sum(0), rb[:, i1].sum(0)) + heads * FLOOR * eps * float(np.abs(rb).max())
    finally:
        for x in hs:
            x.close()


def test_gradcheck_on_the_tiny_golden_split_in_two():
    import torch
    from spmv_amd import autograd
    csr = load_golden("tiny_f64_uniform")[0]
    bounds = [2, csr.n]
    parts = split(csr, bounds)
    assert all(p.nnz > 0 for p, _ in parts)
    hs = [device_handle(p) for p, _ in parts]
    try:
        for heads, kv in ((2, 1), (2, 2)):
            k, dv = 3, 2
            Q = rand((csr.m, heads * k), 0).requires_grad_(True)
            Ks = [rand((p.n, kv * k), 1 + r).requires_grad_(True) for r, (p, _) in enumerate(parts)]
            Vs = [rand((p.n, kv * dv), 4 + r).requires_grad_(True) for r, (p, _) in enumerate(parts)]
            fn = lambda q, k0, k1, v0, v1: autograd.attention_parts(hs, q, [k0, k1], [v0, v1], heads, kv_heads=kv)   # noqa: E731
            assert torch.autograd.gradcheck(fn, (Q, *Ks, *Vs))   # default eps / atol / rtol
            Bs = [rand((heads, parts[0][0].nnz), 8, -2, 2).requires_grad_(True), rand((parts[1][0].nnz,), 9, -2, 2).requires_grad_(True)]
            fb = lambda q, k0, k1, v0, v1, b0, b1: autograd.attention_parts(hs, q, [k0, k1], [v0, v1], heads, 0.6, kv_heads=kv, biases=[b0, b1])   # noqa: E731
            assert torch.autograd.gradcheck(fb, (Q, *Ks, *Vs, *Bs))
    finally:
        for x in hs:
            x.close()


def test_a_part_without_entries_changes_nothing():
    import torch
    from spmv_amd import autograd
    csr = load_golden("tiny_f64_uniform")[0]
    none = load_golden("nnz0_f64_uniform")[0]
    rp0 = np.zeros(csr.m + 1, dtype=np.int32)
    from spmv_amd import synth
    empty = synth.CSR(csr.m, none.n, rp0, np.zeros(0, dtype=np.int32), np.zeros(0))
    heads, kv, k, dv = 2, 1, 3, 2
    with device_handle(csr) as h, device_handle(empty) as h0:
        Q, K, V = (rand(s, i).requires_grad_(True) for i, s in enumerate(((csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv))))
        K0, V0 = rand((empty.n, kv * k), 5).requires_grad_(True), rand((empty.n, kv * dv), 6).requires_grad_(True)
        G = rand((csr.m, heads * dv), 9)
        base = autograd.attention_parts([h], Q, [K], [V], heads, kv_heads=kv)
        g_base = torch.autograd.grad(base, (Q, K, V), G)
        for order in ((0, 1), (1, 0)):   # the empty part first, and last
            hh, Ks, Vs = [[h0, h][i] for i in order], [[K0, K][i] for i in order], [[V0, V][i] for i in order]
            out = autograd.attention_parts(hh, Q, Ks, Vs, heads, kv_heads=kv)
            assert torch.equal(out == 0, base == 0) and torch.equal(bits(out)[base != 0], bits(base)[base != 0])   # the merge with an empty part keeps the values
            g = torch.autograd.grad(out, (Q, K, V, K0, V0), G)
            for a, b in zip(g[:3], g_base):
                assert torch.equal(bits(a), bits(b))
            assert bool((g[3] == 0).all()) and bool((g[4] == 0).all())
        # all parts empty: zeros, and zero gradients
        out = autograd.attention_parts([h0, h0], Q, [K0, K0], [V0, V0], heads, kv_heads=kv)
        assert bool((out == 0).all())
        assert all(bool((t == 0).all()) for t in torch.autograd.grad(out, (Q, K0, V0), G))


def test_gradients_that_are_not_needed_are_not_computed_and_mismatches_raise(monkeypatch):
    import torch
    from spmv_amd import autograd
    csr, parts, bounds = parts_a(np.float64, 2)
    heads, kv, k, dv = 4, 2, 5, 3
    hs = [device_handle(p) for p, _ in parts]
    try:
        Q, K, V = (rand(s, i).requires_grad_(True) for i, s in enumerate(((csr.m, heads * k), (csr.n, kv * k), (csr.n, kv * dv))))
        G = rand((csr.m, heads * dv), 9)
        Ks, Vs = cut(K, V, bounds)
        B1 = rand((heads, parts[1][0].nnz), 3, -2, 2).requires_grad_(True)
        full = torch.autograd.grad(autograd.attention_parts(hs, Q, Ks, Vs, heads, kv_heads=kv, biases=[None, B1]), (Q, *Ks, *Vs, B1), G)
        # only V of the second part and the bias need gradients: the function's backward returns None for every other input
        out = autograd.attention_parts(hs, Q.detach(), [Ks[0].detach(), Ks[1].detach()], [Vs[0].detach(), Vs[1]], heads, kv_heads=kv, biases=[None, B1])
        calls = []
        real = api.Handle.attention_gqa_backward_lse

        def recording(self, *a, **kw):
            res = real(self, *a, **kw)
            calls.append((hs.index(self), tuple(kw["need"]), tuple(r is None for r in res)))
            return res

        monkeypatch.setattr(api.Handle, "attention_gqa_backward_lse", recording)
        got = torch.autograd.grad(out, (Vs[1], B1), G)
        monkeypatch.undo()
        assert torch.equal(bits(got[0]), bits(full[4])) and torch.equal(bits(got[1]), bits(full[5]))
        # part 0 needs nothing and is not visited; part 1 computes dV and dB and nothing else (the outputs not needed are None)
        assert calls == [(1, (False, False, True, True), (True, True, False, False))]
        # mismatched arguments
        with pytest.raises(ValueError):
            autograd.attention_parts(hs, Q, Ks[:1], Vs, heads, kv_heads=kv)
        with pytest.raises(ValueError):
            autograd.attention_parts(hs, Q, [Ks[0][:-1], Ks[1]], Vs, heads, kv_heads=kv)          # a K with another number of rows than its handle has columns
        with pytest.raises(ValueError):
            autograd.attention_parts(hs, Q[:, :-1], Ks, Vs, heads, kv_heads=kv)
        with pytest.raises(ValueError):
            autograd.attention_parts(hs, Q, Ks, [Vs[0], Vs[1][:, :kv]], heads, kv_heads=kv)     # the parts' heads differ in width
        with pytest.raises(ValueError):
            autograd.attention_parts(hs, Q, Ks, Vs, heads, kv_heads=kv, biases=[B1[:, :-1], None])   # a bias that does not have its part's nnz
        with pytest.raises(ValueError):
            autograd.attention_parts(hs, Q, Ks, Vs, heads, kv_heads=3)
        with pytest.raises(TypeError):
            autograd.attention_parts(hs, Q.float(), Ks, Vs, heads, kv_heads=kv)
        small = load_golden("tiny_f64_uniform")[0]
        with device_handle(small) as other, pytest.raises(ValueError):
            autograd.attention_parts([hs[0], other], Q, Ks, Vs, heads, kv_heads=kv)             # another number of rows
    finally:
        for x in hs:
            x.close()
