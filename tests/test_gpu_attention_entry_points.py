"""GPU: which entry points of the library each public attention path of spmv_amd.autograd reaches, how often, in what order and with which sizes
and operands -- and that the modes of one function still give the same bits.

A tap stands in for api._lib: it records (symbol, args) of every attention symbol and the bare name of the operations that the composed backward
is made of, then calls the real library.  Each record is rendered as `stem size=value .. -> the operands that are not NULL`; a run of equal
records is written once with its count.  SEQUENCES, at the end of this file, holds what commit 5747898 ("Test every end of spmv_hip_cg_columns in
mixed company and at every k") recorded on an MI355X, the last commit whose bindings spelled every entry point out by hand.  It is not
regenerated when the bindings change.

The shapes are the smallest at which a group has more than one head (4 query heads over 2), a head's slice is not the whole tensor (k = 3,
dv = 2) and a row has no entries (row 2 of 6); one handle has no entries at all, where the backward must not reach the library."""
import numpy as np
import pytest
import torch

from spmv_amd import api, autograd, build, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M, HEADS, KV, K, DV = 6, 4, 2, 3, 2
LENGTHS = [2, 3, 0, 1, 4, 2]
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

# stem -> (its size arguments, its operands in the prototype's order: a name is an address and its ld, a *_type one int), restated from
# include/spmv_hip.h
LAYOUT = {
    "attention": ("k dv scale", "Q K V O"),
    "attention_heads": ("heads k dv scale", "Q K V O"),
    "attention_backward": ("k dv scale", "Q K V G dQ dK dV"),
    "attention_heads_backward": ("heads k dv scale", "Q K V G dQ dK dV"),
    "attention_bias": ("heads k dv scale", "Q K V B O"),
    "attention_bias_backward": ("heads k dv scale", "Q K V B G dQ dK dV dB"),
    "attention_gqa": ("heads kv_heads k dv scale", "Q K V B O"),
    "attention_gqa_backward": ("heads kv_heads k dv scale", "Q K V B G dQ dK dV dB"),
    "attention_gqa_lse": ("heads kv_heads k dv scale", "Q K V B O L"),
    "attention_gqa_lse_16": ("heads kv_heads k dv scale io_type", "Q K V B O o_type L"),
    "attention_merge": ("heads dv", "O1 L1 O2 L2 O L"),
    "attention_gqa_backward_lse": ("heads kv_heads k dv scale", "Q K V B G O L dQ dK dV dB"),
    "attention_gqa_backward_16": ("heads kv_heads k dv scale io_type", "Q K V B G O L dq_type dQ dkv_type dK dV dB"),
}
COMPOSED = ("sddmm", "row_softmax", "row_softmax_backward", "spmm", "spmm_transpose", "update_values")


class Tap:
    """stands in for api._lib: records the attention calls, and the names of the operations of the composed backward, then makes the call"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, symbol):
        f = getattr(self.lib, symbol)
        stem = symbol[len("spmv_hip_"):] if symbol.startswith("spmv_hip_") else symbol
        if stem not in LAYOUT and stem not in COMPOSED:
            return f

        def g(*args):
            self.calls.append((stem, args))
            return f(*args)
        return g


def show(stem, args):
    if stem in COMPOSED:
        return stem
    sizes, ops = LAYOUT[stem]
    i = 1 if stem == "attention_merge" else 5   # behind the handle, or behind handle, m, RowPtr, ColIdx, Matrix_Val
    out, there = [], []
    for s in sizes.split():
        out.append(f"{s}={args[i]!r}")
        i += 1
    for o in ops.split():
        if o.endswith("_type"):
            out.append(f"{o}={args[i]!r}")
            i += 1
        else:   # an address and its ld
            if args[i]:
                there.append(o)
            i += 2
    assert i == len(args), (stem, i, len(args))
    return f"{stem} {' '.join(out)} -> {' '.join(there)}"


def sequence(calls):
    """the rendered calls, a run of equal ones as `n * record`"""
    out = []
    for line in (show(*c) for c in calls):
        if out and out[-1][1] == line:
            out[-1][0] += 1
        else:
            out.append([1, line])
    return [line if n == 1 else f"{n} * {line}" for n, line in out]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def pattern(lengths, n, seed):
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(lengths) + 1, dtype=np.int32)
    np.cumsum(lengths, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(n, ln, replace=False)) for ln in lengths] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return synth.CSR(len(lengths), n, rp, ci, rng.uniform(-1, 1, int(rp[-1])).astype(np.float32))


def device_handle(csr):
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (csr.rowptr, csr.colidx, csr.val))
    return api.Handle(csr.m, csr.n, rp, ci, va, api.SPMV_METHODS.Method_Parallel)


@pytest.fixture(scope="module")
def handles(_lib):
    """name -> handle: `a` 6 x 6 with row 2 empty, `zero` 6 x 6 without entries, `p0` and `p1` the two parts (6 x 3 each) of attention_parts"""
    hs = {"a": device_handle(pattern(LENGTHS, M, 1)), "zero": device_handle(pattern([0] * M, M, 2)),
          "p0": device_handle(pattern([1, 2, 0, 0, 3, 1], 3, 3)), "p1": device_handle(pattern([2, 0, 0, 1, 1, 3], 3, 4))}
    yield hs
    for h in hs.values():
        h.close()


def rand(shape, seed, dtype=torch.float32):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)).to(DEV).to(dtype)


def cases():
    """-> id -> (function, handle name, dtype name, mode, bias?, kv_heads, the leaves that want a gradient)"""
    out = {}
    for dt in DTYPES:
        for bias in (False, True):
            b = "bias" if bias else "plain"
            for mode in ("composed", "fused"):
                out[f"attention/{dt}/{b}/{mode}"] = ("attention", "a", dt, mode, bias, None, "QKVB")
            for kv in (None, KV):
                for mode in ("per_head", "fused"):
                    out[f"attention_heads/{dt}/kv={kv}/{b}/{mode}"] = ("attention_heads", "a", dt, mode, bias, kv, "QKVB")
        for mode in ("per_head", "fused"):   # only some gradients wanted: the others' outputs are NULL
            out[f"attention_heads/{dt}/kv={KV}/plain,K only/{mode}"] = ("attention_heads", "a", dt, mode, False, KV, "K")
            out[f"attention_heads/{dt}/kv=None/bias,Q and bias only/{mode}"] = ("attention_heads", "a", dt, mode, True, None, "QB")
        out[f"attention_parts/{dt}"] = ("attention_parts", "p0 p1", dt, None, True, KV, "QKVB")
    for dt in ("f32", "f16"):   # no stored entry: the backward is zeros made in torch
        for mode in ("composed", "fused"):
            out[f"attention/{dt}/zero/{mode}"] = ("attention", "zero", dt, mode, False, None, "QKVB")
        for mode in ("per_head", "fused"):
            out[f"attention_heads/{dt}/zero/{mode}"] = ("attention_heads", "zero", dt, mode, False, KV, "QKVB")
    return out


def run(tap, handles, case):
    """-> (the sequence recorded, [O, the gradients asked for]) of one case: the forward, then torch.autograd.grad with a fixed dL/dO"""
    fn, hname, dt, mode, bias, kv, wants = case
    dtype, hs = DTYPES[dt], [handles[n] for n in hname.split()]
    heads = 1 if fn == "attention" else HEADS
    g = heads if kv is None else kv
    leaf = lambda t, name: t.requires_grad_(name in wants)
    Q = leaf(rand((M, heads * K), 10, dtype), "Q")
    Ks = [leaf(rand((h.n, g * K), 20 + i, dtype), "K") for i, h in enumerate(hs)]
    Vs = [leaf(rand((h.n, g * DV), 30 + i, dtype), "V") for i, h in enumerate(hs)]
    # a plane per head, on the first handle only; attention() has the one head
    Bs = [leaf(rand((heads, h.nnz) if heads > 1 else (h.nnz,), 40), "B") if bias and i == 0 else None for i, h in enumerate(hs)]
    G = rand((M, heads * DV), 50, dtype)
    del tap.calls[:]
    if fn == "attention":
        O = autograd.attention(hs[0], Q, Ks[0], Vs[0], None, mode, bias=Bs[0])
    elif fn == "attention_heads":
        O = autograd.attention_heads(hs[0], Q, Ks[0], Vs[0], heads, 0.4, mode, bias=Bs[0], kv_heads=kv)
    else:
        O = autograd.attention_parts(hs, Q, Ks, Vs, heads, kv_heads=kv, biases=Bs)
    wanted = [t for t in (Q, *Ks, *Vs, *Bs) if t is not None and t.requires_grad]
    grads = torch.autograd.grad(O, wanted, G)
    torch.cuda.synchronize()
    return sequence(tap.calls), [O.detach(), *grads]


def same_bits(a, b):
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@pytest.fixture(scope="module")
def recorded(_lib, handles):
    """id -> (sequence, results) of every case, run once through the tap"""
    tap = Tap(_lib)
    api._lib = tap
    try:
        return {cid: run(tap, handles, case) for cid, case in cases().items()}
    finally:
        api._lib = _lib


@pytest.mark.parametrize("cid", list(cases()))
def test_a_path_reaches_the_entry_points_it_reached(recorded, cid):
    assert sorted(SEQUENCES) == sorted(cases())
    got = recorded[cid][0]
    print(cid, got)
    assert got == SEQUENCES[cid]


def test_the_per_head_modes_reach_the_single_head_entry_points():
    """what the bindings' contract names outright, read off the literals: no bias -> spmv_hip_attention_backward per head; a bias ->
    spmv_hip_attention_bias_backward with heads = 1; 16-bit -> spmv_hip_attention_gqa_backward_16 with 1, 1; no entries -> the forward alone"""
    assert SEQUENCES["attention_heads/f32/kv=None/plain/per_head"][1] == "4 * attention_backward k=3 dv=2 scale=0.4 -> Q K V G dQ dK dV"
    assert SEQUENCES["attention_heads/f32/kv=None/bias/per_head"][1] == "4 * attention_bias_backward heads=1 k=3 dv=2 scale=0.4 -> Q K V B G dQ dK dV dB"
    assert SEQUENCES["attention_heads/f16/kv=None/plain/per_head"][1] == \
        "4 * attention_gqa_backward_16 heads=1 kv_heads=1 k=3 dv=2 scale=0.4 io_type=1 dq_type=1 dkv_type=1 -> Q K V G dQ dK dV"
    for cid, seq in SEQUENCES.items():
        if "/zero/" in cid and cid != "attention/f32/zero/fused":
            assert len(seq) == 1, cid


def test_the_modes_of_a_function_give_the_same_bits(recorded):
    groups = {}
    for cid, (_, results) in recorded.items():
        groups.setdefault(cid.rsplit("/", 1)[0], []).append((cid, results))
    compared = 0
    for key, members in groups.items():
        if key.startswith("attention_parts"):
            continue
        assert len(members) == 2, key
        (ida, a), (idb, b) = members
        assert len(a) == len(b) and len(a) >= 2
        for i, (x, y) in enumerate(zip(a, b)):
            assert same_bits(x, y), (ida, idb, i)
            if not key.endswith("/zero"):   # no stored entry: O and every gradient are zeros
                assert bool(x.float().ne(0).any()), (ida, i)
        compared += 1
    assert compared == (len(cases()) - 3) // 2


# ------------------------------------------------------------------------------------------------- recorded on commit 5747898, on an MI355X
_S, _A, _B = "scale=0.5773502691896258", "Q K V G dQ dK dV", "Q K V B G dQ dK dV dB"
_COMPOSED = ["sddmm", "row_softmax", "update_values", "spmm_transpose", "sddmm", "row_softmax_backward", "update_values", "spmm", "spmm_transpose", "update_values"]
_ONE, _MHA, _GQA = "k=3 dv=2 scale=0.4", "heads=4 k=3 dv=2 scale=0.4", "heads=4 kv_heads=2 k=3 dv=2 scale=0.4"
_PART = f"heads=4 kv_heads=2 k=3 dv=2 {_S}"
SEQUENCES = {
    "attention/f32/plain/composed": [f"attention k=3 dv=2 {_S} -> Q K V O", *_COMPOSED],
    "attention/f32/plain/fused": [f"attention k=3 dv=2 {_S} -> Q K V O", f"attention_backward k=3 dv=2 {_S} -> {_A}"],
    "attention/f32/bias/composed": [f"attention_bias heads=1 k=3 dv=2 {_S} -> Q K V B O", *_COMPOSED],
    "attention/f32/bias/fused": [f"attention_bias heads=1 k=3 dv=2 {_S} -> Q K V B O", f"attention_bias_backward heads=1 k=3 dv=2 {_S} -> {_B}"],
    "attention_heads/f32/kv=None/plain/per_head": [f"attention_heads {_MHA} -> Q K V O", f"4 * attention_backward {_ONE} -> {_A}"],
    "attention_heads/f32/kv=None/plain/fused": [f"attention_heads {_MHA} -> Q K V O", f"attention_heads_backward {_MHA} -> {_A}"],
    "attention_heads/f32/kv=2/plain/per_head": [f"attention_gqa {_GQA} -> Q K V O", f"4 * attention_bias_backward heads=1 {_ONE} -> {_A}"],
    "attention_heads/f32/kv=2/plain/fused": [f"attention_gqa {_GQA} -> Q K V O", f"attention_gqa_backward {_GQA} -> {_A}"],
    "attention_heads/f32/kv=None/bias/per_head": [f"attention_bias {_MHA} -> Q K V B O", f"4 * attention_bias_backward heads=1 {_ONE} -> {_B}"],
    "attention_heads/f32/kv=None/bias/fused": [f"attention_bias {_MHA} -> Q K V B O", f"attention_bias_backward {_MHA} -> {_B}"],
    "attention_heads/f32/kv=2/bias/per_head": [f"attention_gqa {_GQA} -> Q K V B O", f"4 * attention_bias_backward heads=1 {_ONE} -> {_B}"],
    "attention_heads/f32/kv=2/bias/fused": [f"attention_gqa {_GQA} -> Q K V B O", f"attention_gqa_backward {_GQA} -> {_B}"],
    "attention_heads/f32/kv=2/plain,K only/per_head": [f"attention_gqa {_GQA} -> Q K V O", f"4 * attention_bias_backward heads=1 {_ONE} -> Q K V G dK"],
    "attention_heads/f32/kv=2/plain,K only/fused": [f"attention_gqa {_GQA} -> Q K V O", f"attention_gqa_backward {_GQA} -> Q K V G dK"],
    "attention_heads/f32/kv=None/bias,Q and bias only/per_head": [f"attention_bias {_MHA} -> Q K V B O", f"4 * attention_bias_backward heads=1 {_ONE} -> Q K V B G dQ dB"],
    "attention_heads/f32/kv=None/bias,Q and bias only/fused": [f"attention_bias {_MHA} -> Q K V B O", f"attention_bias_backward {_MHA} -> Q K V B G dQ dB"],
    "attention_parts/f32": [f"attention_gqa_lse {_PART} -> Q K V B O L", f"attention_gqa_lse {_PART} -> Q K V O L", "attention_merge heads=4 dv=2 -> O1 L1 O2 L2 O L",
                            f"attention_gqa_backward_lse {_PART} -> Q K V B G O L dQ dK dV dB", f"attention_gqa_backward_lse {_PART} -> Q K V G O L dQ dK dV"],
    # no stored entry: the forward alone -- but for attention(backward="fused") in float32, which asks the library for its zeros
    "attention/f32/zero/composed": [f"attention k=3 dv=2 {_S} -> Q K V O"],
    "attention/f32/zero/fused": [f"attention k=3 dv=2 {_S} -> Q K V O", f"attention_backward k=3 dv=2 {_S} -> {_A}"],
    "attention_heads/f32/zero/per_head": [f"attention_gqa {_GQA} -> Q K V O"],
    "attention_heads/f32/zero/fused": [f"attention_gqa {_GQA} -> Q K V O"],
    "attention/f16/zero/composed": [f"attention_gqa_lse_16 heads=1 kv_heads=1 k=3 dv=2 {_S} io_type=1 o_type=1 -> Q K V O"],
    "attention/f16/zero/fused": [f"attention_gqa_lse_16 heads=1 kv_heads=1 k=3 dv=2 {_S} io_type=1 o_type=1 -> Q K V O"],
    "attention_heads/f16/zero/per_head": [f"attention_gqa_lse_16 {_GQA} io_type=1 o_type=1 -> Q K V O"],
    "attention_heads/f16/zero/fused": [f"attention_gqa_lse_16 {_GQA} io_type=1 o_type=1 -> Q K V O"],
}


def _sixteen(dt, t):
    """what a 16-bit type recorded: float16 (type code 1) and bfloat16 (2) differ in nothing but the code.  The per-head mode over groups of heads
    asks for float32 dK and dV terms (dkv_type=0), which it sums itself"""
    f1, f4, fg = f"attention_gqa_lse_16 heads=1 kv_heads=1 k=3 dv=2 {_S} io_type={t} o_type={t}", f"attention_gqa_lse_16 heads=4 kv_heads=4 {_ONE} io_type={t} o_type={t}", \
        f"attention_gqa_lse_16 {_GQA} io_type={t} o_type={t}"
    b1 = f"attention_gqa_backward_16 heads=1 kv_heads=1 k=3 dv=2 {_S} io_type={t} dq_type={t} dkv_type={t}"
    head, head32 = f"4 * attention_gqa_backward_16 heads=1 kv_heads=1 {_ONE} io_type={t} dq_type={t} dkv_type={t}", \
        f"4 * attention_gqa_backward_16 heads=1 kv_heads=1 {_ONE} io_type={t} dq_type={t} dkv_type=0"
    b4, bg = f"attention_gqa_backward_16 heads=4 kv_heads=4 {_ONE} io_type={t} dq_type={t} dkv_type={t}", f"attention_gqa_backward_16 {_GQA} io_type={t} dq_type={t} dkv_type={t}"
    fp, bp = f"attention_gqa_lse_16 {_PART} io_type={t} o_type=0", f"attention_gqa_backward_16 {_PART} io_type={t} dq_type=0 dkv_type={t}"
    return {
        f"attention/{dt}/plain/composed": [f"{f1} -> Q K V O", *_COMPOSED],
        f"attention/{dt}/plain/fused": [f"{f1} -> Q K V O", f"{b1} -> {_A}"],
        f"attention/{dt}/bias/composed": [f"{f1} -> Q K V B O", *_COMPOSED],
        f"attention/{dt}/bias/fused": [f"{f1} -> Q K V B O", f"{b1} -> {_B}"],
        f"attention_heads/{dt}/kv=None/plain/per_head": [f"{f4} -> Q K V O", f"{head} -> {_A}"],
        f"attention_heads/{dt}/kv=None/plain/fused": [f"{f4} -> Q K V O", f"{b4} -> {_A}"],
        f"attention_heads/{dt}/kv=2/plain/per_head": [f"{fg} -> Q K V O", f"{head32} -> {_A}"],
        f"attention_heads/{dt}/kv=2/plain/fused": [f"{fg} -> Q K V O", f"{bg} -> {_A}"],
        f"attention_heads/{dt}/kv=None/bias/per_head": [f"{f4} -> Q K V B O", f"{head} -> {_B}"],
        f"attention_heads/{dt}/kv=None/bias/fused": [f"{f4} -> Q K V B O", f"{b4} -> {_B}"],
        f"attention_heads/{dt}/kv=2/bias/per_head": [f"{fg} -> Q K V B O", f"{head32} -> {_B}"],
        f"attention_heads/{dt}/kv=2/bias/fused": [f"{fg} -> Q K V B O", f"{bg} -> {_B}"],
        f"attention_heads/{dt}/kv=2/plain,K only/per_head": [f"{fg} -> Q K V O", f"{head32} -> Q K V G dK"],
        f"attention_heads/{dt}/kv=2/plain,K only/fused": [f"{fg} -> Q K V O", f"{bg} -> Q K V G dK"],
        f"attention_heads/{dt}/kv=None/bias,Q and bias only/per_head": [f"{f4} -> Q K V B O", f"{head} -> Q K V B G dQ dB"],
        f"attention_heads/{dt}/kv=None/bias,Q and bias only/fused": [f"{f4} -> Q K V B O", f"{b4} -> Q K V B G dQ dB"],
        f"attention_parts/{dt}": [f"{fp} -> Q K V B O L", f"{fp} -> Q K V O L", "attention_merge heads=4 dv=2 -> O1 L1 O2 L2 O L",
                                  f"{bp} -> Q K V B G O L dQ dK dV dB", f"{bp} -> Q K V G O L dQ dK dV"],
    }


SEQUENCES.update(_sixteen("f16", 1))
SEQUENCES.update(_sixteen("bf16", 2))
