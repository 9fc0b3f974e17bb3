"""CPU: what the attention bindings of spmv_amd.api hand the C library, argument for argument.

A recorder stands in for api._lib: every symbol asked of it is a function that appends (symbol, args) and answers success.  A catalogue of calls
-- the 12 attention calls, their 12 timers and the 12 Handle methods, with every optional operand given and None, the bias shared and per head,
the ldb / lddb / ldl overrides, scale None and given, fp32 numpy operands and float16 / bfloat16 torch tensors, column views of wider arrays --
is run through it, addresses are mapped back to operand names, and each record is compared with a literal.

The literals at the end of this file (CALLS, HANDLE_CALLS, PROTOTYPES, SIGNATURES) were written by running this same catalogue on the api.py and
autograd.py of commit 5747898 ("Test every end of spmv_hip_cg_columns in mixed company and at every k"), the last one that spelled every entry
point out by hand.  They are not regenerated when the bindings change: a binding that passes anything else than that commit passed fails here.
"""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from spmv_amd import api, autograd

M, N, K, DV, NNZ, H, HKV = 5, 7, 3, 2, 11, 4, 2
RP, CI, VA = np.zeros(M + 1, dtype=np.int32), np.zeros(NNZ, dtype=np.int32), np.zeros(NNZ, dtype=np.float32)
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32

# python name -> (heads, kv_heads, the size arguments it takes, its operands, those of them that may be None)
RUNGS = {
    "attention": (1, 1, (), "Q K V O", ""),
    "attention_heads": (H, H, ("heads",), "Q K V O", ""),
    "attention_backward": (1, 1, (), "Q K V G dQ dK dV", "dQ dK dV"),
    "attention_heads_backward": (H, H, ("heads",), "Q K V G dQ dK dV", "dQ dK dV"),
    "attention_bias": (H, H, ("heads",), "Q K V B O", "B"),
    "attention_bias_backward": (H, H, ("heads",), "Q K V B G dQ dK dV dB", "B dQ dK dV dB"),
    "attention_gqa": (H, HKV, ("heads", "kv_heads"), "Q K V B O", "B"),
    "attention_gqa_backward": (H, HKV, ("heads", "kv_heads"), "Q K V B G dQ dK dV dB", "B dQ dK dV dB"),
    "attention_gqa_lse": (H, HKV, ("heads", "kv_heads"), "Q K V B O L", "B L"),
    "attention_gqa_lse_16": (H, HKV, ("heads", "kv_heads"), "Q K V B O L", "B L"),
    "attention_gqa_backward_lse": (H, HKV, ("heads", "kv_heads"), "Q K V B G O L dQ dK dV dB", "B dQ dK dV dB"),
    "attention_gqa_backward_16": (H, HKV, ("heads", "kv_heads"), "Q K V B G O L dQ dK dV dB", "B dQ dK dV dB"),
}
OVERRIDES = {"B": ("ldb", 17), "dB": ("lddb", 19), "L": ("ldl", 23)}   # calls only: the timers have none


class Recorder:
    """stands in for api._lib: every attribute is a function that records (symbol, args) and answers success -- 0, or 1.0 ms for a timer"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        def f(*args):
            self.calls.append((symbol, args))
            return 1.0 if symbol.startswith("spmv_hip_time_") else 0
        return f


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(api, "_lib", r)
    return r


def handle(size=4):
    """a public handle struct of that data_size: the 16-bit backward reads the field; nothing else looks at a handle"""
    return C.pointer(api.spmv_Handle(data_size=size))


def block(rows, width, dtype=np.float32, pad=0):
    """a (rows, width) operand, a column view of an array `pad` columns wider: numpy for a numpy dtype, a CPU tensor for a torch one"""
    wide = torch.zeros((rows, width + pad), dtype=dtype) if isinstance(dtype, torch.dtype) else np.zeros((rows, width + pad), dtype=dtype)
    return wide[:, :width]


def operands(heads, kv, io=np.float32, o=None, dq=None, dkv=None):
    """name -> operand of a rung of `heads` query heads over `kv` K / V heads.  Q, V, O, dK, the per-head bias and L are views of wider arrays, so
    their ld is not their width; io: the dtype of Q, K, V and G, o / dq / dkv: those of O, dQ and dK / dV where they differ; the bias, its
    gradient and L are fp32 throughout -- as is O beside a 16-bit G, which is the backward's"""
    f32 = F32 if isinstance(io, torch.dtype) else np.float32
    a = {"Q": block(M, heads * K, io, 1), "K": block(N, kv * K, io), "V": block(N, kv * DV, io, 2), "G": block(M, heads * DV, io),
         "O": block(M, heads * DV, o or io, 3), "L": block(heads, M, f32, 1), "B": block(heads, NNZ, f32, 2), "B1": block(1, NNZ, f32)[0],
         "Bflat": block(heads, NNZ, f32), "Lflat": block(heads, M, f32),   # contiguous, as an ld override wants them
         "dQ": block(M, heads * K, dq or io), "dK": block(N, kv * K, dkv or io, 1), "dV": block(N, kv * DV, dkv or io), "dB": block(heads, NNZ, f32)}
    return a


def address(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def render(args, names):
    """the arguments of one recorded call as a line: an address as its operand's name, a handle struct as `h<data_size>`, the timers' ms array
    as `ms`"""
    def one(x):
        if isinstance(x, api.spmv_Handle_t):
            return f"h{x.contents.data_size}"
        if isinstance(x, C.Array):
            return "ms"
        if x is None:
            return "NULL"
        if isinstance(x, float):
            return repr(x)
        assert type(x) is int, type(x)
        return names.get(x, str(x))
    return " ".join(one(x) for x in args)


def named(a):
    names = {address(v): n for n, v in a.items()}
    names.update({address(RP): "rp", address(CI): "ci", address(VA): "va"})
    return names


def variants(name):
    """-> (id, operand dtypes, changes to the keyword arguments) of every case of a rung"""
    _, _, _, ops, optional = RUNGS[name]
    ops, half = ops.split(), name.endswith("_16")
    types = dict(io=F16) if half else {}
    out = [("base", types, {}), ("scale", types, {"scale": 0.25})]
    out += [(f"{o}=None", types, {o: None}) for o in optional.split()]
    if "B" in ops:
        out.append(("B=shared", types, {"B": "B1"}))
    out += [(key, types, {key: ld, **({"dB": "dB"} if o == "dB" else {o: o + "flat"})}) for o, (key, ld) in OVERRIDES.items() if o in ops]
    if "B" in ops and "dB" in ops:
        out.append(("B=None,ldb,lddb", types, {"B": None, "ldb": 17, "lddb": 19}))
    if half:
        out.append(("bf16", dict(io=BF16), {}))
        if name == "attention_gqa_lse_16":
            out += [("O=fp32", dict(io=F16, o=F32), {}), ("bf16,O=fp32,L=None", dict(io=BF16, o=F32), {"L": None})]
        else:
            out += [("dQ=fp32", dict(io=F16, dq=F32), {}), ("dK,dV=fp32", dict(io=BF16, dkv=F32), {}), ("all fp32", dict(io=BF16, dq=F32, dkv=F32), {}),
                    ("O=L=None", types, {"O": None, "L": None}), ("O=L=None,dK=None,dV fp32", dict(io=F16, dkv=F32), {"O": None, "L": None, "dK": None}),
                    ("dQ=None,dV=None,dK fp32", dict(io=BF16, dkv=F32), {"dQ": None, "dV": None})]
    return out


def record_rung(rec, name):
    """-> {case id: the sizes and operands that the call `name` passed, rendered} over variants(name).  What stands around them is checked here: the
    symbol, the handle, m and the CSR arrays in front of a call, warmup, iters and the ms array behind a timer's -- and that the timer of a case
    passes the very sizes and operands that its call passed"""
    heads, kv, sizes, ops, _ = RUNGS[name]
    h, hname = (handle(4), "h4") if name == "attention_gqa_backward_16" else (1234, "1234")
    lead = {s: {"heads": heads, "kv_heads": kv}[s] for s in sizes}
    out = {}
    for vid, types, changes in variants(name):
        a = operands(heads, kv, **types)
        if name.endswith("_16") and "G" in ops.split():
            a["O"] = block(M, heads * DV, F32, 3)
        kw = {o: a[o] for o in ops.split()}
        kw.update({o: (a[v] if isinstance(v, str) else v) for o, v in changes.items()})
        del rec.calls[:]
        assert getattr(api, name)(h, M, RP, CI, VA, **lead, **kw) == 0
        (symbol, args), = rec.calls
        line, front = render(args, named(a)), f"{hname} {M} rp ci va "
        assert symbol == f"spmv_hip_{name}" and line.startswith(front), (symbol, line)
        out[vid] = line[len(front):]
        if any(o in kw for o in ("ldb", "lddb", "ldl")):
            continue
        del rec.calls[:]
        mean, ms = getattr(api, f"time_{name}_launches")(h, **lead, **kw, warmup=2, iters=3)
        assert mean == 1.0 and ms.shape == (3,) and ms.dtype == np.float32
        (symbol, args), = rec.calls
        assert symbol == f"spmv_hip_time_{name}_launches" and render(args, named(a)) == f"{hname} {out[vid]} 2 3 ms", (vid, symbol, render(args, named(a)))
    return out


def fake_handle(size=4):
    """an api.Handle made without the C create"""
    hd = object.__new__(api.Handle)
    hd.m, hd.n, hd.h, hd._keep, hd._nnz = M, N, handle(size), (RP, CI, VA), NNZ
    return hd


def handle_cases():
    """-> (id, method, the operands' dtypes, heads, kv_heads, the arguments as operand names or values)"""
    need3, need4 = (True, False, True), (False, True, False, True)
    return [
        ("attention", "attention", {}, 1, 1, dict(Q="Q", K="K", V="V")),
        ("attention [out, scale]", "attention", {}, 1, 1, dict(Q="Q", K="K", V="V", scale=0.25, out="O")),
        ("attention_heads", "attention_heads", {}, H, H, dict(Q="Q", K="K", V="V", heads=H)),
        ("attention_heads [out]", "attention_heads", {}, H, H, dict(Q="Q", K="K", V="V", heads=H, out="O")),
        ("attention_backward", "attention_backward", {}, 1, 1, dict(Q="Q", K="K", V="V", G="G")),
        ("attention_backward [need]", "attention_backward", {}, 1, 1, dict(Q="Q", K="K", V="V", G="G", scale=0.25, need=need3)),
        ("attention_heads_backward", "attention_heads_backward", {}, H, H, dict(Q="Q", K="K", V="V", G="G", heads=H)),
        ("attention_heads_backward [need]", "attention_heads_backward", {}, H, H, dict(Q="Q", K="K", V="V", G="G", heads=H, need=need3)),
        ("attention_bias", "attention_bias", {}, H, H, dict(Q="Q", K="K", V="V", heads=H, bias="B")),
        ("attention_bias [shared, out]", "attention_bias", {}, H, H, dict(Q="Q", K="K", V="V", heads=H, bias="B1", out="O")),
        ("attention_bias_backward", "attention_bias_backward", {}, H, H, dict(Q="Q", K="K", V="V", bias="B", G="G", heads=H)),
        ("attention_bias_backward [need]", "attention_bias_backward", {}, H, H, dict(Q="Q", K="K", V="V", bias=None, G="G", heads=H, need=need4)),
        ("attention_gqa", "attention_gqa", {}, H, HKV, dict(Q="Q", K="K", V="V", heads=H, kv_heads=HKV)),
        ("attention_gqa [bias, out]", "attention_gqa", {}, H, HKV, dict(Q="Q", K="K", V="V", heads=H, kv_heads=HKV, bias="B", scale=0.25, out="O")),
        ("attention_gqa_backward", "attention_gqa_backward", {}, H, HKV, dict(Q="Q", K="K", V="V", bias="B1", G="G", heads=H, kv_heads=HKV)),
        ("attention_gqa_backward [need]", "attention_gqa_backward", {}, H, HKV, dict(Q="Q", K="K", V="V", bias="B", G="G", heads=H, kv_heads=HKV, need=need4)),
        ("attention_gqa_lse", "attention_gqa_lse", {}, H, HKV, dict(Q="Q", K="K", V="V", heads=H, kv_heads=HKV)),
        ("attention_gqa_lse [bias, out, lse]", "attention_gqa_lse", {}, H, HKV, dict(Q="Q", K="K", V="V", heads=H, kv_heads=HKV, bias="B", out="O", lse="L")),
        ("attention_gqa_lse_16", "attention_gqa_lse_16", dict(io=F16), H, HKV, dict(Q="Q", K="K", V="V", heads=H, kv_heads=HKV)),
        ("attention_gqa_lse_16 [fp32 out, no lse]", "attention_gqa_lse_16", dict(io=BF16), H, HKV,
         dict(Q="Q", K="K", V="V", heads=H, kv_heads=HKV, B="B", out_dtype=F32, want_l=False)),
        ("attention_merge", "attention_merge", {}, H, H, dict(O1="O", L1="L", O2="G", L2="B", heads=H)),
        ("attention_merge [in place, no lse]", "attention_merge", {}, H, H, dict(O1="O", L1="L", O2="G", L2="B", heads=H, out="O", want_lse=False)),
        ("attention_gqa_backward_lse", "attention_gqa_backward_lse", {}, H, HKV, dict(Q="Q", K="K", V="V", bias="B", G="G", O="O", L="L", heads=H, kv_heads=HKV)),
        ("attention_gqa_backward_lse [need]", "attention_gqa_backward_lse", {}, H, HKV,
         dict(Q="Q", K="K", V="V", bias=None, G="G", O="O", L="L", heads=H, kv_heads=HKV, scale=0.25, need=need4)),
        ("attention_gqa_backward_16", "attention_gqa_backward_16", dict(io=F16), H, HKV, dict(Q="Q", K="K", V="V", B="B", G="G", heads=H, kv_heads=HKV)),
        ("attention_gqa_backward_16 [O, L, fp32 dQ]", "attention_gqa_backward_16", dict(io=BF16, o=F32), H, HKV,
         dict(Q="Q", K="K", V="V", B=None, G="G", heads=H, kv_heads=HKV, O="O", L="L", dq_dtype=F32)),
        ("attention_gqa_backward_16 [need, fp32 dK dV]", "attention_gqa_backward_16", dict(io=F16), H, HKV,
         dict(Q="Q", K="K", V="V", B="B1", G="G", heads=H, kv_heads=HKV, need=need4, dkv_dtype=F32)),
    ]


def record_handle_methods(rec):
    """-> {case id: the rendered record, then kind, dtype and shape of everything the method returned} over handle_cases()"""
    out = {}
    for cid, method, types, heads, kv, args in handle_cases():
        a = operands(heads, kv, **types)
        if method == "attention_merge":   # L2 is a plane per head of m entries
            a["B"] = block(heads, M, np.float32)
        hd = fake_handle()
        try:
            del rec.calls[:]
            got = getattr(hd, method)(**{n: (a[v] if isinstance(v, str) else v) for n, v in args.items()})
            names = named(a)
            shown = []
            for i, r in enumerate(got if isinstance(got, tuple) else (got,)):
                if r is not None:
                    names.setdefault(address(r), f"r{i}")
                shown.append("None" if r is None else f"{names[address(r)]}={type(r).__name__} {r.dtype} {tuple(r.shape)}")
            (symbol, cargs), = rec.calls
            out[cid] = f"{symbol}: {render(cargs, names)} -> " + ", ".join(shown)
        finally:
            hd.h = None   # nothing for close() to destroy
    return out


def bad_inputs():
    """-> (id, exception type, a call that the bindings refuse before they ask the library)"""
    a, t = operands(H, HKV), operands(H, HKV, io=F16)
    s, b = operands(H, H), operands(H, HKV, io=BF16)
    o = operands(1, 1)
    t["O32"] = block(M, H * DV, F32)
    h32, h64 = handle(4), handle(8)
    gqa = lambda f, x, **kw: f(1234, M, RP, CI, VA, H, HKV, **{**{n: x[n] for n in ("Q", "K", "V", "B")}, **kw})
    b16 = lambda h, x, **kw: api.attention_gqa_backward_16(h, M, RP, CI, VA, H, HKV, **{**{n: x[n] for n in ("Q", "K", "V", "B", "G")}, **kw})
    return [
        ("attention: K wider than Q", ValueError, lambda: api.attention(1234, M, RP, CI, VA, o["Q"], s["K"], o["V"], o["O"])),
        ("attention: O wider than V", ValueError, lambda: api.attention(1234, M, RP, CI, VA, o["Q"], o["K"], o["V"], s["O"])),
        ("time_attention: K wider than Q", ValueError, lambda: api.time_attention_launches(1234, o["Q"], s["K"], o["V"], o["O"])),
        ("attention_backward: dK of V's width", ValueError, lambda: api.attention_backward(1234, M, RP, CI, VA, o["Q"], o["K"], o["V"], o["G"], dK=o["dV"])),
        ("attention_heads: 5 heads", ValueError, lambda: api.attention_heads(1234, M, RP, CI, VA, 5, s["Q"], s["K"], s["V"], s["O"])),
        ("attention_heads: 0 heads", ValueError, lambda: api.attention_heads(1234, M, RP, CI, VA, 0, s["Q"], s["K"], s["V"], s["O"])),
        ("time_attention_heads_backward: 3 heads", ValueError, lambda: api.time_attention_heads_backward_launches(1234, 3, s["Q"], s["K"], s["V"], s["G"], s["dQ"])),
        ("attention_bias: a bias of 3 planes", ValueError, lambda: api.attention_bias(1234, M, RP, CI, VA, H, s["Q"], s["K"], s["V"], s["B"][:3], s["O"])),
        ("attention_bias_backward: a shared dB", ValueError,
         lambda: api.attention_bias_backward(1234, M, RP, CI, VA, H, s["Q"], s["K"], s["V"], s["B"], s["G"], dB=s["B1"])),
        ("attention_gqa: 4 heads over 3", ValueError, lambda: api.attention_gqa(1234, M, RP, CI, VA, H, 3, a["Q"], a["K"], a["V"], None, a["O"])),
        ("attention_gqa: K of Q's width", ValueError, lambda: gqa(api.attention_gqa, dict(a, K=a["dQ"]), O=a["O"])),
        ("time_attention_gqa: 4 heads over 3", ValueError, lambda: api.time_attention_gqa_launches(1234, H, 3, a["Q"], a["K"], a["V"], None, a["O"])),
        ("attention_gqa_backward: dK of Q's width", ValueError, lambda: gqa(api.attention_gqa_backward, a, G=a["G"], dK=a["dQ"])),
        ("attention_gqa_backward: dB of kv_heads planes", ValueError, lambda: gqa(api.attention_gqa_backward, a, G=a["G"], dB=a["dB"][:HKV])),
        ("attention_gqa_lse: L of kv_heads planes", ValueError, lambda: gqa(api.attention_gqa_lse, a, O=a["O"], L=a["L"][:HKV])),
        ("attention_gqa_backward_lse: O of K's width", ValueError, lambda: gqa(api.attention_gqa_backward_lse, a, G=a["G"], O=a["dQ"], L=a["L"], dQ=a["dQ"])),
        ("attention_gqa_lse_16: K of the other 16-bit type", TypeError, lambda: gqa(api.attention_gqa_lse_16, dict(t, K=b["K"]), O=t["O"])),
        ("attention_gqa_lse_16: fp32 Q, K, V", TypeError, lambda: gqa(api.attention_gqa_lse_16, operands(H, HKV, io=F32), O=t["O32"])),
        ("attention_gqa_lse_16: numpy Q", TypeError, lambda: gqa(api.attention_gqa_lse_16, dict(t, Q=a["Q"]), O=t["O"])),
        ("attention_gqa_lse_16: O of the other 16-bit type", TypeError, lambda: gqa(api.attention_gqa_lse_16, t, O=b["O"])),
        ("time_attention_gqa_lse_16: V of the other 16-bit type", TypeError,
         lambda: api.time_attention_gqa_lse_16_launches(1234, H, HKV, t["Q"], t["K"], b["V"], None, t["O"])),
        ("attention_gqa_backward_16: G of the other 16-bit type", TypeError, lambda: b16(h32, dict(t, G=b["G"]), dQ=t["dQ"])),
        ("attention_gqa_backward_16: dK and dV of two dtypes", TypeError, lambda: b16(h32, t, dK=t["dK"], dV=block(N, HKV * DV, F32))),
        ("attention_gqa_backward_16: dQ of the other 16-bit type", TypeError, lambda: b16(h32, t, dQ=b["dQ"])),
        ("attention_gqa_backward_16: a 16-bit bias", TypeError, lambda: b16(h32, dict(t, B=t["G"][:H]), dQ=t["dQ"])),
        ("attention_gqa_backward_16: O without L", ValueError, lambda: b16(h32, t, O=t["O32"], dQ=t["dQ"])),
        ("attention_gqa_backward_16: L without O", ValueError, lambda: b16(h32, t, L=t["L"], dQ=t["dQ"])),
        ("attention_gqa_backward_16: a float64 handle", TypeError, lambda: b16(h64, t, dQ=t["dQ"])),
        ("time_attention_gqa_backward_16: a float64 handle", TypeError,
         lambda: api.time_attention_gqa_backward_16_launches(h64, H, HKV, t["Q"], t["K"], t["V"], None, t["G"], dQ=t["dQ"])),
        ("attention_gqa_backward_16: 4 heads over 3", ValueError,
         lambda: api.attention_gqa_backward_16(h32, M, RP, CI, VA, H, 3, t["Q"], t["K"], t["V"], None, t["G"], dQ=t["dQ"])),
        ("Handle.attention_gqa_lse_16: numpy Q", TypeError, lambda: fake_handle_call("attention_gqa_lse_16", a["Q"], a["K"], a["V"], H, HKV)),
        ("Handle.attention_gqa_backward_16: numpy G", TypeError, lambda: fake_handle_call("attention_gqa_backward_16", t["Q"], t["K"], t["V"], None, a["G"], H, HKV)),
        ("Handle.attention_gqa_backward_16: a float64 handle", TypeError,
         lambda: fake_handle_call("attention_gqa_backward_16", t["Q"], t["K"], t["V"], None, t["G"], H, HKV, size=8)),
    ]


def fake_handle_call(method, *args, size=4):
    hd = fake_handle(size)
    try:
        return getattr(hd, method)(*args)
    finally:
        hd.h = None


_CTYPES = {C.c_int: "i", C.c_double: "d", C.c_longlong: "q", C.c_void_p: "p", api.spmv_Handle_t: "H", C.POINTER(C.c_float): "F"}


def prototype(name):
    """FUNCTIONS[name] as a string: the result, a colon, then a letter per argument -- i int, d double, q long long, p void *, H the handle,
    F float *"""
    res, args = api.FUNCTIONS[name]
    return _CTYPES[res] + ":" + "".join(_CTYPES[t] for t in args)


def public_functions():
    """name -> the 24 module functions, the 12 attention methods of Handle and merge's, and the three public functions of autograd"""
    out = {}
    for name in RUNGS:
        out[f"api.{name}"], out[f"api.time_{name}_launches"] = getattr(api, name), getattr(api, f"time_{name}_launches")
        out[f"api.Handle.{name}"] = getattr(api.Handle, name)
    out["api.attention_merge"], out["api.time_attention_merge_launches"], out["api.Handle.attention_merge"] = \
        api.attention_merge, api.time_attention_merge_launches, api.Handle.attention_merge
    out.update({f"autograd.{n}": getattr(autograd, n) for n in ("attention", "attention_heads", "attention_parts")})
    return out


@pytest.mark.parametrize("name", list(RUNGS))
def test_a_call_and_its_timer_pass_what_they_passed(rec, name):
    got = record_rung(rec, name)
    assert sorted(got) == sorted(CALLS[name])
    for vid in got:
        assert got[vid] == CALLS[name][vid], vid


def test_the_issue_s_example(rec):
    """the one record that is written out in words: attention_gqa_lse with Q a 12-column view of a 13-column array"""
    Q, Kk, Vv = np.zeros((M, 13), dtype=np.float32)[:, :12], np.zeros((N, 6), dtype=np.float32), np.zeros((N, 4), dtype=np.float32)
    B, O, L = np.zeros((H, NNZ), dtype=np.float32), np.zeros((M, 8), dtype=np.float32), np.zeros((H, M), dtype=np.float32)
    assert api.attention_gqa_lse(1234, 5, RP, CI, VA, 4, 2, Q, Kk, Vv, B, O, L) == 0
    p = address
    assert rec.calls == [("spmv_hip_attention_gqa_lse", (1234, 5, p(RP), p(CI), p(VA), 4, 2, 3, 2, 0.5773502691896258, p(Q), 13, p(Kk), 6, p(Vv), 4, p(B), 11, p(O), 8, p(L), 5))]
    assert all(type(x) in (int, float) for x in rec.calls[0][1])


def test_the_handle_methods_allocate_and_pass_what_they_did(rec):
    got = record_handle_methods(rec)
    assert sorted(got) == sorted(HANDLE_CALLS)
    assert {m for _, m, *_ in handle_cases()} == set(RUNGS) | {"attention_merge"}
    for cid in got:
        assert got[cid] == HANDLE_CALLS[cid], cid


@pytest.mark.parametrize("cid,exc,call", bad_inputs(), ids=[c[0] for c in bad_inputs()])
def test_a_bad_input_is_refused_before_the_library_is_asked(rec, cid, exc, call):
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and rec.calls == []


def test_the_prototypes_stand(rec):
    assert sorted(PROTOTYPES) == sorted(n for n in api.FUNCTIONS if "attention" in n) and len(PROTOTYPES) == 26
    for name, want in PROTOTYPES.items():
        assert prototype(name) == want, name


def test_the_signatures_stand():
    got = {name: str(inspect.signature(f)) for name, f in public_functions().items()}
    assert sorted(got) == sorted(SIGNATURES) and len(SIGNATURES) == 24 + 2 + 13 + 3
    for name in got:
        assert got[name] == SIGNATURES[name], name


# ---------------------------------------------------------------------------------------------------------------- recorded on commit 5747898
_S = "0.5773502691896258"   # 1 / sqrt(3) in double: what scale=None passes at k = 3
CALLS = {
    'attention': {
        'base': f'3 2 {_S} Q 4 K 3 V 4 O 5',
        'scale': '3 2 0.25 Q 4 K 3 V 4 O 5',
    },
    'attention_heads': {
        'base': f'4 3 2 {_S} Q 13 K 12 V 10 O 11',
        'scale': '4 3 2 0.25 Q 13 K 12 V 10 O 11',
    },
    'attention_backward': {
        'base': f'3 2 {_S} Q 4 K 3 V 4 G 2 dQ 3 dK 4 dV 2',
        'scale': '3 2 0.25 Q 4 K 3 V 4 G 2 dQ 3 dK 4 dV 2',
        'dQ=None': f'3 2 {_S} Q 4 K 3 V 4 G 2 NULL 3 dK 4 dV 2',
        'dK=None': f'3 2 {_S} Q 4 K 3 V 4 G 2 dQ 3 NULL 3 dV 2',
        'dV=None': f'3 2 {_S} Q 4 K 3 V 4 G 2 dQ 3 dK 4 NULL 2',
    },
    'attention_heads_backward': {
        'base': f'4 3 2 {_S} Q 13 K 12 V 10 G 8 dQ 12 dK 13 dV 8',
        'scale': '4 3 2 0.25 Q 13 K 12 V 10 G 8 dQ 12 dK 13 dV 8',
        'dQ=None': f'4 3 2 {_S} Q 13 K 12 V 10 G 8 NULL 12 dK 13 dV 8',
        'dK=None': f'4 3 2 {_S} Q 13 K 12 V 10 G 8 dQ 12 NULL 12 dV 8',
        'dV=None': f'4 3 2 {_S} Q 13 K 12 V 10 G 8 dQ 12 dK 13 NULL 8',
    },
    'attention_bias': {
        'base': f'4 3 2 {_S} Q 13 K 12 V 10 B 13 O 11',
        'scale': '4 3 2 0.25 Q 13 K 12 V 10 B 13 O 11',
        'B=None': f'4 3 2 {_S} Q 13 K 12 V 10 NULL 0 O 11',
        'B=shared': f'4 3 2 {_S} Q 13 K 12 V 10 B1 0 O 11',
        'ldb': f'4 3 2 {_S} Q 13 K 12 V 10 Bflat 17 O 11',
    },
    'attention_bias_backward': {
        'base': f'4 3 2 {_S} Q 13 K 12 V 10 B 13 G 8 dQ 12 dK 13 dV 8 dB 11',
        'scale': '4 3 2 0.25 Q 13 K 12 V 10 B 13 G 8 dQ 12 dK 13 dV 8 dB 11',
        'B=None': f'4 3 2 {_S} Q 13 K 12 V 10 NULL 0 G 8 dQ 12 dK 13 dV 8 dB 11',
        'dQ=None': f'4 3 2 {_S} Q 13 K 12 V 10 B 13 G 8 NULL 12 dK 13 dV 8 dB 11',
        'dK=None': f'4 3 2 {_S} Q 13 K 12 V 10 B 13 G 8 dQ 12 NULL 12 dV 8 dB 11',
        'dV=None': f'4 3 2 {_S} Q 13 K 12 V 10 B 13 G 8 dQ 12 dK 13 NULL 8 dB 11',
        'dB=None': f'4 3 2 {_S} Q 13 K 12 V 10 B 13 G 8 dQ 12 dK 13 dV 8 NULL 0',
        'B=shared': f'4 3 2 {_S} Q 13 K 12 V 10 B1 0 G 8 dQ 12 dK 13 dV 8 dB 11',
        'ldb': f'4 3 2 {_S} Q 13 K 12 V 10 Bflat 17 G 8 dQ 12 dK 13 dV 8 dB 11',
        'lddb': f'4 3 2 {_S} Q 13 K 12 V 10 B 13 G 8 dQ 12 dK 13 dV 8 dB 19',
        'B=None,ldb,lddb': f'4 3 2 {_S} Q 13 K 12 V 10 NULL 17 G 8 dQ 12 dK 13 dV 8 dB 19',
    },
    'attention_gqa': {
        'base': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 O 11',
        'scale': '4 2 3 2 0.25 Q 13 K 6 V 6 B 13 O 11',
        'B=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 NULL 0 O 11',
        'B=shared': f'4 2 3 2 {_S} Q 13 K 6 V 6 B1 0 O 11',
        'ldb': f'4 2 3 2 {_S} Q 13 K 6 V 6 Bflat 17 O 11',
    },
    'attention_gqa_backward': {
        'base': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 dQ 12 dK 7 dV 4 dB 11',
        'scale': '4 2 3 2 0.25 Q 13 K 6 V 6 B 13 G 8 dQ 12 dK 7 dV 4 dB 11',
        'B=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 NULL 0 G 8 dQ 12 dK 7 dV 4 dB 11',
        'dQ=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 NULL 12 dK 7 dV 4 dB 11',
        'dK=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 dQ 12 NULL 6 dV 4 dB 11',
        'dV=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 dQ 12 dK 7 NULL 4 dB 11',
        'dB=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 dQ 12 dK 7 dV 4 NULL 0',
        'B=shared': f'4 2 3 2 {_S} Q 13 K 6 V 6 B1 0 G 8 dQ 12 dK 7 dV 4 dB 11',
        'ldb': f'4 2 3 2 {_S} Q 13 K 6 V 6 Bflat 17 G 8 dQ 12 dK 7 dV 4 dB 11',
        'lddb': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 dQ 12 dK 7 dV 4 dB 19',
        'B=None,ldb,lddb': f'4 2 3 2 {_S} Q 13 K 6 V 6 NULL 17 G 8 dQ 12 dK 7 dV 4 dB 19',
    },
    'attention_gqa_lse': {
        'base': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 O 11 L 6',
        'scale': '4 2 3 2 0.25 Q 13 K 6 V 6 B 13 O 11 L 6',
        'B=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 NULL 0 O 11 L 6',
        'L=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 O 11 NULL 0',
        'B=shared': f'4 2 3 2 {_S} Q 13 K 6 V 6 B1 0 O 11 L 6',
        'ldb': f'4 2 3 2 {_S} Q 13 K 6 V 6 Bflat 17 O 11 L 6',
        'ldl': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 O 11 Lflat 23',
    },
    'attention_gqa_lse_16': {
        'base': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 O 11 1 L 6',
        'scale': '4 2 3 2 0.25 1 Q 13 K 6 V 6 B 13 O 11 1 L 6',
        'B=None': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 NULL 0 O 11 1 L 6',
        'L=None': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 O 11 1 NULL 0',
        'B=shared': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B1 0 O 11 1 L 6',
        'ldb': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 Bflat 17 O 11 1 L 6',
        'ldl': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 O 11 1 Lflat 23',
        'bf16': f'4 2 3 2 {_S} 2 Q 13 K 6 V 6 B 13 O 11 2 L 6',
        'O=fp32': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 O 11 0 L 6',
        'bf16,O=fp32,L=None': f'4 2 3 2 {_S} 2 Q 13 K 6 V 6 B 13 O 11 0 NULL 0',
    },
    'attention_gqa_backward_lse': {
        'base': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 O 11 L 6 dQ 12 dK 7 dV 4 dB 11',
        'scale': '4 2 3 2 0.25 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 dQ 12 dK 7 dV 4 dB 11',
        'B=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 NULL 0 G 8 O 11 L 6 dQ 12 dK 7 dV 4 dB 11',
        'dQ=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 O 11 L 6 NULL 12 dK 7 dV 4 dB 11',
        'dK=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 O 11 L 6 dQ 12 NULL 6 dV 4 dB 11',
        'dV=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 O 11 L 6 dQ 12 dK 7 NULL 4 dB 11',
        'dB=None': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 O 11 L 6 dQ 12 dK 7 dV 4 NULL 0',
        'B=shared': f'4 2 3 2 {_S} Q 13 K 6 V 6 B1 0 G 8 O 11 L 6 dQ 12 dK 7 dV 4 dB 11',
        'ldb': f'4 2 3 2 {_S} Q 13 K 6 V 6 Bflat 17 G 8 O 11 L 6 dQ 12 dK 7 dV 4 dB 11',
        'lddb': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 O 11 L 6 dQ 12 dK 7 dV 4 dB 19',
        'ldl': f'4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 O 11 Lflat 23 dQ 12 dK 7 dV 4 dB 11',
        'B=None,ldb,lddb': f'4 2 3 2 {_S} Q 13 K 6 V 6 NULL 17 G 8 O 11 L 6 dQ 12 dK 7 dV 4 dB 19',
    },
    'attention_gqa_backward_16': {
        'base': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 1 dQ 12 1 dK 7 dV 4 dB 11',
        'scale': '4 2 3 2 0.25 1 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 1 dQ 12 1 dK 7 dV 4 dB 11',
        'B=None': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 NULL 0 G 8 O 11 L 6 1 dQ 12 1 dK 7 dV 4 dB 11',
        'dQ=None': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 1 NULL 12 1 dK 7 dV 4 dB 11',
        'dK=None': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 1 dQ 12 1 NULL 6 dV 4 dB 11',
        'dV=None': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 1 dQ 12 1 dK 7 NULL 4 dB 11',
        'dB=None': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 1 dQ 12 1 dK 7 dV 4 NULL 0',
        'B=shared': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B1 0 G 8 O 11 L 6 1 dQ 12 1 dK 7 dV 4 dB 11',
        'ldb': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 Bflat 17 G 8 O 11 L 6 1 dQ 12 1 dK 7 dV 4 dB 11',
        'lddb': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 1 dQ 12 1 dK 7 dV 4 dB 19',
        'ldl': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 O 11 Lflat 23 1 dQ 12 1 dK 7 dV 4 dB 11',
        'B=None,ldb,lddb': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 NULL 17 G 8 O 11 L 6 1 dQ 12 1 dK 7 dV 4 dB 19',
        'bf16': f'4 2 3 2 {_S} 2 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 2 dQ 12 2 dK 7 dV 4 dB 11',
        'dQ=fp32': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 0 dQ 12 1 dK 7 dV 4 dB 11',
        'dK,dV=fp32': f'4 2 3 2 {_S} 2 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 2 dQ 12 0 dK 7 dV 4 dB 11',
        'all fp32': f'4 2 3 2 {_S} 2 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 0 dQ 12 0 dK 7 dV 4 dB 11',
        'O=L=None': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 NULL 8 NULL 0 1 dQ 12 1 dK 7 dV 4 dB 11',
        'O=L=None,dK=None,dV fp32': f'4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 NULL 8 NULL 0 1 dQ 12 0 NULL 6 dV 4 dB 11',
        'dQ=None,dV=None,dK fp32': f'4 2 3 2 {_S} 2 Q 13 K 6 V 6 B 13 G 8 O 11 L 6 2 NULL 12 0 dK 7 NULL 4 dB 11',
    },
}
_F, _T = "ndarray float32", "Tensor torch."
HANDLE_CALLS = {
    'attention': f'spmv_hip_attention: h4 5 rp ci va 3 2 {_S} Q 4 K 3 V 4 r0 2 -> r0={_F} (5, 2)',
    'attention [out, scale]': f'spmv_hip_attention: h4 5 rp ci va 3 2 0.25 Q 4 K 3 V 4 O 5 -> O={_F} (5, 2)',
    'attention_heads': f'spmv_hip_attention_heads: h4 5 rp ci va 4 3 2 {_S} Q 13 K 12 V 10 r0 8 -> r0={_F} (5, 8)',
    'attention_heads [out]': f'spmv_hip_attention_heads: h4 5 rp ci va 4 3 2 {_S} Q 13 K 12 V 10 O 11 -> O={_F} (5, 8)',
    'attention_backward': f'spmv_hip_attention_backward: h4 5 rp ci va 3 2 {_S} Q 4 K 3 V 4 G 2 r0 3 r1 3 r2 2 -> r0={_F} (5, 3), r1={_F} (7, 3), r2={_F} (7, 2)',
    'attention_backward [need]': f'spmv_hip_attention_backward: h4 5 rp ci va 3 2 0.25 Q 4 K 3 V 4 G 2 r0 3 NULL 3 r2 2 -> r0={_F} (5, 3), None, r2={_F} (7, 2)',
    'attention_heads_backward': f'spmv_hip_attention_heads_backward: h4 5 rp ci va 4 3 2 {_S} Q 13 K 12 V 10 G 8 r0 12 r1 12 r2 8 -> r0={_F} (5, 12), r1={_F} (7, 12), r2={_F} (7, 8)',
    'attention_heads_backward [need]': f'spmv_hip_attention_heads_backward: h4 5 rp ci va 4 3 2 {_S} Q 13 K 12 V 10 G 8 r0 12 NULL 12 r2 8 -> r0={_F} (5, 12), None, r2={_F} (7, 8)',
    'attention_bias': f'spmv_hip_attention_bias: h4 5 rp ci va 4 3 2 {_S} Q 13 K 12 V 10 B 13 r0 8 -> r0={_F} (5, 8)',
    'attention_bias [shared, out]': f'spmv_hip_attention_bias: h4 5 rp ci va 4 3 2 {_S} Q 13 K 12 V 10 B1 0 O 11 -> O={_F} (5, 8)',
    'attention_bias_backward': f'spmv_hip_attention_bias_backward: h4 5 rp ci va 4 3 2 {_S} Q 13 K 12 V 10 B 13 G 8 r0 12 r1 12 r2 8 r3 11 -> '
                               f'r0={_F} (5, 12), r1={_F} (7, 12), r2={_F} (7, 8), r3={_F} (4, 11)',
    'attention_bias_backward [need]': f'spmv_hip_attention_bias_backward: h4 5 rp ci va 4 3 2 {_S} Q 13 K 12 V 10 NULL 0 G 8 NULL 12 r1 12 NULL 8 r3 11 -> '
                                      f'None, r1={_F} (7, 12), None, r3={_F} (4, 11)',
    'attention_gqa': f'spmv_hip_attention_gqa: h4 5 rp ci va 4 2 3 2 {_S} Q 13 K 6 V 6 NULL 0 r0 8 -> r0={_F} (5, 8)',
    'attention_gqa [bias, out]': f'spmv_hip_attention_gqa: h4 5 rp ci va 4 2 3 2 0.25 Q 13 K 6 V 6 B 13 O 11 -> O={_F} (5, 8)',
    'attention_gqa_backward': f'spmv_hip_attention_gqa_backward: h4 5 rp ci va 4 2 3 2 {_S} Q 13 K 6 V 6 B1 0 G 8 r0 12 r1 6 r2 4 r3 11 -> '
                              f'r0={_F} (5, 12), r1={_F} (7, 6), r2={_F} (7, 4), r3={_F} (4, 11)',
    'attention_gqa_backward [need]': f'spmv_hip_attention_gqa_backward: h4 5 rp ci va 4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 NULL 12 r1 6 NULL 4 r3 11 -> '
                                     f'None, r1={_F} (7, 6), None, r3={_F} (4, 11)',
    'attention_gqa_lse': f'spmv_hip_attention_gqa_lse: h4 5 rp ci va 4 2 3 2 {_S} Q 13 K 6 V 6 NULL 0 r0 8 r1 5 -> r0={_F} (5, 8), r1={_F} (4, 5)',
    'attention_gqa_lse [bias, out, lse]': f'spmv_hip_attention_gqa_lse: h4 5 rp ci va 4 2 3 2 {_S} Q 13 K 6 V 6 B 13 O 11 L 6 -> O={_F} (5, 8), L={_F} (4, 5)',
    'attention_gqa_lse_16': f'spmv_hip_attention_gqa_lse_16: h4 5 rp ci va 4 2 3 2 {_S} 1 Q 13 K 6 V 6 NULL 0 r0 8 1 r1 5 -> r0={_T}float16 (5, 8), r1={_T}float32 (4, 5)',
    'attention_gqa_lse_16 [fp32 out, no lse]': f'spmv_hip_attention_gqa_lse_16: h4 5 rp ci va 4 2 3 2 {_S} 2 Q 13 K 6 V 6 B 13 r0 8 0 NULL 0 -> r0={_T}float32 (5, 8), None',
    'attention_merge': f'spmv_hip_attention_merge: h4 4 2 O 11 L 6 G 8 B 5 r0 8 r1 5 -> r0={_F} (5, 8), r1={_F} (4, 5)',
    'attention_merge [in place, no lse]': f'spmv_hip_attention_merge: h4 4 2 O 11 L 6 G 8 B 5 O 11 NULL 0 -> O={_F} (5, 8), None',
    'attention_gqa_backward_lse': f'spmv_hip_attention_gqa_backward_lse: h4 5 rp ci va 4 2 3 2 {_S} Q 13 K 6 V 6 B 13 G 8 O 11 L 6 r0 12 r1 6 r2 4 r3 11 -> '
                                  f'r0={_F} (5, 12), r1={_F} (7, 6), r2={_F} (7, 4), r3={_F} (4, 11)',
    'attention_gqa_backward_lse [need]': f'spmv_hip_attention_gqa_backward_lse: h4 5 rp ci va 4 2 3 2 0.25 Q 13 K 6 V 6 NULL 0 G 8 O 11 L 6 NULL 12 r1 6 NULL 4 r3 11 -> '
                                         f'None, r1={_F} (7, 6), None, r3={_F} (4, 11)',
    'attention_gqa_backward_16': f'spmv_hip_attention_gqa_backward_16: h4 5 rp ci va 4 2 3 2 {_S} 1 Q 13 K 6 V 6 B 13 G 8 NULL 8 NULL 0 1 r0 12 1 r1 6 r2 4 r3 11 -> '
                                 f'r0={_T}float16 (5, 12), r1={_T}float16 (7, 6), r2={_T}float16 (7, 4), r3={_T}float32 (4, 11)',
    'attention_gqa_backward_16 [O, L, fp32 dQ]': f'spmv_hip_attention_gqa_backward_16: h4 5 rp ci va 4 2 3 2 {_S} 2 Q 13 K 6 V 6 NULL 0 G 8 O 11 L 6 0 r0 12 2 r1 6 r2 4 r3 11 -> '
                                                 f'r0={_T}float32 (5, 12), r1={_T}bfloat16 (7, 6), r2={_T}bfloat16 (7, 4), r3={_T}float32 (4, 11)',
    'attention_gqa_backward_16 [need, fp32 dK dV]': f'spmv_hip_attention_gqa_backward_16: h4 5 rp ci va 4 2 3 2 {_S} 1 Q 13 K 6 V 6 B1 0 G 8 NULL 8 NULL 0 1 NULL 12 0 r1 6 NULL 4 r3 11 -> '
                                                    f'None, r1={_T}float32 (7, 6), None, r3={_T}float32 (4, 11)',
}
# the result, a colon, a letter per argument (prototype())
PROTOTYPES = {
    'spmv_hip_attention': 'i:Hipppiidpqpqpqpq',
    'spmv_hip_time_attention_launches': 'd:HiidpqpqpqpqiiF',
    'spmv_hip_attention_heads': 'i:Hipppiiidpqpqpqpq',
    'spmv_hip_time_attention_heads_launches': 'd:HiiidpqpqpqpqiiF',
    'spmv_hip_attention_backward': 'i:Hipppiidpqpqpqpqpqpqpq',
    'spmv_hip_time_attention_backward_launches': 'd:HiidpqpqpqpqpqpqpqiiF',
    'spmv_hip_attention_heads_backward': 'i:Hipppiiidpqpqpqpqpqpqpq',
    'spmv_hip_time_attention_heads_backward_launches': 'd:HiiidpqpqpqpqpqpqpqiiF',
    'spmv_hip_attention_bias': 'i:Hipppiiidpqpqpqpqpq',
    'spmv_hip_time_attention_bias_launches': 'd:HiiidpqpqpqpqpqiiF',
    'spmv_hip_attention_bias_backward': 'i:Hipppiiidpqpqpqpqpqpqpqpqpq',
    'spmv_hip_time_attention_bias_backward_launches': 'd:HiiidpqpqpqpqpqpqpqpqpqiiF',
    'spmv_hip_attention_gqa': 'i:Hipppiiiidpqpqpqpqpq',
    'spmv_hip_time_attention_gqa_launches': 'd:HiiiidpqpqpqpqpqiiF',
    'spmv_hip_attention_gqa_backward': 'i:Hipppiiiidpqpqpqpqpqpqpqpqpq',
    'spmv_hip_time_attention_gqa_backward_launches': 'd:HiiiidpqpqpqpqpqpqpqpqpqiiF',
    'spmv_hip_attention_gqa_lse': 'i:Hipppiiiidpqpqpqpqpqpq',
    'spmv_hip_time_attention_gqa_lse_launches': 'd:HiiiidpqpqpqpqpqpqiiF',
    'spmv_hip_attention_gqa_lse_16': 'i:Hipppiiiidipqpqpqpqpqipq',
    'spmv_hip_time_attention_gqa_lse_16_launches': 'd:HiiiidipqpqpqpqpqipqiiF',
    'spmv_hip_attention_merge': 'i:Hiipqpqpqpqpqpq',
    'spmv_hip_time_attention_merge_launches': 'd:HiipqpqpqpqpqpqiiF',
    'spmv_hip_attention_gqa_backward_lse': 'i:Hipppiiiidpqpqpqpqpqpqpqpqpqpqpq',
    'spmv_hip_time_attention_gqa_backward_lse_launches': 'd:HiiiidpqpqpqpqpqpqpqpqpqpqpqiiF',
    'spmv_hip_attention_gqa_backward_16': 'i:Hipppiiiidipqpqpqpqpqpqpqipqipqpqpq',
    'spmv_hip_time_attention_gqa_backward_16_launches': 'd:HiiiidipqpqpqpqpqpqpqipqipqpqpqiiF',
}
_CSR, _BWD = "handle, m, RowPtr, ColIdx, Matrix_Val", "dQ=None, dK=None, dV=None"
_T0, _N3, _N4 = "warmup=10, iters=100", "need=(True, True, True)", "need=(True, True, True, True)"
SIGNATURES = {
    'api.attention': f'({_CSR}, Q, K, V, O, scale=None, check=True)',
    'api.time_attention_launches': f'(handle, Q, K, V, O, scale=None, {_T0})',
    'api.Handle.attention': '(self, Q, K, V, scale=None, out=None)',
    'api.attention_heads': f'({_CSR}, heads, Q, K, V, O, scale=None, check=True)',
    'api.time_attention_heads_launches': f'(handle, heads, Q, K, V, O, scale=None, {_T0})',
    'api.Handle.attention_heads': '(self, Q, K, V, heads, scale=None, out=None)',
    'api.attention_backward': f'({_CSR}, Q, K, V, G, {_BWD}, scale=None, check=True)',
    'api.time_attention_backward_launches': f'(handle, Q, K, V, G, {_BWD}, scale=None, {_T0})',
    'api.Handle.attention_backward': f'(self, Q, K, V, G, scale=None, {_N3})',
    'api.attention_heads_backward': f'({_CSR}, heads, Q, K, V, G, {_BWD}, scale=None, check=True)',
    'api.time_attention_heads_backward_launches': f'(handle, heads, Q, K, V, G, {_BWD}, scale=None, {_T0})',
    'api.Handle.attention_heads_backward': f'(self, Q, K, V, G, heads, scale=None, {_N3})',
    'api.attention_bias': f'({_CSR}, heads, Q, K, V, B, O, scale=None, check=True, ldb=None)',
    'api.time_attention_bias_launches': f'(handle, heads, Q, K, V, B, O, scale=None, {_T0})',
    'api.Handle.attention_bias': '(self, Q, K, V, heads, bias, scale=None, out=None)',
    'api.attention_bias_backward': f'({_CSR}, heads, Q, K, V, B, G, {_BWD}, dB=None, scale=None, check=True, ldb=None, lddb=None)',
    'api.time_attention_bias_backward_launches': f'(handle, heads, Q, K, V, B, G, {_BWD}, dB=None, scale=None, {_T0})',
    'api.Handle.attention_bias_backward': f'(self, Q, K, V, bias, G, heads, scale=None, {_N4})',
    'api.attention_gqa': f'({_CSR}, heads, kv_heads, Q, K, V, B, O, scale=None, check=True, ldb=None)',
    'api.time_attention_gqa_launches': f'(handle, heads, kv_heads, Q, K, V, B, O, scale=None, {_T0})',
    'api.Handle.attention_gqa': '(self, Q, K, V, heads, kv_heads, bias=None, scale=None, out=None)',
    'api.attention_gqa_backward': f'({_CSR}, heads, kv_heads, Q, K, V, B, G, {_BWD}, dB=None, scale=None, check=True, ldb=None, lddb=None)',
    'api.time_attention_gqa_backward_launches': f'(handle, heads, kv_heads, Q, K, V, B, G, {_BWD}, dB=None, scale=None, {_T0})',
    'api.Handle.attention_gqa_backward': f'(self, Q, K, V, bias, G, heads, kv_heads, scale=None, {_N4})',
    'api.attention_gqa_lse': f'({_CSR}, heads, kv_heads, Q, K, V, B, O, L, scale=None, check=True, ldb=None, ldl=None)',
    'api.time_attention_gqa_lse_launches': f'(handle, heads, kv_heads, Q, K, V, B, O, L, scale=None, {_T0})',
    'api.Handle.attention_gqa_lse': '(self, Q, K, V, heads, kv_heads, bias=None, scale=None, out=None, lse=None)',
    'api.attention_gqa_lse_16': f'({_CSR}, heads, kv_heads, Q, K, V, B, O, L=None, scale=None, check=True, ldb=None, ldl=None)',
    'api.time_attention_gqa_lse_16_launches': f'(handle, heads, kv_heads, Q, K, V, B, O, L=None, scale=None, {_T0})',
    'api.Handle.attention_gqa_lse_16': '(self, Q, K, V, heads, kv_heads, B=None, scale=None, out_dtype=None, want_l=True)',
    'api.attention_gqa_backward_lse': f'({_CSR}, heads, kv_heads, Q, K, V, B, G, O, L, {_BWD}, dB=None, scale=None, check=True, ldb=None, lddb=None, ldl=None)',
    'api.time_attention_gqa_backward_lse_launches': f'(handle, heads, kv_heads, Q, K, V, B, G, O, L, {_BWD}, dB=None, scale=None, {_T0})',
    'api.Handle.attention_gqa_backward_lse': f'(self, Q, K, V, bias, G, O, L, heads, kv_heads, scale=None, {_N4})',
    'api.attention_gqa_backward_16': f'({_CSR}, heads, kv_heads, Q, K, V, B, G, O=None, L=None, {_BWD}, dB=None, scale=None, check=True, ldb=None, lddb=None, ldl=None)',
    'api.time_attention_gqa_backward_16_launches': f'(handle, heads, kv_heads, Q, K, V, B, G, O=None, L=None, {_BWD}, dB=None, scale=None, {_T0})',
    'api.Handle.attention_gqa_backward_16': f'(self, Q, K, V, B, G, heads, kv_heads, scale=None, O=None, L=None, {_N4}, dq_dtype=None, dkv_dtype=None)',
    'api.attention_merge': '(handle, heads, O1, L1, O2, L2, O, L=None, check=True, ldl=None)',
    'api.time_attention_merge_launches': f'(handle, heads, O1, L1, O2, L2, O, L=None, {_T0})',
    'api.Handle.attention_merge': '(self, O1, L1, O2, L2, heads, out=None, lse=None, want_lse=True)',
    'autograd.attention': "(handle, Q, K, V, scale=None, backward='composed', *, bias=None)",
    'autograd.attention_heads': "(handle, Q, K, V, heads, scale=None, backward='per_head', *, bias=None, kv_heads=None)",
    'autograd.attention_parts': '(handles, Q, Ks, Vs, heads, scale=None, *, kv_heads=None, biases=None, return_lse=False)',
}
