"""CPU: the 16-bit attention backward's entry points (spmv_hip_attention_gqa_backward_16 and its timer) are exported, declared and bound; the type
and argument rules hold without any device on a handle without device state (include/spmv_hip.h); the api wrapper's dtype and shape checks raise
before the library is asked; and a numpy restatement shows that rounding the fp32 sum of a group of three heads once and rounding the running sum
after every head differ -- what test_gpu_attention_backward_16.py's rounds test is there to catch."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
T_HANDLE, T_F16, T_BF16 = 0, 1, 2
_V, _LL = C.c_void_p, C.c_longlong
_H = api.spmv_Handle_t
_TAIL = [C.c_int, C.c_int, C.POINTER(C.c_float)]
_GQA = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
# io_type, Q, K, V, B, G, O, L with their lds, dq_type, dQ, dkv_type, dK, dV, dB
_OPS = [C.c_int, *[_V, _LL] * 7, C.c_int, _V, _LL, C.c_int, *[_V, _LL] * 3]
SIGNATURES = {
    "spmv_hip_attention_gqa_backward_16": (C.c_int, [_H, C.c_int, _V, _V, _V, *_GQA, *_OPS]),
    "spmv_hip_time_attention_gqa_backward_16_launches": (C.c_double, [_H, *_GQA, *_OPS, *_TAIL]),
}
M, H, HKV, K, DV, NNZ = 4, 4, 2, 3, 2, 5
WK, WV, GK, GV = H * K, H * DV, HKV * K, HKV * DV


@pytest.fixture(scope="module")
def lib():
    build.build()
    return api.load()


def _failed(lib, monkeypatch, size):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    h = api.spmv_create_handle_all_in_one(-1, 4, None, None, None, 1, api.SPMV_METHODS.Method_Parallel, size, check=False)
    assert h and not h.contents.extraHandle and h.contents.data_size == size
    lib.spmv_hip_clear_error()
    return h


@pytest.fixture
def failed32(lib, monkeypatch):
    """create() with m < 0 fails in its argument check, before any device call: a valid fp32 handle without device state"""
    h = _failed(lib, monkeypatch, 4)
    yield h
    api.spmv_destory_handle(h)


@pytest.fixture
def failed64(lib, monkeypatch):
    h = _failed(lib, monkeypatch, 8)
    yield h
    api.spmv_destory_handle(h)


def buffers():
    """the operands by name, with their bits: the 16-bit ones as raw patterns (with room for fp32 outputs), B, O, L and dB fp32"""
    u16 = lambda rows, w, base: np.arange(rows * w, dtype=np.uint16).reshape(rows, w) + base
    a = {"Q": u16(M, WK, 0x3c00), "K": u16(M, GK, 0x3800), "V": u16(M, GV, 0x4000), "G": u16(M, WV, 0x3400),
         "B": np.arange(H * NNZ, dtype=np.float32).reshape(H, NNZ) * 0.25, "O": np.ones((M, WV), dtype=np.float32), "L": np.ones((H, M), dtype=np.float32),
         "dQ": np.full((M, 2 * WK), 0xbeef, dtype=np.uint16), "dK": np.full((M, 2 * GK), 0xbeef, dtype=np.uint16), "dV": np.full((M, 2 * GV), 0xbeef, dtype=np.uint16),
         "dB": np.full((H, NNZ), -1.5, dtype=np.float32)}
    return a, {n: v.tobytes() for n, v in a.items()}


def unchanged(a, bits):
    return all(v is None or v.tobytes() == bits[n] for n, v in a.items())


def p(x):
    return None if x is None else x.ctypes.data


def _args(a, io, dq, dkv, ld):
    g = lambda name, d: ld.get(name, d)
    return [io, p(a["Q"]), g("ldq", WK), p(a["K"]), g("ldk", GK), p(a["V"]), g("ldv", GV), p(a["B"]), g("ldb", NNZ), p(a["G"]), g("ldg", WV), p(a["O"]), g("ldo", WV),
            p(a["L"]), g("ldl", M), dq, p(a["dQ"]), g("lddq", WK), dkv, p(a["dK"]), g("lddk", GK), p(a["dV"]), g("lddv", GV), p(a["dB"]), g("lddb", NNZ)]


def bwd(lib, h, heads, kv, k, dv, a, io=T_F16, dq=T_F16, dkv=T_F16, m=M, **ld):
    return lib.spmv_hip_attention_gqa_backward_16(h, m, None, None, None, heads, kv, k, dv, 1.0, *_args(a, io, dq, dkv, ld))


def bwd_timer(lib, h, heads, kv, k, dv, a, io=T_F16, dq=T_F16, dkv=T_F16, **ld):
    return lib.spmv_hip_time_attention_gqa_backward_16_launches(h, heads, kv, k, dv, 1.0, *_args(a, io, dq, dkv, ld), 1, 1, None)


def is_arg(lib, rc):
    ok = (rc == E_ARG or (isinstance(rc, float) and rc < 0)) and lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    return ok


def is_nostate(lib, rc):
    ok = (rc == E_NOSTATE or (isinstance(rc, float) and rc < 0)) and lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    return ok


GOOD_TYPES = [(io, dq, dkv) for io in (T_F16, T_BF16) for dq in (T_HANDLE, io) for dkv in (T_HANDLE, io)]
BAD_TYPES = [(0, 0, 0), (3, 0, 0), (-1, 0, 0), (T_BF16, T_F16, 0), (T_F16, T_BF16, 0), (T_F16, 0, T_BF16), (T_BF16, 0, T_F16), (T_F16, 3, 0), (T_F16, 0, 3), (T_BF16, -1, T_BF16)]


def test_exported_declared_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.attention_gqa_backward_16, api.time_attention_gqa_backward_16_launches, api.Handle.attention_gqa_backward_16):
        assert callable(f)
    sig = inspect.signature(api.attention_gqa_backward_16)
    assert list(sig.parameters)[:19] == ["handle", "m", "RowPtr", "ColIdx", "Matrix_Val", "heads", "kv_heads", "Q", "K", "V", "B", "G", "O", "L", "dQ", "dK", "dV", "dB", "scale"]
    assert all(sig.parameters[n].default is None for n in ("O", "L", "dQ", "dK", "dV", "dB", "scale"))
    sig = inspect.signature(api.Handle.attention_gqa_backward_16)
    assert list(sig.parameters)[1:] == ["Q", "K", "V", "B", "G", "heads", "kv_heads", "scale", "O", "L", "need", "dq_dtype", "dkv_dtype"]
    assert sig.parameters["dq_dtype"].default is None and sig.parameters["dkv_dtype"].default is None and sig.parameters["O"].default is None
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert "int spmv_hip_attention_gqa_backward_16(" in open(os.path.join(inc, "spmv_hip.h")).read()
    assert "double spmv_hip_time_attention_gqa_backward_16_launches(" in open(os.path.join(inc, "spmv_hip_tools.h")).read()


def test_good_arguments_get_as_far_as_the_state_on_an_fp32_handle(lib, failed32):
    a, bits = buffers()
    for io, dq, dkv in GOOD_TYPES:
        for call in (bwd, bwd_timer):
            for heads, kv in ((H, HKV), (H, 1), (HKV, HKV)):
                assert is_nostate(lib, call(lib, failed32, heads, kv, K, DV, a, io=io, dq=dq, dkv=dkv)), (call.__name__, io, dq, dkv, heads, kv)
                assert is_nostate(lib, call(lib, failed32, heads, kv, K, DV, dict(a, O=None, L=None), io=io, dq=dq, dkv=dkv)), "the self-normalising form"
        assert is_nostate(lib, bwd(lib, failed32, H, HKV, K, DV, dict(a, O=None, L=None), io=io, dq=dq, dkv=dkv, ldo=0, ldl=-5))   # no O and L: their lds are not looked at
        assert is_nostate(lib, bwd(lib, failed32, H, HKV, K, DV, dict(a, dK=None, dV=None), io=io, dq=dq, dkv=dkv, lddk=0, lddv=0))
    # nothing wanted: no work, the handle's state is not looked at
    assert bwd(lib, failed32, H, HKV, K, DV, dict(a, dQ=None, dK=None, dV=None, dB=None)) == 0 and lib.spmv_hip_last_error() == 0
    assert is_nostate(lib, bwd(lib, failed32, H, HKV, K, DV, {n: (None if n in "QKVGOL" else v) for n, v in a.items()}, m=0, ldl=0))   # m = 0: NULL inputs are no error
    assert unchanged(a, bits)


@pytest.mark.parametrize("io,dq,dkv", BAD_TYPES)
def test_bad_types_are_argument_errors_before_the_gate(lib, failed32, io, dq, dkv):
    a, bits = buffers()
    assert is_arg(lib, bwd(lib, failed32, H, HKV, K, DV, a, io=io, dq=dq, dkv=dkv))
    assert is_arg(lib, bwd_timer(lib, failed32, H, HKV, K, DV, a, io=io, dq=dq, dkv=dkv))
    assert unchanged(a, bits)


def test_an_fp64_handle_is_an_argument_error(lib, failed64):
    a, bits = buffers()
    for io, dq, dkv in GOOD_TYPES:
        assert is_arg(lib, bwd(lib, failed64, H, HKV, K, DV, a, io=io, dq=dq, dkv=dkv)), (io, dq, dkv)
        assert is_arg(lib, bwd_timer(lib, failed64, H, HKV, K, DV, a, io=io, dq=dq, dkv=dkv)), (io, dq, dkv)
    assert unchanged(a, bits)


def test_exactly_one_of_o_and_l_is_an_argument_error(lib, failed32):
    a, bits = buffers()
    for missing in ("O", "L"):
        assert is_arg(lib, bwd(lib, failed32, H, HKV, K, DV, dict(a, **{missing: None}))), missing
        assert is_arg(lib, bwd_timer(lib, failed32, H, HKV, K, DV, dict(a, **{missing: None}))), missing
        assert is_nostate(lib, bwd(lib, failed32, H, HKV, K, DV, dict(a, **{missing: None}), m=0, ldl=0))   # m = 0: nothing is read
    assert unchanged(a, bits)


BIG = 2 ** 30
WIDE = dict(ldq=2 ** 40, ldk=2 ** 40, ldv=2 ** 40, ldg=2 ** 40, ldo=2 ** 40, lddq=2 ** 40, lddk=2 ** 40, lddv=2 ** 40)


@pytest.mark.parametrize("heads,kv,k,dv,ld", [
    # spmv_hip_attention_gqa_backward(_lse)'s rules, every one of them
    (0, 1, K, DV, {}), (-2, 1, K, DV, {}), (H, HKV, 0, DV, {}), (H, HKV, K, 0, {}),
    (H, HKV, K, DV, dict(ldq=WK - 1)), (H, HKV, K, DV, dict(ldk=GK - 1)), (H, HKV, K, DV, dict(ldv=GV - 1)), (H, HKV, K, DV, dict(ldg=WV - 1)),
    (H, HKV, K, DV, dict(lddq=WK - 1)), (H, HKV, K, DV, dict(lddk=GK - 1)), (H, HKV, K, DV, dict(lddv=GV - 1)),
    (H, HKV, K, DV, dict(ldo=WV - 1)), (H, HKV, K, DV, dict(ldl=M - 1)),
    (H, HKV, K, DV, dict(ldb=-1)), (H, HKV, K, DV, dict(lddb=-1)),
    (BIG, BIG, K, 1, WIDE), (H, 0, K, DV, {}), (H, 3, K, DV, WIDE), (3, 2, K, DV, WIDE), (H, H, K, DV, {}),
])
@pytest.mark.parametrize("io,dq,dkv", [(T_F16, T_F16, T_F16), (T_BF16, T_HANDLE, T_BF16)])
def test_bad_sizes_are_argument_errors_before_the_gate(lib, failed32, io, dq, dkv, heads, kv, k, dv, ld):
    """a bad heads, kv_heads, k, dv or ld is E_ARG even on a handle that would answer E_NOSTATE: the sizes are checked first"""
    a, bits = buffers()
    assert is_arg(lib, bwd(lib, failed32, heads, kv, k, dv, a, io=io, dq=dq, dkv=dkv, **ld))
    if "ldl" not in ld:   # the timer has no m: it leaves the planes' stride to the call it times
        assert is_arg(lib, bwd_timer(lib, failed32, heads, kv, k, dv, a, io=io, dq=dq, dkv=dkv, **ld))
    assert unchanged(a, bits)


def test_null_operand_and_null_handle_are_argument_errors(lib, failed32, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    a, bits = buffers()
    for missing in ("Q", "K", "V", "G"):
        assert is_arg(lib, bwd(lib, failed32, H, HKV, K, DV, dict(a, **{missing: None}))), missing
        assert is_arg(lib, bwd_timer(lib, failed32, H, HKV, K, DV, dict(a, **{missing: None}))), missing
    for call in (bwd, bwd_timer):
        assert is_arg(lib, call(lib, None, H, HKV, K, DV, a))
    assert unchanged(a, bits)


def test_the_python_layer_checks_before_any_device_call(lib, failed32, failed64):
    """the types come from the tensors' dtypes; mixed dtypes, a 16-bit tensor with an fp64 handle, a third output type, exactly one of O and L, and
    wrong shapes raise TypeError / ValueError in the wrapper: the handles here have no device state, and good arguments get E_NOSTATE from the library"""
    import torch
    for dt in (torch.float16, torch.bfloat16):
        other = torch.bfloat16 if dt == torch.float16 else torch.float16
        Q, Kk, Vv, G = (torch.ones(s, dtype=dt) for s in ((M, WK), (M, GK), (M, GV), (M, WV)))
        B, O, L = torch.zeros((H, NNZ)), torch.ones((M, WV)), torch.ones((H, M))
        call = lambda *a, **kw: api.attention_gqa_backward_16(failed32, M, None, None, None, H, HKV, *a, **kw)
        for odt in (dt, torch.float32):
            outs = dict(dQ=torch.full((M, WK), -1.0, dtype=odt), dK=torch.full((M, GK), -1.0, dtype=odt), dV=torch.full((M, GV), -1.0, dtype=odt), dB=torch.full((H, NNZ), -1.0))
            for ol in ((None, None), (O, L)):
                assert call(Q, Kk, Vv, B, G, *ol, check=False, **outs) == E_NOSTATE
                lib.spmv_hip_clear_error()
            with pytest.raises(api.SpmvError):
                api.time_attention_gqa_backward_16_launches(failed32, H, HKV, Q, Kk, Vv, B, G, O, L, warmup=1, iters=1, **outs)
            lib.spmv_hip_clear_error()
            with pytest.raises(TypeError):   # 16-bit tensors with an fp64 handle: the wrapper reads the public handle's data_size
                api.attention_gqa_backward_16(failed64, M, None, None, None, H, HKV, Q, Kk, Vv, B, G, **outs)
            assert all(bool((t == -1.0).all()) for t in outs.values())
        dQ = torch.zeros((M, WK), dtype=dt)
        for mixed in ((Q.to(other), Kk, Vv, B, G), (Q, Kk.to(other), Vv, B, G), (Q, Kk, Vv.float(), B, G), (Q, Kk, Vv, B, G.to(other)), (Q, Kk, Vv, B, G.float())):
            with pytest.raises(TypeError):
                call(*mixed, dQ=dQ)
        with pytest.raises(TypeError):   # fp32 operands belong to attention_gqa_backward
            call(Q.float(), Kk.float(), Vv.float(), B, G.float(), dQ=dQ.float())
        with pytest.raises(TypeError):   # numpy has no bfloat16: tensors only
            call(np.ones((M, WK), dtype=np.float16), Kk, Vv, B, G, dQ=dQ)
        with pytest.raises(TypeError):   # a dQ of the other 16-bit type, an fp64 dK
            call(Q, Kk, Vv, B, G, dQ=dQ.to(other))
        with pytest.raises(TypeError):
            call(Q, Kk, Vv, B, G, dK=torch.zeros((M, GK), dtype=torch.float64))
        with pytest.raises(TypeError):   # dK and dV share one type
            call(Q, Kk, Vv, B, G, dK=torch.zeros((M, GK), dtype=dt), dV=torch.zeros((M, GV)))
        with pytest.raises(TypeError):   # the bias, O and L stay fp32
            call(Q, Kk, Vv, B.to(dt), G, dQ=dQ)
        with pytest.raises(TypeError):
            call(Q, Kk, Vv, B, G, O.to(dt), L, dQ=dQ)
        for ol in ((O, None), (None, L)):   # exactly one of O and L
            with pytest.raises(ValueError):
                call(Q, Kk, Vv, B, G, *ol, dQ=dQ)
        with pytest.raises(ValueError):  # G is heads * dv wide
            call(Q, Kk, Vv, B, G[:, :-1], dQ=dQ)
        with pytest.raises(ValueError):  # dK has K's width
            call(Q, Kk, Vv, B, G, dK=torch.zeros((M, WK), dtype=dt))
        with pytest.raises(ValueError):  # O is heads * dv wide, L has a plane per QUERY head
            call(Q, Kk, Vv, B, G, O[:, :-1], L, dQ=dQ)
        with pytest.raises(ValueError):
            call(Q, Kk, Vv, B, G, O, torch.ones((HKV, M)), dQ=dQ)
        assert lib.spmv_hip_last_error() == 0   # none of these reached the library


def _narrow(x, kind):
    """fp32 -> fp16 / bf16 -> fp32, round to nearest even, in numpy"""
    x = np.asarray(x, dtype=np.float32)
    if kind == "f16":
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_one_rounding_of_a_group_sum_differs_from_a_rounding_per_head(kind):
    """a group of three heads whose dK terms are 1, ulp/2 and ulp/2 of the 16-bit type at 1: the fp32 chain (t0 + t1) + t2 is 1 + ulp exactly and
    rounds to 1 + ulp; rounding the running sum after every head -- what a 16-bit element read back between rounds would do -- gives 1 (each half
    ulp is a tie that goes to even).  So a read-back is visible to the rounds test."""
    ulp = np.float32(2.0 ** -10 if kind == "f16" else 2.0 ** -7)
    t = [np.float32(1.0), np.float32(ulp / 2), np.float32(ulp / 2)]
    once = _narrow(np.float32(np.float32(t[0] + t[1]) + t[2]), kind)
    twice = _narrow(_narrow(_narrow(t[0], kind) + t[1], kind) + t[2], kind)
    assert once == np.float32(1.0) + ulp and twice == np.float32(1.0) and once != twice
    # the narrowing restated here is torch's
    import torch
    dt = torch.float16 if kind == "f16" else torch.bfloat16
    x = np.random.default_rng(0).uniform(-70000, 70000, 4096).astype(np.float32)
    with np.errstate(over="ignore"):
        assert np.array_equal(_narrow(x, kind), torch.from_numpy(x).to(dt).float().numpy())
