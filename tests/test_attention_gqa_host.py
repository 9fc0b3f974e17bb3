"""CPU: the grouped-query attention's entry points (spmv_hip_attention_gqa, spmv_hip_attention_gqa_backward and their two timers) are exported
and bound with the declared signatures, the Python layers exist -- kv_heads= is accepted by autograd.attention_heads --, and the argument and
handle rules hold without any device (include/spmv_hip.h: SPMV_HIP_E_ARG for the bias calls' bad arguments, for kv_heads < 1, heads not a
multiple of kv_heads, kv_heads * k or kv_heads * dv beyond int and K / V / dK / dV strides below their kv_heads width, all before the handle's
state is looked at; E_NOSTATE for a handle without device state; every buffer keeps its bits)."""

import ctypes as C
import inspect

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
_V, _LL = C.c_void_p, C.c_longlong
_H = api.spmv_Handle_t
SIGNATURES = {
    "spmv_hip_attention_gqa": (C.c_int, [_H, C.c_int, _V, _V, _V, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL]),
    "spmv_hip_time_attention_gqa_launches": (C.c_double, [_H, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                                          C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "spmv_hip_attention_gqa_backward": (C.c_int, [_H, C.c_int, _V, _V, _V, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                                  _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL]),
    "spmv_hip_time_attention_gqa_backward_launches": (C.c_double, [_H, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                                                   _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL, C.c_int, C.c_int, C.POINTER(C.c_float)]),
}
H, HKV, K, DV, NNZ = 4, 2, 3, 2, 5
WK, WV = H * K, H * DV       # Q, dQ / O, G
GK, GV = HKV * K, HKV * DV   # K, dK / V, dV


@pytest.fixture(scope="module")
def lib():
    build.build()
    return api.load()


@pytest.fixture
def failed_handle(lib, monkeypatch):
    """create() with m < 0 fails in its argument check, before any device call: a valid handle without device state"""
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    h = api.spmv_create_handle_all_in_one(-1, 4, None, None, None, 1, api.SPMV_METHODS.Method_Parallel, 8, check=False)
    assert h and not h.contents.extraHandle
    lib.spmv_hip_clear_error()
    yield h
    api.spmv_destory_handle(h)


def buffers():
    """Q, K, V, B, G and the outputs O, dQ, dK, dV, dB, with their bits"""
    Q = np.arange(4 * WK, dtype=np.float64).reshape(4, WK) - 2
    Kk = np.arange(4 * GK, dtype=np.float64).reshape(4, GK) * 0.5
    Vv = np.arange(4 * GV, dtype=np.float64).reshape(4, GV) + 1
    B = np.arange(H * NNZ, dtype=np.float64).reshape(H, NNZ) * 0.25
    G = np.arange(4 * WV, dtype=np.float64).reshape(4, WV) - 3
    outs = [np.full((4, WV), -1.0), np.full((4, WK), -2.0), np.full((4, GK), -3.0), np.full((4, GV), -4.0), np.full((H, NNZ), -5.0)]
    arrays = [Q, Kk, Vv, B, G, *outs]
    return arrays, tuple(a.tobytes() for a in arrays)


def unchanged(arrays, bits):
    return tuple(a.tobytes() for a in arrays) == bits


def p(a):
    return None if a is None else a.ctypes.data


def fwd(lib, h, heads, kv, k, dv, a, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldo=WV):
    Q, Kk, Vv, B, G, O = a[:6]
    return lib.spmv_hip_attention_gqa(h, 4, None, None, None, heads, kv, k, dv, 1.0, p(Q), ldq, p(Kk), ldk, p(Vv), ldv, p(B), ldb, p(O), ldo)


def fwd_timer(lib, h, heads, kv, k, dv, a, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldo=WV):
    Q, Kk, Vv, B, G, O = a[:6]
    return lib.spmv_hip_time_attention_gqa_launches(h, heads, kv, k, dv, 1.0, p(Q), ldq, p(Kk), ldk, p(Vv), ldv, p(B), ldb, p(O), ldo, 1, 1, None)


def bwd(lib, h, heads, kv, k, dv, a, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldg=WV, lddq=WK, lddk=GK, lddv=GV, lddb=NNZ):
    Q, Kk, Vv, B, G, O, dQ, dK, dV, dB = a
    return lib.spmv_hip_attention_gqa_backward(h, 4, None, None, None, heads, kv, k, dv, 1.0, p(Q), ldq, p(Kk), ldk, p(Vv), ldv, p(B), ldb, p(G), ldg,
                                               p(dQ), lddq, p(dK), lddk, p(dV), lddv, p(dB), lddb)


def bwd_timer(lib, h, heads, kv, k, dv, a, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldg=WV, lddq=WK, lddk=GK, lddv=GV, lddb=NNZ):
    Q, Kk, Vv, B, G, O, dQ, dK, dV, dB = a
    return lib.spmv_hip_time_attention_gqa_backward_launches(h, heads, kv, k, dv, 1.0, p(Q), ldq, p(Kk), ldk, p(Vv), ldv, p(B), ldb, p(G), ldg,
                                                             p(dQ), lddq, p(dK), lddk, p(dV), lddv, p(dB), lddb, 1, 1, None)


def test_exported_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.attention_gqa, api.attention_gqa_backward, api.time_attention_gqa_launches, api.time_attention_gqa_backward_launches,
              api.Handle.attention_gqa, api.Handle.attention_gqa_backward):
        assert callable(f)
    sig = inspect.signature(api.Handle.attention_gqa)
    assert list(sig.parameters)[1:9] == ["Q", "K", "V", "heads", "kv_heads", "bias", "scale", "out"]
    assert sig.parameters["bias"].default is None and sig.parameters["scale"].default is None and sig.parameters["out"].default is None
    sig = inspect.signature(api.Handle.attention_gqa_backward)
    assert list(sig.parameters)[1:10] == ["Q", "K", "V", "bias", "G", "heads", "kv_heads", "scale", "need"]
    assert sig.parameters["need"].default == (True, True, True, True)


def test_headers_declare_the_four_symbols():
    import os
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    hip, tools = open(os.path.join(inc, "spmv_hip.h")).read(), open(os.path.join(inc, "spmv_hip_tools.h")).read()
    assert "int spmv_hip_attention_gqa(" in hip and "int spmv_hip_attention_gqa_backward(" in hip
    assert "double spmv_hip_time_attention_gqa_launches(" in tools and "double spmv_hip_time_attention_gqa_backward_launches(" in tools


def test_autograd_layer_accepts_kv_heads():
    from spmv_amd import autograd
    par = inspect.signature(autograd.attention_heads).parameters["kv_heads"]
    assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY   # trailing keyword: existing calls are untouched
    assert "kv_heads" in autograd.attention_heads.__doc__ and "ascending head" in autograd.attention_heads.__doc__


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    a, bits = buffers()
    for call in (fwd, bwd):
        lib.spmv_hip_clear_error()
        assert call(lib, None, H, HKV, K, DV, a) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
    for call in (fwd_timer, bwd_timer):
        lib.spmv_hip_clear_error()
        assert call(lib, None, H, HKV, K, DV, a) < 0
        assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(a, bits)


def test_failed_handle_has_no_state(lib, failed_handle):
    """good arguments -- a group of two, MQA, a K / V head per query head -- get as far as the handle's state"""
    a, bits = buffers()
    Q, Kk, Vv, B, G, O, dQ, dK, dV, dB = a
    for call in (fwd, bwd):
        assert call(lib, failed_handle, H, HKV, K, DV, a) == E_NOSTATE
        assert lib.spmv_hip_last_error() == E_NOSTATE
        lib.spmv_hip_clear_error()
        assert call(lib, failed_handle, H, 1, K, DV, a) == E_NOSTATE   # MQA: the strides are more than one block
        lib.spmv_hip_clear_error()
        assert call(lib, failed_handle, HKV, HKV, K, DV, a) == E_NOSTATE   # kv_heads = heads
        lib.spmv_hip_clear_error()
    for call in (fwd_timer, bwd_timer):
        assert call(lib, failed_handle, H, HKV, K, DV, a) < 0
        assert lib.spmv_hip_last_error() == E_NOSTATE
        lib.spmv_hip_clear_error()
    # the Python layer: per-head planes, a shared plane, no bias
    for bias in (B, B[0], None):
        assert api.attention_gqa(failed_handle, 4, None, None, None, H, HKV, Q, Kk, Vv, bias, O, check=False) == E_NOSTATE
        lib.spmv_hip_clear_error()
        assert api.attention_gqa_backward(failed_handle, 4, None, None, None, H, HKV, Q, Kk, Vv, bias, G, dQ, dK, dV, dB, check=False) == E_NOSTATE
        lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.attention_gqa(failed_handle, 4, None, None, None, H, HKV, Q, Kk, Vv, B, O, scale=0.5)
    with pytest.raises(ValueError):   # widths that do not divide: four query heads over three K / V heads
        api.attention_gqa(failed_handle, 4, None, None, None, H, 3, Q, Kk, Vv, B, O)
    with pytest.raises(ValueError):   # K as wide as Q: not two K / V heads of Q's head width
        api.attention_gqa(failed_handle, 4, None, None, None, H, HKV, Q, Q, Vv, B, O)
    with pytest.raises(ValueError):   # dK has K's width, not Q's
        api.attention_gqa_backward(failed_handle, 4, None, None, None, H, HKV, Q, Kk, Vv, B, G, dK=dQ)
    with pytest.raises(ValueError):   # dB always has a plane per QUERY head
        api.attention_gqa_backward(failed_handle, 4, None, None, None, H, HKV, Q, Kk, Vv, B, G, dB=np.zeros((HKV, NNZ)))
    assert unchanged(a, bits)


def test_all_outputs_null_returns_after_argument_checking(lib, failed_handle):
    """nothing wanted: 0 without looking at the handle's state -- but the arguments are checked first"""
    a, bits = buffers()
    none = a[:6] + [None] * 4
    assert bwd(lib, failed_handle, H, HKV, K, DV, none) == 0
    assert lib.spmv_hip_last_error() == 0
    assert bwd(lib, failed_handle, H, 3, K, DV, none) == E_ARG
    lib.spmv_hip_clear_error()
    assert bwd(lib, failed_handle, H, HKV, K, DV, none, ldk=GK - 1) == E_ARG
    lib.spmv_hip_clear_error()
    assert bwd(lib, failed_handle, H, HKV, K, DV, none, lddk=0, lddv=0, lddq=0, lddb=-1) == 0   # the strides of outputs that are not wanted are not looked at
    only_db = a[:6] + [None] * 3 + [a[9]]
    assert bwd(lib, failed_handle, H, HKV, K, DV, only_db) == E_NOSTATE   # dB alone is work
    lib.spmv_hip_clear_error()
    assert unchanged(a, bits)


BIG = 2 ** 30
WIDE = dict(ldq=2 ** 40, ldk=2 ** 40, ldv=2 ** 40, ldo=2 ** 40, ldg=2 ** 40, lddq=2 ** 40, lddk=2 ** 40, lddv=2 ** 40)


@pytest.mark.parametrize("heads,kv,k,dv,ld", [
    # the bias calls' rules
    (0, 1, K, DV, {}), (-2, 1, K, DV, {}), (H, HKV, 0, DV, {}), (H, HKV, K, 0, {}), (H, HKV, K, -2, {}),
    (H, HKV, K, DV, dict(ldq=WK - 1)), (H, HKV, K, DV, dict(ldo=WV - 1, ldg=WV - 1)),
    (BIG, BIG, K, 1, WIDE), (65536, 1, 65536, 1, WIDE),                                        # heads * k beyond int
    (H, HKV, K, DV, dict(ldb=-1)), (H, HKV, K, DV, dict(ldb=-2 ** 40)),
    # the new ones
    (H, 0, K, DV, {}), (H, -1, K, DV, {}), (H, -2, K, DV, {}),                                 # kv_heads < 1
    (H, 3, K, DV, WIDE), (H, 8, K, DV, WIDE), (3, 2, K, DV, WIDE), (1, 2, K, DV, WIDE),        # heads % kv_heads != 0
    (H, HKV, K, DV, dict(ldk=GK - 1)), (H, HKV, K, DV, dict(ldv=GV - 1)),                      # K / V below their kv_heads width
    (H, HKV, K, DV, dict(ldk=K)), (H, HKV, K, DV, dict(ldv=DV)),                               # one head's width
    (H, H, K, DV, {}),                                                                         # kv_heads = heads: K and V have to be that wide
])
def test_bad_sizes_are_argument_errors_before_the_gate(lib, failed_handle, heads, kv, k, dv, ld):
    """a bad heads, kv_heads, k, dv or ld is E_ARG even on a handle that would answer E_NOSTATE: the sizes are checked first"""
    a, bits = buffers()
    f_ld = {key: v for key, v in ld.items() if key in ("ldq", "ldk", "ldv", "ldb", "ldo")}
    b_ld = {key: v for key, v in ld.items() if key != "ldo"}
    for call, kw in ((fwd, f_ld), (bwd, b_ld)):
        assert call(lib, failed_handle, heads, kv, k, dv, a, **kw) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    for call, kw in ((fwd_timer, f_ld), (bwd_timer, b_ld)):
        assert call(lib, failed_handle, heads, kv, k, dv, a, **kw) < 0
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    assert unchanged(a, bits)


def test_kv_width_beyond_int_is_an_argument_error(lib, failed_handle):
    """kv_heads * k is never larger than heads * k, so the bias calls' check covers it; it is refused as an argument error either way"""
    a, bits = buffers()
    for heads, kv, k, dv in ((BIG, BIG, 4, 1), (2 * 32768, 32768, 65536, 1), (2 * 32768, 32768, 1, 65536)):
        assert fwd(lib, failed_handle, heads, kv, k, dv, a, **{key: v for key, v in WIDE.items() if key in ("ldq", "ldk", "ldv", "ldo")}) == E_ARG
        lib.spmv_hip_clear_error()
        assert bwd(lib, failed_handle, heads, kv, k, dv, a, **{key: v for key, v in WIDE.items() if key != "ldo"}) == E_ARG
        lib.spmv_hip_clear_error()
    assert unchanged(a, bits)


@pytest.mark.parametrize("ld", [dict(lddq=WK - 1), dict(lddk=GK - 1), dict(lddv=GV - 1), dict(lddk=K), dict(lddv=DV), dict(lddb=-1)])
def test_bad_output_strides_are_argument_errors_before_the_gate(lib, failed_handle, ld):
    a, bits = buffers()
    assert bwd(lib, failed_handle, H, HKV, K, DV, a, **ld) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert bwd_timer(lib, failed_handle, H, HKV, K, DV, a, **ld) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    # of wanted outputs only: without dK and dV their strides are not looked at
    b = list(a)
    b[7] = b[8] = None
    assert bwd(lib, failed_handle, H, HKV, K, DV, b, lddk=0, lddv=0) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(a, bits)


def test_null_operand_is_an_argument_error(lib, failed_handle):
    a, bits = buffers()
    for missing in (0, 1, 2, 5):   # Q, K, V, O
        b = list(a)
        b[missing] = None
        assert fwd(lib, failed_handle, H, HKV, K, DV, b) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    for missing in (0, 1, 2, 4):   # Q, K, V, G
        b = list(a)
        b[missing] = None
        assert bwd(lib, failed_handle, H, HKV, K, DV, b) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    b = list(a)
    b[3] = None                    # no bias is no error: the call gets as far as the handle's state
    assert fwd(lib, failed_handle, H, HKV, K, DV, b, ldb=12345) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert bwd(lib, failed_handle, H, HKV, K, DV, b, ldb=12345) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(a, bits)
