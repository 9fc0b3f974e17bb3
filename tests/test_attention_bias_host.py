"""CPU: the biased attention's entry points (spmv_hip_attention_bias, spmv_hip_attention_bias_backward and their two timers) are exported and
bound with the declared signatures, the Python layers exist -- bias= is accepted by both autograd functions --, and the argument and handle
rules hold without any device (include/spmv_hip.h: SPMV_HIP_E_ARG for the heads calls' bad arguments and for ldb < 0 / lddb < 0, before the
handle's state is looked at; E_NOSTATE for a handle without device state; every buffer keeps its bits)."""

import ctypes as C
import inspect

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
_V, _LL = C.c_void_p, C.c_longlong
_H = api.spmv_Handle_t
SIGNATURES = {
    "spmv_hip_attention_bias": (C.c_int, [_H, C.c_int, _V, _V, _V, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL]),
    "spmv_hip_time_attention_bias_launches": (C.c_double, [_H, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                                           C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "spmv_hip_attention_bias_backward": (C.c_int, [_H, C.c_int, _V, _V, _V, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                                   _V, _LL, _V, _LL, _V, _LL, _V, _LL]),
    "spmv_hip_time_attention_bias_backward_launches": (C.c_double, [_H, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                                                    _V, _LL, _V, _LL, _V, _LL, _V, _LL, C.c_int, C.c_int, C.POINTER(C.c_float)]),
}
H, K, DV, NNZ = 2, 3, 2, 5
WK, WV = H * K, H * DV


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
    Kk = np.arange(4 * WK, dtype=np.float64).reshape(4, WK) * 0.5
    Vv = np.arange(4 * WV, dtype=np.float64).reshape(4, WV) + 1
    B = np.arange(H * NNZ, dtype=np.float64).reshape(H, NNZ) * 0.25
    G = np.arange(4 * WV, dtype=np.float64).reshape(4, WV) - 3
    outs = [np.full((4, WV), -1.0), np.full((4, WK), -2.0), np.full((4, WK), -3.0), np.full((4, WV), -4.0), np.full((H, NNZ), -5.0)]
    arrays = [Q, Kk, Vv, B, G, *outs]
    return arrays, tuple(a.tobytes() for a in arrays)


def unchanged(arrays, bits):
    return tuple(a.tobytes() for a in arrays) == bits


def p(a):
    return None if a is None else a.ctypes.data


def fwd(lib, h, heads, k, dv, a, ldq=WK, ldk=WK, ldv=WV, ldb=NNZ, ldo=WV):
    Q, Kk, Vv, B, G, O = a[:6]
    return lib.spmv_hip_attention_bias(h, 4, None, None, None, heads, k, dv, 1.0, p(Q), ldq, p(Kk), ldk, p(Vv), ldv, p(B), ldb, p(O), ldo)


def fwd_timer(lib, h, heads, k, dv, a, ldq=WK, ldk=WK, ldv=WV, ldb=NNZ, ldo=WV):
    Q, Kk, Vv, B, G, O = a[:6]
    return lib.spmv_hip_time_attention_bias_launches(h, heads, k, dv, 1.0, p(Q), ldq, p(Kk), ldk, p(Vv), ldv, p(B), ldb, p(O), ldo, 1, 1, None)


def bwd(lib, h, heads, k, dv, a, ldq=WK, ldk=WK, ldv=WV, ldb=NNZ, ldg=WV, lddq=WK, lddk=WK, lddv=WV, lddb=NNZ):
    Q, Kk, Vv, B, G, O, dQ, dK, dV, dB = a
    return lib.spmv_hip_attention_bias_backward(h, 4, None, None, None, heads, k, dv, 1.0, p(Q), ldq, p(Kk), ldk, p(Vv), ldv, p(B), ldb, p(G), ldg,
                                                p(dQ), lddq, p(dK), lddk, p(dV), lddv, p(dB), lddb)


def bwd_timer(lib, h, heads, k, dv, a, ldq=WK, ldk=WK, ldv=WV, ldb=NNZ, ldg=WV, lddq=WK, lddk=WK, lddv=WV, lddb=NNZ):
    Q, Kk, Vv, B, G, O, dQ, dK, dV, dB = a
    return lib.spmv_hip_time_attention_bias_backward_launches(h, heads, k, dv, 1.0, p(Q), ldq, p(Kk), ldk, p(Vv), ldv, p(B), ldb, p(G), ldg,
                                                              p(dQ), lddq, p(dK), lddk, p(dV), lddv, p(dB), lddb, 1, 1, None)


def test_exported_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.attention_bias, api.attention_bias_backward, api.time_attention_bias_launches, api.time_attention_bias_backward_launches,
              api.Handle.attention_bias, api.Handle.attention_bias_backward):
        assert callable(f)
    assert list(inspect.signature(api.Handle.attention_bias).parameters)[1:7] == ["Q", "K", "V", "heads", "bias", "scale"]
    sig = inspect.signature(api.Handle.attention_bias_backward)
    assert list(sig.parameters)[1:9] == ["Q", "K", "V", "bias", "G", "heads", "scale", "need"]
    assert sig.parameters["need"].default == (True, True, True, True)


def test_autograd_layer_accepts_a_bias():
    from spmv_amd import autograd
    for f in (autograd.attention, autograd.attention_heads):
        par = inspect.signature(f).parameters["bias"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY   # trailing keyword: existing calls are untouched
        assert "bias" in f.__doc__ and "gradient" in f.__doc__
    assert "order is not part of the contract" in autograd.attention_heads.__doc__   # the shared plane's sum is torch's


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    a, bits = buffers()
    for call in (fwd, bwd):
        lib.spmv_hip_clear_error()
        assert call(lib, None, H, K, DV, a) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
    for call in (fwd_timer, bwd_timer):
        lib.spmv_hip_clear_error()
        assert call(lib, None, H, K, DV, a) < 0
        assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(a, bits)


def test_failed_handle_has_no_state(lib, failed_handle):
    a, bits = buffers()
    Q, Kk, Vv, B, G, O, dQ, dK, dV, dB = a
    for call in (fwd, bwd):
        assert call(lib, failed_handle, H, K, DV, a) == E_NOSTATE
        assert lib.spmv_hip_last_error() == E_NOSTATE
        lib.spmv_hip_clear_error()
    for call in (fwd_timer, bwd_timer):
        assert call(lib, failed_handle, H, K, DV, a) < 0
        assert lib.spmv_hip_last_error() == E_NOSTATE
        lib.spmv_hip_clear_error()
    # the Python layer: per-head planes, a shared plane, no bias
    for bias in (B, B[0], None):
        assert api.attention_bias(failed_handle, 4, None, None, None, H, Q, Kk, Vv, bias, O, check=False) == E_NOSTATE
        lib.spmv_hip_clear_error()
        assert api.attention_bias_backward(failed_handle, 4, None, None, None, H, Q, Kk, Vv, bias, G, dQ, dK, dV, dB, check=False) == E_NOSTATE
        lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.attention_bias(failed_handle, 4, None, None, None, H, Q, Kk, Vv, B, O, scale=0.5)
    with pytest.raises(ValueError):   # three planes for two heads
        api.attention_bias(failed_handle, 4, None, None, None, H, Q, Kk, Vv, np.zeros((3, NNZ)), O)
    with pytest.raises(ValueError):   # dB always has a plane per head
        api.attention_bias_backward(failed_handle, 4, None, None, None, H, Q, Kk, Vv, B, G, dB=np.zeros(NNZ))
    assert unchanged(a, bits)


def test_all_outputs_null_returns_after_argument_checking(lib, failed_handle):
    """nothing wanted: 0 without looking at the handle's state -- but the arguments are checked first"""
    a, bits = buffers()
    none = a[:6] + [None] * 4
    assert bwd(lib, failed_handle, H, K, DV, none) == 0
    assert lib.spmv_hip_last_error() == 0
    assert bwd(lib, failed_handle, H, K, DV, none, ldb=-1) == E_ARG
    lib.spmv_hip_clear_error()
    assert bwd(lib, failed_handle, H, K, DV, none, lddb=-1) == 0   # the stride of an output that is not wanted is not looked at
    only_db = a[:6] + [None] * 3 + [a[9]]
    assert bwd(lib, failed_handle, H, K, DV, only_db) == E_NOSTATE   # dB alone is work
    lib.spmv_hip_clear_error()
    assert unchanged(a, bits)


BIG = 2 ** 30   # BIG * K and 2 * BIG do not fit an int


@pytest.mark.parametrize("heads,k,dv,ld", [
    (0, K, DV, {}), (-1, K, DV, {}), (H, 0, DV, {}), (H, K, 0, {}), (H, K, -2, {}),
    (H, K, DV, dict(ldq=WK - 1)), (H, K, DV, dict(ldk=WK - 1)), (H, K, DV, dict(ldv=WV - 1)), (H, K, DV, dict(ldo=WV - 1, ldg=WV - 1)),
    (H, K, DV, dict(ldq=K, ldk=K, ldv=DV, ldo=DV, ldg=DV)),                                   # one head's width as ld
    (BIG, K, 1, dict(ldq=2 ** 40, ldk=2 ** 40, ldv=2 ** 40, ldo=2 ** 40, ldg=2 ** 40, lddq=2 ** 40, lddk=2 ** 40, lddv=2 ** 40)),
    (65536, 65536, 1, dict(ldq=2 ** 40, ldk=2 ** 40, ldv=2 ** 40, ldo=2 ** 40, ldg=2 ** 40, lddq=2 ** 40, lddk=2 ** 40, lddv=2 ** 40)),
    (H, K, DV, dict(ldb=-1)), (H, K, DV, dict(ldb=-NNZ)), (H, K, DV, dict(ldb=-2 ** 40)),      # the new rules: a negative plane stride
])
def test_bad_sizes_are_argument_errors_before_the_gate(lib, failed_handle, heads, k, dv, ld):
    """a bad heads, k, dv, ld or ldb is E_ARG even on a handle that would answer E_NOSTATE: the sizes are checked first"""
    a, bits = buffers()
    f_ld = {key: v for key, v in ld.items() if key in ("ldq", "ldk", "ldv", "ldb", "ldo")}
    b_ld = {key: v for key, v in ld.items() if key != "ldo"}
    for call, kw in ((fwd, f_ld), (bwd, b_ld)):
        assert call(lib, failed_handle, heads, k, dv, a, **kw) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    for call, kw in ((fwd_timer, f_ld), (bwd_timer, b_ld)):
        assert call(lib, failed_handle, heads, k, dv, a, **kw) < 0
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    assert unchanged(a, bits)


@pytest.mark.parametrize("ld", [dict(lddq=WK - 1), dict(lddk=WK - 1), dict(lddv=WV - 1), dict(lddb=-1), dict(lddb=-2 ** 40)])
def test_bad_output_strides_are_argument_errors_before_the_gate(lib, failed_handle, ld):
    a, bits = buffers()
    assert bwd(lib, failed_handle, H, K, DV, a, **ld) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert bwd_timer(lib, failed_handle, H, K, DV, a, **ld) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(a, bits)


def test_null_operand_is_an_argument_error(lib, failed_handle):
    a, bits = buffers()
    for missing in (0, 1, 2, 5):   # Q, K, V, O
        b = list(a)
        b[missing] = None
        assert fwd(lib, failed_handle, H, K, DV, b) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    for missing in (0, 1, 2, 4):   # Q, K, V, G
        b = list(a)
        b[missing] = None
        assert bwd(lib, failed_handle, H, K, DV, b) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    b = list(a)
    b[3] = None                    # no bias is no error: the call gets as far as the handle's state
    assert fwd(lib, failed_handle, H, K, DV, b, ldb=12345) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert bwd(lib, failed_handle, H, K, DV, b, ldb=12345) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(a, bits)
