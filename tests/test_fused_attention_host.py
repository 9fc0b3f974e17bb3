"""CPU: the fused attention's entry points (spmv_hip_attention, spmv_hip_time_attention_launches) are exported and bound with the declared
signatures, the Python layers exist, and the argument and handle rules hold without any device (include/spmv_hip.h: SPMV_HIP_E_ARG for a NULL
handle and for a bad k, dv or leading dimension -- before the handle's state is looked at --, E_NOSTATE for a handle without device state;
every buffer keeps its bits)."""

import ctypes as C

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
_V, _LL = C.c_void_p, C.c_longlong
SIGNATURES = {
    "spmv_hip_attention": (C.c_int, [api.spmv_Handle_t, C.c_int, _V, _V, _V, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL]),
    "spmv_hip_time_attention_launches": (C.c_double, [api.spmv_Handle_t, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL, C.c_int, C.c_int,
                                                      C.POINTER(C.c_float)]),
}
K, DV = 3, 2


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
    Q = np.arange(4 * K, dtype=np.float64).reshape(4, K) - 2
    Kk = np.arange(4 * K, dtype=np.float64).reshape(4, K) * 0.5
    Vv = np.arange(4 * DV, dtype=np.float64).reshape(4, DV) + 1
    O = np.full((4, DV), -1.0)
    return Q, Kk, Vv, O, tuple(a.tobytes() for a in (Q, Kk, Vv, O))


def unchanged(Q, Kk, Vv, O, bits):
    return tuple(a.tobytes() for a in (Q, Kk, Vv, O)) == bits


def raw(lib, h, k, dv, Q, ldq, Kk, ldk, Vv, ldv, O, ldo):
    return lib.spmv_hip_attention(h, 4, None, None, None, k, dv, 1.0, Q.ctypes.data, ldq, Kk.ctypes.data, ldk, Vv.ctypes.data, ldv, O.ctypes.data, ldo)


def test_exported_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.attention, api.time_attention_launches, api.Handle.attention):
        assert callable(f)


def test_autograd_layer_exists():
    from spmv_amd import autograd
    assert callable(autograd.attention)
    doc = autograd.attention.__doc__
    assert "three" in doc and "update_values" in doc   # the cost of a backward pass is stated


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    Q, Kk, Vv, O, bits = buffers()
    lib.spmv_hip_clear_error()
    assert raw(lib, None, K, DV, Q, K, Kk, K, Vv, DV, O, DV) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_time_attention_launches(None, K, DV, 1.0, Q.ctypes.data, K, Kk.ctypes.data, K, Vv.ctypes.data, DV, O.ctypes.data, DV, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(Q, Kk, Vv, O, bits)


def test_failed_handle_has_no_state(lib, failed_handle):
    Q, Kk, Vv, O, bits = buffers()
    assert api.attention(failed_handle, 4, None, None, None, Q, Kk, Vv, O, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.attention(failed_handle, 4, None, None, None, Q, Kk, Vv, O, scale=0.5)
    assert lib.spmv_hip_time_attention_launches(failed_handle, K, DV, 1.0, Q.ctypes.data, K, Kk.ctypes.data, K, Vv.ctypes.data, DV, O.ctypes.data, DV, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(Q, Kk, Vv, O, bits)


@pytest.mark.parametrize("k,dv,ldq,ldk,ldv,ldo", [(0, DV, K, K, DV, DV), (-1, DV, K, K, DV, DV), (K, 0, K, K, DV, DV), (K, -2, K, K, DV, DV),
                                                  (K, DV, K - 1, K, DV, DV), (K, DV, K, K - 1, DV, DV), (K, DV, K, K, DV - 1, DV), (K, DV, K, K, DV, DV - 1)])
def test_bad_sizes_are_argument_errors_before_the_gate(lib, failed_handle, k, dv, ldq, ldk, ldv, ldo):
    """a bad k, dv or ld is E_ARG even on a handle that would answer E_NOSTATE: the sizes are checked first"""
    Q, Kk, Vv, O, bits = buffers()
    assert raw(lib, failed_handle, k, dv, Q, ldq, Kk, ldk, Vv, ldv, O, ldo) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_time_attention_launches(failed_handle, k, dv, 1.0, Q.ctypes.data, ldq, Kk.ctypes.data, ldk, Vv.ctypes.data, ldv, O.ctypes.data, ldo, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(Q, Kk, Vv, O, bits)


def test_null_operand_is_an_argument_error(lib, failed_handle):
    Q, Kk, Vv, O, bits = buffers()
    ptrs = [Q.ctypes.data, Kk.ctypes.data, Vv.ctypes.data, O.ctypes.data]
    for missing in range(4):
        p = [None if i == missing else a for i, a in enumerate(ptrs)]
        assert lib.spmv_hip_attention(failed_handle, 4, None, None, None, K, DV, 1.0, p[0], K, p[1], K, p[2], DV, p[3], DV) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    assert unchanged(Q, Kk, Vv, O, bits)
