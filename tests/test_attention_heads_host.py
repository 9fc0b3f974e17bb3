"""CPU: the multi-head attention's entry points (spmv_hip_attention_heads, spmv_hip_time_attention_heads_launches) are exported and bound with
the declared signatures, the Python layers exist, and the argument and handle rules hold without any device (include/spmv_hip.h:
SPMV_HIP_E_ARG for a NULL handle and for a bad heads, k, dv or leading dimension, or a width heads * k that does not fit an int -- before the
handle's state is looked at --, E_NOSTATE for a handle without device state; every buffer keeps its bits)."""

import ctypes as C

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
_V, _LL = C.c_void_p, C.c_longlong
SIGNATURES = {
    "spmv_hip_attention_heads": (C.c_int, [api.spmv_Handle_t, C.c_int, _V, _V, _V, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL]),
    "spmv_hip_time_attention_heads_launches": (C.c_double, [api.spmv_Handle_t, C.c_int, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                                            C.c_int, C.c_int, C.POINTER(C.c_float)]),
}
H, K, DV = 2, 3, 2
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
    Q = np.arange(4 * WK, dtype=np.float64).reshape(4, WK) - 2
    Kk = np.arange(4 * WK, dtype=np.float64).reshape(4, WK) * 0.5
    Vv = np.arange(4 * WV, dtype=np.float64).reshape(4, WV) + 1
    O = np.full((4, WV), -1.0)
    return Q, Kk, Vv, O, tuple(a.tobytes() for a in (Q, Kk, Vv, O))


def unchanged(Q, Kk, Vv, O, bits):
    return tuple(a.tobytes() for a in (Q, Kk, Vv, O)) == bits


def raw(lib, h, heads, k, dv, Q, ldq, Kk, ldk, Vv, ldv, O, ldo):
    return lib.spmv_hip_attention_heads(h, 4, None, None, None, heads, k, dv, 1.0, Q.ctypes.data, ldq, Kk.ctypes.data, ldk, Vv.ctypes.data, ldv, O.ctypes.data, ldo)


def timer(lib, h, heads, k, dv, Q, ldq, Kk, ldk, Vv, ldv, O, ldo):
    return lib.spmv_hip_time_attention_heads_launches(h, heads, k, dv, 1.0, Q.ctypes.data, ldq, Kk.ctypes.data, ldk, Vv.ctypes.data, ldv, O.ctypes.data, ldo, 1, 1, None)


def test_exported_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.attention_heads, api.time_attention_heads_launches, api.Handle.attention_heads):
        assert callable(f)


def test_autograd_layer_exists():
    from spmv_amd import autograd
    assert callable(autograd.attention_heads)
    doc = autograd.attention_heads.__doc__
    assert "once per head" in doc and "update_values" in doc   # what a backward pass costs is stated


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    Q, Kk, Vv, O, bits = buffers()
    lib.spmv_hip_clear_error()
    assert raw(lib, None, H, K, DV, Q, WK, Kk, WK, Vv, WV, O, WV) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert timer(lib, None, H, K, DV, Q, WK, Kk, WK, Vv, WV, O, WV) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(Q, Kk, Vv, O, bits)


def test_failed_handle_has_no_state(lib, failed_handle):
    Q, Kk, Vv, O, bits = buffers()
    assert api.attention_heads(failed_handle, 4, None, None, None, H, Q, Kk, Vv, O, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.attention_heads(failed_handle, 4, None, None, None, H, Q, Kk, Vv, O, scale=0.5)
    assert timer(lib, failed_handle, H, K, DV, Q, WK, Kk, WK, Vv, WV, O, WV) < 0
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(Q, Kk, Vv, O, bits)


BIG = 2 ** 30   # BIG * K and 2 * BIG do not fit an int


@pytest.mark.parametrize("heads,k,dv,ldq,ldk,ldv,ldo", [
    (0, K, DV, WK, WK, WV, WV), (-1, K, DV, WK, WK, WV, WV), (H, 0, DV, WK, WK, WV, WV), (H, K, 0, WK, WK, WV, WV), (H, K, -2, WK, WK, WV, WV),
    (H, K, DV, WK - 1, WK, WV, WV), (H, K, DV, WK, WK - 1, WV, WV), (H, K, DV, WK, WK, WV - 1, WV), (H, K, DV, WK, WK, WV, WV - 1),
    (H, K, DV, K, K, DV, DV),                                     # one head's width as ld: below heads * k
    (BIG, K, 1, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40),              # heads * k overflows int, heads * dv does not
    (BIG, 1, 2, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40),              # heads * dv = 2^31
    (2, BIG, 1, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40),
    (65536, 65536, 1, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40),        # the product wraps to 0 in 32 bits
])
def test_bad_sizes_are_argument_errors_before_the_gate(lib, failed_handle, heads, k, dv, ldq, ldk, ldv, ldo):
    """a bad heads, k, dv or ld is E_ARG even on a handle that would answer E_NOSTATE: the sizes are checked first"""
    Q, Kk, Vv, O, bits = buffers()
    assert raw(lib, failed_handle, heads, k, dv, Q, ldq, Kk, ldk, Vv, ldv, O, ldo) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert timer(lib, failed_handle, heads, k, dv, Q, ldq, Kk, ldk, Vv, ldv, O, ldo) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(Q, Kk, Vv, O, bits)


def test_null_operand_is_an_argument_error(lib, failed_handle):
    Q, Kk, Vv, O, bits = buffers()
    ptrs = [Q.ctypes.data, Kk.ctypes.data, Vv.ctypes.data, O.ctypes.data]
    for missing in range(4):
        p = [None if i == missing else a for i, a in enumerate(ptrs)]
        assert lib.spmv_hip_attention_heads(failed_handle, 4, None, None, None, H, K, DV, 1.0, p[0], WK, p[1], WK, p[2], WV, p[3], WV) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    assert unchanged(Q, Kk, Vv, O, bits)


@pytest.mark.parametrize("heads", [0, -1, 4, 5])
def test_widths_must_divide_into_heads(lib, failed_handle, heads):
    """6 columns of Q / K and 4 of V / O: 4 heads divide only V's, 5 neither; no call reaches the library"""
    Q, Kk, Vv, O, bits = buffers()
    with pytest.raises(ValueError):
        api.attention_heads(failed_handle, 4, None, None, None, heads, Q, Kk, Vv, O)
    with pytest.raises(ValueError):
        api.time_attention_heads_launches(failed_handle, heads, Q, Kk, Vv, O, warmup=0, iters=1)
    assert lib.spmv_hip_last_error() == 0
    assert unchanged(Q, Kk, Vv, O, bits)


def test_one_head_takes_the_whole_width(lib, failed_handle):
    """heads = 1 passes k and dv as the full widths: the call gets as far as the handle's state"""
    Q, Kk, Vv, O, bits = buffers()
    assert api.attention_heads(failed_handle, 4, None, None, None, 1, Q, Kk, Vv, O, check=False) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(Q, Kk, Vv, O, bits)
