"""CPU: the fused attention backward's entry points (spmv_hip_attention_backward, spmv_hip_time_attention_backward_launches) are exported and
bound with the declared signatures, the Python layers exist, and the argument and handle rules hold without any device (include/spmv_hip.h:
SPMV_HIP_E_ARG for a NULL handle and for a bad k, dv or leading dimension -- before the handle's state is looked at, and for the requested
outputs only --, E_NOSTATE for a handle without device state; every buffer keeps its bits)."""

import ctypes as C
import inspect

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
_V, _LL = C.c_void_p, C.c_longlong
SIGNATURES = {
    "spmv_hip_attention_backward": (C.c_int, [api.spmv_Handle_t, C.c_int, _V, _V, _V, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                              _V, _LL, _V, _LL, _V, _LL]),
    "spmv_hip_time_attention_backward_launches": (C.c_double, [api.spmv_Handle_t, C.c_int, C.c_int, C.c_double, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                                               _V, _LL, _V, _LL, _V, _LL, C.c_int, C.c_int, C.POINTER(C.c_float)]),
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
    """Q, K, V, G, dQ, dK, dV and their bits"""
    Q = np.arange(4 * K, dtype=np.float64).reshape(4, K) - 2
    Kk = np.arange(4 * K, dtype=np.float64).reshape(4, K) * 0.5
    Vv = np.arange(4 * DV, dtype=np.float64).reshape(4, DV) + 1
    G = np.arange(4 * DV, dtype=np.float64).reshape(4, DV) - 3
    bufs = [Q, Kk, Vv, G, np.full((4, K), -1.0), np.full((4, K), -2.0), np.full((4, DV), -3.0)]
    return bufs, tuple(a.tobytes() for a in bufs)


def unchanged(bufs, bits):
    return tuple(a.tobytes() for a in bufs) == bits


def lds(k=K, dv=DV):
    return [k, k, dv, dv, k, k, dv]


def pairs(bufs, ld, null=()):
    out = []
    for i, (a, l) in enumerate(zip(bufs, ld)):
        out += [None if i in null else a.ctypes.data, l]
    return out


def raw(lib, h, k, dv, bufs, ld, null=()):
    return lib.spmv_hip_attention_backward(h, 4, None, None, None, k, dv, 1.0, *pairs(bufs, ld, null))


def raw_timer(lib, h, k, dv, bufs, ld, null=()):
    return lib.spmv_hip_time_attention_backward_launches(h, k, dv, 1.0, *pairs(bufs, ld, null), 1, 1, None)


def test_exported_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.attention_backward, api.time_attention_backward_launches, api.Handle.attention_backward):
        assert callable(f)
    assert inspect.signature(api.Handle.attention_backward).parameters["need"].default == (True, True, True)


def test_autograd_layer_has_the_backward_keyword():
    from spmv_amd import autograd
    p = inspect.signature(autograd.attention).parameters["backward"]
    assert p.default == "composed"
    assert "fused" in autograd.attention.__doc__ and "attention_backward" in autograd.attention.__doc__
    with pytest.raises(ValueError, match="backward"):
        autograd.attention(None, None, None, None, backward="both")   # refused before anything else is looked at


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    bufs, bits = buffers()
    lib.spmv_hip_clear_error()
    assert raw(lib, None, K, DV, bufs, lds()) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert raw_timer(lib, None, K, DV, bufs, lds()) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(bufs, bits)


def test_failed_handle_has_no_state(lib, failed_handle):
    bufs, bits = buffers()
    Q, Kk, Vv, G, dQ, dK, dV = bufs
    assert api.attention_backward(failed_handle, 4, None, None, None, Q, Kk, Vv, G, dQ, dK, dV, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.attention_backward(failed_handle, 4, None, None, None, Q, Kk, Vv, G, dQ, None, None, scale=0.5)
    assert raw(lib, failed_handle, K, DV, bufs, lds(), null=(4, 5, 6)) == E_NOSTATE   # no output wanted: still behind the gate
    assert raw_timer(lib, failed_handle, K, DV, bufs, lds()) < 0
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(bufs, bits)


BAD = [(0, DV, None), (-1, DV, None), (K, 0, None), (K, -2, None)] + [(K, DV, i) for i in range(7)]


@pytest.mark.parametrize("k,dv,short", BAD)
def test_bad_sizes_are_argument_errors_before_the_gate(lib, failed_handle, k, dv, short):
    """a bad k, dv or ld is E_ARG even on a handle that would answer E_NOSTATE: the sizes are checked first"""
    bufs, bits = buffers()
    ld = lds()
    if short is not None:
        ld[short] -= 1
    assert raw(lib, failed_handle, k, dv, bufs, ld) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert raw_timer(lib, failed_handle, k, dv, bufs, ld) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(bufs, bits)


@pytest.mark.parametrize("out", [4, 5, 6])
def test_the_ld_of_an_output_that_is_not_wanted_is_not_checked(lib, failed_handle, out):
    bufs, bits = buffers()
    ld = lds()
    ld[out] = 0
    assert raw(lib, failed_handle, K, DV, bufs, ld, null=(out,)) == E_NOSTATE   # past the argument check
    lib.spmv_hip_clear_error()
    assert unchanged(bufs, bits)


def test_null_operand_is_an_argument_error(lib, failed_handle):
    bufs, bits = buffers()
    for missing in range(4):
        assert raw(lib, failed_handle, K, DV, bufs, lds(), null=(missing,)) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    assert unchanged(bufs, bits)
