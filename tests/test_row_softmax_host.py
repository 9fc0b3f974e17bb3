"""CPU: the row softmax's entry points (spmv_hip_row_softmax, _row_softmax_backward, _time_row_softmax_launches) are exported and bound with
the declared signatures, the Python layers exist, and the handle rules hold on a NULL or a failed handle without any device
(include/spmv_hip.h: SPMV_HIP_E_ARG for a NULL handle, E_NOSTATE for a handle without device state; every buffer keeps its bits)."""

import ctypes as C

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
_V = C.c_void_p
SIGNATURES = {
    "spmv_hip_row_softmax": (C.c_int, [api.spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V]),
    "spmv_hip_row_softmax_backward": (C.c_int, [api.spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V, _V]),
    "spmv_hip_time_row_softmax_launches": (C.c_double, [api.spmv_Handle_t, _V, _V, C.c_int, C.c_int, C.POINTER(C.c_float)]),
}


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
    S = np.arange(5, dtype=np.float64) - 2
    G = np.arange(5, dtype=np.float64) * 0.5
    out = np.full(5, -1.0)
    return S, G, out, (S.tobytes(), G.tobytes(), out.tobytes())


def unchanged(S, G, out, bits):
    return (S.tobytes(), G.tobytes(), out.tobytes()) == bits


def test_exported_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.row_softmax, api.row_softmax_backward, api.time_row_softmax_launches, api.Handle.row_softmax, api.Handle.row_softmax_backward):
        assert callable(f)


def test_autograd_layer_exists():
    from spmv_amd import autograd
    assert callable(autograd.row_softmax) and callable(autograd.sddmm) and callable(autograd.matmul)
    assert "two" in autograd.sddmm.__doc__ and "update_values" in autograd.sddmm.__doc__   # the cost of a backward pass is stated


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    S, G, out, bits = buffers()
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_row_softmax(None, 3, None, None, None, S.ctypes.data, out.ctypes.data) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_row_softmax_backward(None, 3, None, None, None, S.ctypes.data, G.ctypes.data, out.ctypes.data) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_time_row_softmax_launches(None, S.ctypes.data, out.ctypes.data, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(S, G, out, bits)


def test_failed_handle_has_no_state(lib, failed_handle):
    S, G, out, bits = buffers()
    assert api.row_softmax(failed_handle, 3, None, None, None, S, out, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert api.row_softmax_backward(failed_handle, 3, None, None, None, S, G, out, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.row_softmax(failed_handle, 3, None, None, None, S, out)
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.row_softmax_backward(failed_handle, 3, None, None, None, S, G, out)
    assert lib.spmv_hip_time_row_softmax_launches(failed_handle, S.ctypes.data, out.ctypes.data, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(S, G, out, bits)
