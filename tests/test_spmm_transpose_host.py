"""CPU: the k-column transpose entry points (spmv_hip_spmm_transpose, _time_spmm_transpose_launches) are exported and bound, and their handle
rules hold on a NULL or a failed handle without any device (include/spmv_hip.h: SPMV_HIP_E_ARG for a NULL handle, E_NOSTATE for a handle
without device state; X and Y keep their bits)."""

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
NAMES = ("spmv_hip_spmm_transpose", "spmv_hip_time_spmm_transpose_launches")


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


def blocks():
    X = np.arange(6, dtype=np.float64).reshape(3, 2) + 1
    Y = np.full((4, 2), -1.0)
    return X, Y, X.tobytes(), Y.tobytes()


def test_exported_and_bound(lib):
    for name in NAMES:
        assert name in api.FUNCTIONS
        f = getattr(lib, name)
        assert f.restype is api.FUNCTIONS[name][0] and f.argtypes == api.FUNCTIONS[name][1]
    assert callable(api.spmm_transpose) and callable(api.time_spmm_transpose_launches) and callable(api.Handle.spmm_transpose)


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    X, Y, xb, yb = blocks()
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_spmm_transpose(None, 3, None, None, None, 2, X.ctypes.data, 2, Y.ctypes.data, 2) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_time_spmm_transpose_launches(None, 2, X.ctypes.data, 2, Y.ctypes.data, 2, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert X.tobytes() == xb and Y.tobytes() == yb


def test_failed_handle_has_no_state(lib, failed_handle):
    X, Y, xb, yb = blocks()
    assert api.spmm_transpose(failed_handle, 3, None, None, None, X, Y, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.spmm_transpose(failed_handle, 3, None, None, None, X, Y)
    assert lib.spmv_hip_time_spmm_transpose_launches(failed_handle, 2, X.ctypes.data, 2, Y.ctypes.data, 2, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert X.tobytes() == xb and Y.tobytes() == yb


def test_bad_shapes_are_argument_errors_before_the_handle_is_looked_at(lib, failed_handle):
    X, Y, xb, yb = blocks()
    for k, ldx, ldy in ((0, 2, 2), (2, 1, 2), (2, 2, 1)):
        lib.spmv_hip_clear_error()
        assert lib.spmv_hip_spmm_transpose(failed_handle, 3, None, None, None, k, X.ctypes.data, ldx, Y.ctypes.data, ldy) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert X.tobytes() == xb and Y.tobytes() == yb
