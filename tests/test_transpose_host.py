"""CPU: the transpose entry points (spmv_hip_spmv_transpose, _prepare_transpose, _get_transpose_info, _time_transpose_launches,
_transpose_map) are exported and bound, and their handle rules hold on a NULL or a failed handle without any device (include/spmv_hip.h:
SPMV_HIP_E_ARG for a NULL handle, E_NOSTATE for a handle without device state; Y untouched)."""

import ctypes as C

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
NAMES = ("spmv_hip_spmv_transpose", "spmv_hip_prepare_transpose", "spmv_hip_get_transpose_info", "spmv_hip_time_transpose_launches",
         "spmv_hip_transpose_map")


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


def test_exported_and_bound(lib):
    for name in NAMES:
        assert name in api.FUNCTIONS
        f = getattr(lib, name)
        assert f.restype is api.FUNCTIONS[name][0] and f.argtypes == api.FUNCTIONS[name][1]


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    x, y = np.ones(3), np.full(4, -1.0)
    rp, perm = np.full(5, -9, np.int32), np.full(8, -9, np.int32)
    info = api.spmv_hip_info()
    calls = (lambda: lib.spmv_hip_spmv_transpose(None, 3, None, None, None, x.ctypes.data, y.ctypes.data),
             lambda: lib.spmv_hip_prepare_transpose(None),
             lambda: lib.spmv_hip_get_transpose_info(None, C.byref(info)),
             lambda: lib.spmv_hip_transpose_map(None, rp.ctypes.data_as(api._I), perm.ctypes.data_as(api._I)))
    for call in calls:
        lib.spmv_hip_clear_error()
        assert call() == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
    assert (y == -1.0).all() and (rp == -9).all() and (perm == -9).all()
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_time_transpose_launches(None, x.ctypes.data, y.ctypes.data, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()


def test_failed_handle_has_no_state(lib, failed_handle):
    x, y = np.ones(3), np.full(4, -1.0)
    assert api.spmv_transpose(failed_handle, 3, None, None, None, x, y, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE and (y == -1.0).all()
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.spmv_transpose(failed_handle, 3, None, None, None, x, y)
    assert api.prepare_transpose(failed_handle, check=False) == E_NOSTATE
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.get_transpose_info(failed_handle)
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.transpose_map(failed_handle, 4, 8)
    assert lib.spmv_hip_time_transpose_launches(failed_handle, x.ctypes.data, y.ctypes.data, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
