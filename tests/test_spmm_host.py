"""CPU: spmv_hip_spmm and spmv_hip_time_spmm_launches are exported and bound, and their argument rules hold on a NULL or a failed
handle without any device (include/spmv_hip.h: SPMV_HIP_E_ARG for bad k / leading dimensions / NULL blocks, E_NOSTATE for a handle
without device state; Y untouched)."""

import numpy as np
import pytest

from spmv_amd import api, build, synth

E_ARG, E_NOSTATE = 3, 5


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
    for name in ("spmv_hip_spmm", "spmv_hip_time_spmm_launches"):
        assert name in api.FUNCTIONS
        f = getattr(lib, name)
        assert f.restype is api.FUNCTIONS[name][0] and f.argtypes == api.FUNCTIONS[name][1]


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    X, Y = np.ones((4, 2)), np.full((3, 2), -1.0)
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_spmm(None, 3, None, None, None, 2, X.ctypes.data, 2, Y.ctypes.data, 2) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG and (Y == -1.0).all()
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_time_spmm_launches(None, 2, X.ctypes.data, 2, Y.ctypes.data, 2, 1, 1, None) < 0
    lib.spmv_hip_clear_error()


@pytest.mark.parametrize("k,ldx,ldy,nullx,nully", [(0, 2, 2, 0, 0), (-1, 2, 2, 0, 0), (2, 1, 2, 0, 0), (2, 2, 1, 0, 0),
                                                   (2, 2, 2, 1, 0), (2, 2, 2, 0, 1)])
def test_argument_errors_on_a_failed_handle(lib, failed_handle, k, ldx, ldy, nullx, nully):
    X, Y = np.ones((4, 3)), np.full((3, 3), -1.0)
    rc = lib.spmv_hip_spmm(failed_handle, 3, None, None, None, k, None if nullx else X.ctypes.data, ldx, None if nully else Y.ctypes.data, ldy)
    assert rc == E_ARG and lib.spmv_hip_last_error() == E_ARG
    assert (Y == -1.0).all()
    lib.spmv_hip_clear_error()


def test_failed_handle_has_no_state(lib, failed_handle):
    X, Y = np.ones((4, 2)), np.full((3, 2), -1.0)
    assert api.spmm(failed_handle, 3, None, None, None, X, Y, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE and (Y == -1.0).all()
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.spmm(failed_handle, 3, None, None, None, X, Y)


def test_python_wrapper_passes_row_strides_as_leading_dimensions(lib, failed_handle):
    """api.spmm: the row stride of a 2-D block with column stride 1 is its leading dimension; other layouts are refused"""
    assert api._block(np.zeros((5, 7))[:, 2:5], "X")[1:] == (5, 3, 7)
    assert api._block(np.zeros((5, 1)), "X")[1:] == (5, 1, 1)
    with pytest.raises(ValueError):
        api._block(np.zeros((5, 7)).T, "X")
    with pytest.raises(ValueError):
        api._block(np.zeros(5), "X")
    with pytest.raises(ValueError):
        api.spmm(failed_handle, 3, None, None, None, np.zeros((4, 2)), np.zeros((3, 3)))
