"""CPU: the sampled dense-dense product's entry points (spmv_hip_sddmm, _time_sddmm_launches) are exported and bound, and their handle rules
hold on a NULL or a failed handle without any device (include/spmv_hip.h: SPMV_HIP_E_ARG for a NULL handle, E_NOSTATE for a handle without
device state; U, V and Out keep their bits)."""

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
NAMES = ("spmv_hip_sddmm", "spmv_hip_time_sddmm_launches")


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
    U = np.arange(6, dtype=np.float64).reshape(3, 2) + 1
    V = np.arange(8, dtype=np.float64).reshape(4, 2) - 3
    out = np.full(5, -1.0)
    return U, V, out, (U.tobytes(), V.tobytes(), out.tobytes())


def unchanged(U, V, out, bits):
    return (U.tobytes(), V.tobytes(), out.tobytes()) == bits


def test_exported_and_bound(lib):
    for name in NAMES:
        assert name in api.FUNCTIONS
        f = getattr(lib, name)
        assert f.restype is api.FUNCTIONS[name][0] and f.argtypes == api.FUNCTIONS[name][1]
    assert callable(api.sddmm) and callable(api.time_sddmm_launches) and callable(api.Handle.sddmm)


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    U, V, out, bits = blocks()
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_sddmm(None, 3, None, None, None, 2, U.ctypes.data, 2, V.ctypes.data, 2, out.ctypes.data) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert lib.spmv_hip_time_sddmm_launches(None, 2, U.ctypes.data, 2, V.ctypes.data, 2, out.ctypes.data, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(U, V, out, bits)


def test_failed_handle_has_no_state(lib, failed_handle):
    U, V, out, bits = blocks()
    assert api.sddmm(failed_handle, 3, None, None, None, U, V, out, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.sddmm(failed_handle, 3, None, None, None, U, V, out)
    assert lib.spmv_hip_time_sddmm_launches(failed_handle, 2, U.ctypes.data, 2, V.ctypes.data, 2, out.ctypes.data, 1, 1, None) < 0
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(U, V, out, bits)


def test_bad_shapes_are_argument_errors_before_the_handle_is_looked_at(lib, failed_handle):
    U, V, out, bits = blocks()
    for k, ldu, ldv in ((0, 2, 2), (2, 1, 2), (2, 2, 1)):
        lib.spmv_hip_clear_error()
        assert lib.spmv_hip_sddmm(failed_handle, 3, None, None, None, k, U.ctypes.data, ldu, V.ctypes.data, ldv, out.ctypes.data) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(U, V, out, bits)


def test_autograd_module_is_the_only_torch_importer():
    """libspmv_hip.so and spmv_amd.api stay free of torch at import time; spmv_amd.autograd is where torch comes in"""
    import subprocess
    import sys
    code = "import sys; import spmv_amd.api; assert 'torch' not in sys.modules; import spmv_amd.autograd; assert 'torch' in sys.modules; assert callable(spmv_amd.autograd.matmul)"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
