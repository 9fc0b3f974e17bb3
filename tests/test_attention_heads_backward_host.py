"""CPU: the multi-head attention backward's entry points (spmv_hip_attention_heads_backward, spmv_hip_time_attention_heads_backward_launches) are
exported and bound with the declared signatures, the Python layers exist, option "attention_backward_heads" has its default and range, and the
argument and handle rules hold without any device (include/spmv_hip.h: SPMV_HIP_E_ARG for a NULL handle and for a bad heads, k, dv or leading
dimension, or a width heads * k that does not fit an int -- before the handle's state is looked at --, E_NOSTATE for a handle without device
state, 0 when no output is wanted; every buffer keeps its bits)."""

import ctypes as C
import inspect

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
_V, _LL = C.c_void_p, C.c_longlong
SIGNATURES = {
    "spmv_hip_attention_heads_backward": (C.c_int, [api.spmv_Handle_t, C.c_int, _V, _V, _V, C.c_int, C.c_int, C.c_int, C.c_double,
                                                    _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL]),
    "spmv_hip_time_attention_heads_backward_launches": (C.c_double, [api.spmv_Handle_t, C.c_int, C.c_int, C.c_int, C.c_double,
                                                                     _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL, _V, _LL,
                                                                     C.c_int, C.c_int, C.POINTER(C.c_float)]),
}
H, K, DV = 2, 3, 2
WK, WV = H * K, H * DV
GOOD_LD = [WK, WK, WV, WV, WK, WK, WV]
OPTION = b"attention_backward_heads"


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
    """Q, K, V, G and the three outputs, 4 rows each; -> (arrays, their bits)"""
    arrays = [np.arange(4 * WK, dtype=np.float64).reshape(4, WK) - 2, np.arange(4 * WK, dtype=np.float64).reshape(4, WK) * 0.5,
              np.arange(4 * WV, dtype=np.float64).reshape(4, WV) + 1, np.arange(4 * WV, dtype=np.float64).reshape(4, WV) - 3,
              np.full((4, WK), -1.0), np.full((4, WK), -2.0), np.full((4, WV), -3.0)]
    return arrays, tuple(a.tobytes() for a in arrays)


def unchanged(arrays, bits):
    return tuple(a.tobytes() for a in arrays) == bits


def interleave(ptrs, ld):
    return [v for pair in zip(ptrs, ld) for v in pair]


def raw(lib, h, heads, k, dv, ptrs, ld):
    return lib.spmv_hip_attention_heads_backward(h, 4, None, None, None, heads, k, dv, 1.0, *interleave(ptrs, ld))


def timer(lib, h, heads, k, dv, ptrs, ld):
    return lib.spmv_hip_time_attention_heads_backward_launches(h, heads, k, dv, 1.0, *interleave(ptrs, ld), 1, 1, None)


def test_exported_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.attention_heads_backward, api.time_attention_heads_backward_launches, api.Handle.attention_heads_backward):
        assert callable(f)
    sig = inspect.signature(api.attention_heads_backward)
    assert list(sig.parameters) == ["handle", "m", "RowPtr", "ColIdx", "Matrix_Val", "heads", "Q", "K", "V", "G", "dQ", "dK", "dV", "scale", "check"]
    sig = inspect.signature(api.Handle.attention_heads_backward)
    assert list(sig.parameters) == ["self", "Q", "K", "V", "G", "heads", "scale", "need"] and sig.parameters["need"].default == (True, True, True)


def test_autograd_layer_takes_the_backward_mode():
    from spmv_amd import autograd
    sig = inspect.signature(autograd.attention_heads)
    assert sig.parameters["backward"].default == "per_head"          # the default stays the per-head loop
    assert "fused" in autograd.attention_heads.__doc__ and "attention_heads_backward" in autograd.attention_heads.__doc__
    with pytest.raises(ValueError, match="backward"):
        autograd.attention_heads(None, None, None, None, 2, backward="both")
    with pytest.raises(Exception) as e:                               # "fused" is accepted: the next check (the handle) is what refuses None
        autograd.attention_heads(None, None, None, None, 2, backward="fused")
    assert "backward must be" not in str(e.value)


def test_option_default_and_range(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    assert lib.spmv_hip_get_option(OPTION) == 0
    try:
        for v in (0, 1, 1024):
            assert lib.spmv_hip_set_option(OPTION, v) == 0 and lib.spmv_hip_get_option(OPTION) == v
        for v in (-1, 1025):
            assert lib.spmv_hip_set_option(OPTION, v) == E_ARG and lib.spmv_hip_get_option(OPTION) == 1024
    finally:
        assert lib.spmv_hip_set_option(OPTION, 0) == 0
        lib.spmv_hip_clear_error()


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    arrays, bits = buffers()
    ptrs = [a.ctypes.data for a in arrays]
    lib.spmv_hip_clear_error()
    assert raw(lib, None, H, K, DV, ptrs, GOOD_LD) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert timer(lib, None, H, K, DV, ptrs, GOOD_LD) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(arrays, bits)


def test_failed_handle_has_no_state(lib, failed_handle):
    arrays, bits = buffers()
    assert api.attention_heads_backward(failed_handle, 4, None, None, None, H, *arrays, check=False) == E_NOSTATE
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.attention_heads_backward(failed_handle, 4, None, None, None, H, *arrays, scale=0.5)
    assert timer(lib, failed_handle, H, K, DV, [a.ctypes.data for a in arrays], GOOD_LD) < 0
    assert lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(arrays, bits)


BIG = 2 ** 30   # BIG * K and 2 * BIG do not fit an int
HUGE = [2 ** 40] * 7


@pytest.mark.parametrize("heads,k,dv,ld", [
    (0, K, DV, GOOD_LD), (-1, K, DV, GOOD_LD), (H, 0, DV, GOOD_LD), (H, -1, DV, GOOD_LD), (H, K, 0, GOOD_LD), (H, K, -2, GOOD_LD),
    *[(H, K, DV, [l - (i == j) for j, l in enumerate(GOOD_LD)]) for i in range(7)],   # each ld one below its full width
    (H, K, DV, [K, K, DV, DV, K, K, DV]),                                             # one head's width as ld
    (BIG, K, 1, HUGE),                                                                # heads * k overflows int, heads * dv does not
    (BIG, 1, 2, HUGE),                                                                # heads * dv = 2^31
    (2, BIG, 1, HUGE),
    (65536, 65536, 1, HUGE),                                                          # the product wraps to 0 in 32 bits
])
def test_bad_sizes_are_argument_errors_before_the_gate(lib, failed_handle, heads, k, dv, ld):
    """a bad heads, k, dv or ld is E_ARG even on a handle that would answer E_NOSTATE: the sizes are checked first"""
    arrays, bits = buffers()
    ptrs = [a.ctypes.data for a in arrays]
    assert raw(lib, failed_handle, heads, k, dv, ptrs, ld) == E_ARG
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert timer(lib, failed_handle, heads, k, dv, ptrs, ld) < 0
    assert lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(arrays, bits)


def test_the_ld_of_an_output_that_is_not_wanted_is_not_checked(lib, failed_handle):
    arrays, bits = buffers()
    ptrs = [a.ctypes.data for a in arrays[:4]] + [arrays[4].ctypes.data, None, None]
    assert raw(lib, failed_handle, H, K, DV, ptrs, [WK, WK, WV, WV, WK, 0, 0]) == E_NOSTATE   # as far as the handle's state
    lib.spmv_hip_clear_error()
    assert unchanged(arrays, bits)


def test_null_operand_is_an_argument_error(lib, failed_handle):
    arrays, bits = buffers()
    ptrs = [a.ctypes.data for a in arrays]
    for missing in range(4):
        p = [None if i == missing else a for i, a in enumerate(ptrs)]
        assert raw(lib, failed_handle, H, K, DV, p, GOOD_LD) == E_ARG
        assert lib.spmv_hip_last_error() == E_ARG
        lib.spmv_hip_clear_error()
    assert unchanged(arrays, bits)


def test_no_output_wanted_is_no_work(lib, failed_handle):
    """all outputs NULL: 0 after argument checking, whatever their leading dimensions say; bad arguments are still refused"""
    arrays, bits = buffers()
    ptrs = [a.ctypes.data for a in arrays[:4]] + [None] * 3
    assert raw(lib, failed_handle, H, K, DV, ptrs, GOOD_LD) == 0
    assert raw(lib, failed_handle, H, K, DV, ptrs, [WK, WK, WV, WV, 0, 0, 0]) == 0
    assert api.attention_heads_backward(failed_handle, 4, None, None, None, H, *arrays[:4]) == 0
    assert lib.spmv_hip_last_error() == 0
    assert raw(lib, failed_handle, H, K, DV, ptrs, [WK - 1, WK, WV, WV, 0, 0, 0]) == E_ARG
    assert raw(lib, None, H, K, DV, ptrs, GOOD_LD) == E_ARG
    lib.spmv_hip_clear_error()
    assert unchanged(arrays, bits)


@pytest.mark.parametrize("heads", [0, -1, 4, 5])
def test_widths_must_divide_into_heads(lib, failed_handle, heads):
    """6 columns of Q / K and 4 of V / G: 4 heads divide only V's, 5 neither; no call reaches the library"""
    arrays, bits = buffers()
    with pytest.raises(ValueError):
        api.attention_heads_backward(failed_handle, 4, None, None, None, heads, *arrays)
    with pytest.raises(ValueError):
        api.time_attention_heads_backward_launches(failed_handle, heads, *arrays, warmup=0, iters=1)
    assert lib.spmv_hip_last_error() == 0
    assert unchanged(arrays, bits)


def test_one_head_takes_the_whole_width(lib, failed_handle):
    """heads = 1 passes k and dv as the full widths: the call gets as far as the handle's state"""
    arrays, bits = buffers()
    assert api.attention_heads_backward(failed_handle, 4, None, None, None, 1, *arrays, check=False) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert unchanged(arrays, bits)
