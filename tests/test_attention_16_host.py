"""CPU: the 16-bit attention's entry points (spmv_hip_attention_gqa_lse_16 and its timer) are exported and bound with the declared signatures, the
Python layers exist, and the type, argument and handle rules hold without any device (include/spmv_hip.h): on an fp32 handle without device state a
bad io_type or o_type and every argument error of spmv_hip_attention_gqa_lse are SPMV_HIP_E_ARG before the handle's state is looked at and good
arguments get as far as SPMV_HIP_E_NOSTATE; on an fp64 handle good arguments are SPMV_HIP_E_ARG; every buffer keeps its bits."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
T_HANDLE, T_F16, T_BF16 = 0, 1, 2
_V, _LL = C.c_void_p, C.c_longlong
_H = api.spmv_Handle_t
_TAIL = [C.c_int, C.c_int, C.POINTER(C.c_float)]
_GQA = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
_OPS = [C.c_int, *[_V, _LL] * 5, C.c_int, _V, _LL]   # io_type, Q, K, V, B, O with their lds, o_type, L and ldl
SIGNATURES = {
    "spmv_hip_attention_gqa_lse_16": (C.c_int, [_H, C.c_int, _V, _V, _V, *_GQA, *_OPS]),
    "spmv_hip_time_attention_gqa_lse_16_launches": (C.c_double, [_H, *_GQA, *_OPS, *_TAIL]),
}
M, H, HKV, K, DV, NNZ = 4, 4, 2, 3, 2, 5
WK, WV = H * K, H * DV       # Q / O
GK, GV = HKV * K, HKV * DV   # K / V


@pytest.fixture(scope="module")
def lib():
    build.build()
    return api.load()


def _failed(lib, monkeypatch, size):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    h = api.spmv_create_handle_all_in_one(-1, 4, None, None, None, 1, api.SPMV_METHODS.Method_Parallel, size, check=False)
    assert h and not h.contents.extraHandle and h.contents.data_size == size
    lib.spmv_hip_clear_error()
    return h


@pytest.fixture
def failed32(lib, monkeypatch):
    """create() with m < 0 fails in its argument check, before any device call: a valid fp32 handle without device state"""
    h = _failed(lib, monkeypatch, 4)
    yield h
    api.spmv_destory_handle(h)


@pytest.fixture
def failed64(lib, monkeypatch):
    h = _failed(lib, monkeypatch, 8)
    yield h
    api.spmv_destory_handle(h)


def buffers():
    """the operands by name, with their bits: Q, K, V and a 16-bit O as raw 16-bit patterns, B and L fp32"""
    a = {
        "Q": (np.arange(M * WK, dtype=np.uint16).reshape(M, WK) + 0x3c00), "K": (np.arange(M * GK, dtype=np.uint16).reshape(M, GK) + 0x3800),
        "V": (np.arange(M * GV, dtype=np.uint16).reshape(M, GV) + 0x4000), "B": np.arange(H * NNZ, dtype=np.float32).reshape(H, NNZ) * 0.25,
        "O": np.full((M, 2 * WV), 0xbeef, dtype=np.uint16),   # room for an fp32 O as well
        "L": np.full((H, M), -1.5, dtype=np.float32),
    }
    return a, {n: v.tobytes() for n, v in a.items()}


def unchanged(a, bits):
    return all(v is None or v.tobytes() == bits[n] for n, v in a.items())


def p(x):
    return None if x is None else x.ctypes.data


def fwd(lib, h, heads, kv, k, dv, a, io=T_F16, ot=T_F16, m=M, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldo=WV, ldl=M):
    return lib.spmv_hip_attention_gqa_lse_16(h, m, None, None, None, heads, kv, k, dv, 1.0, io, p(a["Q"]), ldq, p(a["K"]), ldk, p(a["V"]), ldv, p(a["B"]), ldb,
                                             p(a["O"]), ldo, ot, p(a["L"]), ldl)


def fwd_timer(lib, h, heads, kv, k, dv, a, io=T_F16, ot=T_F16, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldo=WV, ldl=M):
    return lib.spmv_hip_time_attention_gqa_lse_16_launches(h, heads, kv, k, dv, 1.0, io, p(a["Q"]), ldq, p(a["K"]), ldk, p(a["V"]), ldv, p(a["B"]), ldb, p(a["O"]), ldo,
                                                           ot, p(a["L"]), ldl, 1, 1, None)


def is_arg(lib, rc):
    ok = (rc == E_ARG or (isinstance(rc, float) and rc < 0)) and lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    return ok


def is_nostate(lib, rc):
    ok = (rc == E_NOSTATE or (isinstance(rc, float) and rc < 0)) and lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    return ok


GOOD_TYPES = [(T_F16, T_F16), (T_F16, T_HANDLE), (T_BF16, T_BF16), (T_BF16, T_HANDLE)]
BAD_TYPES = [(0, T_HANDLE), (3, T_HANDLE), (0, 0), (3, 3), (-1, T_HANDLE), (T_BF16, T_F16), (T_F16, T_BF16), (T_BF16, 3), (T_F16, 3), (T_F16, -1)]


def test_exported_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.attention_gqa_lse_16, api.time_attention_gqa_lse_16_launches, api.Handle.attention_gqa_lse_16):
        assert callable(f)
    sig = inspect.signature(api.attention_gqa_lse_16)
    assert list(sig.parameters)[:14] == ["handle", "m", "RowPtr", "ColIdx", "Matrix_Val", "heads", "kv_heads", "Q", "K", "V", "B", "O", "L", "scale"]
    assert sig.parameters["L"].default is None and sig.parameters["scale"].default is None
    sig = inspect.signature(api.Handle.attention_gqa_lse_16)
    assert list(sig.parameters)[1:10] == ["Q", "K", "V", "heads", "kv_heads", "B", "scale", "out_dtype", "want_l"]
    assert sig.parameters["out_dtype"].default is None and sig.parameters["want_l"].default is True
    assert (api.T_HANDLE, api.T_F16, api.T_BF16) == (T_HANDLE, T_F16, T_BF16)


def test_headers_declare_the_two_symbols_and_the_types():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    hip, tools = open(os.path.join(inc, "spmv_hip.h")).read(), open(os.path.join(inc, "spmv_hip_tools.h")).read()
    assert "int spmv_hip_attention_gqa_lse_16(" in hip
    assert "double spmv_hip_time_attention_gqa_lse_16_launches(" in tools
    assert "enum { SPMV_HIP_T_HANDLE = 0, SPMV_HIP_T_F16 = 1, SPMV_HIP_T_BF16 = 2 };" in hip


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    a, bits = buffers()
    for call in (fwd, fwd_timer):
        lib.spmv_hip_clear_error()
        assert is_arg(lib, call(lib, None, H, HKV, K, DV, a))
    assert unchanged(a, bits)


def test_good_arguments_get_as_far_as_the_state_on_an_fp32_handle(lib, failed32):
    a, bits = buffers()
    for io, ot in GOOD_TYPES:
        for call in (fwd, fwd_timer):
            for heads, kv in ((H, HKV), (H, 1), (HKV, HKV)):
                assert is_nostate(lib, call(lib, failed32, heads, kv, K, DV, a, io=io, ot=ot)), (call.__name__, io, ot, heads, kv)
        assert is_nostate(lib, fwd(lib, failed32, H, HKV, K, DV, dict(a, L=None), io=io, ot=ot, ldl=-5))      # no L: ldl is not looked at
        assert is_nostate(lib, fwd(lib, failed32, H, HKV, K, DV, dict(a, B=None), io=io, ot=ot, ldb=12345))   # no bias is no error
    # m = 0: nothing is read or written, NULL operands and ldl = 0 are no error
    assert is_nostate(lib, fwd(lib, failed32, H, HKV, K, DV, {n: None for n in a}, m=0, ldl=0))
    assert unchanged(a, bits)


@pytest.mark.parametrize("io,ot", BAD_TYPES)
def test_bad_types_are_argument_errors_before_the_gate(lib, failed32, io, ot):
    a, bits = buffers()
    assert is_arg(lib, fwd(lib, failed32, H, HKV, K, DV, a, io=io, ot=ot))
    assert is_arg(lib, fwd_timer(lib, failed32, H, HKV, K, DV, a, io=io, ot=ot))
    assert unchanged(a, bits)


def test_an_fp64_handle_is_an_argument_error(lib, failed64):
    a, bits = buffers()
    for io, ot in GOOD_TYPES:
        assert is_arg(lib, fwd(lib, failed64, H, HKV, K, DV, a, io=io, ot=ot)), (io, ot)
        assert is_arg(lib, fwd_timer(lib, failed64, H, HKV, K, DV, a, io=io, ot=ot)), (io, ot)
    assert is_arg(lib, fwd(lib, failed64, H, HKV, K, DV, {n: None for n in a}, m=0, ldl=0))   # the handle's precision comes before any work, m = 0 included
    assert unchanged(a, bits)


BIG = 2 ** 30
WIDE = dict(ldq=2 ** 40, ldk=2 ** 40, ldv=2 ** 40, ldo=2 ** 40)


@pytest.mark.parametrize("heads,kv,k,dv,ld", [
    # spmv_hip_attention_gqa_lse's rules, every one of them
    (0, 1, K, DV, {}), (-2, 1, K, DV, {}), (H, HKV, 0, DV, {}), (H, HKV, K, 0, {}), (H, HKV, K, -2, {}),
    (H, HKV, K, DV, dict(ldq=WK - 1)), (H, HKV, K, DV, dict(ldo=WV - 1)),
    (BIG, BIG, K, 1, WIDE), (65536, 1, 65536, 1, WIDE),
    (H, HKV, K, DV, dict(ldb=-1)),
    (H, 0, K, DV, {}), (H, 3, K, DV, WIDE), (3, 2, K, DV, WIDE),
    (H, HKV, K, DV, dict(ldk=GK - 1)), (H, HKV, K, DV, dict(ldv=GV - 1)), (H, H, K, DV, {}),
    (H, HKV, K, DV, dict(ldl=M - 1)), (H, HKV, K, DV, dict(ldl=0)), (H, HKV, K, DV, dict(ldl=-1)), (H, HKV, K, DV, dict(ldl=-2 ** 40)),
])
@pytest.mark.parametrize("io,ot", [(T_F16, T_F16), (T_BF16, T_HANDLE)])
def test_bad_sizes_are_argument_errors_before_the_gate(lib, failed32, io, ot, heads, kv, k, dv, ld):
    """a bad heads, kv_heads, k, dv or ld is E_ARG even on a handle that would answer E_NOSTATE: the sizes are checked first"""
    a, bits = buffers()
    assert is_arg(lib, fwd(lib, failed32, heads, kv, k, dv, a, io=io, ot=ot, **ld))
    if "ldl" not in ld:   # the timer has no m: it leaves the planes' stride to the call it times
        assert is_arg(lib, fwd_timer(lib, failed32, heads, kv, k, dv, a, io=io, ot=ot, **ld))
    assert unchanged(a, bits)


def test_a_cleared_handle_has_no_state(lib, failed32, failed64):
    """spmv_clear_handle resets data_size with everything else: a cleared handle, whatever it held, is E_NOSTATE as in every other call"""
    a, bits = buffers()
    for h in (failed32, failed64):
        api.spmv_clear_handle(h)
        assert h.contents.data_size == 0
        assert is_nostate(lib, fwd(lib, h, H, HKV, K, DV, a))
        assert is_nostate(lib, fwd_timer(lib, h, H, HKV, K, DV, a))
        assert is_arg(lib, fwd(lib, h, H, HKV, K, DV, a, io=3))
    assert unchanged(a, bits)


def test_null_operand_is_an_argument_error(lib, failed32):
    a, bits = buffers()
    for missing in ("Q", "K", "V", "O"):
        assert is_arg(lib, fwd(lib, failed32, H, HKV, K, DV, dict(a, **{missing: None}))), missing
        assert is_arg(lib, fwd_timer(lib, failed32, H, HKV, K, DV, dict(a, **{missing: None}))), missing
    assert unchanged(a, bits)


def test_the_python_layer(lib, failed32, failed64):
    """io_type and o_type come from the tensors' dtypes; tensors that are not 16-bit, disagree, or an O of a third type never reach the library"""
    import torch
    for dt in (torch.float16, torch.bfloat16):
        Q, Kk, Vv = torch.ones((M, WK), dtype=dt), torch.ones((M, GK), dtype=dt), torch.ones((M, GV), dtype=dt)
        B, L = torch.zeros((H, NNZ)), torch.full((H, M), -1.5)
        for O in (torch.full((M, WV), -1.0, dtype=dt), torch.full((M, WV), -1.0)):
            for bias in (B, B[0], None):
                assert api.attention_gqa_lse_16(failed32, M, None, None, None, H, HKV, Q, Kk, Vv, bias, O, L, check=False) == E_NOSTATE
                lib.spmv_hip_clear_error()
            assert api.attention_gqa_lse_16(failed32, M, None, None, None, H, HKV, Q, Kk, Vv, B, O, check=False) == E_NOSTATE   # L defaults to None
            lib.spmv_hip_clear_error()
            assert api.attention_gqa_lse_16(failed64, M, None, None, None, H, HKV, Q, Kk, Vv, B, O, L, check=False) == E_ARG
            lib.spmv_hip_clear_error()
            with pytest.raises(api.SpmvError, match=r"\[5\]"):
                api.attention_gqa_lse_16(failed32, M, None, None, None, H, HKV, Q, Kk, Vv, B, O, L, scale=0.5)
            with pytest.raises(api.SpmvError):
                api.time_attention_gqa_lse_16_launches(failed32, H, HKV, Q, Kk, Vv, B, O, L, warmup=1, iters=1)
            lib.spmv_hip_clear_error()
            assert (O == -1.0).all() and (L == -1.5).all()
        other = torch.bfloat16 if dt == torch.float16 else torch.float16
        O = torch.zeros((M, WV), dtype=dt)
        with pytest.raises(TypeError):   # mixed operands
            api.attention_gqa_lse_16(failed32, M, None, None, None, H, HKV, Q, Kk.to(other), Vv, None, O)
        with pytest.raises(TypeError):   # an O of the other 16-bit type
            api.attention_gqa_lse_16(failed32, M, None, None, None, H, HKV, Q, Kk, Vv, None, O.to(other))
        with pytest.raises(TypeError):   # fp64 O
            api.attention_gqa_lse_16(failed32, M, None, None, None, H, HKV, Q, Kk, Vv, None, O.double())
        with pytest.raises(TypeError):   # fp32 operands belong to attention_gqa_lse
            api.attention_gqa_lse_16(failed32, M, None, None, None, H, HKV, Q.float(), Kk.float(), Vv.float(), None, O.float())
        with pytest.raises(TypeError):   # numpy has no bfloat16: tensors only
            api.attention_gqa_lse_16(failed32, M, None, None, None, H, HKV, np.ones((M, WK), dtype=np.float16), Kk, Vv, None, O)
        with pytest.raises(ValueError):  # L has a plane per QUERY head
            api.attention_gqa_lse_16(failed32, M, None, None, None, H, HKV, Q, Kk, Vv, None, O, torch.zeros((HKV, M)))


def test_the_autograd_docstrings_state_the_contract():
    from spmv_amd import autograd
    for f in (autograd.attention_heads, autograd.attention, autograd.attention_parts):
        assert "fp32_result.to(dtype)" in f.__doc__ and "fp32_gradient.to(dtype)" in f.__doc__ and "attention_gqa_lse_16" in f.__doc__, f.__name__
