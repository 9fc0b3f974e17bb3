"""CPU: the log-sum-exp attention's entry points (spmv_hip_attention_gqa_lse, spmv_hip_attention_merge, spmv_hip_attention_gqa_backward_lse and
their three timers) are exported and bound with the declared signatures, the Python layers exist, and the argument and handle rules hold
without any device (include/spmv_hip.h: SPMV_HIP_E_ARG for the GQA calls' bad arguments and for ldl < m, ldo < heads*dv, a NULL O or L before
the handle's state is looked at; E_NOSTATE for a handle without device state; every buffer keeps its bits).  The merge has no m argument: its
plane strides and NULL operands are looked at once the handle's m is known, so on a handle without state they are E_NOSTATE."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from spmv_amd import api, build

E_ARG, E_NOSTATE = 3, 5
_V, _LL = C.c_void_p, C.c_longlong
_H = api.spmv_Handle_t
_TAIL = [C.c_int, C.c_int, C.POINTER(C.c_float)]
_GQA = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
SIGNATURES = {
    "spmv_hip_attention_gqa_lse": (C.c_int, [_H, C.c_int, _V, _V, _V, *_GQA, *[_V, _LL] * 6]),
    "spmv_hip_time_attention_gqa_lse_launches": (C.c_double, [_H, *_GQA, *[_V, _LL] * 6, *_TAIL]),
    "spmv_hip_attention_merge": (C.c_int, [_H, C.c_int, C.c_int, *[_V, _LL] * 6]),
    "spmv_hip_time_attention_merge_launches": (C.c_double, [_H, C.c_int, C.c_int, *[_V, _LL] * 6, *_TAIL]),
    "spmv_hip_attention_gqa_backward_lse": (C.c_int, [_H, C.c_int, _V, _V, _V, *_GQA, *[_V, _LL] * 11]),
    "spmv_hip_time_attention_gqa_backward_lse_launches": (C.c_double, [_H, *_GQA, *[_V, _LL] * 11, *_TAIL]),
}
M, H, HKV, K, DV, NNZ = 4, 4, 2, 3, 2, 5
WK, WV = H * K, H * DV       # Q, dQ / O, G
GK, GV = HKV * K, HKV * DV   # K, dK / V, dV


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


NAMES = ["Q", "K", "V", "B", "G", "O", "L", "O2", "L2", "Oout", "Lout", "dQ", "dK", "dV", "dB"]


def buffers():
    """the inputs and outputs of the three calls by name, with their bits"""
    a = {
        "Q": np.arange(M * WK, dtype=np.float64).reshape(M, WK) - 2, "K": np.arange(M * GK, dtype=np.float64).reshape(M, GK) * 0.5,
        "V": np.arange(M * GV, dtype=np.float64).reshape(M, GV) + 1, "B": np.arange(H * NNZ, dtype=np.float64).reshape(H, NNZ) * 0.25,
        "G": np.arange(M * WV, dtype=np.float64).reshape(M, WV) - 3, "O": np.full((M, WV), -1.0), "L": np.full((H, M), -1.5),
        "O2": np.full((M, WV), -6.0), "L2": np.full((H, M), -6.5), "Oout": np.full((M, WV), -7.0), "Lout": np.full((H, M), -7.5),
        "dQ": np.full((M, WK), -2.0), "dK": np.full((M, GK), -3.0), "dV": np.full((M, GV), -4.0), "dB": np.full((H, NNZ), -5.0),
    }
    return a, {n: v.tobytes() for n, v in a.items()}


def unchanged(a, bits):
    return all(v is None or v.tobytes() == bits[n] for n, v in a.items())


def p(x):
    return None if x is None else x.ctypes.data


def fwd(lib, h, heads, kv, k, dv, a, m=M, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldo=WV, ldl=M):
    return lib.spmv_hip_attention_gqa_lse(h, m, None, None, None, heads, kv, k, dv, 1.0, p(a["Q"]), ldq, p(a["K"]), ldk, p(a["V"]), ldv, p(a["B"]), ldb,
                                          p(a["O"]), ldo, p(a["L"]), ldl)


def fwd_timer(lib, h, heads, kv, k, dv, a, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldo=WV, ldl=M):
    return lib.spmv_hip_time_attention_gqa_lse_launches(h, heads, kv, k, dv, 1.0, p(a["Q"]), ldq, p(a["K"]), ldk, p(a["V"]), ldv, p(a["B"]), ldb, p(a["O"]), ldo,
                                                        p(a["L"]), ldl, 1, 1, None)


def bwd(lib, h, heads, kv, k, dv, a, m=M, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldg=WV, ldo=WV, ldl=M, lddq=WK, lddk=GK, lddv=GV, lddb=NNZ):
    return lib.spmv_hip_attention_gqa_backward_lse(h, m, None, None, None, heads, kv, k, dv, 1.0, p(a["Q"]), ldq, p(a["K"]), ldk, p(a["V"]), ldv, p(a["B"]), ldb,
                                                   p(a["G"]), ldg, p(a["O"]), ldo, p(a["L"]), ldl, p(a["dQ"]), lddq, p(a["dK"]), lddk, p(a["dV"]), lddv, p(a["dB"]), lddb)


def bwd_timer(lib, h, heads, kv, k, dv, a, ldq=WK, ldk=GK, ldv=GV, ldb=NNZ, ldg=WV, ldo=WV, ldl=M, lddq=WK, lddk=GK, lddv=GV, lddb=NNZ):
    return lib.spmv_hip_time_attention_gqa_backward_lse_launches(h, heads, kv, k, dv, 1.0, p(a["Q"]), ldq, p(a["K"]), ldk, p(a["V"]), ldv, p(a["B"]), ldb, p(a["G"]), ldg,
                                                                 p(a["O"]), ldo, p(a["L"]), ldl, p(a["dQ"]), lddq, p(a["dK"]), lddk, p(a["dV"]), lddv, p(a["dB"]), lddb,
                                                                 1, 1, None)


def mrg(lib, h, heads, dv, a, ldo1=WV, ldl1=M, ldo2=WV, ldl2=M, ldo=WV, ldl=M):
    return lib.spmv_hip_attention_merge(h, heads, dv, p(a["O"]), ldo1, p(a["L"]), ldl1, p(a["O2"]), ldo2, p(a["L2"]), ldl2, p(a["Oout"]), ldo, p(a["Lout"]), ldl)


def mrg_timer(lib, h, heads, dv, a, ldo1=WV, ldl1=M, ldo2=WV, ldl2=M, ldo=WV, ldl=M):
    return lib.spmv_hip_time_attention_merge_launches(h, heads, dv, p(a["O"]), ldo1, p(a["L"]), ldl1, p(a["O2"]), ldo2, p(a["L2"]), ldl2, p(a["Oout"]), ldo,
                                                      p(a["Lout"]), ldl, 1, 1, None)


def is_arg(lib, rc):
    ok = (rc == E_ARG or (isinstance(rc, float) and rc < 0)) and lib.spmv_hip_last_error() == E_ARG
    lib.spmv_hip_clear_error()
    return ok


def is_nostate(lib, rc):
    ok = (rc == E_NOSTATE or (isinstance(rc, float) and rc < 0)) and lib.spmv_hip_last_error() == E_NOSTATE
    lib.spmv_hip_clear_error()
    return ok


def test_exported_and_bound(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        assert api.FUNCTIONS[name] == (restype, argtypes), name
        f = getattr(lib, name)
        assert f.restype is restype and f.argtypes == argtypes
    for f in (api.attention_gqa_lse, api.attention_merge, api.attention_gqa_backward_lse, api.time_attention_gqa_lse_launches, api.time_attention_merge_launches,
              api.time_attention_gqa_backward_lse_launches, api.Handle.attention_gqa_lse, api.Handle.attention_merge, api.Handle.attention_gqa_backward_lse):
        assert callable(f)
    sig = inspect.signature(api.Handle.attention_gqa_lse)
    assert list(sig.parameters)[1:10] == ["Q", "K", "V", "heads", "kv_heads", "bias", "scale", "out", "lse"]
    sig = inspect.signature(api.Handle.attention_gqa_backward_lse)
    assert list(sig.parameters)[1:12] == ["Q", "K", "V", "bias", "G", "O", "L", "heads", "kv_heads", "scale", "need"]
    assert sig.parameters["need"].default == (True, True, True, True)
    sig = inspect.signature(api.Handle.attention_merge)
    assert list(sig.parameters)[1:6] == ["O1", "L1", "O2", "L2", "heads"]


def test_headers_declare_the_six_symbols():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    hip, tools = open(os.path.join(inc, "spmv_hip.h")).read(), open(os.path.join(inc, "spmv_hip_tools.h")).read()
    for name in ("spmv_hip_attention_gqa_lse", "spmv_hip_attention_merge", "spmv_hip_attention_gqa_backward_lse"):
        assert f"int {name}(" in hip
    for name in ("spmv_hip_time_attention_gqa_lse_launches", "spmv_hip_time_attention_merge_launches", "spmv_hip_time_attention_gqa_backward_lse_launches"):
        assert f"double {name}(" in tools


def test_null_handle_is_an_argument_error(lib, monkeypatch):
    monkeypatch.setenv("SPMV_HIP_QUIET", "1")
    a, bits = buffers()
    for call in (fwd, bwd, fwd_timer, bwd_timer):
        lib.spmv_hip_clear_error()
        assert is_arg(lib, call(lib, None, H, HKV, K, DV, a))
    for call in (mrg, mrg_timer):
        lib.spmv_hip_clear_error()
        assert is_arg(lib, call(lib, None, H, DV, a))
    assert unchanged(a, bits)


def test_failed_handle_has_no_state(lib, failed_handle):
    """good arguments get as far as the handle's state"""
    a, bits = buffers()
    for call in (fwd, bwd, fwd_timer, bwd_timer):
        for heads, kv in ((H, HKV), (H, 1), (HKV, HKV)):
            assert is_nostate(lib, call(lib, failed_handle, heads, kv, K, DV, a)), (call.__name__, heads, kv)
    b = dict(a, L=None)   # L = NULL is spmv_hip_attention_gqa: ldl is not looked at
    assert is_nostate(lib, fwd(lib, failed_handle, H, HKV, K, DV, b, ldl=-5))
    b = dict(a, B=None)   # no bias is no error
    assert is_nostate(lib, fwd(lib, failed_handle, H, HKV, K, DV, b, ldb=12345))
    assert is_nostate(lib, bwd(lib, failed_handle, H, HKV, K, DV, b, ldb=12345))
    for call in (mrg, mrg_timer):
        assert is_nostate(lib, call(lib, failed_handle, H, DV, a))
        assert is_nostate(lib, call(lib, failed_handle, 1, H * DV, a))
    assert is_nostate(lib, mrg(lib, failed_handle, H, DV, dict(a, Lout=None), ldl=-1))   # no merged L wanted: its stride is not looked at
    # m is the handle's in the merge: plane strides below it and NULL operands are found once it is known
    assert is_nostate(lib, mrg(lib, failed_handle, H, DV, a, ldl1=1))
    assert is_nostate(lib, mrg(lib, failed_handle, H, DV, dict(a, O2=None)))
    # the Python layer
    Q, Kk, Vv, B, G, O, L = (a[n] for n in ("Q", "K", "V", "B", "G", "O", "L"))
    for bias in (B, B[0], None):
        assert api.attention_gqa_lse(failed_handle, M, None, None, None, H, HKV, Q, Kk, Vv, bias, O, L, check=False) == E_NOSTATE
        lib.spmv_hip_clear_error()
        assert api.attention_gqa_backward_lse(failed_handle, M, None, None, None, H, HKV, Q, Kk, Vv, bias, G, O, L, a["dQ"], a["dK"], a["dV"], a["dB"], check=False) == E_NOSTATE
        lib.spmv_hip_clear_error()
    assert api.attention_merge(failed_handle, H, O, L, a["O2"], a["L2"], a["Oout"], a["Lout"], check=False) == E_NOSTATE
    lib.spmv_hip_clear_error()
    assert api.attention_merge(failed_handle, H, O, L, a["O2"], a["L2"], O, L, check=False) == E_NOSTATE   # the accumulator form
    lib.spmv_hip_clear_error()
    with pytest.raises(api.SpmvError, match=r"\[5\]"):
        api.attention_gqa_lse(failed_handle, M, None, None, None, H, HKV, Q, Kk, Vv, B, O, L, scale=0.5)
    with pytest.raises(ValueError):   # L has a plane per QUERY head
        api.attention_gqa_lse(failed_handle, M, None, None, None, H, HKV, Q, Kk, Vv, B, O, np.zeros((HKV, M)))
    with pytest.raises(ValueError):   # O of the backward is heads * dv wide
        api.attention_gqa_backward_lse(failed_handle, M, None, None, None, H, HKV, Q, Kk, Vv, B, G, a["dK"], L, dQ=a["dQ"])
    with pytest.raises(ValueError):   # the merge's O operands have one width
        api.attention_merge(failed_handle, H, O, L, a["dQ"], a["L2"], a["Oout"], a["Lout"])
    with pytest.raises(ValueError):   # ... a multiple of heads
        api.attention_merge(failed_handle, 3, O, np.zeros((3, M)), a["O2"], np.zeros((3, M)), a["Oout"], np.zeros((3, M)))
    assert unchanged(a, bits)


def test_all_outputs_null_returns_after_argument_checking(lib, failed_handle):
    """nothing wanted: 0 without looking at the handle's state -- but the arguments, the new ones included, are checked first"""
    a, bits = buffers()
    none = dict(a, dQ=None, dK=None, dV=None, dB=None)
    assert bwd(lib, failed_handle, H, HKV, K, DV, none) == 0 and lib.spmv_hip_last_error() == 0
    assert is_arg(lib, bwd(lib, failed_handle, H, HKV, K, DV, none, ldl=M - 1))
    assert is_arg(lib, bwd(lib, failed_handle, H, HKV, K, DV, none, ldo=WV - 1))
    assert is_arg(lib, bwd(lib, failed_handle, H, HKV, K, DV, dict(none, L=None)))
    assert is_nostate(lib, bwd(lib, failed_handle, H, HKV, K, DV, dict(none, dB=a["dB"])))   # dB alone is work
    assert unchanged(a, bits)


BIG = 2 ** 30
WIDE = dict(ldq=2 ** 40, ldk=2 ** 40, ldv=2 ** 40, ldo=2 ** 40, ldg=2 ** 40, lddq=2 ** 40, lddk=2 ** 40, lddv=2 ** 40)


@pytest.mark.parametrize("heads,kv,k,dv,ld", [
    # the GQA calls' rules
    (0, 1, K, DV, {}), (-2, 1, K, DV, {}), (H, HKV, 0, DV, {}), (H, HKV, K, 0, {}), (H, HKV, K, -2, {}),
    (H, HKV, K, DV, dict(ldq=WK - 1)), (H, HKV, K, DV, dict(ldo=WV - 1, ldg=WV - 1)),
    (BIG, BIG, K, 1, WIDE), (65536, 1, 65536, 1, WIDE),
    (H, HKV, K, DV, dict(ldb=-1)),
    (H, 0, K, DV, {}), (H, 3, K, DV, WIDE), (3, 2, K, DV, WIDE),
    (H, HKV, K, DV, dict(ldk=GK - 1)), (H, HKV, K, DV, dict(ldv=GV - 1)), (H, H, K, DV, {}),
    # the new ones: the planes of L are m apart at the least; the backward's O is heads * dv wide
    (H, HKV, K, DV, dict(ldl=M - 1)), (H, HKV, K, DV, dict(ldl=0)), (H, HKV, K, DV, dict(ldl=-1)), (H, HKV, K, DV, dict(ldl=-2 ** 40)),
])
def test_bad_sizes_are_argument_errors_before_the_gate(lib, failed_handle, heads, kv, k, dv, ld):
    """a bad heads, kv_heads, k, dv or ld is E_ARG even on a handle that would answer E_NOSTATE: the sizes are checked first"""
    a, bits = buffers()
    f_ld = {key: v for key, v in ld.items() if key in ("ldq", "ldk", "ldv", "ldb", "ldo", "ldl")}
    b_ld = {key: v for key, v in ld.items() if key != "ldo"}   # ldo: the forward's output there, the backward's own input is tested below
    assert is_arg(lib, fwd(lib, failed_handle, heads, kv, k, dv, a, **f_ld))
    assert is_arg(lib, bwd(lib, failed_handle, heads, kv, k, dv, a, **b_ld))
    if "ldl" not in ld:   # the timers have no m: they leave the planes' stride to the call they time
        assert is_arg(lib, fwd_timer(lib, failed_handle, heads, kv, k, dv, a, **f_ld))
        assert is_arg(lib, bwd_timer(lib, failed_handle, heads, kv, k, dv, a, **b_ld))
    assert unchanged(a, bits)


@pytest.mark.parametrize("ld", [dict(ldo=WV - 1), dict(ldo=DV), dict(ldo=0), dict(lddq=WK - 1), dict(lddk=GK - 1), dict(lddv=GV - 1), dict(lddb=-1)])
def test_bad_backward_strides_are_argument_errors_before_the_gate(lib, failed_handle, ld):
    a, bits = buffers()
    assert is_arg(lib, bwd(lib, failed_handle, H, HKV, K, DV, a, **ld))
    assert is_arg(lib, bwd_timer(lib, failed_handle, H, HKV, K, DV, a, **ld))
    assert unchanged(a, bits)


def test_null_operand_is_an_argument_error(lib, failed_handle):
    a, bits = buffers()
    for missing in ("Q", "K", "V", "O"):
        assert is_arg(lib, fwd(lib, failed_handle, H, HKV, K, DV, dict(a, **{missing: None}))), missing
    for missing in ("Q", "K", "V", "G", "O", "L"):
        assert is_arg(lib, bwd(lib, failed_handle, H, HKV, K, DV, dict(a, **{missing: None}))), missing
        assert is_arg(lib, bwd_timer(lib, failed_handle, H, HKV, K, DV, dict(a, **{missing: None}))), missing
    # m = 0: nothing is read or written, NULL operands and ldl = 0 are no error
    empty = {n: None for n in a}
    assert is_nostate(lib, fwd(lib, failed_handle, H, HKV, K, DV, empty, m=0, ldl=0))
    assert is_nostate(lib, bwd(lib, failed_handle, H, HKV, K, DV, dict(empty, dQ=a["dQ"]), m=0, ldl=0))
    assert unchanged(a, bits)


@pytest.mark.parametrize("heads,dv,ld", [
    (0, DV, {}), (-1, DV, {}), (H, 0, {}), (H, -3, {}), (BIG, 4, dict(ldo1=2 ** 40, ldo2=2 ** 40, ldo=2 ** 40)), (65536, 65536, dict(ldo1=2 ** 40, ldo2=2 ** 40, ldo=2 ** 40)),
    (H, DV, dict(ldo1=WV - 1)), (H, DV, dict(ldo2=WV - 1)), (H, DV, dict(ldo=WV - 1)), (H, DV, dict(ldo=DV)),
    (H, DV, dict(ldl1=-1)), (H, DV, dict(ldl2=-1)), (H, DV, dict(ldl=-1)),
])
def test_merge_bad_sizes_are_argument_errors_before_the_gate(lib, failed_handle, heads, dv, ld):
    a, bits = buffers()
    assert is_arg(lib, mrg(lib, failed_handle, heads, dv, a, **ld))
    if not any(key.startswith("ldl") for key in ld):   # the timer leaves the plane strides to the call it times
        assert is_arg(lib, mrg_timer(lib, failed_handle, heads, dv, a, **ld))
    assert unchanged(a, bits)


def test_attention_parts_is_there_and_rejects_mismatched_arguments():
    """the argument rules that need no device: the counts of handles, K, V and biases, and heads against kv_heads"""
    from spmv_amd import autograd
    sig = inspect.signature(autograd.attention_parts)
    assert list(sig.parameters)[:6] == ["handles", "Q", "Ks", "Vs", "heads", "scale"]
    for name in ("kv_heads", "biases"):
        assert sig.parameters[name].default is None and sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert "attention_gqa_backward_lse" in autograd.attention_parts.__doc__ and "attention_merge" in autograd.attention_parts.__doc__
    h = object()
    with pytest.raises(ValueError, match="per handle"):
        autograd.attention_parts([], None, [], [], 2)
    with pytest.raises(ValueError, match="per handle"):
        autograd.attention_parts([h, h], None, [None], [None, None], 2)
    with pytest.raises(ValueError, match="per handle"):
        autograd.attention_parts([h, h], None, [None, None], [None, None], 2, biases=[None])
    with pytest.raises(ValueError, match="multiple"):
        autograd.attention_parts([h], None, [None], [None], 4, kv_heads=3)
    with pytest.raises(ValueError, match="multiple"):
        autograd.attention_parts([h], None, [None], [None], 0)


def test_the_documented_order_restated_in_float32_stays_within_the_bound_for_l():
    """the bound of test_gpu_attention_lse.py is derived (lse_cases.l_bound); here a float32 numpy restatement of the documented order -- W chains,
    the tree over neighbours, four waves for a long row; numpy's exp and log, which are within the bounds used for the device's -- is held against
    it on every row length of the GPU tests, so a bound that the order itself cannot meet shows up without a device"""
    import gqa_cases as gc
    import lse_cases as lc
    assert [lc.a_len(n) for n in (1, 2, 3, 64, 65, 512, 513, 5000)] == [0, 1, 2, 6, 7, 13, 10, 27]
    rng = np.random.default_rng(5)
    worst = 0.0
    for n in [x for x in gc.LENGTHS if x > 0]:
        for spread in (0.5, 4.0, 30.0):   # scores close together, apart, and far apart (most weights underflow)
            r = rng.uniform(-spread, spread, n).astype(np.float32)
            ref = r.astype(np.longdouble)
            ref = ref.max() + np.log(np.exp(ref - ref.max()).sum())
            got = lc.lse_restated(r)
            assert got.dtype == np.float32
            e, b = abs(np.longdouble(got) - ref), lc.l_bound(n, ref, np.float32)
            worst = max(worst, float(e / b))
            assert e <= b, (n, spread, float(e), b)
    assert worst > 0   # the restatement rounds: the test is not comparing the reference with itself
