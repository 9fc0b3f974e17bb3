"""Python host side above the C ABI of libspmv_hip.so (include/spmv.h, include/spmv_hip.h).

It mirrors the reference's operator interface one to one -- same function names, same argument
order and meaning, same void returns (reference: include/spmv.h:19-71, common.c:123-190,
278-304) -- so the parity tests read like the reference's own harness (test_spmv.c:62-156).
Arrays may be numpy arrays (host) or torch tensors (host or cuda); only their raw pointers cross
the boundary.  torch is used for device memory, streams and torch.distributed only.

There is no fallback: if libspmv_hip.so is missing or cannot be loaded `load()` raises, and without
a GPU every call reports SPMV_HIP_E_NODEVICE.  (The library's one host loop -- VECTOR_NONE with option
"host_rows", BASELINE config 1 -- is a configuration the caller switches on, csrc/host_rows.c.)
"""
from __future__ import annotations

import ctypes as C
import enum
import math
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libspmv_hip.so")


class VECTORIZED_WAY(enum.IntEnum):  # include/spmv_Defines.h
    VECTOR_NONE = 0
    VECTOR_AVX2 = 1
    VECTOR_AVX512 = 2
    VECTOR_HIP = 3
    VECTOR_TOTAL_SIZE = 4


class SPMV_METHODS(enum.IntEnum):  # include/spmv_Defines.h
    Method_Serial = 0
    Method_Parallel = 1
    Method_Balanced = 2
    Method_Balanced2 = 3
    Method_Balanced_Yid = 4
    Method_SellCSigma = 5
    Method_CSR5SPMV = 6
    Method_Total_Size = 7
    Method_Numa = 8


_I = C.POINTER(C.c_int)
_V = C.c_void_p


class spmv_Handle(C.Structure):
    """struct spmv_Handle (include/spmv_Defines.h; field order is the reference's)."""
    _fields_ = [("spmvMethod", C.c_int), ("data_size", C.c_ulong), ("nthreads", C.c_ulong),
                ("vectorizedWay", C.c_int), ("Level_3_opt_used", C.c_int), ("RowPtr", _I),
                ("ColIdx", _I), ("index", _I), ("Matrix_Val", _V), ("Y_temp", _V),
                ("extraHandle", _V)]


spmv_Handle_t = C.POINTER(spmv_Handle)


class spmv_hip_info(C.Structure):
    _fields_ = [("device", C.c_int), ("schedule", C.c_int), ("lanes_per_row", C.c_int),
                ("sell_c", C.c_int), ("sell_sigma", C.c_int), ("tile_nnz", C.c_int),
                ("m", C.c_int), ("n", C.c_int), ("nnz", C.c_longlong), ("stored_nnz", C.c_longlong),
                ("max_row_len", C.c_int), ("min_row_len", C.c_int), ("empty_rows", C.c_int),
                ("mean_row_len", C.c_double), ("device_bytes", C.c_longlong),
                ("alg_bytes", C.c_longlong), ("inspect_ms", C.c_double),
                ("schedule_name", C.c_char_p), ("kernel_name", C.c_char_p),
                ("tuned_choice", C.c_int), ("tune_ms", C.c_float * 3),
                ("x_groups", C.c_int), ("x_groups_staged", C.c_int), ("cache_blocked", C.c_int),
                ("stream_bytes", C.c_longlong), ("x_bytes", C.c_longlong), ("route_ms", C.c_float * 2), ("split_ms", C.c_float * 2), ("far_nnz", C.c_longlong), ("run_nnz", C.c_longlong), ("byte_nnz", C.c_longlong), ("tmpl_nnz", C.c_longlong),
                ("blk_waves", C.c_int), ("launch_kernels", C.c_char * 160), ("reproducible", C.c_int),
                ("x_span_max", C.c_int), ("lds_bytes", C.c_int),
                ("packed_nnz", C.c_longlong), ("pack_ms", C.c_float * 2)]


class spmv_hip_cg_options(C.Structure):  # include/spmv_hip.h
    _fields_ = [("rtol", C.c_double), ("atol", C.c_double), ("max_iterations", C.c_int), ("check_every", C.c_int), ("use_x0", C.c_int),
                ("Dinv", C.c_void_p), ("history", C.POINTER(C.c_double))]


class spmv_hip_cg_result(C.Structure):  # include/spmv_hip.h
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("rr", C.c_double), ("bb", C.c_double)]


class spmv_hip_cg_mixed_options(C.Structure):  # include/spmv_hip.h
    _fields_ = [("rtol", C.c_double), ("atol", C.c_double), ("max_iterations", C.c_int), ("check_every", C.c_int), ("use_x0", C.c_int),
                ("Dinv", C.c_void_p), ("history", C.POINTER(C.c_double)), ("update_drop", C.c_double), ("update_every", C.c_int)]


class spmv_hip_cg_mixed_result(C.Structure):  # include/spmv_hip.h
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("updates", C.c_int), ("rr", C.c_double), ("bb", C.c_double)]


class spmv_hip_lsqr_options(C.Structure):  # include/spmv_hip.h
    _fields_ = [("rtol", C.c_double), ("atol", C.c_double), ("ls_tol", C.c_double), ("damp", C.c_double), ("max_iterations", C.c_int), ("check_every", C.c_int),
                ("use_x0", C.c_int), ("history", C.POINTER(C.c_double))]


class spmv_hip_lsqr_result(C.Structure):  # include/spmv_hip.h
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("rr", C.c_double), ("bb", C.c_double), ("ar", C.c_double), ("anorm", C.c_double)]


CG_STATUS = ("converged", "max_iterations", "breakdown", "nonfinite")  # SPMV_HIP_CG_*
CG_MIXED_STATUS = CG_STATUS + ("stagnated",)  # spmv_hip_cg_mixed alone has SPMV_HIP_CG_STAGNATED
LSQR_STATUS = CG_MIXED_STATUS + ("least_squares",)  # spmv_hip_lsqr alone has SPMV_HIP_LSQR_LEAST_SQUARES (5); it never returns 2 or 4

# The fused attention's entry points (include/spmv_hip.h, spmv_hip_tools.h), a row each: the stem, then the size arguments and the operands in
# the prototype's order.  A size is an int -- scale a double --, an operand a void * followed by its leading dimension or plane stride, a
# long long; a *_type is a SPMV_HIP_T_* code, an int.  Both the prototypes in FUNCTIONS (the call's and its timer's) and the arguments that
# are passed (_attention_args, which looks every name up in a record) come from the row: a new rung is a new row, and nothing else lists
# C arguments.
_GQA = "heads kv_heads k dv scale"
_ATTENTION = {stem: tuple((sizes + " " + operands).split()) for stem, sizes, operands in (
    ("attention", "k dv scale", "Q K V O"),
    ("attention_heads", "heads k dv scale", "Q K V O"),
    ("attention_backward", "k dv scale", "Q K V G dQ dK dV"),
    ("attention_heads_backward", "heads k dv scale", "Q K V G dQ dK dV"),
    ("attention_bias", "heads k dv scale", "Q K V B O"),
    ("attention_bias_backward", "heads k dv scale", "Q K V B G dQ dK dV dB"),
    ("attention_gqa", _GQA, "Q K V B O"),
    ("attention_gqa_backward", _GQA, "Q K V B G dQ dK dV dB"),
    ("attention_gqa_lse", _GQA, "Q K V B O L"),
    ("attention_gqa_lse_16", _GQA + " io_type", "Q K V B O o_type L"),
    ("attention_gqa_backward_lse", _GQA, "Q K V B G O L dQ dK dV dB"),
    ("attention_gqa_backward_16", _GQA + " io_type", "Q K V B G O L dq_type dQ dkv_type dK dV dB"),
)}
_CSR = [spmv_Handle_t, C.c_int, _V, _V, _V]          # handle, m, RowPtr, ColIdx, Matrix_Val: what a call begins with
_TIMED = [spmv_Handle_t]                               # ... a timer takes the handle alone
_TAIL = [C.c_int, C.c_int, C.POINTER(C.c_float)]       # ... and ends with warmup, iters, ms_out


def _attention_prototypes():
    """-> the FUNCTIONS entries of every row's call spmv_hip_<stem> and timer spmv_hip_time_<stem>_launches"""
    out = {}
    for stem, row in _ATTENTION.items():
        args = []
        for name in row:
            args += [C.c_double] if name == "scale" else [C.c_int] if name.islower() else [_V, C.c_longlong]   # only an operand has a capital
        out[f"spmv_hip_{stem}"] = (C.c_int, _CSR + args)
        out[f"spmv_hip_time_{stem}_launches"] = (C.c_double, _TIMED + args + _TAIL)
    return out


# Every symbol include/*.h declares: functions with their prototypes, then data symbols.
FUNCTIONS = {
    "spmv_create_handle_all_in_one": (None, [C.POINTER(spmv_Handle_t), C.c_int, C.c_int, _V, _V, _V,
                                             C.c_ulong, C.c_int, C.c_ulong, C.c_int, C.c_char_p]),
    "spmv": (None, [spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V]),
    "spmv_destory_handle": (None, [spmv_Handle_t]),
    "spmv_clear_handle": (None, [spmv_Handle_t]),
    "spmv_hip_last_error": (C.c_int, []),
    "spmv_hip_last_error_string": (C.c_char_p, []),
    "spmv_hip_clear_error": (None, []),
    "spmv_hip_device_count": (C.c_int, []),
    "spmv_hip_trim_pool": (None, []),
    "spmv_hip_set_stream": (C.c_int, [spmv_Handle_t, _V]),
    "spmv_hip_set_async": (C.c_int, [spmv_Handle_t, C.c_int]),
    "spmv_hip_synchronize": (C.c_int, [spmv_Handle_t]),
    "spmv_hip_set_option": (C.c_int, [C.c_char_p, C.c_long]),
    "spmv_hip_get_option": (C.c_long, [C.c_char_p]),
    "spmv_hip_set_thread_option": (C.c_int, [C.c_char_p, C.c_long]),
    "spmv_hip_clear_thread_options": (None, []),
    "spmv_hip_get_handle_option": (C.c_long, [spmv_Handle_t, C.c_char_p]),
    "spmv_hip_update_values": (C.c_int, [spmv_Handle_t, _V]),
    "spmv_hip_multi_gpus": (C.c_int, [spmv_Handle_t]),
    "spmv_hip_multi_uses_rccl": (C.c_int, [spmv_Handle_t]),
    "spmv_hip_multi_slices": (C.c_int, [spmv_Handle_t, C.c_int, C.POINTER(_V), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                        C.POINTER(_V), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _I]),
    "spmv_hip_multi_step": (C.c_int, [spmv_Handle_t]),
    "spmv_hip_multi_step_async": (C.c_int, [spmv_Handle_t]),
    "spmv_hip_multi_synchronize": (C.c_int, [spmv_Handle_t]),
    "spmv_hip_create_handle_from_blocks": (None, [C.POINTER(spmv_Handle_t), C.c_int, _I, C.c_int, C.POINTER(_V), C.POINTER(_V), C.POINTER(_V),
                                                  C.c_int, C.c_ulong]),
    "spmv_hip_get_info": (C.c_int, [spmv_Handle_t, C.POINTER(spmv_hip_info)]),
    "spmv_hip_time_launches": (C.c_double, [spmv_Handle_t, _V, _V, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "spmv_hip_spmm": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, C.c_int, _V, C.c_longlong, _V, C.c_longlong]),
    "spmv_hip_time_spmm_launches": (C.c_double, [spmv_Handle_t, C.c_int, _V, C.c_longlong, _V, C.c_longlong, C.c_int, C.c_int,
                                                 C.POINTER(C.c_float)]),
    "spmv_hip_spmv_transpose": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V]),
    "spmv_hip_prepare_transpose": (C.c_int, [spmv_Handle_t]),
    "spmv_hip_get_transpose_info": (C.c_int, [spmv_Handle_t, C.POINTER(spmv_hip_info)]),
    "spmv_hip_time_transpose_launches": (C.c_double, [spmv_Handle_t, _V, _V, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "spmv_hip_transpose_map": (C.c_int, [spmv_Handle_t, _I, _I]),
    "spmv_hip_spmm_transpose": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, C.c_int, _V, C.c_longlong, _V, C.c_longlong]),
    "spmv_hip_time_spmm_transpose_launches": (C.c_double, [spmv_Handle_t, C.c_int, _V, C.c_longlong, _V, C.c_longlong, C.c_int, C.c_int,
                                                           C.POINTER(C.c_float)]),
    "spmv_hip_sddmm": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, C.c_int, _V, C.c_longlong, _V, C.c_longlong, _V]),
    "spmv_hip_time_sddmm_launches": (C.c_double, [spmv_Handle_t, C.c_int, _V, C.c_longlong, _V, C.c_longlong, _V, C.c_int, C.c_int,
                                                  C.POINTER(C.c_float)]),
    "spmv_hip_row_softmax": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V]),
    "spmv_hip_row_softmax_backward": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V, _V]),
    "spmv_hip_time_row_softmax_launches": (C.c_double, [spmv_Handle_t, _V, _V, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    **_attention_prototypes(),   # the fused attention: a call and its timer per row of _ATTENTION
    "spmv_hip_attention_merge": (C.c_int, [spmv_Handle_t, C.c_int, C.c_int, _V, C.c_longlong, _V, C.c_longlong, _V, C.c_longlong, _V, C.c_longlong,
                                           _V, C.c_longlong, _V, C.c_longlong]),
    "spmv_hip_time_attention_merge_launches": (C.c_double, [spmv_Handle_t, C.c_int, C.c_int, _V, C.c_longlong, _V, C.c_longlong, _V, C.c_longlong, _V, C.c_longlong,
                                                            _V, C.c_longlong, _V, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "spmv_hip_cg": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V, C.POINTER(spmv_hip_cg_options), C.POINTER(spmv_hip_cg_result)]),
    "spmv_hip_time_cg_iterations": (C.c_double, [spmv_Handle_t, _V, _V, C.POINTER(spmv_hip_cg_options), C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "spmv_hip_bicgstab": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V, C.POINTER(spmv_hip_cg_options), C.POINTER(spmv_hip_cg_result)]),
    "spmv_hip_time_bicgstab_iterations": (C.c_double, [spmv_Handle_t, _V, _V, C.POINTER(spmv_hip_cg_options), C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "spmv_hip_gmres": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V, C.c_int, C.POINTER(spmv_hip_cg_options), C.POINTER(spmv_hip_cg_result)]),
    "spmv_hip_time_gmres_iterations": (C.c_double, [spmv_Handle_t, _V, _V, C.c_int, C.POINTER(spmv_hip_cg_options), C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "spmv_hip_gmres_device_sqrt": (C.c_int, [_V, _V, C.c_longlong]),
    "spmv_hip_cg_columns": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, C.c_int, _V, C.c_longlong, _V, C.c_longlong, C.POINTER(spmv_hip_cg_options),
                                      C.POINTER(spmv_hip_cg_result)]),
    "spmv_hip_time_cg_columns_iterations": (C.c_double, [spmv_Handle_t, C.c_int, _V, C.c_longlong, _V, C.c_longlong, C.POINTER(spmv_hip_cg_options), C.c_int, C.c_int,
                                                         C.POINTER(C.c_float)]),
    "spmv_hip_cg_mixed": (C.c_int, [spmv_Handle_t, spmv_Handle_t, _V, _V, C.POINTER(spmv_hip_cg_mixed_options), C.POINTER(spmv_hip_cg_mixed_result)]),
    "spmv_hip_time_cg_mixed_iterations": (C.c_double, [spmv_Handle_t, spmv_Handle_t, _V, _V, C.POINTER(spmv_hip_cg_mixed_options), C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "spmv_hip_lsqr": (C.c_int, [spmv_Handle_t, C.c_int, _V, _V, _V, _V, _V, C.POINTER(spmv_hip_lsqr_options), C.POINTER(spmv_hip_lsqr_result)]),
    "spmv_hip_time_lsqr_iterations": (C.c_double, [spmv_Handle_t, _V, _V, C.POINTER(spmv_hip_lsqr_options), C.c_int, C.c_int, C.POINTER(C.c_float)]),
    # include/spmv_io.h (host only)
    "spmv_io_read_mtx": (C.c_int, [C.c_char_p, C.c_size_t, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_V)]),
    "spmv_io_cache_path": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t]),
    "spmv_io_write_bin": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, _V, _V, _V, C.c_size_t]),
    "spmv_io_read_bin": (C.c_int, [C.c_char_p, C.c_size_t, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_V)]),
    "spmv_io_load": (C.c_int, [C.c_char_p, C.c_size_t, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_V), _I]),
    "spmv_io_free": (None, [_V]),
}
DATA_SYMBOLS = ("Methods_names", "Vectorized_names", "funcNames", "Dot_s_Products", "Dot_d_Products")

_lib = None


def load():
    """dlopen libspmv_hip.so (building it is spmv_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: run `python -m spmv_amd.build` "
                               "(there is no CPU fallback for the HIP library)")
        try:  # make sure one HIP runtime serves torch and this library (same SONAME)
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for pure-numpy callers
            pass
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in FUNCTIONS.items():
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
        _lib = lib
    return _lib


def methods_names():
    lib = load()
    arr = (C.c_char_p * int(SPMV_METHODS.Method_Total_Size)).in_dll(lib, "Methods_names")
    return [s.decode() for s in arr]


def vectorized_names():
    lib = load()
    arr = (C.c_char_p * int(VECTORIZED_WAY.VECTOR_TOTAL_SIZE)).in_dll(lib, "Vectorized_names")
    return [s.decode() for s in arr]


class SpmvError(RuntimeError):
    pass


def last_error():
    lib = load()
    return lib.spmv_hip_last_error(), lib.spmv_hip_last_error_string().decode()


def _raise_if_error(where):
    code, text = last_error()
    if code:
        load().spmv_hip_clear_error()
        raise SpmvError(f"{where}: [{code}] {text}")


def _checked(rc, symbol, check=True):
    """-> rc, the return code of the C function `symbol`; a failure is raised when `check` is set."""
    if check and rc != 0:
        _raise_if_error(symbol)
    return rc


def _timed(symbol, args, warmup, iters):
    """-> (mean_ms, per-launch ms array) of the timing entry point `symbol`: hipEvents on the handle's stream around each launch."""
    ms = (C.c_float * iters)()
    mean = getattr(load(), symbol)(*args, warmup, iters, ms)
    if mean < 0:
        _raise_if_error(symbol)
    return mean, np.frombuffer(ms, dtype=np.float32).copy()


def _ptr(a):
    """Raw address of a numpy array / torch tensor / None / int."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be contiguous")
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        if not a.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return a.data_ptr()
    raise TypeError(type(a))


def _itemsize(a):
    return a.dtype.itemsize if isinstance(a, np.ndarray) else a.element_size()


# ----------------------------------------------------------------------------- the four functions
def spmv_create_handle_all_in_one(m, n, RowPtr, ColIdx, Matrix_Val, nthreads, Function, size,
                                  vectorizedWay=VECTORIZED_WAY.VECTOR_HIP, MtxToken=None, check=True):
    """-> spmv_Handle_t.  Same arguments as the C function; the handle is the return value instead
    of an out-parameter.  The arrays must stay alive as long as spmv() is called with them."""
    lib = load()
    lib.spmv_hip_clear_error()
    h = spmv_Handle_t()
    tok = MtxToken.encode() if isinstance(MtxToken, str) else MtxToken
    lib.spmv_create_handle_all_in_one(C.byref(h), int(m), int(n), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val),
                                      int(nthreads), int(Function), int(size), int(vectorizedWay), tok)
    if check:
        _raise_if_error("spmv_create_handle_all_in_one")
    return h


def spmv(handle, m, RowPtr, ColIdx, Matrix_Val, Vector_Val_X, Vector_Val_Y, check=True):
    lib = load()
    lib.spmv(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), _ptr(Vector_Val_X), _ptr(Vector_Val_Y))
    if check:
        _raise_if_error("spmv")


def spmv_destory_handle(handle):
    load().spmv_destory_handle(handle)


def spmv_clear_handle(handle):
    load().spmv_clear_handle(handle)


# ----------------------------------------------------------------------------- extensions
def set_option(key, value):
    if load().spmv_hip_set_option(key.encode(), int(value)) != 0:
        load().spmv_hip_clear_error()
        raise ValueError(f"bad option {key}={value}")


def get_option(key):
    return load().spmv_hip_get_option(key.encode())


def set_thread_option(key, value):
    """Override for handles created by the calling thread (spmv_hip_set_thread_option)."""
    if load().spmv_hip_set_thread_option(key.encode(), int(value)) != 0:
        load().spmv_hip_clear_error()
        raise ValueError(f"bad option {key}={value}")


def clear_thread_options():
    load().spmv_hip_clear_thread_options()


def update_values(handle, Matrix_Val):
    """New values behind the same pattern (spmv_hip_update_values): no re-inspection."""
    _checked(load().spmv_hip_update_values(handle, _ptr(Matrix_Val)), "spmv_hip_update_values")


def _info_dict(info):
    out = {k: getattr(info, k) for k, _ in spmv_hip_info._fields_}
    out["schedule_name"] = (out["schedule_name"] or b"").decode()
    out["kernel_name"] = (out["kernel_name"] or b"").decode()
    out["launch_kernels"] = [k for k in (out["launch_kernels"] or b"").decode().split("+") if k]
    out["tune_ms"] = [float(v) for v in out["tune_ms"]]
    out["route_ms"] = [float(v) for v in out["route_ms"]]
    out["split_ms"] = [float(v) for v in out["split_ms"]]
    out["pack_ms"] = [float(v) for v in out["pack_ms"]]
    return out


def get_info(handle):
    info = spmv_hip_info()
    _checked(load().spmv_hip_get_info(handle, C.byref(info)), "spmv_hip_get_info")
    return _info_dict(info)


def get_transpose_info(handle):
    """spmv_hip_get_transpose_info as a dict shaped like get_info's: the schedule of A^T (raises until the transpose is built)."""
    info = spmv_hip_info()
    _checked(load().spmv_hip_get_transpose_info(handle, C.byref(info)), "spmv_hip_get_transpose_info")
    return _info_dict(info)


def set_stream(handle, stream_ptr, async_=True):
    lib = load()
    lib.spmv_hip_set_stream(handle, stream_ptr)
    lib.spmv_hip_set_async(handle, 1 if async_ else 0)
    _raise_if_error("spmv_hip_set_stream")


def time_launches(handle, x, y, warmup=10, iters=100):
    """-> (mean_ms, per-launch ms array): hipEvents on the handle's stream around each launch."""
    return _timed("spmv_hip_time_launches", (handle, _ptr(x), _ptr(y)), warmup, iters)


def _block(a, name):
    """(address, rows, k, ld) of a 2-D numpy array / torch tensor whose column stride is 1 (the row stride is its leading dimension)."""
    if a is None:
        return None, 0, 0, 0
    if isinstance(a, np.ndarray):
        if a.ndim == 2 and a.size == 0:
            return a.ctypes.data, a.shape[0], a.shape[1], max(a.shape[1], 1)
        if a.ndim != 2 or (a.strides[1] != a.itemsize and a.shape[1] > 1) or a.strides[0] % a.itemsize:
            raise ValueError(f"{name} must be 2-D with column stride 1")
        return a.ctypes.data, a.shape[0], a.shape[1], a.strides[0] // a.itemsize
    if hasattr(a, "data_ptr"):
        if a.dim() != 2 or (a.stride(1) != 1 and a.shape[1] > 1):
            raise ValueError(f"{name} must be 2-D with column stride 1")
        return a.data_ptr(), a.shape[0], a.shape[1], a.stride(0)
    raise TypeError(type(a))


def _blocks(A, a_name, B, b_name):
    """-> (k, address of A, ld of A, address of B, ld of B) for two 2-D blocks of k columns each (_block); a block that is None has a NULL
    address, k is the other block's and its ld is k."""
    pa, _, k, lda = _block(A, a_name)
    pb, _, kb, ldb = _block(B, b_name)
    if A is not None and B is not None and kb != k:
        raise ValueError(f"{a_name} has {k} columns, {b_name} {kb}")
    if A is None:
        k = kb
    return int(k), pa, int(max(lda, 1) if A is not None else k), pb, int(max(ldb, 1) if B is not None else k)


def spmm(handle, m, RowPtr, ColIdx, Matrix_Val, X, Y, check=True):
    """Y = A X for the k columns of X (spmv_hip_spmm).  X (n x k) and Y (m x k): 2-D numpy arrays or torch tensors with column
    stride 1; their row strides are passed as ldx / ldy, so views into wider arrays work.  -> the return code (0 on success)."""
    k, px, ldx, py, ldy = _blocks(X, "X", Y, "Y")
    return _checked(load().spmv_hip_spmm(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), k, px, ldx, py, ldy), "spmv_hip_spmm", check)


def time_spmm_launches(handle, X, Y, warmup=10, iters=100):
    """-> (mean_ms, per-launch ms array) of spmv_hip_spmm on device X / Y (spmv_hip_time_spmm_launches)."""
    px, _, k, ldx = _block(X, "X")
    py, _, _, ldy = _block(Y, "Y")
    return _timed("spmv_hip_time_spmm_launches", (handle, int(k), px, int(max(ldx, 1)), py, int(max(ldy, 1))), warmup, iters)


def spmv_transpose(handle, m, RowPtr, ColIdx, Matrix_Val, X, Y, check=True):
    """y = A^T x (spmv_hip_spmv_transpose): X has m entries, Y n.  -> the return code (0 on success)."""
    return _checked(load().spmv_hip_spmv_transpose(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), _ptr(X), _ptr(Y)), "spmv_hip_spmv_transpose", check)


def prepare_transpose(handle, check=True):
    """Build (and plan) A^T now rather than at the first spmv_transpose (spmv_hip_prepare_transpose)."""
    return _checked(load().spmv_hip_prepare_transpose(handle), "spmv_hip_prepare_transpose", check)


def time_transpose_launches(handle, x, y, warmup=10, iters=100):
    """-> (mean_ms, per-launch ms array) of y = A^T x on device x / y (spmv_hip_time_transpose_launches)."""
    return _timed("spmv_hip_time_transpose_launches", (handle, _ptr(x), _ptr(y)), warmup, iters)


def transpose_map(handle, n, nnz):
    """-> (rowptr_T, perm) of the built transpose as int32 numpy arrays (n + 1 and nnz entries; spmv_hip_transpose_map)."""
    rp = np.empty(int(n) + 1, dtype=np.int32)
    perm = np.empty(max(int(nnz), 1), dtype=np.int32)
    _checked(load().spmv_hip_transpose_map(handle, rp.ctypes.data_as(_I), perm.ctypes.data_as(_I)), "spmv_hip_transpose_map")
    return rp, perm[:int(nnz)]


def spmm_transpose(handle, m, RowPtr, ColIdx, Matrix_Val, X, Y, check=True):
    """Y = A^T X for the k columns of X (spmv_hip_spmm_transpose).  X (m x k) and Y (n x k): 2-D numpy arrays or torch tensors with column
    stride 1; their row strides are passed as ldx / ldy.  -> the return code (0 on success)."""
    k, px, ldx, py, ldy = _blocks(X, "X", Y, "Y")
    return _checked(load().spmv_hip_spmm_transpose(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), k, px, ldx, py, ldy), "spmv_hip_spmm_transpose", check)


def time_spmm_transpose_launches(handle, X, Y, warmup=10, iters=100):
    """-> (mean_ms, per-launch ms array) of spmv_hip_spmm_transpose on device X / Y (spmv_hip_time_spmm_transpose_launches)."""
    px, _, k, ldx = _block(X, "X")
    py, _, _, ldy = _block(Y, "Y")
    return _timed("spmv_hip_time_spmm_transpose_launches", (handle, int(k), px, int(max(ldx, 1)), py, int(max(ldy, 1))), warmup, iters)


def sddmm(handle, m, RowPtr, ColIdx, Matrix_Val, U, V, Out, check=True):
    """Out[p] = sum_c U[row(p), c] * V[col(p), c] over the handle's pattern (spmv_hip_sddmm).  U (m x k) and V (n x k): 2-D numpy arrays or
    torch tensors with column stride 1 (row strides are passed as ldu / ldv); Out: nnz contiguous elements.  -> the return code."""
    k, pu, ldu, pv, ldv = _blocks(U, "U", V, "V")
    return _checked(load().spmv_hip_sddmm(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), k, pu, ldu, pv, ldv, _ptr(Out)), "spmv_hip_sddmm", check)


def time_sddmm_launches(handle, U, V, Out, warmup=10, iters=100):
    """-> (mean_ms, per-launch ms array) of spmv_hip_sddmm on device U / V / Out (spmv_hip_time_sddmm_launches)."""
    pu, _, k, ldu = _block(U, "U")
    pv, _, _, ldv = _block(V, "V")
    return _timed("spmv_hip_time_sddmm_launches", (handle, int(k), pu, int(max(ldu, 1)), pv, int(max(ldv, 1)), _ptr(Out)), warmup, iters)


def row_softmax(handle, m, RowPtr, ColIdx, Matrix_Val, S, Out, check=True):
    """Out[p] = exp(S[p] - max_row) / sum_row over every row of the handle's pattern (spmv_hip_row_softmax).  S and Out: nnz contiguous elements
    in CSR order (numpy arrays or torch tensors); Out may be S.  -> the return code."""
    return _checked(load().spmv_hip_row_softmax(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), _ptr(S), _ptr(Out)), "spmv_hip_row_softmax", check)


def row_softmax_backward(handle, m, RowPtr, ColIdx, Matrix_Val, P, G, Out, check=True):
    """Out[p] = P[p] * (G[p] - sum over the row of P * G): dL/dS from P = row_softmax(S) and G = dL/dP (spmv_hip_row_softmax_backward).  Out may
    be G.  -> the return code."""
    return _checked(load().spmv_hip_row_softmax_backward(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), _ptr(P), _ptr(G), _ptr(Out)),
                    "spmv_hip_row_softmax_backward", check)


def time_row_softmax_launches(handle, S, Out, warmup=10, iters=100):
    """-> (mean_ms, per-launch ms array) of spmv_hip_row_softmax on device S / Out (spmv_hip_time_row_softmax_launches)."""
    return _timed("spmv_hip_time_row_softmax_launches", (handle, _ptr(S), _ptr(Out)), warmup, iters)


def _planes(a, name, heads, shared_ok):
    """-> (address, ld) of bias planes: None -> (None, 0); a 1-D array / tensor of nnz elements is ONE plane for all heads (ld 0, only where
    `shared_ok`); a 2-D one of (heads, nnz) with column stride 1 has a plane per head, its row stride as ld."""
    if a is None:
        return None, 0
    if len(a.shape) == 1:
        if not shared_ok and int(heads) != 1:
            raise ValueError(f"{name} must be 2-D, (heads, nnz)")
        p, _, _, _ = _block(a.reshape(1, -1), name)
        return p, (0 if shared_ok else int(a.shape[0]))
    if len(a.shape) != 2 or a.shape[0] != int(heads):
        raise ValueError(f"{name} must be (nnz,) or ({int(heads)}, nnz), not {tuple(a.shape)}")
    p, _, w, ld = _block(a, name)
    return p, int(max(ld, w, 1))


def _lse_planes(a, name, heads):
    """-> (address, ld) of log-sum-exp planes: None -> (None, 0); a 2-D array / tensor of (heads, >= m) with column stride 1, its row stride as ld
    (a 1-D one is the one plane of heads = 1)"""
    if a is None:
        return None, 0
    if len(a.shape) == 1:
        a = a.reshape(1, -1)
    if len(a.shape) != 2 or a.shape[0] != int(heads):
        raise ValueError(f"{name} must be ({int(heads)}, m), not {tuple(a.shape)}")
    p, _, w, ld = _block(a, name)
    return p, int(max(ld, w, 1))


def _gqa_widths(heads, kv_heads, wq, wkk, wv, wo, o_name):
    """-> (k, dv) of ONE head from the column counts of Q, K, V and O / G: Q and O / G hold `heads` blocks, K and V `kv_heads`"""
    if heads < 1 or kv_heads < 1 or heads % kv_heads:
        raise ValueError(f"heads = {heads} is not a multiple of kv_heads = {kv_heads}")
    if wq % heads or wo % heads or wkk % kv_heads or wv % kv_heads or wq // heads != wkk // kv_heads or wo // heads != wv // kv_heads:
        raise ValueError(f"Q has {wq} columns, K {wkk}, V {wv} and {o_name} {wo}: not {heads} query heads over {kv_heads} K / V heads of equal widths")
    return wq // heads, wo // heads


def _operand(a, name, width, optional=True):
    """-> (address, ld) of a 2-D block that must have `width` columns; None -- an output that is not wanted, or an input the call can do
    without -- is a NULL address with the width as ld"""
    if a is None:
        if width and not optional:
            raise ValueError(f"{name} has 0 columns, expected {width}")
        return None, int(width)
    p, _, w, ld = _block(a, name)
    if w != width:
        raise ValueError(f"{name} has {w} columns, expected {width}")
    return p, int(max(ld, 1))


T_HANDLE, T_F16, T_BF16 = 0, 1, 2   # include/spmv_hip.h: SPMV_HIP_T_*


def _types_16(handle, ops):
    """-> the SPMV_HIP_T_* codes of a 16-bit call, by their names in the prototype, from the operands' dtypes.  Q, K and V -- and G, where
    there is one -- are torch tensors (CPU or device), all torch.float16 or all torch.bfloat16; an output -- O of the forward, dQ, dK and dV --
    has that dtype or torch.float32, the handle's; dK and dV, where both are given, share one.  The backward also wants a float32 handle (the
    forward leaves a float64 one to the library, which answers E_ARG), float32 B, dB, O and L, and O and L together or not at all."""
    import torch
    codes = {torch.float16: T_F16, torch.bfloat16: T_BF16}
    backward = "G" in ops
    ins = ("Q", "K", "V", "G") if backward else ("Q", "K", "V")
    for name in ins if backward else (*ins, "O"):
        if not isinstance(ops[name], torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor (numpy has no bfloat16), not {type(ops[name]).__name__}")
    dtype = ops["Q"].dtype
    if dtype not in codes or any(ops[name].dtype != dtype for name in ins):
        raise TypeError(f"{', '.join(ins)} must all be torch.float16 or all torch.bfloat16, not {', '.join(str(ops[name].dtype) for name in ins)}")

    def code(name):   # of an output; one that is not wanted (None) gets the inputs' code, which is never looked at
        t = ops[name]
        if t is not None and (not isinstance(t, torch.Tensor) or (t.dtype != dtype and t.dtype != torch.float32)):
            raise TypeError(f"{name} must be a torch.Tensor of {dtype} or torch.float32")
        return (T_HANDLE,) if t is not None and t.dtype == torch.float32 else (codes[dtype],)
    if not backward:
        return {"io_type": (codes[dtype],), "o_type": code("O")}
    if handle and handle.contents.data_size == 8:   # the public handle's own field: no device call
        raise TypeError("16-bit Q, K, V and G need a float32 handle, not a float64 one")
    dq, dk, dv = code("dQ"), code("dK"), code("dV")
    if ops["dK"] is not None and ops["dV"] is not None and ops["dK"].dtype != ops["dV"].dtype:
        raise TypeError(f"dK and dV share one type, not {ops['dK'].dtype} and {ops['dV'].dtype}")
    for name in ("B", "dB", "O", "L"):
        if isinstance(ops[name], torch.Tensor) and ops[name].dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, not {ops[name].dtype}")
    if (ops["O"] is None) != (ops["L"] is None):
        raise ValueError("O and L are given together (the backward driven by them) or not at all")
    return {"io_type": (codes[dtype],), "dq_type": dq, "dkv_type": dv if ops["dK"] is None else dk}


def _attention_args(stem, handle, heads, kv_heads, scale, ops, ldb=None, lddb=None, ldl=None):
    """-> the arguments of spmv_hip_<stem> and of its timer from the sizes on, in the order of the row _ATTENTION[stem]: the one marshaller of
    the family, every rule of which is written once, here.  ops: the row's operands by name -- numpy arrays, torch tensors or None --; heads: 1
    on the rungs that have none; kv_heads: None on the rungs that have none, where it is `heads`; ldb / lddb / ldl: plane strides that replace
    what B, dB and L give (flat buffers holding padded planes).  Everything is checked here, before any device call."""
    row = _ATTENTION[stem]
    heads, grouped = int(heads), kv_heads is not None
    kv_heads = int(kv_heads) if grouped else heads
    rec = {"heads": (heads,), "kv_heads": (kv_heads,)}   # name -> what the prototype has under that name, as a tuple
    if "io_type" in row:
        rec.update(_types_16(handle, ops))
    # the four blocks of every rung: Q holds `heads` heads of k columns and K `kv_heads`; V holds `kv_heads` heads of dv columns and the query
    # side -- O of a forward, G of a backward -- `heads`
    side = "G" if "G" in ops else "O"
    Q, K, V, S = ops["Q"], ops["K"], ops["V"], ops[side]
    (pq, _, wq, ldq), (pk, _, wk, ldk), (pv, _, wv, ldv), (ps, _, ws, lds) = _block(Q, "Q"), _block(K, "K"), _block(V, "V"), _block(S, side)
    if not grouped:   # before kv_heads, a block that is None has its partner's width and the NULL is the library's to refuse (as in _blocks)
        wq, wk = (wk if Q is None else wq), (wq if K is None else wk)
        wv, ws = (ws if V is None else wv), (wv if S is None else ws)
    k, dv = _gqa_widths(heads, kv_heads, wq, wk, wv, ws, side)
    rec["Q"], rec["K"] = (pq, wq if Q is None else max(ldq, 1)), (pk, wk if K is None else max(ldk, 1))   # None: NULL with its width as ld
    rec["V"], rec[side] = (pv, wv if V is None else max(ldv, 1)), (ps, ws if S is None else max(lds, 1))
    rec["k"], rec["dv"] = (k,), (dv,)
    # scale None is 1 / sqrt(k) in double: math.sqrt and numpy's sqrt are both the correctly rounded root, so the bits are those of either; 0
    # stands beside a k that the library refuses before it reads scale
    rec["scale"] = ((1.0 / math.sqrt(k) if k > 0 else 0.0) if scale is None else float(scale),)
    for name, width in (("dQ", wq), ("dK", wk), ("dV", wv)):
        if name in ops:
            rec[name] = _operand(ops[name], name, width)
    if side == "G" and "O" in ops:   # the final output that drives a backward: only the 16-bit call can do without it (and without L, _types_16)
        rec["O"] = _operand(ops["O"], "O", heads * dv, optional="io_type" in row)
    if "B" in ops:
        rec["B"] = (_ptr(ops["B"]), int(ldb)) if ldb is not None else _planes(ops["B"], "B", heads, True)
    if "dB" in ops:
        rec["dB"] = (_ptr(ops["dB"]), int(lddb)) if lddb is not None else _planes(ops["dB"], "dB", heads, False)
    if "L" in ops:
        rec["L"] = (_ptr(ops["L"]), int(ldl)) if ldl is not None else _lse_planes(ops["L"], "L", heads)
    return [x for name in row for x in rec[name]]


def _attention_call(stem, handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, scale, check, ops, **ld):
    """spmv_hip_<stem> on the named operands `ops` (_attention_args) -> the return code; a failure is raised when `check` is set"""
    args = _attention_args(stem, handle, heads, kv_heads, scale, ops, **ld)
    return _checked(getattr(load(), "spmv_hip_" + stem)(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), *args), "spmv_hip_" + stem, check)


def _attention_time(stem, handle, heads, kv_heads, scale, warmup, iters, ops):
    """-> (mean_ms, per-call ms array) of spmv_hip_<stem> on the named device operands `ops`: spmv_hip_time_<stem>_launches"""
    return _timed(f"spmv_hip_time_{stem}_launches", (handle, *_attention_args(stem, handle, heads, kv_heads, scale, ops)), warmup, iters)


def attention(handle, m, RowPtr, ColIdx, Matrix_Val, Q, K, V, O, scale=None, check=True):
    """O = softmax_rows(scale * Q K^T on the handle's pattern) V in one pass (spmv_hip_attention).  Q (m x k), K (n x k), V (n x dv) and O
    (m x dv): 2-D numpy arrays or torch tensors with column stride 1 (row strides are passed as leading dimensions); scale None means
    1 / sqrt(k).  The handle's values are neither read nor changed.  -> the return code."""
    return _attention_call("attention", handle, m, RowPtr, ColIdx, Matrix_Val, 1, None, scale, check, dict(Q=Q, K=K, V=V, O=O))


def time_attention_launches(handle, Q, K, V, O, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention on device Q / K / V / O (spmv_hip_time_attention_launches)."""
    return _attention_time("attention", handle, 1, None, scale, warmup, iters, dict(Q=Q, K=K, V=V, O=O))


def attention_heads(handle, m, RowPtr, ColIdx, Matrix_Val, heads, Q, K, V, O, scale=None, check=True):
    """`heads` attention heads over the handle's pattern in one pass (spmv_hip_attention_heads).  Q (m x heads*k), K (n x heads*k),
    V (n x heads*dv) and O (m x heads*dv) hold the heads side by side -- the (rows, heads, k) layout --: 2-D numpy arrays or torch tensors with
    column stride 1 (row strides are passed as leading dimensions); head h of O has the bits of attention() on the h-th column slices.  scale
    None means 1 / sqrt(k) with k ONE head's width.  The handle's values are neither read nor changed.  -> the return code."""
    return _attention_call("attention_heads", handle, m, RowPtr, ColIdx, Matrix_Val, heads, None, scale, check, dict(Q=Q, K=K, V=V, O=O))


def time_attention_heads_launches(handle, heads, Q, K, V, O, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_heads on device Q / K / V / O (spmv_hip_time_attention_heads_launches)."""
    return _attention_time("attention_heads", handle, heads, None, scale, warmup, iters, dict(Q=Q, K=K, V=V, O=O))


def attention_backward(handle, m, RowPtr, ColIdx, Matrix_Val, Q, K, V, G, dQ=None, dK=None, dV=None, scale=None, check=True):
    """dQ, dK, dV of O = softmax_rows(scale * Q K^T on the handle's pattern) V from G = dL/dO in two passes over A
    (spmv_hip_attention_backward).  Q (m x k), K (n x k), V (n x dv), G (m x dv) and the outputs dQ (m x k), dK (n x k), dV (n x dv): 2-D numpy
    arrays or torch tensors with column stride 1 (row strides are passed as leading dimensions); an output that is None is not computed; scale
    None means 1 / sqrt(k).  The handle's values are neither read nor changed.  -> the return code."""
    return _attention_call("attention_backward", handle, m, RowPtr, ColIdx, Matrix_Val, 1, None, scale, check, dict(Q=Q, K=K, V=V, G=G, dQ=dQ, dK=dK, dV=dV))


def time_attention_backward_launches(handle, Q, K, V, G, dQ=None, dK=None, dV=None, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_backward on device operands (spmv_hip_time_attention_backward_launches)."""
    return _attention_time("attention_backward", handle, 1, None, scale, warmup, iters, dict(Q=Q, K=K, V=V, G=G, dQ=dQ, dK=dK, dV=dV))


def attention_heads_backward(handle, m, RowPtr, ColIdx, Matrix_Val, heads, Q, K, V, G, dQ=None, dK=None, dV=None, scale=None, check=True):
    """dQ, dK, dV of attention_heads(Q, K, V) from G = dL/dO, all heads in two passes per group of heads (spmv_hip_attention_heads_backward).
    Q, dQ (m x heads*k), K, dK (n x heads*k), V, dV (n x heads*dv) and G (m x heads*dv) hold the heads side by side: 2-D numpy arrays or torch
    tensors with column stride 1 (row strides are passed as leading dimensions); an output that is None is not computed; head h of every output
    has the bits of attention_backward() on the h-th column slices.  scale None means 1 / sqrt(k) with k ONE head's width.  The handle's
    values are neither read nor changed.  -> the return code."""
    return _attention_call("attention_heads_backward", handle, m, RowPtr, ColIdx, Matrix_Val, heads, None, scale, check, dict(Q=Q, K=K, V=V, G=G, dQ=dQ, dK=dK, dV=dV))


def time_attention_heads_backward_launches(handle, heads, Q, K, V, G, dQ=None, dK=None, dV=None, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_heads_backward on device operands (spmv_hip_time_attention_heads_backward_launches)."""
    return _attention_time("attention_heads_backward", handle, heads, None, scale, warmup, iters, dict(Q=Q, K=K, V=V, G=G, dQ=dQ, dK=dK, dV=dV))


def attention_bias(handle, m, RowPtr, ColIdx, Matrix_Val, heads, Q, K, V, B, O, scale=None, check=True, ldb=None):
    """attention_heads() with the additive bias B on the scaled scores (spmv_hip_attention_bias): t = (s * scale) + B.  B: None (then this IS
    attention_heads), an (nnz,) array / tensor -- one plane shared by all heads -- or (heads, nnz) -- a plane per head, any row stride --, in
    CSR order; ldb overrides the plane stride derived from B (for flat buffers holding padded planes).  -> the return code."""
    return _attention_call("attention_bias", handle, m, RowPtr, ColIdx, Matrix_Val, heads, None, scale, check, dict(Q=Q, K=K, V=V, B=B, O=O), ldb=ldb)


def time_attention_bias_launches(handle, heads, Q, K, V, B, O, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_bias on device operands (spmv_hip_time_attention_bias_launches)."""
    return _attention_time("attention_bias", handle, heads, None, scale, warmup, iters, dict(Q=Q, K=K, V=V, B=B, O=O))


def attention_bias_backward(handle, m, RowPtr, ColIdx, Matrix_Val, heads, Q, K, V, B, G, dQ=None, dK=None, dV=None, dB=None, scale=None, check=True,
                            ldb=None, lddb=None):
    """dQ, dK, dV and dB of attention_bias(Q, K, V, B) from G = dL/dO (spmv_hip_attention_bias_backward).  B as in attention_bias(); dB: None
    (not wanted) or (heads, nnz) -- always a plane per head, dB[h, p] = P (dP - D) of head h --; the other operands as in
    attention_heads_backward(); ldb / lddb override the plane strides.  With B None, dQ, dK and dV are attention_heads_backward()'s to the
    bit.  -> the return code."""
    return _attention_call("attention_bias_backward", handle, m, RowPtr, ColIdx, Matrix_Val, heads, None, scale, check,
                           dict(Q=Q, K=K, V=V, B=B, G=G, dQ=dQ, dK=dK, dV=dV, dB=dB), ldb=ldb, lddb=lddb)


def time_attention_bias_backward_launches(handle, heads, Q, K, V, B, G, dQ=None, dK=None, dV=None, dB=None, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_bias_backward on device operands (spmv_hip_time_attention_bias_backward_launches)."""
    return _attention_time("attention_bias_backward", handle, heads, None, scale, warmup, iters, dict(Q=Q, K=K, V=V, B=B, G=G, dQ=dQ, dK=dK, dV=dV, dB=dB))


def attention_gqa(handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, Q, K, V, B, O, scale=None, check=True, ldb=None):
    """attention_bias() with `kv_heads` K / V heads for `heads` query heads (spmv_hip_attention_gqa; grouped-query attention, kv_heads = 1:
    multi-query).  Q (m x heads*k) and O (m x heads*dv) as there; K is (n x kv_heads*k) and V (n x kv_heads*dv); query head h uses K / V head
    h // (heads // kv_heads), the grouping of repeat_interleave, and has the bits of the single-head call on those slices.  B: None, (nnz,) or
    (heads, nnz) -- per QUERY head.  kv_heads = heads is attention_bias().  -> the return code."""
    return _attention_call("attention_gqa", handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, scale, check, dict(Q=Q, K=K, V=V, B=B, O=O), ldb=ldb)


def time_attention_gqa_launches(handle, heads, kv_heads, Q, K, V, B, O, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_gqa on device operands (spmv_hip_time_attention_gqa_launches)."""
    return _attention_time("attention_gqa", handle, heads, kv_heads, scale, warmup, iters, dict(Q=Q, K=K, V=V, B=B, O=O))


def attention_gqa_backward(handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, Q, K, V, B, G, dQ=None, dK=None, dV=None, dB=None, scale=None, check=True,
                           ldb=None, lddb=None):
    """dQ, dK, dV and dB of attention_gqa(Q, K, V, B) from G = dL/dO (spmv_hip_attention_gqa_backward).  Q, G, dQ hold `heads` blocks, K, V, dK, dV
    `kv_heads`; dB: None or (heads, nnz).  dQ and dB of head h are the single-head backward's bits on its slices; dK / dV of a K / V head are the
    sums of its query heads' single-head dK / dV, added in ascending head in the handle's precision, the first taken as it is.  kv_heads = heads
    is attention_bias_backward().  -> the return code."""
    return _attention_call("attention_gqa_backward", handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, scale, check,
                           dict(Q=Q, K=K, V=V, B=B, G=G, dQ=dQ, dK=dK, dV=dV, dB=dB), ldb=ldb, lddb=lddb)


def time_attention_gqa_backward_launches(handle, heads, kv_heads, Q, K, V, B, G, dQ=None, dK=None, dV=None, dB=None, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_gqa_backward on device operands (spmv_hip_time_attention_gqa_backward_launches)."""
    return _attention_time("attention_gqa_backward", handle, heads, kv_heads, scale, warmup, iters, dict(Q=Q, K=K, V=V, B=B, G=G, dQ=dQ, dK=dK, dV=dV, dB=dB))


def attention_gqa_lse(handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, Q, K, V, B, O, L, scale=None, check=True, ldb=None, ldl=None):
    """attention_gqa() that also writes the rows' log-sum-exps (spmv_hip_attention_gqa_lse): L is (heads, m) -- any row stride; ldl overrides it for
    flat buffers holding padded planes --, L[h, i] = M_i + log Z_i of query head h, -inf on a row without entries.  O has attention_gqa()'s bits;
    L None IS attention_gqa().  -> the return code."""
    return _attention_call("attention_gqa_lse", handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, scale, check, dict(Q=Q, K=K, V=V, B=B, O=O, L=L), ldb=ldb, ldl=ldl)


def time_attention_gqa_lse_launches(handle, heads, kv_heads, Q, K, V, B, O, L, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_gqa_lse on device operands (spmv_hip_time_attention_gqa_lse_launches)."""
    return _attention_time("attention_gqa_lse", handle, heads, kv_heads, scale, warmup, iters, dict(Q=Q, K=K, V=V, B=B, O=O, L=L))


def attention_gqa_lse_16(handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, Q, K, V, B, O, L=None, scale=None, check=True, ldb=None, ldl=None):
    """attention_gqa_lse() on 16-bit Q, K and V over an fp32 handle (spmv_hip_attention_gqa_lse_16): Q, K and V are torch tensors, all
    torch.float16 or all torch.bfloat16, on the CPU or the device; O is a tensor of that dtype or of torch.float32; B (None, (nnz,) or (heads, nnz))
    and L (None or (heads, m)) are fp32.  An fp32 O and L have the bits of attention_gqa_lse() on Q.float(), K.float(), V.float(); a 16-bit O is that
    result rounded once, O32.to(dtype).  Row strides are passed as leading dimensions in elements of each tensor's own dtype.  -> the return code."""
    return _attention_call("attention_gqa_lse_16", handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, scale, check, dict(Q=Q, K=K, V=V, B=B, O=O, L=L), ldb=ldb, ldl=ldl)


def time_attention_gqa_lse_16_launches(handle, heads, kv_heads, Q, K, V, B, O, L=None, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_gqa_lse_16 on device operands (spmv_hip_time_attention_gqa_lse_16_launches)."""
    return _attention_time("attention_gqa_lse_16", handle, heads, kv_heads, scale, warmup, iters, dict(Q=Q, K=K, V=V, B=B, O=O, L=L))


def _attention_merge_args(heads, O1, L1, O2, L2, O, L, ldl):
    """-> (dv, the C arguments from O1 on) of an attention_merge call; ldl: None, or the plane strides (ldl1, ldl2, ldl) of flat L buffers"""
    heads = int(heads)
    args, width = [], None
    for o, l, no, nl, i in ((O1, L1, "O1", "L1", 0), (O2, L2, "O2", "L2", 1), (O, L, "O", "L", 2)):
        p, _, w, ld = _block(o, no)
        if heads < 1 or w % heads or (width is not None and w != width):
            raise ValueError(f"{no} has {w} columns: not {heads} heads of the other operands' width")
        width = w
        pl, ll = (_ptr(l), int(ldl[i])) if ldl is not None else _lse_planes(l, nl, heads)
        args += [p, int(max(ld, 1)), pl, ll]
    return width // heads, args


def attention_merge(handle, heads, O1, L1, O2, L2, O, L=None, check=True, ldl=None):
    """O, L = two partial attention results over disjoint parts of a key / value set, combined by their log-sum-exps
    (spmv_hip_attention_merge): the O operands are (m, heads*dv), the L operands (heads, m).  O may be O1 and L may be L1 (a running
    accumulator); L None: the merged log-sum-exp is not wanted.  The handle gives m, the precision and the stream; its matrix is not read.
    -> the return code."""
    dv, args = _attention_merge_args(heads, O1, L1, O2, L2, O, L, ldl)
    return _checked(load().spmv_hip_attention_merge(handle, int(heads), dv, *args), "spmv_hip_attention_merge", check)


def time_attention_merge_launches(handle, heads, O1, L1, O2, L2, O, L=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_merge on device operands (spmv_hip_time_attention_merge_launches)."""
    dv, args = _attention_merge_args(heads, O1, L1, O2, L2, O, L, None)
    return _timed("spmv_hip_time_attention_merge_launches", (handle, int(heads), dv, *args), warmup, iters)


def attention_gqa_backward_lse(handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, Q, K, V, B, G, O, L, dQ=None, dK=None, dV=None, dB=None, scale=None,
                               check=True, ldb=None, lddb=None, ldl=None):
    """attention_gqa_backward() driven by the FINAL output O (m x heads*dv) and log-sum-exp L (heads, m) of the attention this handle's entries are
    a part of (spmv_hip_attention_gqa_backward_lse): P = exp(t - L), D = <G row, O row>; for one handle, its own attention_gqa_lse() results; for
    parts, the merged ones -- then the parts' dQ are the caller's to add, dK, dV and dB are each part's own.  -> the return code."""
    return _attention_call("attention_gqa_backward_lse", handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, scale, check,
                           dict(Q=Q, K=K, V=V, B=B, G=G, O=O, L=L, dQ=dQ, dK=dK, dV=dV, dB=dB), ldb=ldb, lddb=lddb, ldl=ldl)


def time_attention_gqa_backward_lse_launches(handle, heads, kv_heads, Q, K, V, B, G, O, L, dQ=None, dK=None, dV=None, dB=None, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_gqa_backward_lse on device operands (spmv_hip_time_attention_gqa_backward_lse_launches)."""
    return _attention_time("attention_gqa_backward_lse", handle, heads, kv_heads, scale, warmup, iters,
                           dict(Q=Q, K=K, V=V, B=B, G=G, O=O, L=L, dQ=dQ, dK=dK, dV=dV, dB=dB))


def attention_gqa_backward_16(handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, Q, K, V, B, G, O=None, L=None, dQ=None, dK=None, dV=None, dB=None, scale=None,
                              check=True, ldb=None, lddb=None, ldl=None):
    """attention_gqa_backward() (O and L None) or attention_gqa_backward_lse() (both given, torch.float32) on 16-bit Q, K, V and G over an fp32 handle
    (spmv_hip_attention_gqa_backward_16): Q, K, V and G are torch tensors, all torch.float16 or all torch.bfloat16, on the CPU or the device; dQ, and
    dK / dV together, are tensors of that dtype or of torch.float32 (None: not wanted); B and dB are fp32.  An fp32 output and dB have the bits of the
    fp32 call on Q.float(), K.float(), V.float(), G.float(); a 16-bit output is that result rounded once, g32.to(dtype) -- also over groups of heads
    (kv_heads < heads), whose sums are made in fp32 whatever option "attention_backward_heads" says.  Mixed dtypes or a float64 handle: TypeError.
    On a band the call is no faster than widening first; what it saves is the fp32 copies.  -> the return code."""
    return _attention_call("attention_gqa_backward_16", handle, m, RowPtr, ColIdx, Matrix_Val, heads, kv_heads, scale, check,
                           dict(Q=Q, K=K, V=V, B=B, G=G, O=O, L=L, dQ=dQ, dK=dK, dV=dV, dB=dB), ldb=ldb, lddb=lddb, ldl=ldl)


def time_attention_gqa_backward_16_launches(handle, heads, kv_heads, Q, K, V, B, G, O=None, L=None, dQ=None, dK=None, dV=None, dB=None, scale=None, warmup=10, iters=100):
    """-> (mean_ms, per-call ms array) of spmv_hip_attention_gqa_backward_16 on device operands (spmv_hip_time_attention_gqa_backward_16_launches)."""
    return _attention_time("attention_gqa_backward_16", handle, heads, kv_heads, scale, warmup, iters,
                           dict(Q=Q, K=K, V=V, B=B, G=G, O=O, L=L, dQ=dQ, dK=dK, dV=dV, dB=dB))


def _cg_options(rtol, atol, max_iterations, check_every, x0, dinv, history, columns=None, mixed=None):
    """-> (spmv_hip_cg_options, the history array or None).  mixed = (update_drop, update_every): spmv_hip_cg_mixed_options, which appends the two;
    columns = k: spmv_hip_cg_columns' history, (max_iterations + 1) x k, NaN where a column wrote nothing"""
    hist = None
    if history and max_iterations >= 0:
        hist = np.zeros(int(max_iterations) + 1, dtype=np.float64) if columns is None else np.full((int(max_iterations) + 1, columns), np.nan, dtype=np.float64)
    common = (float(rtol), float(atol), int(max_iterations), int(check_every), 1 if x0 else 0, _ptr(dinv), hist.ctypes.data_as(C.POINTER(C.c_double)) if hist is not None else None)
    return (spmv_hip_cg_mixed_options(*common, float(mixed[0]), int(mixed[1])) if mixed else spmv_hip_cg_options(*common)), hist


def _solve_result(res, names, rc=0, hist=None):
    """a spmv_hip_cg_result, spmv_hip_cg_mixed_result or spmv_hip_lsqr_result -> the result dict; names: CG_STATUS, CG_MIXED_STATUS or LSQR_STATUS"""
    out = {"status": res.status, "status_name": names[res.status] if 0 <= res.status < len(names) else "?", "iterations": res.iterations}
    if hasattr(res, "updates"):
        out["updates"] = res.updates
    out.update(rr=res.rr, bb=res.bb)
    if hasattr(res, "ar"):
        out.update(ar=res.ar, anorm=res.anorm)
    if hist is not None:
        out["history"] = hist[:res.iterations + 1].copy() if rc == 0 else hist[:0].copy()
    return out


def _solve(name, handle, m, RowPtr, ColIdx, Matrix_Val, B, X, rtol, atol, max_iterations, check_every, x0, dinv, history, check, extra=()):
    """cg(), bicgstab() and gmres(): one call of the entry point `name`; extra: what it takes between X and the options"""
    opt, hist = _cg_options(rtol, atol, max_iterations, check_every, x0, dinv, history)
    res = spmv_hip_cg_result()
    rc = _checked(getattr(load(), name)(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), _ptr(B), _ptr(X), *extra, C.byref(opt), C.byref(res)), name, check)
    return rc, _solve_result(res, CG_STATUS, rc, hist)


def _time_solve(name, handle, B, X, iterations, x0, dinv, warmup, iters, extra=()):
    opt, _ = _cg_options(0.0, 0.0, iterations, 0, x0, dinv, False)
    return _timed(name, (handle, _ptr(B), _ptr(X), *extra, C.byref(opt)), warmup, iters)


def cg(handle, m, RowPtr, ColIdx, Matrix_Val, B, X, rtol=1e-8, atol=0.0, max_iterations=1000, check_every=0, x0=False, dinv=None, history=False,
       check=True):
    """Solve A x = B by preconditioned conjugate gradients on the device (spmv_hip_cg): B, X, dinv of m elements, host or device; x0: X holds the
    initial guess.  -> (rc, result dict: status, status_name, iterations, rr, bb[, history: rr after iteration 0 .. iterations])."""
    return _solve("spmv_hip_cg", handle, m, RowPtr, ColIdx, Matrix_Val, B, X, rtol, atol, max_iterations, check_every, x0, dinv, history, check)


def time_cg_iterations(handle, B, X, iterations, x0=False, dinv=None, warmup=2, iters=20):
    """-> (mean ms per run, per-run ms array) of `iters` runs of `iterations` CG iterations each, stop tests off, on device B / X / dinv
    (spmv_hip_time_cg_iterations)."""
    return _time_solve("spmv_hip_time_cg_iterations", handle, B, X, iterations, x0, dinv, warmup, iters)


def bicgstab(handle, m, RowPtr, ColIdx, Matrix_Val, B, X, rtol=1e-8, atol=0.0, max_iterations=1000, check_every=0, x0=False, dinv=None, history=False,
             check=True):
    """Solve A x = B by right-preconditioned BiCGStab on the device (spmv_hip_bicgstab; A need not be symmetric): B, X, dinv of m elements, host
    or device; x0: X holds the initial guess.  -> (rc, result dict: status, status_name, iterations, rr, bb[, history: rr after iteration
    0 .. iterations]), as cg()."""
    return _solve("spmv_hip_bicgstab", handle, m, RowPtr, ColIdx, Matrix_Val, B, X, rtol, atol, max_iterations, check_every, x0, dinv, history, check)


def time_bicgstab_iterations(handle, B, X, iterations, x0=False, dinv=None, warmup=2, iters=20):
    """-> (mean ms per run, per-run ms array) of `iters` runs of `iterations` BiCGStab iterations each, stop tests off, on device B / X / dinv
    (spmv_hip_time_bicgstab_iterations)."""
    return _time_solve("spmv_hip_time_bicgstab_iterations", handle, B, X, iterations, x0, dinv, warmup, iters)


GMRES_RESTART_MAX = 32  # SPMV_HIP_GMRES_RESTART_MAX


def gmres(handle, m, RowPtr, ColIdx, Matrix_Val, B, X, restart=30, rtol=1e-8, atol=0.0, max_iterations=1000, check_every=0, x0=False, dinv=None,
          history=False, check=True):
    """Solve A x = B by right-preconditioned restarted GMRES(restart) on the device (spmv_hip_gmres; A need not be symmetric; 1 <= restart <=
    32): B, X, dinv of m elements, host or device; x0: X holds the initial guess.  An iteration is one inner step.  -> (rc, result dict:
    status, status_name, iterations, rr, bb[, history: the residual estimate after iteration 0 .. iterations]), as cg()."""
    return _solve("spmv_hip_gmres", handle, m, RowPtr, ColIdx, Matrix_Val, B, X, rtol, atol, max_iterations, check_every, x0, dinv, history, check, (int(restart),))


def time_gmres_iterations(handle, B, X, iterations, restart=30, x0=False, dinv=None, warmup=2, iters=20):
    """-> (mean ms per run, per-run ms array) of `iters` runs of `iterations` GMRES(restart) steps each, the cycle ends and restarts among
    them included, stop tests off, on device B / X / dinv (spmv_hip_time_gmres_iterations)."""
    return _time_solve("spmv_hip_time_gmres_iterations", handle, B, X, iterations, x0, dinv, warmup, iters, (int(restart),))


def gmres_device_sqrt(values, out):
    """out[i] = the fp64 square root of values[i] as spmv_hip_gmres's kernels take it (spmv_hip_gmres_device_sqrt): device fp64 tensors."""
    _checked(load().spmv_hip_gmres_device_sqrt(_ptr(values), _ptr(out), int(values.numel())), "spmv_hip_gmres_device_sqrt", True)
    return out


def cg_mixed(high, low, B, X, rtol=1e-10, atol=0.0, max_iterations=1000, check_every=0, x0=False, dinv=None, history=False, update_drop=0.0,
             update_every=0, check=True):
    """Solve A x = B in fp64 by conjugate gradients with reliable updates (spmv_hip_cg_mixed): the iterations run in fp32 on `low`, an fp32
    handle of the same matrix, and every so often the true residual is formed again in fp64 on `high`.  B, X: m fp64 elements, dinv: m
    fp32 elements or None, host or device; x0: X holds the initial guess; update_drop (0: the default, 0.01) and update_every (0: no cap) say
    when a segment of fp32 iterations ends.  -> (rc, result dict: status, status_name, iterations, updates, rr (the TRUE one of X), bb[,
    history: rr after iteration 0 .. iterations, the recurrence's but where an update was committed])."""
    opt, hist = _cg_options(rtol, atol, max_iterations, check_every, x0, dinv, history, mixed=(update_drop, update_every))
    res = spmv_hip_cg_mixed_result()
    rc = _checked(load().spmv_hip_cg_mixed(high, low, _ptr(B), _ptr(X), C.byref(opt), C.byref(res)), "spmv_hip_cg_mixed", check)
    return rc, _solve_result(res, CG_MIXED_STATUS, rc, hist)


def time_cg_mixed_iterations(high, low, B, X, iterations, update_every=0, x0=False, dinv=None, warmup=2, iters=20):
    """-> (mean ms per run, per-run ms array) of `iters` runs of `iterations` mixed iterations each, an fp64 update behind every
    update_every-th one (0: none), stop tests off, on device B / X / dinv (spmv_hip_time_cg_mixed_iterations)."""
    opt, _ = _cg_options(0.0, 0.0, iterations, 0, x0, dinv, False, mixed=(0.0, update_every))
    return _timed("spmv_hip_time_cg_mixed_iterations", (high, low, _ptr(B), _ptr(X), C.byref(opt)), warmup, iters)


def _lsqr_options(rtol, atol, ls_tol, damp, max_iterations, check_every, x0, history):
    """-> (spmv_hip_lsqr_options, the history array or None)"""
    hist = np.zeros(int(max_iterations) + 1, dtype=np.float64) if history and max_iterations >= 0 else None
    return spmv_hip_lsqr_options(float(rtol), float(atol), float(ls_tol), float(damp), int(max_iterations), int(check_every), 1 if x0 else 0,
                                 hist.ctypes.data_as(C.POINTER(C.c_double)) if hist is not None else None), hist


def lsqr(handle, m, RowPtr, ColIdx, Matrix_Val, B, X, damp=0.0, rtol=1e-8, atol=0.0, ls_tol=1e-8, max_iterations=1000, check_every=0, x0=False, history=False,
         check=True):
    """Minimise |A x - B|^2 + damp^2 |x|^2 by LSQR on the device (spmv_hip_lsqr; A of any shape): B of m elements, X of n, host or device; x0: X
    holds the initial guess.  -> (rc, result dict: status, status_name, iterations, rr, bb, ar, anorm[, history: the residual estimate after
    iteration 0 .. iterations]); status "least_squares": the normal-equations test ar <= ls_tol * anorm * sqrt(rr) held."""
    opt, hist = _lsqr_options(rtol, atol, ls_tol, damp, max_iterations, check_every, x0, history)
    res = spmv_hip_lsqr_result()
    rc = _checked(load().spmv_hip_lsqr(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), _ptr(B), _ptr(X), C.byref(opt), C.byref(res)), "spmv_hip_lsqr", check)
    return rc, _solve_result(res, LSQR_STATUS, rc, hist)


def time_lsqr_iterations(handle, B, X, iterations, damp=0.0, x0=False, warmup=2, iters=20):
    """-> (mean ms per run, per-run ms array) of `iters` runs of `iterations` LSQR iterations each, stop tests off, on device B (m elements) and
    X (n elements) (spmv_hip_time_lsqr_iterations)."""
    opt, _ = _lsqr_options(0.0, 0.0, 0.0, damp, iterations, 0, x0, False)
    return _timed("spmv_hip_time_lsqr_iterations", (handle, _ptr(B), _ptr(X), C.byref(opt)), warmup, iters)


CG_COLUMNS_MAX = 16  # SPMV_HIP_CG_COLUMNS_MAX


def _cg_columns_blocks(B, X):
    """-> (k, address of B, ldb, address of X, ldx) of spmv_hip_cg_columns' two m x k blocks, with the checks that need no library"""
    k, pb, ldb, px, ldx = _blocks(B, "B", X, "X")
    if B is not None and X is not None and B.shape[0] != X.shape[0]:
        raise ValueError(f"B has {B.shape[0]} rows, X {X.shape[0]}")
    if not 1 <= k <= CG_COLUMNS_MAX:
        raise ValueError(f"cg_columns solves 1 .. {CG_COLUMNS_MAX} right-hand sides per call, not {k}")
    return k, pb, ldb, px, ldx


def cg_columns(handle, m, RowPtr, ColIdx, Matrix_Val, B, X, rtol=1e-8, atol=0.0, max_iterations=1000, check_every=0, x0=False, dinv=None, history=False,
               check=True):
    """Solve A X = B for the k <= 16 columns of B by k independent conjugate-gradient recurrences that share one pass over A per iteration
    (spmv_hip_cg_columns).  B, X: m x k, 2-D numpy arrays or torch tensors with column stride 1 (their row strides are passed as ldb / ldx);
    dinv: None or ONE vector of m elements; x0: X holds the initial guesses.
    -> (rc, list of k result dicts as cg()'s[, and with history: the array of (max_iterations + 1) x k, NaN where a column wrote nothing])."""
    k, pb, ldb, px, ldx = _cg_columns_blocks(B, X)
    if int(max_iterations) < 0:
        raise ValueError("max_iterations must be >= 0")
    opt, hist = _cg_options(rtol, atol, max_iterations, check_every, x0, dinv, history, columns=k)
    res = (spmv_hip_cg_result * k)()
    rc = _checked(load().spmv_hip_cg_columns(handle, int(m), _ptr(RowPtr), _ptr(ColIdx), _ptr(Matrix_Val), k, pb, ldb, px, ldx, C.byref(opt), res), "spmv_hip_cg_columns", check)
    out = [_solve_result(r, CG_STATUS) for r in res]
    return (rc, out, hist) if history else (rc, out)


def time_cg_columns_iterations(handle, B, X, iterations, x0=False, dinv=None, warmup=2, iters=20):
    """-> (mean ms per run, per-run ms array) of `iters` runs of `iterations` k-column CG iterations each, stop tests off, on device B / X / dinv
    (spmv_hip_time_cg_columns_iterations)."""
    k, pb, ldb, px, ldx = _cg_columns_blocks(B, X)
    opt, _ = _cg_options(0.0, 0.0, iterations, 0, x0, dinv, False)
    return _timed("spmv_hip_time_cg_columns_iterations", (handle, k, pb, ldb, px, ldx, C.byref(opt)), warmup, iters)


def _take_csr(m, n, nnz, rp, ci, va, dtype):
    """Copy malloc'ed C arrays into numpy arrays and free the C side."""
    from .synth import CSR
    lib = load()
    rowptr = np.ctypeslib.as_array(rp, shape=(m.value + 1,)).copy()
    colidx = np.ctypeslib.as_array(ci, shape=(max(nnz.value, 1),))[: nnz.value].copy()
    vt = C.c_double if dtype == np.float64 else C.c_float
    val = np.ctypeslib.as_array(C.cast(va, C.POINTER(vt)), shape=(max(nnz.value, 1),))[: nnz.value].copy()
    for p in (rp, ci, va):
        lib.spmv_io_free(C.cast(p, _V))
    return CSR(m.value, n.value, rowptr, colidx, val)


def read_mtx(path, dtype=np.float64):
    """Matrix Market coordinate file -> (CSR, is_symmetric)   [spmv_io_read_mtx]."""
    lib = load()
    m, n, nnz, sym = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rp, ci, va = _I(), _I(), _V()
    rc = lib.spmv_io_read_mtx(os.fsencode(path), np.dtype(dtype).itemsize, C.byref(m), C.byref(n), C.byref(nnz), C.byref(sym),
                              C.byref(rp), C.byref(ci), C.byref(va))
    if rc != 0:
        raise OSError(f"spmv_io_read_mtx({path!r}) failed with {rc}")
    return _take_csr(m, n, nnz, rp, ci, va, np.dtype(dtype)), bool(sym.value)


def write_bin(path, csr):
    rc = load().spmv_io_write_bin(os.fsencode(path), csr.m, csr.n, csr.nnz, _ptr(np.ascontiguousarray(csr.rowptr, np.int32)),
                                  _ptr(np.ascontiguousarray(csr.colidx, np.int32)), _ptr(np.ascontiguousarray(csr.val)),
                                  csr.val.dtype.itemsize)
    if rc != 0:
        raise OSError(f"spmv_io_write_bin({path!r}) failed with {rc}")


def read_bin(path, dtype=np.float64):
    lib = load()
    m, n, nnz = C.c_int(), C.c_int(), C.c_int()
    rp, ci, va = _I(), _I(), _V()
    rc = lib.spmv_io_read_bin(os.fsencode(path), np.dtype(dtype).itemsize, C.byref(m), C.byref(n), C.byref(nnz),
                              C.byref(rp), C.byref(ci), C.byref(va))
    if rc != 0:
        raise OSError(f"spmv_io_read_bin({path!r}) failed with {rc}")
    return _take_csr(m, n, nnz, rp, ci, va, np.dtype(dtype))


def cache_path(mtx_path):
    buf = C.create_string_buffer(4096)
    if load().spmv_io_cache_path(os.fsencode(mtx_path), buf, len(buf)) != 0:
        raise ValueError("path too long")
    return buf.value.decode()


class Handle:
    """RAII convenience around the four functions (create in __init__, destroy in close())."""

    def __init__(self, m, n, rowptr, colidx, val, method=SPMV_METHODS.Method_Parallel, nthreads=1,
                 way=VECTORIZED_WAY.VECTOR_HIP, token=None):
        self.m, self.n = int(m), int(n)
        self._keep = (rowptr, colidx, val)  # the C side keeps the caller's pointers for identity checks
        self.h = spmv_create_handle_all_in_one(m, n, rowptr, colidx, val, nthreads, method,
                                               _itemsize(val), way, token)

    @property
    def method(self):
        return SPMV_METHODS(self.h.contents.spmvMethod)

    def info(self):
        return get_info(self.h)

    @property
    def nnz(self):
        """stored entries of the resident matrix (asked once, then remembered)"""
        if getattr(self, "_nnz", None) is None:
            self._nnz = int(self.info()["nnz"])
        return self._nnz

    @property
    def index(self):
        """handle->index as a numpy array (the RCM permutation when option "reorder" is on), else None."""
        p = self.h.contents.index
        if not p:
            return None
        return np.ctypeslib.as_array(p, shape=(self.m,)).copy()

    def spmv(self, x, y):
        rp, ci, va = self._keep
        spmv(self.h, self.m, rp, ci, va, x, y)
        return y

    def spmm(self, X, Y=None):
        """Y = A X (spmv_hip_spmm) for a 2-D X of n x k; Y (m x k) is allocated like X -- same kind, dtype and device -- when None."""
        if Y is None:
            k = X.shape[1]
            if isinstance(X, np.ndarray):
                Y = np.empty((self.m, k), dtype=X.dtype)
            else:
                import torch
                Y = torch.empty((self.m, k), dtype=X.dtype, device=X.device)
        rp, ci, va = self._keep
        spmm(self.h, self.m, rp, ci, va, X, Y)
        return Y

    def spmv_transpose(self, x, y=None):
        """y = A^T x (spmv_hip_spmv_transpose) for x of m entries; y (n entries) is allocated like x -- same kind, dtype and device -- when None."""
        if y is None:
            if isinstance(x, np.ndarray):
                y = np.empty(self.n, dtype=x.dtype)
            else:
                import torch
                y = torch.empty(self.n, dtype=x.dtype, device=x.device)
        rp, ci, va = self._keep
        spmv_transpose(self.h, self.m, rp, ci, va, x, y)
        return y

    def _like(self, a, shape, dtype=None):
        """an uninitialised array of `shape`, of a's kind, dtype -- or `dtype` -- and device"""
        if isinstance(a, np.ndarray):
            return np.empty(shape, dtype=dtype or a.dtype)
        import torch
        return torch.empty(shape, dtype=dtype or a.dtype, device=a.device)

    def spmm_transpose(self, X, Y=None):
        """Y = A^T X (spmv_hip_spmm_transpose) for a 2-D X of m x k; Y (n x k) is allocated like X -- same kind, dtype and device -- when None."""
        if Y is None:
            Y = self._like(X, (self.n, X.shape[1]))
        rp, ci, va = self._keep
        spmm_transpose(self.h, self.m, rp, ci, va, X, Y)
        return Y

    def sddmm(self, U, V, out=None):
        """out[p] = <U[row(p)], V[col(p)]> over the pattern (spmv_hip_sddmm) for 2-D U (m x k) and V (n x k); out (nnz elements in CSR order) is
        allocated like U -- same kind, dtype and device -- when None."""
        if out is None:
            out = self._like(U, (self.nnz,))
        rp, ci, va = self._keep
        sddmm(self.h, self.m, rp, ci, va, U, V, out)
        return out

    def row_softmax(self, S, out=None):
        """out[p] = softmax of S over the stored entries of p's row (spmv_hip_row_softmax); S: nnz elements in CSR order; out is allocated like
        S -- same kind, dtype and device -- when None, and may be S itself."""
        if out is None:
            out = self._like(S, (self.nnz,))
        rp, ci, va = self._keep
        row_softmax(self.h, self.m, rp, ci, va, S, out)
        return out

    def row_softmax_backward(self, P, G, out=None):
        """out = dL/dS from P = row_softmax(S) and G = dL/dP (spmv_hip_row_softmax_backward); out is allocated like P when None, and may be G."""
        if out is None:
            out = self._like(P, (self.nnz,))
        rp, ci, va = self._keep
        row_softmax_backward(self.h, self.m, rp, ci, va, P, G, out)
        return out

    def _solve(self, solve, b, x, x0, rtol, atol, max_iterations, check_every, dinv, history):
        if x is None:
            if x0:
                raise ValueError("x0 needs an x that holds the initial guess")
            x = self._like(b, (self.m,))
        rp, ci, va = self._keep
        _, res = solve(self.h, self.m, rp, ci, va, b, x, rtol, atol, max_iterations, check_every, x0, dinv, history)
        if history:
            return x, res, res.pop("history")
        return x, res

    def cg(self, b, x=None, x0=False, rtol=1e-8, atol=0.0, max_iterations=1000, check_every=0, dinv=None, history=False):
        """Solve A x = b by preconditioned conjugate gradients that stay on the device (spmv_hip_cg; A symmetric positive definite).  x is
        allocated like b when None (then x0 must be off); x0: x holds the initial guess; dinv: None or 1 / diag(A) (Jacobi).
        -> (x, result dict) or (x, result dict, history) when history is set: rr after iteration 0 .. iterations."""
        return self._solve(cg, b, x, x0, rtol, atol, max_iterations, check_every, dinv, history)

    def cg_mixed(self, low, b, x=None, x0=False, rtol=1e-10, atol=0.0, max_iterations=1000, check_every=0, update_drop=0.0, update_every=0, dinv=None, history=False):
        """Solve A x = b in fp64 with this fp64 handle and `low`, a float32 Handle of the same matrix (the values rounded to float), by conjugate
        gradients with reliable updates (spmv_hip_cg_mixed): fp32 iterations on `low`, the solution and the true residual in fp64.  b, x:
        float64; x is allocated like b when None (then x0 must be off); dinv: None or float32 1 / diag(A); update_drop (0: the default, 0.01) and
        update_every (0: no cap) end a segment of iterations.  The result's rr is the TRUE residual's, `updates` the fp64 updates.
        -> (x, result dict) or (x, result dict, history) when history is set.
        Measured on an MI355X: whether this beats cg() on the fp64 handle depends on the matrix; see there."""
        if x is None:
            if x0:
                raise ValueError("x0 needs an x that holds the initial guess")
            x = self._like(b, (self.m,))
        _, res = cg_mixed(self.h, low.h if isinstance(low, Handle) else low, b, x, rtol, atol, max_iterations, check_every, x0, dinv, history, update_drop, update_every)
        if history:
            return x, res, res.pop("history")
        return x, res

    def cg_columns(self, B, X=None, x0=False, rtol=1e-8, atol=0.0, max_iterations=1000, check_every=0, dinv=None, history=False):
        """Solve A X = B for the k <= 16 columns of a 2-D B (m x k) by k INDEPENDENT conjugate-gradient recurrences that stay on the device
        and share one pass over A per iteration (spmv_hip_cg_columns; A symmetric positive definite).  Every column has its own alpha, beta,
        stop test, status and iteration count, and its bits do not depend on k, on its position or on the other columns.  X (m x k) is
        allocated like B when None (then x0 must be off); x0: X holds the initial guesses; dinv: None or ONE vector 1 / diag(A) for all
        columns.  B and X may be views into wider arrays (column stride 1).
        -> (X, list of k result dicts) or (X, list, history) when history is set: history[it, j] is column j's rr after iteration it, rows 0 ..
        the largest iteration count, NaN behind a column's own end.
        When to loop over cg() instead: the multiply here is spmm's, which does not use the handle's tuned spmv() schedule.  Measured on an
        MI355X: at k = 2 a loop of cg() was faster on five of six cases (this call took 1.15 to 1.95 times as long), at k = 4 this
        call was 1.17 to 1.57 times faster on five cases and 10 % slower in fp32 on a 1e7-row band, from k = 8 on it was 1.3 to 2.3 times
        faster everywhere.  Also prefer a loop when the columns' iteration counts differ widely: a finished column is still
        multiplied until the last one ends."""
        if X is None:
            if x0:
                raise ValueError("x0 needs an X that holds the initial guesses")
            X = self._like(B, (self.m, B.shape[1]))
        rp, ci, va = self._keep
        out = cg_columns(self.h, self.m, rp, ci, va, B, X, rtol, atol, max_iterations, check_every, x0, dinv, history)
        if history:
            rows = 1 + max((r["iterations"] for r in out[1]), default=0)
            return X, out[1], out[2][:rows].copy()
        return X, out[1]

    def bicgstab(self, b, x=None, x0=False, rtol=1e-8, atol=0.0, max_iterations=1000, check_every=0, dinv=None, history=False):
        """Solve A x = b by right-preconditioned BiCGStab that stays on the device (spmv_hip_bicgstab; A square, not necessarily symmetric).
        The arguments and the return value are cg()'s: x is allocated like b when None (then x0 must be off); x0: x holds the initial guess;
        dinv: None or 1 / diag(A) (Jacobi, applied from the right: x solves the original system).
        -> (x, result dict) or (x, result dict, history) when history is set: rr after iteration 0 .. iterations."""
        return self._solve(bicgstab, b, x, x0, rtol, atol, max_iterations, check_every, dinv, history)

    def gmres(self, b, x=None, restart=30, x0=False, rtol=1e-8, atol=0.0, max_iterations=1000, check_every=0, dinv=None, history=False):
        """Solve A x = b by right-preconditioned restarted GMRES(restart) that stays on the device (spmv_hip_gmres; A square, not necessarily
        symmetric; 1 <= restart <= 32).  An iteration is one inner step: one multiply and one new basis vector.  The other arguments and the
        return value are bicgstab()'s; rr and the history are the recurrence's residual estimate, which never rises inside a cycle.
        -> (x, result dict) or (x, result dict, history) when history is set."""
        def solve(h, m, rp, ci, va, b, x, rtol, atol, max_iterations, check_every, x0, dinv, history):
            return gmres(h, m, rp, ci, va, b, x, restart, rtol, atol, max_iterations, check_every, x0, dinv, history)
        return self._solve(solve, b, x, x0, rtol, atol, max_iterations, check_every, dinv, history)

    def lsqr(self, b, x=None, x0=False, damp=0.0, rtol=1e-8, atol=0.0, ls_tol=1e-8, max_iterations=1000, check_every=0, history=False):
        """Minimise |A x - b|^2 + damp^2 |x|^2 by LSQR that stays on the device (spmv_hip_lsqr; A of any shape: an overdetermined fit, the
        minimum-norm solution of an underdetermined system, a ridge regression).  b has m elements; x (n elements) is allocated like b when
        None (then x0 must be off); x0: x holds the initial guess.  The result's status is "converged" (the residual estimate rr fell to
        max(rtol^2 bb, atol^2): a consistent system), "least_squares" (ar <= ls_tol * anorm * sqrt(rr): a least-squares solution),
        "max_iterations" or "nonfinite"; ar estimates |A^T r - damp^2 x|, anorm the Frobenius norm of [A; damp I].  The transpose is built at
        the first call.  Measured on an MI355X: DESIGN 3.31.
        -> (x, result dict) or (x, result dict, history) when history is set: rr after iteration 0 .. iterations."""
        if x is None:
            if x0:
                raise ValueError("x0 needs an x that holds the initial guess")
            x = self._like(b, (self.n,))
        rp, ci, va = self._keep
        _, res = lsqr(self.h, self.m, rp, ci, va, b, x, damp, rtol, atol, ls_tol, max_iterations, check_every, x0, history)
        if history:
            return x, res, res.pop("history")
        return x, res

    def _attention_out(self, Q, V, heads, kv_heads, out, dtype=None):
        """-> `out`, or when that is None the uninitialised output of an attention forward: (m, heads * dv) like Q -- of `dtype` where one is
        given --, dv the width of one of V's kv_heads heads (kv_heads None: as wide as V, a head of V for every head of out)"""
        if out is None:
            out = self._like(Q, (self.m, V.shape[1] if kv_heads is None else (V.shape[1] // int(kv_heads)) * int(heads)), dtype)
        return out

    def _attention_grads(self, Q, K, V, heads, need, dtypes=(None, None, None, None)):
        """-> the outputs of an attention backward that `need` asks for, None for the others: dQ, dK and dV as wide as Q, K and V and, where
        `need` has a fourth entry, dB (heads, nnz); uninitialised, like Q, of `dtypes` where those are given"""
        shapes = [(self.m, Q.shape[1]), (self.n, K.shape[1]), (self.n, V.shape[1])]
        if len(need) > 3:
            shapes.append((int(heads), self.nnz) if need[3] else None)
        return tuple(self._like(Q, shape, dtype) if want else None for shape, want, dtype in zip(shapes, need, dtypes))

    def attention(self, Q, K, V, scale=None, out=None):
        """out = softmax_rows(scale * Q K^T on the pattern) V in one pass (spmv_hip_attention) for 2-D Q (m x k), K (n x k) and V (n x dv); scale
        None means 1 / sqrt(k); out (m x dv) is allocated like Q -- same kind, dtype and device -- when None.  The handle's values are not
        used and not changed."""
        out = self._attention_out(Q, V, 1, None, out)
        attention(self.h, self.m, *self._keep, Q, K, V, out, scale)
        return out

    def attention_heads(self, Q, K, V, heads, scale=None, out=None):
        """out = `heads` attention heads over the pattern in one pass (spmv_hip_attention_heads) for 2-D Q (m x heads*k), K (n x heads*k) and
        V (n x heads*dv) holding the heads side by side; scale None means 1 / sqrt(k), k one head's width; out (m x heads*dv) is allocated like
        Q -- same kind, dtype and device -- when None.  The handle's values are not used and not changed."""
        out = self._attention_out(Q, V, heads, None, out)
        attention_heads(self.h, self.m, *self._keep, heads, Q, K, V, out, scale)
        return out

    def attention_backward(self, Q, K, V, G, scale=None, need=(True, True, True)):
        """-> (dQ, dK, dV), the gradients of attention(Q, K, V, scale) for G = dL/dO (m x dv), in two passes over A (spmv_hip_attention_backward);
        need: which of the three are wanted -- the others are None and nothing is computed for them.  The outputs are allocated like Q -- same
        kind, dtype and device.  The handle's values are not used and not changed."""
        grads = self._attention_grads(Q, K, V, 1, need)
        attention_backward(self.h, self.m, *self._keep, Q, K, V, G, *grads, scale)
        return grads

    def attention_heads_backward(self, Q, K, V, G, heads, scale=None, need=(True, True, True)):
        """-> (dQ, dK, dV), the gradients of attention_heads(Q, K, V, heads, scale) for G = dL/dO (m x heads*dv), all heads in two passes per group
        of heads (spmv_hip_attention_heads_backward); need: which of the three are wanted -- the others are None and nothing is computed for
        them.  The outputs are allocated like Q -- same kind, dtype and device -- at the full widths.  The handle's values are not used and
        not changed."""
        grads = self._attention_grads(Q, K, V, heads, need)
        attention_heads_backward(self.h, self.m, *self._keep, heads, Q, K, V, G, *grads, scale)
        return grads

    def attention_bias(self, Q, K, V, heads, bias, scale=None, out=None):
        """out = attention_heads(Q, K, V, heads, scale) with `bias` added to the scaled scores before the softmax (spmv_hip_attention_bias);
        bias: None, (nnz,) -- one plane for all heads -- or (heads, nnz), in CSR order, of Q's kind.  The handle's values are not used and not
        changed."""
        out = self._attention_out(Q, V, heads, None, out)
        attention_bias(self.h, self.m, *self._keep, heads, Q, K, V, bias, out, scale)
        return out

    def attention_bias_backward(self, Q, K, V, bias, G, heads, scale=None, need=(True, True, True, True)):
        """-> (dQ, dK, dV, dB), the gradients of attention_bias(Q, K, V, heads, bias, scale) for G = dL/dO (spmv_hip_attention_bias_backward);
        need: which of the four are wanted -- the others are None and nothing is computed for them.  dB is (heads, nnz), a plane per head also
        when the bias is one shared plane (its gradient is dB.sum(0)).  The outputs are allocated like Q."""
        grads = self._attention_grads(Q, K, V, heads, need)
        attention_bias_backward(self.h, self.m, *self._keep, heads, Q, K, V, bias, G, *grads, scale)
        return grads

    def attention_gqa(self, Q, K, V, heads, kv_heads, bias=None, scale=None, out=None):
        """out = attention_bias(Q, K, V, heads, bias, scale) with `kv_heads` K / V heads: K is (n, kv_heads*k), V (n, kv_heads*dv), and query head
        h uses K / V head h // (heads // kv_heads) (spmv_hip_attention_gqa).  out is (m, heads*dv)."""
        out = self._attention_out(Q, V, heads, kv_heads, out)
        attention_gqa(self.h, self.m, *self._keep, heads, kv_heads, Q, K, V, bias, out, scale)
        return out

    def attention_gqa_backward(self, Q, K, V, bias, G, heads, kv_heads, scale=None, need=(True, True, True, True)):
        """-> (dQ, dK, dV, dB), the gradients of attention_gqa(Q, K, V, heads, kv_heads, bias, scale) for G = dL/dO
        (spmv_hip_attention_gqa_backward); need: which of the four are wanted.  dK and dV have K's and V's widths (kv_heads blocks): the sums over
        each group's query heads in ascending head.  dB is (heads, nnz).  The outputs are allocated like Q."""
        grads = self._attention_grads(Q, K, V, heads, need)
        attention_gqa_backward(self.h, self.m, *self._keep, heads, kv_heads, Q, K, V, bias, G, *grads, scale)
        return grads

    def attention_gqa_lse(self, Q, K, V, heads, kv_heads, bias=None, scale=None, out=None, lse=None):
        """-> (out, lse): attention_gqa(Q, K, V, heads, kv_heads, bias, scale) and the rows' log-sum-exps, lse (heads, m), -inf on a row without
        entries (spmv_hip_attention_gqa_lse).  out has attention_gqa()'s bits."""
        out = self._attention_out(Q, V, heads, kv_heads, out)
        if lse is None:
            lse = self._like(Q, (int(heads), self.m))
        attention_gqa_lse(self.h, self.m, *self._keep, heads, kv_heads, Q, K, V, bias, out, lse, scale)
        return out, lse

    def attention_gqa_lse_16(self, Q, K, V, heads, kv_heads, B=None, scale=None, out_dtype=None, want_l=True):
        """-> (out, lse): attention_gqa_lse() on torch.float16 or torch.bfloat16 Q, K and V over this fp32 handle (spmv_hip_attention_gqa_lse_16).
        out is (m, heads*dv) of out_dtype -- None: Q's dtype; or torch.float32 --, allocated on Q's device; lse is (heads, m) fp32, None when
        want_l is False; B is fp32.  An fp32 out and lse have the bits of attention_gqa_lse() on the .float() copies; a 16-bit out is that result
        rounded once."""
        import torch
        if not isinstance(Q, torch.Tensor) or not isinstance(V, torch.Tensor):
            raise TypeError("Q, K and V must be torch tensors")
        out = self._attention_out(Q, V, heads, kv_heads, None, out_dtype)
        lse = self._like(Q, (int(heads), self.m), torch.float32) if want_l else None
        attention_gqa_lse_16(self.h, self.m, *self._keep, heads, kv_heads, Q, K, V, B, out, lse, scale)
        return out, lse

    def attention_merge(self, O1, L1, O2, L2, heads, out=None, lse=None, want_lse=True):
        """-> (out, lse): two partial results over disjoint parts of a key / value set combined by their log-sum-exps (spmv_hip_attention_merge).
        out may be O1 and lse may be L1 (a running accumulator); want_lse False: lse is not computed (None).  The matrix is not read."""
        if out is None:
            out = self._like(O1, tuple(O1.shape))
        if lse is None and want_lse:
            lse = self._like(O1, (int(heads), self.m))
        attention_merge(self.h, heads, O1, L1, O2, L2, out, lse)
        return out, lse

    def attention_gqa_backward_lse(self, Q, K, V, bias, G, O, L, heads, kv_heads, scale=None, need=(True, True, True, True)):
        """-> (dQ, dK, dV, dB) like attention_gqa_backward(), driven by the FINAL output O and log-sum-exp L of the attention this handle's entries
        are a part of (spmv_hip_attention_gqa_backward_lse)."""
        grads = self._attention_grads(Q, K, V, heads, need)
        attention_gqa_backward_lse(self.h, self.m, *self._keep, heads, kv_heads, Q, K, V, bias, G, O, L, *grads, scale)
        return grads

    def attention_gqa_backward_16(self, Q, K, V, B, G, heads, kv_heads, scale=None, O=None, L=None, need=(True, True, True, True), dq_dtype=None, dkv_dtype=None):
        """-> (dQ, dK, dV, dB): attention_gqa_backward() -- O and L None -- or attention_gqa_backward_lse() -- the final fp32 O and L given -- on
        torch.float16 or torch.bfloat16 Q, K, V and G over this fp32 handle (spmv_hip_attention_gqa_backward_16), nothing widened in memory.  dQ is of
        dq_dtype and dK and dV of dkv_dtype -- None: Q's dtype; or torch.float32 --, allocated on Q's device; dB is (heads, nnz) fp32; need: which
        of the four are wanted.  An fp32 gradient and dB have the bits of the fp32 call on the .float() copies; a 16-bit gradient is that result
        rounded once."""
        import torch
        if not all(isinstance(t, torch.Tensor) for t in (Q, K, V, G)):
            raise TypeError("Q, K, V and G must be torch tensors")
        grads = self._attention_grads(Q, K, V, heads, need, (dq_dtype, dkv_dtype, dkv_dtype, torch.float32))
        attention_gqa_backward_16(self.h, self.m, *self._keep, heads, kv_heads, Q, K, V, B, G, O, L, *grads, scale)
        return grads


    def update_values(self, val):
        """The caller changed the values (in place or in a new array of the same pattern)."""
        update_values(self.h, val)
        self._keep = (self._keep[0], self._keep[1], val)

    def option(self, key):
        return load().spmv_hip_get_handle_option(self.h, key.encode())

    # multi-GPU handles (option "gpus")
    def multi_gpus(self):
        return load().spmv_hip_multi_gpus(self.h)

    def multi_slices(self, gpu):
        """-> dict(x_ptr, x_first, x_count, y_ptr, y_first, y_count, device) of device `gpu`'s slice of x and block of y."""
        xs, ys = _V(), _V()
        xf, xc, yf, yc, dv = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_int()
        _checked(load().spmv_hip_multi_slices(self.h, gpu, C.byref(xs), C.byref(xf), C.byref(xc), C.byref(ys), C.byref(yf), C.byref(yc), C.byref(dv)), "spmv_hip_multi_slices")
        return dict(x_ptr=xs.value, x_first=xf.value, x_count=xc.value, y_ptr=ys.value, y_first=yf.value, y_count=yc.value, device=dv.value)

    def multi_step(self):
        _checked(load().spmv_hip_multi_step(self.h), "spmv_hip_multi_step")

    def multi_step_async(self):
        _checked(load().spmv_hip_multi_step_async(self.h), "spmv_hip_multi_step_async")

    def multi_synchronize(self):
        _checked(load().spmv_hip_multi_synchronize(self.h), "spmv_hip_multi_synchronize")

    @classmethod
    def from_blocks(cls, blocks, n, method=SPMV_METHODS.Method_Parallel):
        """Multi-GPU handle from separate row blocks [(rowptr, colidx, val), ...]: local int32 RowPtr, GLOBAL columns
        (spmv_hip_create_handle_from_blocks).  spmv() takes full-length x / y; the CSR arguments are ignored."""
        lib = load()
        lib.spmv_hip_clear_error()
        G = len(blocks)
        rows = (C.c_int * G)(*[int(b[0].shape[0]) - 1 for b in blocks])
        rps = (_V * G)(*[_ptr(b[0]) for b in blocks])
        cis = (_V * G)(*[_ptr(b[1]) for b in blocks])
        vas = (_V * G)(*[_ptr(b[2]) for b in blocks])
        self = cls.__new__(cls)
        self.m, self.n = int(sum(rows)), int(n)
        self._keep = (None, None, None)
        self._blocks = blocks
        self.h = spmv_Handle_t()
        lib.spmv_hip_create_handle_from_blocks(C.byref(self.h), G, rows, int(n), rps, cis, vas, int(method), _itemsize(blocks[0][2]))
        _raise_if_error("spmv_hip_create_handle_from_blocks")
        return self

    def attach_stream(self, stream_ptr, async_=True):
        set_stream(self.h, stream_ptr, async_)
        self._attached = (int(stream_ptr or 0), bool(async_))

    @property
    def attached(self):
        """(stream pointer, async) last given to attach_stream; (0, False) -- the default stream, synchronous -- before any"""
        return getattr(self, "_attached", (0, False))

    def close(self):
        if self.h:
            spmv_destory_handle(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
