"""What the GPU tests of the six device-resident solves share, each written once (a helper module like cg_cases: no fixture, no pytest hook).

ROWS mirrors kSolvers of spmv_amd/csrc/shim/solve.hpp: one row per solver with, as data, everything in which the solvers' tests legitimately
differ -- the model and how it is called, the Handle method, the timer, the C symbol and structs, the extra result fields, the workspace
formula, the matrices, and where a check leaves rr, bb and the history out.  The helpers, the checks and the shared test bodies below are
functions of a row; a test module keeps its test functions, their names and their parameters and calls in here with its row."""
import contextlib
import ctypes as C
import functools
import types

import numpy as np

import bicgstab_cases as bc
import cg_cases as cgc
import cg_columns_cases as ccc
import cg_mixed_cases as mix
import gmres_cases as gc
import lsqr_cases as lc
import packed_cases as pc
import solve_end_cases as sec
from spmv_amd import api, build

M = api.SPMV_METHODS
DEV = "cuda:0"
CANARY = -7.25
NAMES = {np.float32: "f32", np.float64: "f64"}
DTYPES = [np.float64, np.float32]
E_ARG, E_NOSTATE = 3, 5
# slot, step and workgroup edges: P = 1, 2 and 3 workgroups, two steps per workgroup and empty workgroups (2^20 + 1: P = 1024, L = 2048)
BIG = 1024 * 1024 + 1
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2049, BIG]
EVERY = (1, 2, 3, 0, 64)           # check_every: the end falls first, in the middle and last in an enqueued batch
METHODS = [mth for mth in M if mth != M.Method_Total_Size]
LONG_ROW_KERNELS = ("csr5_group_kernel", "csr5_group_pipe_kernel", "csr5_kernel")   # the long rows' CSR5 sub-matrix, behind the row-granular kernel
# launch_kernels of a multiply on the 2049-row arrow matrices, as spmv_hip_info reports them: the first kernel; is a long-row launch beside it
EXECUTORS = {
    M.Method_Serial: ("csr_scalar_kernel", False), M.Method_Numa: ("csr_scalar_kernel", False),
    M.Method_Parallel: ("csr_vector_rows_kernel", True), M.Method_SellCSigma: ("sell_window_kernel", True),
    M.Method_Balanced: ("nat_group_kernel", False), M.Method_Balanced2: ("nat_group_kernel", False), M.Method_Balanced_Yid: ("nat_group_kernel", False),
    M.Method_CSR5SPMV: (None, False),                                                  # csr5_group_kernel or, in fp32, its two-deep form
}
# options that every solver refuses
BAD_OPTIONS = (dict(max_iterations=-1), dict(check_every=-1), dict(rtol=-1e-3), dict(atol=-1.0), dict(rtol=float("nan")), dict(atol=float("nan")))


# ----------------------------------------------------------------------------- the library, handles, multiplies
def library():
    """build, load, and a device is present: what every module's autouse fixture returns"""
    build.build()
    lib = api.load()
    assert lib.spmv_hip_device_count() > 0, "GPU tests need a device"
    return lib


def handle(csr, method=M.Method_Parallel, way=api.VECTORIZED_WAY.VECTOR_HIP, **opts):
    for key, v in opts.items():
        api.set_thread_option(key, v)
    try:
        return api.Handle(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val, method, way=way)
    finally:
        api.clear_thread_options()


@contextlib.contextmanager
def pair(high, low=None, method=M.Method_Parallel, low_method=None, high_opts=None, low_opts=None):
    """the fp64 handle of `high` and the fp32 handle of `low` (default: high's float copy) -> (hi, lo), what cg_mixed's row takes for `h`"""
    low = mix.narrowed(high) if low is None else low
    with handle(high, method, **(high_opts or {})) as hi, handle(low, method if low_method is None else low_method, **(low_opts or {})) as lo:
        yield hi, lo


def multiply_of(h):
    """the model's multiply: this handle's spmv() on host vectors"""
    def multiply(x):
        return h.spmv(np.ascontiguousarray(x), np.empty_like(x))
    return multiply


def multiplies_of(hi, lo):
    """cg_mixed's two multiplies: the pair's own spmv() on host vectors, each on its own type"""
    high, low = multiply_of(hi), multiply_of(lo)

    def high64(x):
        assert x.dtype == np.float64
        return high(x)

    def low32(x):
        assert x.dtype == np.float32
        return low(x)
    return high64, low32


def multiplies_with_transpose(h):
    """lsqr's two multiplies: this handle's spmv() and spmv_transpose() on host vectors"""
    def multiply(v):
        return h.spmv(np.ascontiguousarray(v), np.empty(h.m, dtype=v.dtype))

    def multiply_t(u):
        return h.spmv_transpose(np.ascontiguousarray(u))
    return multiply, multiply_t


def empty_csr(dtype=np.float64, n=0):
    return cgc.synth.CSR(0, n, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))


# ----------------------------------------------------------------------------- comparisons
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same(a, b):
    """the same type, shape and bits; a NaN equals a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    both = np.isnan(a) & np.isnan(b)
    return np.where(both, 0, a).tobytes() == np.where(both, 0, b).tobytes()


def f64(v):
    return np.float64(v)


def ended(r):
    return r["status"], r["iterations"], r["end"]


def run_id(run):
    return f"{run[0].name}-{NAMES[run[1]]}"


def converged_at_zero(res, *more):
    """what m = 0 and B = 0 report; more: the row's counters, all 0"""
    return (res["status"], res["iterations"], res["rr"], res["bb"]) + tuple(res[f] for f in more) == (cgc.CONVERGED, 0, 0.0, 0.0) + (0,) * len(more)


# ----------------------------------------------------------------------------- the rows
def block_bytes(m, item, vectors, partials, state=256):
    """a workspace of `vectors` m-vectors, `partials` partial arrays of 1024 doubles and the state, each rounded up to 256 bytes"""
    return vectors * ((m * item + 255) // 256 * 256) + partials * 1024 * 8 + state


def _row(name, cases, model, **kw):
    base = dict(
        name=name, cases=cases, model=model,                       # model(h, b, **keywords) on the multiplies of h itself
        open=handle,                                               # open(csr, ...) -> what model, call and solve take for `h`
        call=lambda h: getattr(h, name),                           # the Handle method, bound
        api=getattr(api, name), timer=getattr(api, f"time_{name}_iterations"),
        symbol=f"spmv_hip_{name}", options=api.spmv_hip_cg_options, result=api.spmv_hip_cg_result,
        base=dict(rtol=1e-8, atol=0.0, max_iterations=10, check_every=0, use_x0=0), bad=BAD_OPTIONS,
        positional={},                                             # the C call's arguments between X and the options, with their defaults
        zero_tols=dict(rtol=0.0),                                  # the keywords that switch every stop test off
        has_dinv=True, x_len=lambda h, b: b.size,
        counts=(), estimates=(),                                   # the result's extra fields: integers, doubles
        workspace=None,                                            # workspace(m, item, ...) -> the bytes the first solve adds to device_bytes
        skip_ends=(),                                              # the model's `end`s at which rr, bb and the history are not compared
        strict_skips_nonfinite=False,                              # check_same_end leaves them out at NONFINITE: bit for bit, a NaN equals none
        running_models_only=False,                                 # check_against takes a model that CONVERGED or ran out of budget
        rr_by_bits=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


ROWS = {
    "cg": _row("cg", cgc, lambda h, b, **kw: cgc.cg(multiply_of(h), b, **kw), running_models_only=True, strict_skips_nonfinite=True,
               workspace=functools.partial(block_bytes, vectors=3, partials=5),           # r, p, q, the five partial arrays, the state
               tri=cgc.tri, grid=cgc.lap2d, dominant=cgc.dominant, convergence=("lap2d32", "dominant4096"), bits_short_at=None),
    "bicgstab": _row("bicgstab", bc, lambda h, b, **kw: bc.bicgstab(multiply_of(h), b, **kw), running_models_only=True, strict_skips_nonfinite=True,
                     # r, rhat, p, v, t, y; <rhat,v>, <s,s>, <t,s>, <t,t>, rho twice, <r,r>, <b,b>; the state
                     workspace=functools.partial(block_bytes, vectors=6, partials=8),
                     tri=bc.tri_ns, grid=bc.upwind, dominant=bc.nonsym_dominant, convergence=("upwind32", "nonsym_dominant4096"),
                     bits_short_at=BIG),                                                   # there: one x0 / Dinv combination, a guess and a random Dinv
    "cg_columns": _row("cg_columns", cgc, None, workspace=ccc.workspace_bytes),
    "gmres": _row("gmres", gc, lambda h, b, restart, **kw: gc.gmres(multiply_of(h), b, restart, **kw), positional=dict(restart=5),
                  workspace=lambda m, item, restart: gc.workspace_bytes(m, item, restart), skip_ends=("begin:nonfinite",),
                  tri=gc.tri_ns, grid=gc.upwind, dominant=gc.nonsym_dominant),
    "cg_mixed": _row("cg_mixed", mix, lambda h, b, **kw: mix.cg_mixed(*multiplies_of(*h), b, **kw), open=pair,
                     call=lambda h: functools.partial(h[0].cg_mixed, h[1]), options=api.spmv_hip_cg_mixed_options, result=api.spmv_hip_cg_mixed_result,
                     base=dict(rtol=1e-10, atol=0.0, max_iterations=10, check_every=0, use_x0=0, update_drop=0.0, update_every=0), counts=("updates",),
                     # xn, q64; r, p, q, y; six partial arrays; the state
                     workspace=lambda m: block_bytes(m, 8, 2, 0, 0) + block_bytes(m, 4, 4, 6)),
    "lsqr": _row("lsqr", lc, lambda h, b, **kw: lc.lsqr(*multiplies_with_transpose(h), b, h.n, **kw), options=api.spmv_hip_lsqr_options,
                 result=api.spmv_hip_lsqr_result, base=dict(rtol=1e-8, atol=0.0, ls_tol=1e-8, damp=0.0, max_iterations=10, check_every=0, use_x0=0),
                 zero_tols=dict(rtol=0.0, ls_tol=0.0), has_dinv=False, x_len=lambda h, b: h.n, estimates=("ar", "anorm"),
                 workspace=lc.workspace_bytes, skip_ends=("begin:nonfinite",), rr_by_bits=True),
}


def solve(row, h, b, x0=None, **kw):
    """through host pointers, with a canary in X when there is no guess -> (x, result dict with history)"""
    x = np.full(row.x_len(h, b), CANARY, dtype=b.dtype) if x0 is None else x0.copy()
    x, res, hist = row.call(h)(b, x, x0=x0 is not None, history=True, **kw)
    res["history"] = hist
    return x, res


def solve0(row, h, b, x0=None, **kw):
    """solve with every stop test off unless the call sets one"""
    return solve(row, h, b, x0, **dict(row.zero_tols, **kw))


# ----------------------------------------------------------------------------- the checks
def check_same_end(row, model, x, res):
    """bit for bit: a run with the model's own arguments, whatever way the model ended"""
    end = model.get("end")
    got = (res["status"], res["iterations"]) + tuple(res[f] for f in row.counts + row.estimates)
    assert got == (model["status"], model["iterations"]) + tuple(model[f] for f in row.counts + row.estimates), (got, end, model.get("segments"))
    assert same_bits(x, model["x"]), end
    if end in row.skip_ends or (row.strict_skips_nonfinite and model["status"] == cgc.NONFINITE):
        return
    assert same_bits(f64(res["rr"]), f64(model["rr"])) if row.rr_by_bits else res["rr"] == model["rr"], end
    assert res["bb"] == model["bb"] and same_bits(res["history"], model["history"]), end


def check_against(row, model, k, x, res):
    """bit for bit: a run with max_iterations = k against ONE model run with a budget of at least k: iterate k of it while it goes on, its own
    end from there on"""
    assert not row.running_models_only or model["status"] in (cgc.CONVERGED, cgc.MAX_ITERATIONS)
    if k >= model["iterations"]:
        assert model["status"] != cgc.MAX_ITERATIONS or k == model["iterations"]
        return check_same_end(row, model, x, res)
    assert (res["status"], res["iterations"]) == (cgc.MAX_ITERATIONS, k)
    assert same_bits(x, model["iterates"][k])
    assert res["bb"] == model["bb"] and res["rr"] == model["history"][k] and same_bits(res["history"], model["history"][:k + 1])
    if row.estimates:
        assert tuple(res[f] for f in row.estimates) == model["estimates"][k]


def check(row, model, x, res, what=None):
    """a NaN equals a NaN: a run against a model run with the same arguments, however either ended"""
    got = (res["status"], res["iterations"]) + tuple(res[f] for f in row.counts)
    assert got == (model["status"], model["iterations"]) + tuple(model[f] for f in row.counts), (what, res, model["end"], model.get("segments"))
    assert same(x, model["x"]), (what, "x", model["end"])
    assert all(same(f64(res[f]), f64(model[f])) for f in row.estimates), (what, res, [model[f] for f in row.estimates])
    if model["end"] in row.skip_ends:
        return
    assert same(f64(res["rr"]), f64(model["rr"])) and same(f64(res["bb"]), f64(model["bb"])), (what, res, model["rr"], model["bb"])
    assert same(res["history"], model["history"]), (what, res["history"], model["history"])


# ----------------------------------------------------------------------------- shared bodies: the solver files
def bits_against_the_model(row, m, dtype, budgets=(0, 1, 2, 5)):
    """cg, bicgstab: every budget, without and with a guess, without Dinv, with Dinv = 1 and with a random Dinv"""
    csr = row.tri(m, dtype)
    rng = np.random.default_rng(m)
    b, guess = row.cases.rhs(m, dtype), rng.uniform(-1, 1, m).astype(dtype)
    jac = rng.uniform(0.5, 1.5, m).astype(dtype)
    ones = np.ones(m, dtype=dtype)
    short = m == row.bits_short_at
    with handle(csr) as h:
        for x0 in (guess,) if short else (None, guess):
            plain = None if short else row.model(h, b, x0=x0, max_iterations=5)
            pre = row.model(h, b, x0=x0, dinv=jac, max_iterations=5)
            for k in budgets:
                if not short:
                    x_none, r_none = solve(row, h, b, x0, rtol=0.0, max_iterations=k)
                    check_against(row, plain, k, x_none, r_none)
                    x_ones, r_ones = solve(row, h, b, x0, rtol=0.0, max_iterations=k, dinv=ones)
                    assert same_bits(x_ones, x_none) and same_bits(r_ones["history"], r_none["history"]) and r_ones["iterations"] == r_none["iterations"]
                x_jac, r_jac = solve(row, h, b, x0, rtol=0.0, max_iterations=k, dinv=jac)
                check_against(row, pre, k, x_jac, r_jac)


def every_method(row, method, dtype, **kw):
    csr = row.grid(32, dtype)
    b = row.cases.rhs(csr.m, dtype, 1)
    with handle(csr, method) as h:
        model = row.model(h, b, max_iterations=12, **kw)
        x, res = solve(row, h, b, rtol=0.0, max_iterations=12, **kw)
        check_against(row, model, 12, x, res)


def convergence(row, name, dtype, rtol):
    """cg, bicgstab: the model's iteration count and bits, and the true-residual bound that the host test shows the model alone to meet"""
    csr = row.grid(32, dtype) if name == row.convergence[0] else row.dominant(4096, dtype)
    b = row.cases.rhs(csr.m, dtype)
    with handle(csr) as h:
        model = row.model(h, b, rtol=rtol, max_iterations=500)
        x, res = solve(row, h, b, rtol=rtol, max_iterations=500)
    assert model["status"] == cgc.CONVERGED
    assert res["status"] == cgc.CONVERGED and res["status_name"] == "converged" and res["iterations"] == model["iterations"]
    assert same_bits(x, model["x"]) and same_bits(res["history"], model["history"]) and res["rr"] == model["rr"] and res["bb"] == model["bb"]
    true = cgc.true_residual(csr, b, x)
    print(f"{name}: {res['iterations']} iterations, true residual {true:.3e}")
    assert true <= 10 * rtol


def check_every_changes_nothing(row, dtype):
    """cg, bicgstab"""
    csr = row.grid(32, dtype)
    b = row.cases.rhs(csr.m, dtype, 2)
    rtol = 1e-8 if dtype == np.float64 else 1e-4
    with handle(csr) as h:
        model = row.model(h, b, rtol=rtol, max_iterations=400)
        assert model["status"] == cgc.CONVERGED and 8 < model["iterations"] < 400
        for every in (1, 3, 64, 0):
            x, res = solve(row, h, b, rtol=rtol, max_iterations=400, check_every=every)
            # the early exit really exits: nothing is applied behind the iteration that met the test, however many were enqueued
            assert (res["status"], res["iterations"]) == (cgc.CONVERGED, model["iterations"]), every
            assert same_bits(x, model["x"]) and same_bits(res["history"], model["history"]) and res["rr"] == model["rr"], every
        short = model["iterations"] // 2
        for every in (1, 3, 64):
            x, res = solve(row, h, b, rtol=rtol, max_iterations=short, check_every=every)
            assert (res["status"], res["status_name"], res["iterations"]) == (cgc.MAX_ITERATIONS, "max_iterations", short), every
            assert same_bits(x, model["iterates"][short]) and same_bits(res["history"], model["history"][:short + 1]), every


def pointers_give_the_same_bits(row, csr, b, guess, kw, ran, dinv=None, shift_dinv=False, each=None, last=None):
    """A solve through host pointers, then the same solve on device operands: B and X aligned and offset by one element (shift_dinv: Dinv
    too), X between canaries of one 16-byte unit each side; then device B and Dinv with a host X.  ran(result) says that the host solve did
    what the test is about; each(h, x0, want) and last(h) add what one solver has more"""
    import torch
    m, n = csr.m, guess.size
    pad = 16 // b.dtype.itemsize                         # canaries of one 16-byte unit each side keep X aligned; + 1 element: not
    shifts = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)) if shift_dinv else ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0))
    call = row.call

    def with_dinv(d):
        return kw if dinv is None else dict(kw, dinv=d)
    with row.open(csr) as h:
        for x0 in (None, guess):
            want, wres = solve(row, h, b, x0, **with_dinv(dinv))
            assert ran(wres), wres
            for shift_b, shift_x, shift_d in shifts:
                bd = torch.zeros(m + 1, dtype=torch.from_numpy(b).dtype, device=DEV)[shift_b:shift_b + m]
                bd.copy_(torch.from_numpy(b))
                jd = None
                if dinv is not None and shift_dinv:
                    jd = torch.zeros(m + 1, dtype=torch.from_numpy(dinv).dtype, device=DEV)[shift_d:shift_d + m]
                    jd.copy_(torch.from_numpy(dinv))
                elif dinv is not None:
                    jd = torch.from_numpy(dinv).to(DEV)
                buf = torch.full((n + 2 * pad + 1,), CANARY, dtype=bd.dtype, device=DEV)
                xd = buf[pad + shift_x:pad + shift_x + n]
                assert (bd.data_ptr() % 16 != 0) == bool(shift_b) and (xd.data_ptr() % 16 != 0) == bool(shift_x)
                if x0 is not None:
                    xd.copy_(torch.from_numpy(x0))
                got, res, hist = call(h)(bd, xd, x0=x0 is not None, history=True, **with_dinv(jd))
                torch.cuda.synchronize()
                assert got is xd and same_bits(xd.cpu().numpy(), want), (shift_b, shift_x, shift_d)
                assert same_bits(hist, wres["history"]) and all(res[f] == wres[f] for f in ("rr",) + row.counts + row.estimates)
                out = buf.cpu().numpy()
                assert (out[:pad + shift_x] == CANARY).all() and (out[pad + shift_x + n:] == CANARY).all(), "written outside X"
            # mixed: device B, host X, device Dinv
            xh = np.full(n, CANARY, dtype=guess.dtype) if x0 is None else x0.copy()
            bd = torch.from_numpy(b).to(DEV)
            call(h)(bd, xh, x0=x0 is not None, **with_dinv(None if dinv is None else torch.from_numpy(dinv).to(DEV)))
            assert same_bits(xh, want)
            if each is not None:
                each(h, x0, want)
        if last is not None:
            last(h)


def caller(lib, raw):
    """raw(h, opt, res, ...) -> rc, between a cleared error state and the assertion that the call left its code there"""
    def call(*args, **kw):
        lib.spmv_hip_clear_error()
        rc = raw(*args, **kw)
        assert lib.spmv_hip_last_error() == rc
        lib.spmv_hip_clear_error()
        return rc
    return call


def options_of(row):
    def options(**kw):
        return C.byref(row.options(**dict(row.base, **kw)))
    return options


def raw_call(row, lib, csr, b, x):
    """the C entry point on csr's own arrays: call(h, opt, res, B=b, X=x, mat=csr, and the row's positional arguments by name)"""
    def raw(h, opt, res, B=b, X=x, mat=csr, **kw):
        between = [kw.get(key, default) for key, default in row.positional.items()]
        return getattr(lib, row.symbol)(h, mat.m, api._ptr(mat.rowptr), api._ptr(mat.colidx), api._ptr(mat.val), api._ptr(B), api._ptr(X), *between, opt, res)
    return caller(lib, raw)


def common_argument_errors(csr, x, call, options, res, bad=BAD_OPTIONS, more=None, good=None, square=True, after=None):
    """What every single-handle solver refuses, X untouched: null options, result, B, X and handle; bad options; (square) a handle created
    with m != n; multi-GPU and host_rows handles; a cleared handle.  more(h): the solver's own refusals; good: the arguments of the call that
    then runs; after(): more handles to refuse"""
    with handle(csr) as h:
        assert call(h.h, None, res) == E_ARG and call(h.h, options(), None) == E_ARG
        assert call(h.h, options(), res, B=None) == E_ARG and call(h.h, options(), res, X=None) == E_ARG
        for kw in bad:
            assert call(h.h, options(**kw), res) == E_ARG, kw
        if more is not None:
            more(h)
        assert call(None, options(), res) == E_ARG
        assert (x == CANARY).all()
        assert call(h.h, options(), res, **(good or {})) == 0 and not (x == CANARY).any()      # the same call with good arguments runs
    x[:] = CANARY
    if square:
        wide = cgc.synth.CSR(csr.m, csr.m + 1, csr.rowptr, csr.colidx, csr.val)               # m != n at create
        with handle(wide) as h:
            assert call(h.h, options(), res) == E_ARG
    for key, way in (("gpus", api.VECTORIZED_WAY.VECTOR_HIP), ("host_rows", api.VECTORIZED_WAY.VECTOR_NONE)):
        with handle(csr, M.Method_Serial, way, **{key: 1}) as h:
            assert call(h.h, options(), res) == E_ARG, key
    if after is not None:
        after()
    h = handle(csr)
    api.spmv_clear_handle(h.h)
    assert call(h.h, options(), res) == E_NOSTATE
    h.close()
    assert (x == CANARY).all()


def argument_errors(row, lib, csr, **kw):
    """common_argument_errors through the row's C entry point; kw["more"] and kw["after"] take (call, options, res)"""
    b, x = row.cases.rhs(csr.m, np.float64), np.full(csr.n, CANARY)
    call, options, res = raw_call(row, lib, csr, b, x), options_of(row), C.byref(row.result())
    for key in ("more", "after"):
        if key in kw:
            kw[key] = functools.partial(kw[key], call, options, res)
    common_argument_errors(csr, x, call, options, res, **kw)


def m_zero_is_converged(row, **kw):
    empty = empty_csr()
    with handle(empty) as h:
        rc, res = row.api(h.h, 0, empty.rowptr, empty.colidx, empty.val, None, None, max_iterations=5, **kw)
    assert rc == 0 and converged_at_zero(res)


def a_reordered_handle_solves_the_permuted_system(row, **kw):
    csr = row.dominant(4096, np.float64)
    b = row.cases.rhs(csr.m, np.float64, 6)
    with handle(csr, reorder=1) as h:
        perm = h.index
        assert perm is not None and sorted(perm.tolist()) == list(range(csr.m))
        bp = np.ascontiguousarray(b[perm])                                         # XX[i] = X[index[i]], as for spmv()
        model = row.model(h, bp, rtol=1e-10, max_iterations=200, **kw)
        xp, res = solve(row, h, bp, rtol=1e-10, max_iterations=200, **kw)
    assert res["status"] == cgc.CONVERGED
    check_same_end(row, model, xp, res)
    x = np.empty_like(xp)
    x[perm] = xp
    assert cgc.true_residual(csr, b, x) <= 1e-9


# ----------------------------------------------------------------------------- shared bodies: the ends files
def budget_edges(k, model_at, solve_at, expect, what, check_, everys=(0, 1), budgets=None):
    """budgets of k - 1, k and k + 1 around an end at iteration k, each run against a model run with that budget.  model_at(budget) -> model;
    expect(budget, short): the assertions on that model; solve_at(budget, every) -> (x, res)"""
    for budget in (k - 1, k, k + 1) if budgets is None else budgets:
        if budget < 0:
            continue
        short = model_at(budget)
        expect(budget, short)
        for every in everys:
            x, res = solve_at(budget, every)
            check_(short, x, res, what + (budget, every))


def atol_ladder(model, run, check_, a, k, what, before, same_end=lambda p, q: ended(p) == ended(q), target=lambda at, a: at["rr"], converges=True):
    """The value that the stop test compares at iteration k is the square of the double a.  atol = a ends the run there (the test is <=) and
    the next double below does not: before(at, under) asserts that of the two models; with a small rtol beside it atol still decides, and with
    a small atol beside a large rtol, rtol does.  model(atol, rtol=0.0) -> model run; run(**keywords) -> (x, res) of the solve"""
    below = float(np.nextafter(a, 0.0))
    at, under = model(a), model(below)
    before(at, under)
    for every in (1, 0):
        x, res = run(atol=a, check_every=every)
        check_(at, x, res, what)
        x, res = run(atol=below, check_every=every)
        check_(under, x, res, what + ("below",))
    # rtol^2 bb is the smaller: atol still decides, at the same place
    small = 2.0 ** -30
    while small * small * at["bb"] >= a * a:
        small *= 2.0 ** -30
    assert small * small * at["bb"] < a * a
    both = model(a, rtol=small)
    assert same_end(both, at), what
    x, res = run(rtol=small, atol=a)
    check_(both, x, res, what + ("rtol below",))
    # ... and the reverse: atol^2 is the smaller, rtol decides: the run ends where atol alone does not end it
    goal = target(at, a)
    rtol = 2.0 ** 20
    while rtol * rtol * at["bb"] / 4 >= goal:
        rtol /= 2                                                      # the smallest power of two with rtol^2 bb >= the goal
    low = a * 2.0 ** -10
    by_rtol, alone = model(low, rtol=rtol), model(low)
    assert rtol * rtol * at["bb"] >= goal > low * low
    assert not converges or (by_rtol["status"] == cgc.CONVERGED and by_rtol["iterations"] <= k)
    assert not same_end(alone, by_rtol), what
    x, res = run(rtol=rtol, atol=low)
    check_(by_rtol, x, res, what + ("rtol above",))


def guess_and_jacobi_iterations(row, h, csr, dtype, seed, budget, jac=None, **kw):
    """cg, bicgstab, gmres: `budget` iterations without and with a guess and Dinv (1 / diagonal unless one is given), against the model on this
    handle's spmv()"""
    rng = np.random.default_rng(seed)
    b, guess = cgc.rhs(csr.m, dtype, seed), rng.uniform(-1, 1, csr.m).astype(dtype)
    if jac is None:
        jac = (1.0 / cgc.diagonal(csr).astype(np.float64)).astype(dtype)
    for x0, dinv in ((None, None), (guess, jac)):
        model = row.model(h, b, x0=x0, dinv=dinv, max_iterations=budget, **kw)
        assert model["iterations"] == budget and np.isfinite(model["x"]).all(), ended(model)
        x, res = solve0(row, h, b, x0, dinv=dinv, max_iterations=budget, **kw)
        check(row, model, x, res, (x0 is not None,))


def check_executor_layout(info, method, longest=2049):
    """a matrix with a dense first row of `longest` entries, as built under `method`"""
    first, long_rows = EXECUTORS[method]
    names = info["launch_kernels"]
    assert info["max_row_len"] == longest and info["cache_blocked"] == 0 and info["far_nnz"] == 0, info
    assert first is None or names[0] == first, names
    if long_rows:
        assert len(names) == 3 and names[1] in LONG_ROW_KERNELS and names[2] == "csr5_fixup_kernel", names
    elif first != "csr_scalar_kernel":
        assert names[-1] == "csr5_fixup_kernel" and names[0] in ("nat_group_kernel",) + LONG_ROW_KERNELS, names   # carries and their fix-up


def check_blocked_layout(info):
    """the row-block x column-slab executor (cache_block = 2)"""
    assert info["cache_blocked"] == 1 and info["launch_kernels"] in (["blk_kernel"], ["blk_wide_kernel"]), info


def check_tile_layout(info, csr, pack):
    """sec.band32(1280, long_row=300) at 8 lanes per row: the CSR-vector TILE kernel with the long-row launch behind it; pack: every tile but
    row 300's streams 7-byte values"""
    names = info["launch_kernels"]
    assert info["lanes_per_row"] == 8 and info["max_row_len"] == 544, info
    assert len(names) == 3 and names[0] == pc.TILE_KERNEL and names[1] in LONG_ROW_KERNELS and names[2] == "csr5_fixup_kernel", names
    if pack:
        want, flags = pc.model_packed(csr.rowptr, csr.val, 8)
        assert flags == [True, False, True, True, True] and info["packed_nnz"] == want == info["nnz"] - (255 * 32 + 544) > 0, info
    else:
        assert info["packed_nnz"] == 0


def every_executor(csr, method, iterate, longest=2049):
    """a dense first row and column: a row longer than any long-row threshold, a carry across every CSR5 / nnz-split tile boundary.  As built,
    and on the row-block x column-slab executor (cache_block = 2; CSR-scalar schedules never take it); iterate(h, seed) solves on each"""
    with handle(csr, method) as h:
        check_executor_layout(h.info(), method, longest)
        iterate(h, 1)
    if EXECUTORS[method][0] == "csr_scalar_kernel":
        return
    with handle(csr, method, cache_block=2) as h:
        check_blocked_layout(h.info())
        iterate(h, 2)


def the_long_row_launch_beside_the_tile_kernel(dtype, iterate):
    """rows of 32 aligned entries at 8 lanes per row run on the CSR-vector TILE kernel; row 300 (544 entries > long_thr = 512) goes to the
    long-row launch behind it.  fp64 also with pack_values = 1: every tile but row 300's streams 7-byte values; iterate(h, csr, seed) solves"""
    csr = sec.band32(1280, dtype, long_row=300)
    for pack in (0, 1) if dtype == np.float64 else (0,):
        with handle(csr, M.Method_Parallel, lanes_per_row=8, pack_values=pack) as h:
            check_tile_layout(h.info(), csr, pack)
            iterate(h, csr, 3 + pack)


# ----------------------------------------------------------------------------- cg_columns: k columns in one call
def solve_columns(h, B, X0=None, **kw):
    """through host pointers -> (X, list of result dicts, history)"""
    X = np.full(B.shape, CANARY, dtype=B.dtype) if X0 is None else np.ascontiguousarray(X0).copy()
    return h.cg_columns(np.ascontiguousarray(B), X, x0=X0 is not None, history=True, **kw)


def same_values(a, b):
    """same_bits, but a NaN matches a NaN whatever its payload (the model's NaN is numpy's, the device's is the hardware's)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and same_bits(np.where(nan, 0.0, a), np.where(nan, 0.0, b))


def check_column(model, budget, x, res, hist):
    """column of a run with max_iterations = budget against its model run with a budget of at least that"""
    its = min(budget, model["iterations"])
    over = model["status"] != cgc.MAX_ITERATIONS and model["iterations"] <= budget
    assert (res["status"], res["iterations"]) == (model["status"] if over else cgc.MAX_ITERATIONS, its)
    assert same_bits(x, model["iterates"][its])
    assert same_values(res["bb"], model["bb"]) and same_values(res["rr"], model["history"][its])
    assert same_values(hist[:its + 1], model["history"][:its + 1])
    assert np.isnan(hist[its + 1:]).all()                  # behind the column's end nothing was written (api.cg_columns fills with NaN)


def check_columns(models, budget, X, res, hist):
    assert len(res) == X.shape[1] == len(models) and hist.shape == (1 + max(r["iterations"] for r in res), len(models))
    for j, model in enumerate(models):
        check_column(model, budget, X[:, j], res[j], hist[:, j])


def run_bits(csr, dtype, ks, seed, budgets=(0, 1, 2, 5)):
    """the first k columns for every k of ks at every budget, without and with guesses, without Dinv, with Dinv = 1 and with a random Dinv"""
    m = csr.m
    rng = np.random.default_rng(m + seed)
    kmax = max(ks)
    B, G = ccc.columns(m, kmax, dtype, seed), rng.uniform(-1, 1, (m, kmax)).astype(dtype)
    jac = rng.uniform(0.5, 1.5, m).astype(dtype)
    with handle(csr) as h:
        mul = ccc.spmm_column(h)
        for X0 in (None, G):
            plain = ccc.solve(mul, B, X0, max_iterations=5)
            pre = ccc.solve(mul, B, X0, dinv=jac, max_iterations=5)
            for k in ks:
                Bk, X0k = B[:, :k], None if X0 is None else np.ascontiguousarray(X0[:, :k])
                for budget in budgets:
                    X, res, hist = solve_columns(h, Bk, X0k, rtol=0.0, max_iterations=budget)
                    check_columns(plain[:k], budget, X, res, hist)
                    X1, res1, hist1 = solve_columns(h, Bk, X0k, rtol=0.0, max_iterations=budget, dinv=np.ones(m, dtype=dtype))
                    assert same_bits(X1, X) and same_bits(hist1, hist) and res1 == res
                    X, res, hist = solve_columns(h, Bk, X0k, rtol=0.0, max_iterations=budget, dinv=jac)
                    check_columns(pre[:k], budget, X, res, hist)
