"""The host model of spmv_hip_cg_mixed and the cases its tests share (tests/test_cg_mixed_host.py, tests/test_gpu_cg_mixed.py).

`cg_mixed` restates the arithmetic contract of include/spmv_hip.h ("mixed-precision conjugate gradients") in numpy on cg_cases.dot, so that a
solve can be compared BIT FOR BIT.  It takes TWO multiply callbacks: `high` multiplies a float64 vector, `low` a float32 one.  On the GPU they
are the two handles' own spmv(), on the CPU cg_cases.matvec of the matrix and of its float copy.

The contract, restated.  "dot" is cg_cases.dot over float64 elements, or over float32 elements widened.  All scalars are fp64; every product,
sum and quotient is separate; "narrow" is round-to-nearest-even to float32 (astype), widening is exact.  thr = max(rtol^2 bb, atol^2).
  start          x = x0 or 0; r64 = b - high(x), or b; bb = dot(b,b); rr = dot(r64,r64); non-finite -> NONFINITE; bb == 0 -> x = 0, CONVERGED;
                 rr <= thr -> CONVERGED; max_iterations == 0 -> MAX_ITERATIONS
  segment start  r = narrow(r64); y = 0; z = dinv*r or r; rz = dot(r,z); rs = dot(r,r); seg = rs; n = 0; non-finite -> NONFINITE; rs == 0 ->
                 STAGNATED; rz <= 0 -> BREAKDOWN; p = z in the first segment and behind an "exact" end, else p is KEPT
  iteration      cg_cases.cg's in float32 on y; then 1. non-finite rs or rzn -> NONFINITE; 2. rs == 0 ends the segment "exact", p untouched;
                 3. rzn <= 0 -> BREAKDOWN; 4. beta = float(rzn / rz), non-finite -> NONFINITE; 5. p = z + beta*p; 6. the segment ends on the first
                 of "estimate" rs <= thr, "drop" rs <= (update_drop*update_drop)*seg, "every" n == update_every, "budget" iterations == max_iterations
  update         xn = x + widen(y); r64n = b - high(xn); rrn = dot(r64n,r64n); non-finite -> NONFINITE, x kept; rrn >= rr behind "exact",
                 "estimate" or "drop" -> STAGNATED, x and rr kept; else commit x, r64, rr, updates + 1; rr <= thr -> CONVERGED; iterations ==
                 max_iterations -> MAX_ITERATIONS; else a new segment
  history        [0] the initial rr; [k] rs after iteration k, overwritten by the committed rr where a committed update follows iteration k"""
import numpy as np

import cg_cases as cgc
from spmv_amd import synth

CONVERGED, MAX_ITERATIONS, BREAKDOWN, NONFINITE, STAGNATED = 0, 1, 2, 3, 4
UPDATE_DROP = 0.01  # SPMV_HIP_CG_MIXED_UPDATE_DROP


def cg_mixed(high, low, b, x0=None, dinv=None, rtol=0.0, atol=0.0, max_iterations=0, update_drop=0.0, update_every=0, watch=None):
    """-> dict: x, status, iterations, updates, rr (the TRUE one of x), bb, history, iterates (iterates[k] = committed x + widen(y) after
    iteration k: what an update behind iteration k would try), segments (the test that ended each segment, in order) and end (where and why
    the solve ended).  watch(*values, what=None), when given, sees every vector and every scalar, float or fp64, as it is formed; what="iteration":
    the call behind cg_update, its last value the recurrence's <r,r>; what="update": the call behind an update's residual, its last value the rr tried."""
    f32, f64 = np.float32, np.float64
    assert b.dtype == f64 and (dinv is None or dinv.dtype == f32)
    m = b.size
    if m == 0:
        return dict(x=b.copy(), status=CONVERGED, iterations=0, updates=0, rr=0.0, bb=0.0, history=np.zeros(0), iterates=[], segments=[], end="start:empty")
    fin, dot = np.isfinite, cgc.dot
    drop = update_drop if update_drop > 0 else UPDATE_DROP
    drop2 = drop * drop
    st = dict(k=0, updates=0)
    see = watch if watch is not None else (lambda *values, what=None: None)
    history, iterates, segments = [], [], []

    def out(x, status, rr, bb, end):
        return dict(x=x, status=status, iterations=st["k"], updates=st["updates"], rr=rr, bb=bb, history=np.array(history), iterates=iterates, segments=segments, end=end)

    with np.errstate(all="ignore"):
        if x0 is None:
            x, r64 = np.zeros_like(b), b.copy()
        else:
            x = x0.copy()
            ax = high(x)
            r64 = b - ax
            see(ax)
        bb, rr = dot(b, b), dot(r64, r64)
        see(b, x, r64, f64(bb), f64(rr)) if dinv is None else see(b, x, r64, f64(bb), f64(rr), dinv)
        thr = max(rtol * rtol * bb, atol * atol)
        see(f64(rtol * rtol), f64(rtol * rtol * bb), f64(atol * atol), f64(drop2))
        history.append(rr)
        iterates.append(x.copy())
        if not (fin(bb) and fin(rr)):
            return out(x, NONFINITE, rr, bb, "start:nonfinite")
        if bb == 0:
            history[0] = 0.0
            return out(np.zeros_like(b), CONVERGED, 0.0, bb, "start:bb_zero")
        if rr <= thr:
            return out(x, CONVERGED, rr, bb, "start:converged")
        if max_iterations == 0:
            return out(x, MAX_ITERATIONS, rr, bb, "start:budget")
        p = None
        while True:
            r = r64.astype(f32)                           # narrow
            y = np.zeros(m, dtype=f32)
            z = dinv * r if dinv is not None else r.copy()
            rz, rs = dot(r, z), dot(r, r)
            see(r, z, f64(rz), f64(rs))
            seg, n = rs, 0
            if not (fin(rs) and fin(rz)):
                return out(x, NONFINITE, rr, bb, "segment:nonfinite")
            if rs == 0:
                return out(x, STAGNATED, rr, bb, "segment:zero")
            if rz <= 0:
                return out(x, BREAKDOWN, rr, bb, "segment:rz_breakdown")
            if p is None:
                p = z.copy()
            reason = None
            while reason is None:
                q = low(p)
                pq = dot(p, q)
                see(p, q, f64(pq))
                if not (fin(pq) and fin(rz)):
                    return out(x, NONFINITE, rr, bb, "update:dot_nonfinite")
                if pq <= 0:
                    return out(x, BREAKDOWN, rr, bb, "update:pq_breakdown")
                alpha = f32(f64(rz) / f64(pq))           # fp64 quotient, rounded to float once
                see(f64(rz) / f64(pq), alpha)
                if not fin(alpha):
                    return out(x, NONFINITE, rr, bb, "update:alpha_nonfinite")
                ap, aq = alpha * p, alpha * q
                y = y + ap                                 # a multiply, then an add, in float
                r = r - aq
                z = dinv * r if dinv is not None else r
                rzn, rs = dot(r, z), dot(r, r)
                see(ap, aq, y, r, z, f64(rzn), f64(rs), what="iteration")
                st["k"] += 1
                n += 1
                history.append(rs)
                iterates.append(x + y.astype(f64))
                if not (fin(rs) and fin(rzn)):
                    return out(x, NONFINITE, rr, bb, "direction:nonfinite")
                if rs == 0:
                    reason = "exact"                       # p untouched
                    break
                if rzn <= 0:
                    return out(x, BREAKDOWN, rr, bb, "direction:rz_breakdown")
                beta = f32(f64(rzn) / f64(rz))
                see(f64(rzn) / f64(rz), beta)
                if not fin(beta):
                    return out(x, NONFINITE, rr, bb, "direction:beta_nonfinite")
                bp = beta * p
                p = z + bp
                see(bp, p)
                rz = rzn
                if rs <= thr:
                    reason = "estimate"
                elif rs <= drop2 * seg:
                    reason = "drop"
                elif update_every > 0 and n == update_every:
                    reason = "every"
                elif st["k"] == max_iterations:
                    reason = "budget"
            segments.append(reason)
            xn = x + y.astype(f64)                        # widen, an fp64 add
            axn = high(xn)
            r64n = b - axn
            rrn = dot(r64n, r64n)
            see(axn, xn, r64n, f64(rrn), what="update")
            if not fin(rrn):
                return out(x, NONFINITE, rr, bb, "resume:nonfinite")
            if reason in ("exact", "estimate", "drop") and rrn >= rr:
                return out(x, STAGNATED, rr, bb, "resume:stagnated")
            x, r64, rr = xn, r64n, rrn
            st["updates"] += 1
            history[st["k"]] = rr
            if rr <= thr:
                return out(x, CONVERGED, rr, bb, "resume:converged")
            if st["k"] == max_iterations:
                return out(x, MAX_ITERATIONS, rr, bb, "resume:budget")
            if reason == "exact":
                p = None


# ----------------------------------------------------------------------------- matrices and callbacks
def narrowed(csr):
    """the float copy of a float64 matrix: the same pattern, the values rounded to float32"""
    return synth.CSR(csr.m, csr.n, csr.rowptr, csr.colidx, csr.val.astype(np.float32))


def with_values(csr, val):
    return synth.CSR(csr.m, csr.n, csr.rowptr, csr.colidx, np.ascontiguousarray(val))


def callbacks(csr, low=None):
    """(high, low) multiplies on the CPU: cg_cases.matvec of a float64 matrix and of `low` (default: its float copy)"""
    return cgc.matvec(csr), cgc.matvec(narrowed(csr) if low is None else low)


def almost_identity(m):
    """(1 + 2^-30) I in float64, whose float copy is I: the first iteration of every segment leaves r = 0 exactly"""
    i = np.arange(m, dtype=np.int32)
    return synth.CSR(m, m, np.arange(m + 1, dtype=np.int32), i, np.full(m, 1.0 + 2.0 ** -30))


# every segment end and every status, by name: -> (high matrix, low matrix, b, keyword arguments, the status, the segment end or solve end the
# case is there for).  Small: one workgroup or two.  "stagnated": `low` is A / 4, so a segment's y is 4 A^-1 r and the true residual becomes -3 r:
# the recurrence claims a drop that the truth does not show.  (A `low` of 2 A would not do: y = A^-1 r / 2 halves the true residual at every
# update, which is slow progress, not stagnation.)
def named_cases():
    tri, lap = cgc.tri(1025), cgc.lap2d(12)
    b_tri, b_lap = cgc.rhs(1025, np.float64), cgc.rhs(144, np.float64, 3)
    sg = cgc.signs(1025)
    inf_b = b_tri.copy()
    inf_b[7] = np.inf
    big_b = b_tri.copy()
    big_b[7] = 1e39                                           # finite in fp64, an infinity on narrowing
    ident = almost_identity(1025)
    return {
        "estimate": (tri, narrowed(tri), b_tri, dict(rtol=0.5, max_iterations=50), CONVERGED, "estimate"),
        "drop": (lap, narrowed(lap), b_lap, dict(rtol=1e-12, max_iterations=500), CONVERGED, "drop"),
        "every": (lap, narrowed(lap), b_lap, dict(rtol=1e-12, max_iterations=500, update_drop=0.001, update_every=3), CONVERGED, "every"),
        "budget": (lap, narrowed(lap), b_lap, dict(rtol=1e-12, max_iterations=7, update_drop=1e-6), MAX_ITERATIONS, "budget"),
        "exact": (ident, narrowed(ident), b_tri, dict(rtol=1e-14, max_iterations=20), CONVERGED, "exact"),
        "stagnated": (tri, with_values(tri, (0.25 * tri.val).astype(np.float32)), b_tri, dict(rtol=1e-12, max_iterations=200), STAGNATED, "resume:stagnated"),
        "vanished": (tri, narrowed(tri), 1e-50 * b_tri, dict(rtol=1e-12, max_iterations=200), STAGNATED, "segment:zero"),
        "breakdown": (sg, narrowed(sg), np.ones(1025), dict(rtol=0.0, max_iterations=9, update_drop=1e-6), BREAKDOWN, "update:pq_breakdown"),
        "inf_in_b": (tri, narrowed(tri), inf_b, dict(rtol=1e-12, max_iterations=50), NONFINITE, "start:nonfinite"),
        "overflow_on_narrowing": (tri, narrowed(tri), big_b, dict(rtol=1e-12, max_iterations=50), NONFINITE, "segment:nonfinite"),
    }
