"""What the wide-spread attention tests share: a bias that spreads a row's scores over [-S, 0] below a per-row constant, and DERIVED error bars
for every output of the bias entry points against the wide reference lse_cases.reference (float64 for fp32 handles, np.longdouble for fp64),
taken from the operands as the kernel receives them.

The bars, first order in u (the unit roundoff of the handle's type; eps = 2u), for one row i of n entries and one head.  Reference values:
t_p = s_p * scale + B_p, M = max t, d_p = t_p - M, P_p = exp(d_p) / Z, L = M + log Z, dP_p = <G_i, V_p>, D = sum P dP, dB_p = P_p (dP_p - D),
dS_p = dB_p * scale.  E = 2 ulp for exp (test_gpu_fused_attention.py); tiny is the smallest normal number: whatever falls below it may be flushed.

  delta_p  = (k + 2) u |scale| sum_c |Q_ic K_pc| + u |t_p|      the dot and the scaling (test_gpu_fused_attention.check_accuracy) and the bias
                                                                addition's rounding: the absolute error of the kernel's t_p
  barP_p   = 2 P_p (u (|d_p| + sum_q P_q |d_q| + 4E + a(n) + 1) + delta_p + sd) + 2 tiny,   sd = sum_q P_q delta_q
                                                                check_accuracy's bar with its `n` for Z's sum replaced by a(n) = lse_cases.a_len(n),
                                                                the additions on the longest path of the documented order (27 or less; all
                                                                terms are positive, so the sum errs by a(n) u relatively), and 1 for the
                                                                quotient; exp(d_p) and the quotient may each be flushed
  barO_c   = sum_p barP_p |V_pc| + (n + 1) u sum_p P_p |V_pc| + (n + 1) tiny          P's error through the chain, the chain's gamma_n
  errL     = l_bound(n, L) + 2 sd                               lse_cases.l_bound is for the kernel's own t_p; a change delta of the scores
                                                                moves log-sum-exp by sum_q P_q delta_q (doubled like barP's first-order terms)
  bdP_p    = (dv + 1) u sum_c |G_ic V_pc|                        the dot's gamma_dv
  bD       = sum_p (barP_p |dP_p| + P_p bdP_p) + (n + 1) u sum_p P_p |dP_p|
  bdB_p    = barP_p |dP_p - D| + P_p (bdP_p + bD) + 2 u |dB_p| + tiny                 the subtraction and the product round once each
  bdS_p    = |scale| bdB_p + u |dS_p| + tiny
  bdQ_c    = sum_p bdS_p |K_pc| + (n + 1) u sum_p |dS_p K_pc| + (n + 1) tiny
  bdK_jc   = sum over column j's entries and the group's heads of bdS_p |Q_ic|, + (len_j + gs + 1) u sum |dS_p Q_ic| + (len_j gs + 1) tiny
                                                                a chain of len_j terms per head, gs - 1 additions over the group
  bdV_jc   = the same with barP_p |G_ic| and |P_p G_ic|

Driven by L (spmv_hip_attention_gqa_backward_lse on the forward's own O and L): P_p = exp(t_p - L) is not normalised, so the error of L itself --
its rounding, half an eps of |L|, is inside l_bound -- enters P relatively and does not cancel:
  barP'_p  = 2 P_p (u |t_p - L| + 4E u + delta_p + errL) + 2 tiny                     errL grows like u |L|: the limit of the L-driven paths
  bD'      = sum_c |G_ic| barO_c + (dv + 1) u sum_c |G_ic O_ic|                        D = <G_i, O_i> from the forward's O
and bdB', bdS', bdQ', bdK', bdV' follow from them as above.

The merge of two parts r = 1, 2 (spmv_hip_attention_merge), w_r = exp(L_r - Lm), W = w_1 + w_2, omega_r = exp(L_r - L) the exact weights:
  ew       = max_r (u |L_r - Lm| + 4E u + errL_r) + max_r errL_r                       the relative error of a weight: its own L's and Lm's
  barO_c   = 2 sum_r omega_r (barO_r,c + |O_r,c| (2 ew + 4u)) + 2 tiny                 w_r / W errs by ew + (ew + u); three more roundings
  barL     = max_r errL_r + ew + (LOG_ULP ln 2 + 1) u + u max(1, |L|)                  Lm's error, log W's (W in [1, 2]), the addition's
A part without entries on the row has omega_r = 0 and contributes nothing."""
import numpy as np

import lse_cases as lc

UNIT = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
E_ULP = 2
SPREADS = {np.dtype(np.float32): [30, 95, 120], np.dtype(np.float64): [30, 730, 800]}   # both sides of exp's denormal and zero thresholds
CONSTANTS = [0.0, 4096.0, -4096.0]
HEADS, KV, K, DV = 2, 1, 5, 3


def spread_bias(csr, heads, S, seed=0):
    """(heads, nnz) planes: C_i + a spread in [-S, 0]; C_i cycles through 0, 2^12, -2^12 by row; a row's first entry has spread 0 and its last -S"""
    rng = np.random.default_rng(1000 * S + heads + seed)
    lens = np.diff(csr.rowptr)
    rows = np.repeat(np.arange(csr.m), lens)
    sp = rng.uniform(-S, 0, (heads, csr.nnz))
    has = lens > 0
    sp[:, csr.rowptr[1:][has] - 1] = -S
    sp[:, csr.rowptr[:-1][has]] = 0
    return (np.asarray(CONSTANTS)[rows % 3] + sp).astype(csr.val.dtype)


class Bars:
    pass


def bars(csr, heads, kv, Q, K, V, B, scale, G):
    """-> the bars of the module's docstring as arrays shaped like the outputs: O, errL (heads, m), dQ, dK, dV, dB and, for the L-driven
    backward, dQl, dKl, dVl, dBl; also the reference's own O and L (for the merge's bars)"""
    dt = np.dtype(csr.val.dtype)
    T, u = lc.hp(dt), UNIT[dt]
    tiny = T(np.finfo(dt).tiny)
    gs, k, dv = heads // kv, Q.shape[1] // heads, V.shape[1] // kv
    Qh, Kh, Vh, Gh = Q.astype(T), K.astype(T), V.astype(T), G.astype(T)
    sc = T(dt.type(scale))
    clen = np.bincount(csr.colidx, minlength=csr.n).astype(T)[:, None]
    b = Bars()
    b.O, b.Oref, b.dQ, b.dQl = (np.zeros((csr.m, w), dtype=T) for w in (heads * dv, heads * dv, heads * k, heads * k))
    b.errL, b.Lref = np.zeros((heads, csr.m), dtype=T), np.full((heads, csr.m), -np.inf, dtype=T)
    b.dB, b.dBl = np.zeros((heads, csr.nnz), dtype=T), np.zeros((heads, csr.nnz), dtype=T)
    eK, eKl, aK = (np.zeros((csr.n, kv * k), dtype=T) for _ in range(3))
    eV, eVl, aV = (np.zeros((csr.n, kv * dv), dtype=T) for _ in range(3))
    for i in range(csr.m):
        s, e = int(csr.rowptr[i]), int(csr.rowptr[i + 1])
        n = e - s
        if n == 0:
            continue
        cols = csr.colidx[s:e]
        for hd in range(heads):
            g = hd // gs
            kc, vc = slice(g * k, (g + 1) * k), slice(g * dv, (g + 1) * dv)
            Kr, Vr, q, gi = Kh[cols, kc], Vh[cols, vc], Qh[i, hd * k:(hd + 1) * k], Gh[i, hd * dv:(hd + 1) * dv]
            aKr, aVr = np.abs(Kr), np.abs(Vr)
            t = (Kr @ q) * sc + B[hd, s:e].astype(T)
            delta = (k + 2) * u * abs(sc) * (aKr @ np.abs(q)) + u * np.abs(t)
            M = t.max()
            d = t - M
            ex = np.exp(d)
            Z = ex.sum()
            P = ex / Z
            L = M + np.log(Z)
            sd = (P * delta).sum()
            barP = 2 * P * (u * (np.abs(d) + (P * np.abs(d)).sum() + 4 * E_ULP + lc.a_len(n) + 1) + delta + sd) + 2 * tiny
            O = P @ Vr
            barO = barP @ aVr + (n + 1) * u * (P @ aVr) + (n + 1) * tiny
            errL = T(lc.l_bound(n, L, dt)) + 2 * sd
            b.O[i, hd * dv:(hd + 1) * dv], b.Oref[i, hd * dv:(hd + 1) * dv], b.errL[hd, i], b.Lref[hd, i] = barO, O, errL, L
            dP = Vr @ gi
            bdP = (dv + 1) * u * (aVr @ np.abs(gi))
            D = (P * dP).sum()
            x = dP - D
            dB = P * x
            dS = dB * sc
            barPl = 2 * P * (u * np.abs(t - L) + 4 * E_ULP * u + delta + errL) + 2 * tiny
            bD = (barP * np.abs(dP) + P * bdP).sum() + (n + 1) * u * (P * np.abs(dP)).sum()
            bDl = np.abs(gi) @ barO + (dv + 1) * u * (np.abs(gi) @ np.abs(O))
            for bp, bd, odb, odq, ek, ev in ((barP, bD, b.dB, b.dQ, eK, eV), (barPl, bDl, b.dBl, b.dQl, eKl, eVl)):
                bdB = bp * np.abs(x) + P * (bdP + bd) + 2 * u * np.abs(dB) + tiny
                bdS = abs(sc) * bdB + u * np.abs(dS) + tiny
                odb[hd, s:e] = bdB
                odq[i, hd * k:(hd + 1) * k] = bdS @ aKr + (n + 1) * u * (np.abs(dS) @ aKr) + (n + 1) * tiny
                np.add.at(ek[:, kc], cols, np.outer(bdS, np.abs(q)))
                np.add.at(ev[:, vc], cols, np.outer(bp, np.abs(gi)))
            np.add.at(aK[:, kc], cols, np.outer(np.abs(dS), np.abs(q)))
            np.add.at(aV[:, vc], cols, np.outer(P, np.abs(gi)))
    chain = (clen + gs + 1) * u
    flush = (clen * gs + 1) * tiny
    b.dK, b.dKl, b.dV, b.dVl = eK + chain * aK + flush, eKl + chain * aK + flush, eV + chain * aV + flush, eVl + chain * aV + flush
    return b


def merge_bars(parts, heads, dtype):
    """-> (barO (m, heads * dv), barL (heads, m)) of the two parts' merge from their Bars (the module's docstring)"""
    dt = np.dtype(dtype)
    T, u = lc.hp(dt), UNIT[dt]
    tiny = T(np.finfo(dt).tiny)
    p1, p2 = parts
    dv = p1.O.shape[1] // heads
    Lm = np.maximum(p1.Lref, p2.Lref)
    with np.errstate(invalid="ignore"):
        L = Lm + np.log(np.exp(p1.Lref - Lm) + np.exp(p2.Lref - Lm))
        om = [np.where(np.isfinite(p.Lref), np.exp(p.Lref - L), 0) for p in parts]
        rel = [np.where(np.isfinite(p.Lref), u * np.abs(p.Lref - Lm) + 4 * E_ULP * u + p.errL, 0) for p in parts]
    worst = np.maximum(p1.errL, p2.errL)
    ew = np.maximum(*rel) + worst
    barL = worst + ew + (lc.LOG_ULP * np.log(2) + 1) * u + u * np.maximum(1, np.abs(L))
    barO = np.zeros(p1.O.shape, dtype=T)
    for hd in range(heads):
        c = slice(hd * dv, (hd + 1) * dv)
        for p, w in zip(parts, om):
            barO[:, c] += 2 * w[hd][:, None] * (p.O[:, c] + np.abs(p.Oref[:, c]) * (2 * ew[hd][:, None] + 4 * u))
    return barO + 2 * tiny, barL


def ratio(got, ref, bar):
    """max |got - ref| / bar over ALL elements: the reference must be finite everywhere except L = -inf on rows without entries, which must agree"""
    fin = np.isfinite(ref)
    assert (fin | np.isneginf(ref)).all() and np.array_equal(np.isneginf(got), ~fin), "an element would be left out of the comparison"
    assert np.isfinite(got[fin]).all() and (bar[fin] >= 0).all()
    err, bar = np.abs(got[fin].astype(ref.dtype) - ref[fin]), bar[fin]
    zero = bar == 0   # O and dQ of a row without entries: nothing but an exact 0 is within the bar
    r = np.where(zero, np.where(err == 0, 0, np.inf), err / np.where(zero, 1, bar))
    return float(r.max()) if r.size else 0.0


# ----------------------------------------------------------------------------- the formulas restated in the handle's type (the CPU check)
def restated(csr, heads, kv, Q, K, V, B, scale, G):
    """forward, backward and L-driven backward in the operands' dtype, numpy's exp, log and sums in place of the device's:
    -> (O, L, (dQ, dK, dV, dB), (dQ, dK, dV, dB) driven by that O and L)"""
    dt = csr.val.dtype.type
    gs, k, dv = heads // kv, Q.shape[1] // heads, V.shape[1] // kv
    O, L = np.zeros((csr.m, heads * dv), dtype=dt), np.full((heads, csr.m), -np.inf, dtype=dt)
    outs = [[np.zeros(Q.shape, dtype=dt), np.zeros(K.shape, dtype=dt), np.zeros(V.shape, dtype=dt), np.zeros((heads, csr.nnz), dtype=dt)] for _ in range(2)]
    sc = dt(scale)
    for i in range(csr.m):
        s, e = int(csr.rowptr[i]), int(csr.rowptr[i + 1])
        if s == e:
            continue
        cols = csr.colidx[s:e]
        for hd in range(heads):
            g = hd // gs
            kc, vc = slice(g * k, (g + 1) * k), slice(g * dv, (g + 1) * dv)
            Kr, Vr, q, gi = K[cols, kc], V[cols, vc], Q[i, hd * k:(hd + 1) * k], G[i, hd * dv:(hd + 1) * dv]
            t = (Kr @ q) * sc + B[hd, s:e]
            M = t.max()
            ex = np.exp(t - M)
            Z = ex.sum()
            P = ex / Z
            L[hd, i] = M + np.log(Z)
            o = P @ Vr
            O[i, hd * dv:(hd + 1) * dv] = o
            dP = Vr @ gi
            for (dQ, dK, dV, dB), Pw, D in ((outs[0], P, (P * dP).sum()), (outs[1], np.exp(t - L[hd, i]), gi @ o)):
                db = Pw * (dP - D)
                assert db.dtype == dt
                dB[hd, s:e] = db
                ds = db * sc
                dQ[i, hd * k:(hd + 1) * k] = ds @ Kr
                np.add.at(dK[:, kc], cols, np.outer(ds, q))
                np.add.at(dV[:, vc], cols, np.outer(Pw, gi))
    return O, L, tuple(outs[0]), tuple(outs[1])
