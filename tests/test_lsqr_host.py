"""Host: the numpy model of spmv_hip_lsqr (tests/lsqr_cases.py) against two references that share no code with it, every end of its loop, and
the declarations the feature needs.  No GPU.

The two bounds below were MEASURED on these cases and carry a 16x margin, because the references add their dots in another order (BLAS) or
solve the problem another way (an SVD); DESIGN 3.31 quotes the measurements:
  against scipy.sparse.linalg.lsqr, tolerances 0, the same fixed iteration count:     max |x - x_scipy| / |x_scipy| = 9.2e-16
  against np.linalg.lstsq on [A; damp I], stopped by ls_tol = 1e-12, cond < 10:        max |x - x_lstsq| / |x_lstsq| = 5.3e-13"""
import os
import re

import numpy as np
import pytest

import lsqr_cases as lc
from spmv_amd import api

SCIPY_BOUND = 16 * 9.2e-16
LSTSQ_BOUND = 16 * 5.3e-13
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (matrix, damp); b is random, so the tall systems are inconsistent
SCIPY_CASES = {
    "tall": (lambda: lc.sparse_rect(200, 30, seed=2), 0.0),
    "wide": (lambda: lc.sparse_rect(30, 200, seed=3), 0.0),
    "damped": (lambda: lc.sparse_rect(200, 30, seed=2), 0.7),
    "wide_damped": (lambda: lc.sparse_rect(30, 200, seed=3), 0.3),
    "inconsistent": (lambda: lc.well_conditioned(120, 10, seed=1), 0.0),
}


@pytest.mark.parametrize("k", [5, 12])
@pytest.mark.parametrize("name", list(SCIPY_CASES))
def test_model_against_scipy_lsqr(name, k):
    sp = pytest.importorskip("scipy.sparse")
    spla = pytest.importorskip("scipy.sparse.linalg")
    make, damp = SCIPY_CASES[name]
    csr = make()
    k = min(k, csr.n // 2)                                      # both still iterate: scipy ends by itself once the Krylov space is exhausted
    b = lc.rhs(csr.m, np.float64, 9)
    mul, mul_t = lc.products(csr)
    model = lc.lsqr(mul, mul_t, b, csr.n, damp=damp, max_iterations=k)
    ref = spla.lsqr(sp.csr_matrix((csr.val, csr.colidx, csr.rowptr), shape=(csr.m, csr.n)), b, damp=damp, atol=0, btol=0, conlim=0, iter_lim=k)
    assert (model["iterations"], model["end"], ref[2]) == (k, "budget", k)
    err = np.linalg.norm(model["x"] - ref[0]) / np.linalg.norm(ref[0])
    # scipy's r2norm is sqrt(rr); its arnorm is ar (not bounded here: near convergence it is a difference of nearly equal numbers)
    print(f"{name} k={k}: |x - x_scipy| / |x_scipy| = {err:.3e}, sqrt(rr) {np.sqrt(model['rr']):.6e} scipy {ref[4]:.6e}, ar {model['ar']:.3e} scipy {ref[7]:.3e}")
    assert err <= SCIPY_BOUND
    assert abs(np.sqrt(model["rr"]) - ref[4]) <= 1e-12 * ref[4]


LSTSQ_CASES = {"tall": (120, 10, 0.0, 1), "damped": (120, 10, 0.8, 2), "square": (24, 24, 0.0, 3), "wide_damped": (10, 40, 1.5, 4)}


@pytest.mark.parametrize("name", list(LSTSQ_CASES))
def test_model_against_lstsq_on_the_stacked_system(name):
    m, n, damp, seed = LSTSQ_CASES[name]
    csr = lc.well_conditioned(m, n, seed=seed) if m >= n else lc.from_dense(lc.dense(lc.well_conditioned(n, m, seed=seed)).T.copy())
    stacked = np.vstack([lc.dense(csr), damp * np.eye(n)])
    sv = np.linalg.svd(stacked, compute_uv=False)
    assert sv[0] / sv[-1] < 10
    b = lc.rhs(m, np.float64, 5)
    mul, mul_t = lc.products(csr)
    model = lc.lsqr(mul, mul_t, b, n, damp=damp, ls_tol=1e-12, max_iterations=200)
    want = np.linalg.lstsq(stacked, np.concatenate([b, np.zeros(n)]), rcond=None)[0]
    err = np.linalg.norm(model["x"] - want) / np.linalg.norm(want)
    print(f"{name}: cond {sv[0] / sv[-1]:.3f}, {model['end']} after {model['iterations']} iterations, |x - x_lstsq| / |x_lstsq| = {err:.3e}")
    assert model["end"] in ("step:least_squares", "step:converged") and model["iterations"] < 200
    assert err <= LSTSQ_BOUND


STATUS_OF_END = {"begin:nonfinite": lc.NONFINITE, "begin:bb_zero": lc.CONVERGED, "begin:converged": lc.CONVERGED, "first:nonfinite": lc.NONFINITE,
                 "first:alpha_zero": lc.LEAST_SQUARES, "step:uu_nonfinite": lc.NONFINITE, "step:vv_nonfinite": lc.NONFINITE, "step:factor_nonfinite": lc.NONFINITE,
                 "step:nonfinite": lc.NONFINITE, "step:converged": lc.CONVERGED, "step:least_squares": lc.LEAST_SQUARES, "budget": lc.MAX_ITERATIONS}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_end_is_reached(dtype):
    cases = lc.end_cases(dtype)
    reached = set()
    for name, (csr, b, kw, end) in cases.items():
        mul, mul_t = lc.products(csr)
        model = lc.lsqr(mul, mul_t, b, csr.n, **kw)
        assert model["end"] == end, name
        assert model["status"] == STATUS_OF_END[end], name
        assert len(model["history"]) == len(model["iterates"]) == model["iterations"] + 1, name
        assert model["x"].dtype == dtype and model["x"].shape == (csr.n,), name
        reached.add(end)
    if dtype == np.float64:
        assert reached == set(STATUS_OF_END)                                  # no end of the model is left without a case
    m = cases["beta_zero"]
    mul, mul_t = lc.products(m[0])
    model = lc.lsqr(mul, mul_t, m[1], m[0].n, **m[2])
    assert (model["iterations"], model["rr"], model["ar"]) == (1, 0.0, 0.0) and model["x"].tolist() == [3.0, 0.0, 0.0, 0.0]
    m = cases["orthogonal_b"]
    mul, mul_t = lc.products(m[0])
    model = lc.lsqr(mul, mul_t, m[1], m[0].n, **m[2])
    assert (model["iterations"], model["ar"], model["rr"], model["x"].tolist()) == (0, 0.0, 2.0, [0.0])


def test_a_budget_returns_the_iterate_of_a_longer_run_and_the_empty_column_stays_zero():
    csr = lc.sparse_rect(40, 6, seed=1)
    b = lc.rhs(40, np.float64, 3)
    mul, mul_t = lc.products(csr)
    full = lc.lsqr(mul, mul_t, b, 6, damp=0.25, max_iterations=6)
    for k in range(7):
        short = lc.lsqr(mul, mul_t, b, 6, damp=0.25, max_iterations=k)
        assert short["x"].tobytes() == full["iterates"][k].tobytes() and short["rr"] == full["history"][k]
        assert (short["ar"], short["anorm"]) == full["estimates"][k]
    assert all(x[4] == 0 for x in full["iterates"]) and np.delete(full["x"], 4).all()


def test_declarations():
    with open(os.path.join(ROOT, "include", "spmv_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+spmv_hip_lsqr\s*\(", header)
    assert "SPMV_HIP_LSQR_LEAST_SQUARES = 5" in header
    for field in ("rtol, atol", "ls_tol", "damp", "max_iterations", "check_every", "use_x0", "*history"):
        assert field in header.split("typedef struct spmv_hip_lsqr_options")[1].split("}")[0], field
    with open(os.path.join(ROOT, "include", "spmv_hip_tools.h")) as f:
        assert re.search(r"\bdouble\s+spmv_hip_time_lsqr_iterations\s*\(", f.read())
    assert "spmv_hip_lsqr" in api.FUNCTIONS and "spmv_hip_time_lsqr_iterations" in api.FUNCTIONS
    assert [n for n, _ in api.spmv_hip_lsqr_options._fields_] == ["rtol", "atol", "ls_tol", "damp", "max_iterations", "check_every", "use_x0", "history"]
    assert [n for n, _ in api.spmv_hip_lsqr_result._fields_] == ["status", "iterations", "rr", "bb", "ar", "anorm"]
    assert api.LSQR_STATUS[lc.LEAST_SQUARES] == "least_squares" and callable(api.lsqr) and callable(api.time_lsqr_iterations) and callable(api.Handle.lsqr)
