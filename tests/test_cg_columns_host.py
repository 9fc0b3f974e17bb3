"""CPU: the ctypes mirrors of spmv_hip_cg_columns against the headers, api.cg_columns' own argument checks, and the conditions that
tests/test_gpu_cg_columns.py relies on, shown here on the host model alone (tests/cg_columns_cases.py around cg_cases.matvec): the mixed
right-hand sides really end differently, and `signs` breaks down."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cg_cases as cgc
import cg_columns_cases as ccc
from spmv_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES_C = r"""
#include <stdio.h>
#include "spmv_hip.h"
#include "spmv_hip_tools.h"
/* the prototypes, restated: a mismatch with the headers does not compile */
int spmv_hip_cg_columns(spmv_Handle_t, BASIC_INT_TYPE, const BASIC_INT_TYPE *, const BASIC_INT_TYPE *, const void *, int, const void *, long long, void *, long long,
                        const spmv_hip_cg_options *, spmv_hip_cg_result *);
double spmv_hip_time_cg_columns_iterations(spmv_Handle_t, int, const void *, long long, void *, long long, const struct spmv_hip_cg_options *, int, int, float *);
int main(void)
{
    printf("%d %zu\n", SPMV_HIP_CG_COLUMNS_MAX, sizeof(BASIC_INT_TYPE));
    return 0;
}
"""


def test_prototypes_and_ctypes_signatures(tmp_path):
    src, exe = tmp_path / "proto.c", tmp_path / "proto"
    src.write_text(PROTOTYPES_C)
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kmax, int_size = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(kmax) == api.CG_COLUMNS_MAX == 16 and int(int_size) == C.sizeof(C.c_int)
    V, LL, I = C.c_void_p, C.c_longlong, C.c_int
    opt, res = C.POINTER(api.spmv_hip_cg_options), C.POINTER(api.spmv_hip_cg_result)
    assert api.FUNCTIONS["spmv_hip_cg_columns"] == (I, [api.spmv_Handle_t, I, V, V, V, I, V, LL, V, LL, opt, res])
    assert api.FUNCTIONS["spmv_hip_time_cg_columns_iterations"] == (C.c_double, [api.spmv_Handle_t, I, V, LL, V, LL, opt, I, I, C.POINTER(C.c_float)])
    # one column with ld = 1 is spmv_hip_cg: the two calls take the same options and results
    assert api.FUNCTIONS["spmv_hip_cg"][1][-2:] == [opt, res]


def test_the_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    block = text[text.index("conjugate gradients for k right-hand sides"):text.index("int spmv_hip_cg_columns(")]
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", block))   # across the comment's line breaks
    for phrase in ("per-column contract", "FROZEN", "changes no bit of any other", "IS spmv_hip_cg", "4 * k * 8192 + 1024", "(max_iterations + 1) * k", "it * k + j"):
        assert phrase in flat, phrase


def test_python_side_argument_checks():
    B, X = np.zeros((8, 3)), np.zeros((8, 3))
    with pytest.raises(ValueError):
        api._cg_columns_blocks(np.zeros((8, 17)), np.zeros((8, 17)))           # more than 16 columns
    with pytest.raises(ValueError):
        api._cg_columns_blocks(np.zeros((8, 0)), np.zeros((8, 0)))             # none
    with pytest.raises(ValueError):
        api._cg_columns_blocks(B, np.zeros((8, 4)))                            # k differs
    with pytest.raises(ValueError):
        api._cg_columns_blocks(B, np.zeros((9, 3)))                            # m differs
    with pytest.raises(ValueError):
        api._cg_columns_blocks(np.zeros(8), np.zeros(8))                       # not 2-D
    with pytest.raises(ValueError):
        api._cg_columns_blocks(np.asfortranarray(B), X)                        # column stride is not 1
    k, pb, ldb, px, ldx = api._cg_columns_blocks(np.zeros((8, 6))[:, 1:4], X)
    assert (k, ldb, ldx) == (3, 6, 3) and pb % 8 == 0
    assert api._cg_columns_blocks(np.zeros((8, 1)), np.zeros((8, 4))[:, :1])[::2] == (1, 1, 4)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_mixed_right_hand_sides_end_differently(dtype):
    g = 24
    csr = cgc.lap2d(g, dtype)
    B = ccc.mixed_ends(g, dtype)
    rtol = 1e-6 if dtype == np.float64 else 1e-4
    out = dict(zip(ccc.MIXED, ccc.solve(cgc.matvec(csr), B, rtol=rtol, max_iterations=400)))
    print({name: (o["status"], o["iterations"], o["end"]) for name, o in out.items()})
    assert (out["eigenvector"]["status"], out["eigenvector"]["iterations"]) == (cgc.CONVERGED, 1)
    assert (out["zero"]["status"], out["zero"]["iterations"], out["zero"]["rr"], out["zero"]["bb"]) == (cgc.CONVERGED, 0, 0.0, 0.0) and not out["zero"]["x"].any()
    assert out["nan"]["status"] == cgc.NONFINITE and out["nan"]["iterations"] == 0
    for name in ("generic", "generic2"):
        assert out[name]["status"] == cgc.CONVERGED and 10 < out[name]["iterations"] < 400
        assert cgc.true_residual(csr, B[:, ccc.MIXED.index(name)], out[name]["x"]) <= 10 * rtol
    assert len({o["iterations"] for o in out.values()}) >= 3          # the columns really leave the loop at different times
    # a column is its own solve: the model of the columns is cg_cases.cg on each
    alone = cgc.cg(cgc.matvec(csr), np.ascontiguousarray(B[:, 1]), rtol=rtol, max_iterations=400)
    assert alone["x"].tobytes() == out["generic"]["x"].tobytes() and alone["iterations"] == out["generic"]["iterations"]


def test_signs_breaks_down_and_the_columns_are_the_same_whatever_k():
    sg = cgc.signs(1025)
    out = ccc.solve(cgc.matvec(sg), np.ones((sg.m, 2)), max_iterations=5)
    assert all(o["status"] == cgc.BREAKDOWN and np.isfinite(o["x"]).all() for o in out)
    a, b = ccc.columns(300, 5, np.float64, 3), ccc.columns(300, 16, np.float64, 3)
    assert a.tobytes() == np.ascontiguousarray(b[:, :5]).tobytes() and a.shape == (300, 5)
    assert ccc.workspace_bytes(1000, 3, 8) == 3 * 24064 + 12 * 8192 + 1024
