"""CPU: the struct mirrors of spmv_hip_cg against the header, and the host model of tests/cg_cases.py against exact arithmetic and against the
conditions the GPU tests rely on (tests/test_gpu_cg.py): before the model is the yardstick there, it has to meet them alone.

The dot's bars: the issue sets |dot - fsum| <= 1 ulp sqrt(m), taken here as 2^-52 sqrt(m) sum |a_i b_i| (the scale a cancelling sum is measured
against).  The model adds the fp64 products in a tree of depth d <= 2 + 2 + 6 + 2 + 2 + 6 + 2 = 22 for the sizes used (steps of one accumulator,
slots, lanes, waves, and slots, lanes, waves again for the partials), so the rigorous bound gamma_22 sum |a_i b_i| <= 24 * 2^-53 sum |a_i b_i| holds
too and is asserted beside it.  On integer-valued data every partial sum is exact and the test asks for equality."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cg_cases as cgc
from spmv_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "spmv_hip.h"
#include "spmv_hip_tools.h"
int main(void)
{
    printf("options %zu rtol %zu atol %zu max_iterations %zu check_every %zu use_x0 %zu Dinv %zu history %zu\n", sizeof(spmv_hip_cg_options),
           offsetof(spmv_hip_cg_options, rtol), offsetof(spmv_hip_cg_options, atol), offsetof(spmv_hip_cg_options, max_iterations),
           offsetof(spmv_hip_cg_options, check_every), offsetof(spmv_hip_cg_options, use_x0), offsetof(spmv_hip_cg_options, Dinv),
           offsetof(spmv_hip_cg_options, history));
    printf("result %zu status %zu iterations %zu rr %zu bb %zu\n", sizeof(spmv_hip_cg_result), offsetof(spmv_hip_cg_result, status),
           offsetof(spmv_hip_cg_result, iterations), offsetof(spmv_hip_cg_result, rr), offsetof(spmv_hip_cg_result, bb));
    printf("status %d %d %d %d\n", SPMV_HIP_CG_CONVERGED, SPMV_HIP_CG_MAX_ITERATIONS, SPMV_HIP_CG_BREAKDOWN, SPMV_HIP_CG_NONFINITE);
    return 0;
}
"""


def test_struct_mirrors_match_sizeof_and_offsetof(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, struct in zip(lines[:2], (api.spmv_hip_cg_options, api.spmv_hip_cg_result)):
        words = line.split()
        assert int(words[1]) == C.sizeof(struct), line
        assert [name for name, _ in struct._fields_] == words[2::2], line
        for name, off in zip(words[2::2], words[3::2]):
            assert getattr(struct, name).offset == int(off), (line, name)
    assert lines[2].split()[1:] == ["0", "1", "2", "3"]
    assert (cgc.CONVERGED, cgc.MAX_ITERATIONS, cgc.BREAKDOWN, cgc.NONFINITE) == (0, 1, 2, 3) and len(api.CG_STATUS) == 4


@pytest.mark.parametrize("m", [1, 3, 4, 5, 1023, 1024, 1025, 2049, 5000, 1024 * 1024 + 1])
def test_geometry_covers_every_element_once(m):
    P, L = cgc.geometry(m)
    assert 1 <= P <= 1024 and L % 1024 == 0 and P * L >= m
    assert P == min(1024, math.ceil(m / 1024)) and L == 1024 * math.ceil(m / (1024 * P))
    assert (P - 1) * L < m or P == 1024   # below the cap no workgroup is empty; at it (m = 2^20 + 1: L = 2048) the upper half is


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [1, 5, 1023, 1025, 2049, 70001, 1024 * 1024 + 1])
def test_dot_is_within_one_ulp_sqrt_m_of_fsum(m, dtype):
    rng = np.random.default_rng(m)
    a, b = rng.uniform(-1, 1, m).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)
    prods = a.astype(np.float64) * b.astype(np.float64)
    got = cgc.dot(a, b)
    exact = math.fsum(prods.tolist())   # of the fp64 products (exact for float operands; for double their one rounding is part of the contract)
    scale = math.fsum(np.abs(prods).tolist())
    print(f"m={m} {np.dtype(dtype).name}: |dot - fsum| = {abs(got - exact):.3e}, bar = {2.0 ** -52 * math.sqrt(m) * scale:.3e}")
    assert abs(got - exact) <= 2.0 ** -52 * math.sqrt(m) * scale
    assert abs(got - exact) <= 24 * 2.0 ** -53 * scale


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [1, 4, 1025, 2049, 1024 * 1024 + 1])
def test_dot_is_exact_on_integer_valued_data(m, dtype):
    rng = np.random.default_rng(7 * m)
    a, b = rng.integers(-64, 65, m).astype(dtype), rng.integers(-64, 65, m).astype(dtype)
    assert cgc.dot(a, b) == float(np.dot(a.astype(np.int64), b.astype(np.int64)))


def test_dot_follows_the_stated_order():
    """one element per (workgroup, step, thread, slot) position that matters, with magnitudes that make the order visible"""
    m = 2049                                   # P = 3, L = 1024: workgroup 2 holds one element
    a = np.zeros(m)
    a[0], a[2], a[3] = 1.0, 2.0 ** -53, 2.0 ** -53          # slots 0, 2, 3 of thread 0: (1 + 0) + (2^-53 + 2^-53) = 1 + 2^-52; left to right: 1
    assert cgc.dot(a, np.ones(m)) == 1.0 + 2.0 ** -52
    a[:] = 0
    a[0], a[1], a[4] = 1.0, 2.0 ** -53, 2.0 ** -53          # thread 0 rounds 1 + 2^-53 to 1 first; thread 1's 2^-53 is then lost too
    assert cgc.dot(a, np.ones(m)) == 1.0
    a[:] = 0
    a[1024], a[2048] = 2.0 ** -53, 2.0 ** -53                 # partials 1 and 2 meet partial 0 as (p0 + p1) + (p2 + 0)
    a[0] = 1.0
    assert cgc.dot(a, np.ones(m)) == 1.0


# the two solves the GPU tests repeat: (matrix, dtype, rtol)
SOLVES = [("lap2d32", np.float64, 1e-8), ("dominant4096", np.float32, 1e-3)]


def build(name, dtype):
    return cgc.lap2d(32, dtype) if name == "lap2d32" else cgc.dominant(4096, dtype)


@pytest.mark.parametrize("name,dtype,rtol", SOLVES)
def test_model_converges_and_the_true_residual_follows(name, dtype, rtol):
    csr = build(name, dtype)
    b = cgc.rhs(csr.m, dtype)
    out = cgc.cg(cgc.matvec(csr), b, rtol=rtol, max_iterations=500)
    res = cgc.true_residual(csr, b, out["x"])
    print(f"{name}: {out['iterations']} iterations, rr/bb = {out['rr'] / out['bb']:.3e}, true residual = {res:.3e}")
    assert out["status"] == cgc.CONVERGED and 0 < out["iterations"] < 500
    assert out["rr"] <= rtol * rtol * out["bb"] and len(out["history"]) == out["iterations"] + 1
    assert res <= 10 * rtol
    # a smaller budget stops at the same iterate
    part = cgc.cg(cgc.matvec(csr), b, rtol=rtol, max_iterations=3)
    assert part["status"] == cgc.MAX_ITERATIONS and part["iterations"] == 3 and np.array_equal(part["x"], out["iterates"][3])


def test_jacobi_needs_strictly_fewer_iterations_on_the_scaled_laplacian():
    csr = cgc.scaled(24)
    b = cgc.rhs(csr.m, np.float64)
    plain = cgc.cg(cgc.matvec(csr), b, rtol=1e-8, max_iterations=20000)
    jacobi = cgc.cg(cgc.matvec(csr), b, dinv=1.0 / cgc.diagonal(csr), rtol=1e-8, max_iterations=20000)
    print(f"scaled(24): {plain['iterations']} iterations without, {jacobi['iterations']} with Jacobi")
    assert plain["status"] == jacobi["status"] == cgc.CONVERGED
    assert jacobi["iterations"] < plain["iterations"]


def test_dinv_of_ones_is_no_preconditioner_and_special_cases():
    csr = cgc.tri(1025)
    b = cgc.rhs(csr.m, np.float64)
    mul = cgc.matvec(csr)
    none, ones = cgc.cg(mul, b, max_iterations=5), cgc.cg(mul, b, dinv=np.ones_like(b), max_iterations=5)
    assert np.array_equal(none["x"], ones["x"]) and np.array_equal(none["history"], ones["history"])
    zero = cgc.cg(mul, np.zeros_like(b), x0=b, max_iterations=5)
    assert zero["status"] == cgc.CONVERGED and zero["iterations"] == 0 and not zero["x"].any() and zero["rr"] == 0 == zero["bb"]
    nan = b.copy()
    nan[7] = np.nan
    bad = cgc.cg(mul, nan, max_iterations=5)
    assert bad["status"] == cgc.NONFINITE and bad["iterations"] <= 1
    sg = cgc.signs(1025)
    brk = cgc.cg(cgc.matvec(sg), np.ones(sg.m), max_iterations=5)     # <p, Ap> = 513 - 512 > 0 once, then r = p has <p, Ap> <= 0
    assert brk["status"] == cgc.BREAKDOWN and np.isfinite(brk["x"]).all() and np.array_equal(brk["x"], brk["iterates"][brk["iterations"]])
