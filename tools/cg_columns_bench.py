"""spmv_hip_cg_columns per iteration against k single solves, against the k-column multiply alone and against a bytes model.

    python tools/cg_columns_bench.py [--cases web,s27,band] [--dtypes float64,float32] [--ks 2,4,8,16] [--iterations 30] [--runs 10] [--out profiles/cg_columns_bench.json]

All in one process, on one GPU, on the three matrices of tools/cg_bench.py (its `case`).  Per case, value type and k, the minimum over --runs
event-timed runs of --iterations iterations each, divided by --iterations, in us per iteration:
    columns         spmv_hip_time_cg_columns_iterations (stop tests off; the start of a solve is outside the events)
    columns_jacobi  the same with Dinv given
    k_singles       k times the per-iteration figure of spmv_hip_time_cg_iterations on the same handle: what a loop of k spmv_hip_cg calls costs
    spmm            the k-column multiply alone: spmv_hip_time_spmm_launches on compact m x k device arrays
and columns against the bytes model
    bytes = A + 2 k m s + 11 k m s  (+ 2 m s with Dinv)
    A = nnz (s + 4) + 4 (m + 1): the CSR arrays spmm streams once; 2 k m s: it reads P and writes Q; 11 passes over m k elements by the vector
    kernels: ccg_dot reads p, q; ccg_update reads p, q, x, r and writes x, r; ccg_direction reads r, p and writes p
as model_us = bytes / (the rate at which `spmm` moved A + 2 k m s), i.e. the vector kernels are asked to run at the multiply's rate.
check_every in {1, 4, 8, 16, 32} at k = 8 on the smallest and the largest case: wall clock around spmv_hip_cg_columns with rtol = 0 and a fixed
budget, min of 5; every column of those solves must use up its budget, or the tool stops.
A number from one box at one time: compare ratios taken in one run, not milliseconds across runs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from cg_bench import DEV, case  # noqa: E402
from spmv_amd import api, build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="web,s27,band")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--ks", default="2,4,8,16")
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    api.load()
    names = a.cases.split(",")
    ks = [int(k) for k in a.ks.split(",")]
    N = a.iterations
    rows = []
    for name in names:
        for dt in a.dtypes.split(","):
            dtype = getattr(torch, dt)
            desc, method, (m, n, rp, ci, va) = case(name, dtype)
            s = va.element_size()
            with api.Handle(m, n, rp, ci, va, method) as h:
                info = h.info()
                nnz = int(info["nnz"])
                g = torch.Generator(device=DEV)
                g.manual_seed(1)
                b = torch.rand(m, generator=g, dtype=dtype, device=DEV) * 2 - 1
                x = torch.empty_like(b)
                single = float(api.time_cg_iterations(h.h, b, x, N, warmup=2, iters=a.runs)[1].min()) / N
                single_jac = float(api.time_cg_iterations(h.h, b, x, N, dinv=torch.ones_like(b), warmup=2, iters=a.runs)[1].min()) / N
                spmv = float(api.time_launches(h.h, b, x, 10, 50)[1].min())
                base = dict(case=name, desc=desc, dtype=dt, m=m, nnz=nnz, schedule=info["schedule_name"], iterations_per_run=N, runs=a.runs,
                            single_cg_us=round(single * 1e3, 2), single_cg_jacobi_us=round(single_jac * 1e3, 2), spmv_us=round(spmv * 1e3, 2))
                a_bytes = nnz * (s + 4) + 4 * (m + 1)
                for k in ks:
                    B = torch.rand((m, k), generator=g, dtype=dtype, device=DEV) * 2 - 1
                    X = torch.empty_like(B)
                    cols = float(api.time_cg_columns_iterations(h.h, B, X, N, warmup=2, iters=a.runs)[1].min()) / N
                    cols_jac = float(api.time_cg_columns_iterations(h.h, B, X, N, dinv=torch.ones_like(b), warmup=2, iters=a.runs)[1].min()) / N
                    spmm = float(api.time_spmm_launches(h.h, B, X, 5, 30)[1].min())
                    spmm_bytes = a_bytes + 2 * k * m * s
                    rate = spmm_bytes / spmm          # bytes per ms
                    model = (spmm_bytes + 11 * k * m * s) / rate
                    model_jac = (spmm_bytes + 11 * k * m * s + 2 * m * s) / rate
                    r = dict(base, k=k, columns_us=round(cols * 1e3, 2), columns_jacobi_us=round(cols_jac * 1e3, 2), k_singles_us=round(k * single * 1e3, 2),
                             k_singles_jacobi_us=round(k * single_jac * 1e3, 2), spmm_us=round(spmm * 1e3, 2), k_spmv_us=round(k * spmv * 1e3, 2),
                             speedup_over_k_singles=round(k * single / cols, 3), speedup_over_k_singles_jacobi=round(k * single_jac / cols_jac, 3),
                             columns_per_column_us=round(cols / k * 1e3, 2), columns_over_spmm=round(cols / spmm, 3), bytes_model=spmm_bytes + 11 * k * m * s,
                             spmm_gbs=round(rate / 1e6, 1), model_us=round(model * 1e3, 2), columns_over_model=round(cols / model, 3),
                             columns_jacobi_over_model=round(cols_jac / model_jac, 3))
                    if k == 8 and name in (names[0], names[-1]):   # the smallest and the largest case
                        budget, every = 128, {}
                        for ce in (1, 4, 8, 16, 32):
                            best = float("inf")
                            for _ in range(5):
                                torch.cuda.synchronize()
                                t0 = time.perf_counter()
                                _, got = api.cg_columns(h.h, m, rp, ci, va, B, X, rtol=0.0, max_iterations=budget, check_every=ce)
                                best = min(best, time.perf_counter() - t0)
                                if any((c["status_name"], c["iterations"]) != ("max_iterations", budget) for c in got):
                                    raise SystemExit(f"{name} {dt}: a column ended before its budget: {got}")
                            every[str(ce)] = round(best / budget * 1e6, 2)
                        r["check_every_us_per_iteration"] = every
                        r["check_every_budget"] = budget
                    print(json.dumps(r), flush=True)
                    rows.append(r)
                    del B, X
            del rp, ci, va, b, x
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
