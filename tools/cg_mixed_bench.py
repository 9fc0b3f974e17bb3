"""spmv_hip_cg_mixed against spmv_hip_cg on the fp64 handle: time and iterations to a TRUE relative residual of 1e-10.

    python tools/cg_mixed_bench.py [--cases web,s27,band] [--runs 3] [--iterations 64] [--out profiles/cg_mixed_bench.json]

All in one process, on one GPU, on the three symmetric cases of tools/cg_bench.py (its matrices, its right-hand side).  Per case one fp64 handle
and one fp32 handle of the same matrix with the values rounded to float, the case's method on both.
    solve     wall clock around the synchronous call on device B / X, rtol = 1e-10, the contenders ALTERNATING inside every repetition: cg on the
              fp64 handle, then cg_mixed for update_drop in {0.5, 0.1, 0.01} x update_every in {0, 32}; the minimum over --runs repetitions.
              The whole pass is made TWICE; both passes are reported and `spread` is the largest relative difference between them.
              Every X is checked: ||b - A x|| / ||b|| formed again in fp64 with the fp64 handle's multiply and torch.
    iteration us per iteration from the timers (stop tests off, --iterations per run, min of 20 runs as tools/cg_bench.py): spmv_hip_time_cg_iterations
              on the fp64 and on the fp32 handle, spmv_hip_time_cg_mixed_iterations with update_every = 0 (no update: the static schedule of the
              iteration alone) and with update_every = 32; the update's cost is the difference of the last two per update.
    memory    the extra HBM of the mixed solve: the fp32 handle's device_bytes plus the workspace.
    model     tools/cg_mixed_model.py: fp32 CG's bytes per iteration, per update one fp64 multiply plus 60 B per row.
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

import cg_bench  # noqa: E402
import cg_mixed_model as model  # noqa: E402
from spmv_amd import api, build  # noqa: E402

DEV = cg_bench.DEV
RTOL = 1e-10
DROPS, EVERYS = (0.5, 0.1, 0.01), (0, 32)
BUDGET = 20000


def true_residual(hi, b, x):
    r = b - hi.spmv(x, torch.empty_like(x))
    return float(torch.linalg.vector_norm(r) / torch.linalg.vector_norm(b))


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def one_pass(hi, lo, b, runs):
    """-> {contender: dict(ms, iterations, updates, status, true_residual)}; contenders alternate inside every repetition"""
    contenders = {"cg_fp64": lambda x: hi.cg(b, x, rtol=RTOL, max_iterations=BUDGET)}
    for drop in DROPS:
        for every in EVERYS:
            contenders[f"mixed_drop{drop}_every{every}"] = lambda x, drop=drop, every=every: hi.cg_mixed(lo, b, x, rtol=RTOL, max_iterations=BUDGET, update_drop=drop,
                                                                                                        update_every=every)
    out = {}
    x = torch.empty_like(b)
    for rep in range(runs):
        for name, call in contenders.items():
            ms, (_, res) = wall(lambda: call(x))
            row = out.setdefault(name, dict(ms=float("inf")))
            row["ms"] = min(row["ms"], ms)
            if rep == 0:
                row.update(iterations=res["iterations"], updates=res.get("updates", 0), status=res["status_name"], true_residual=true_residual(hi, b, x))
    for row in out.values():
        row["ms"] = round(row["ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="web,s27,band")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    api.load()
    rows = []
    for name in a.cases.split(","):
        desc, method, (m, n, rp, ci, va) = cg_bench.case(name, torch.float64)
        va32 = va.float()
        with api.Handle(m, n, rp, ci, va, method) as hi, api.Handle(m, n, rp, ci, va32, method) as lo:
            ih, il = hi.info(), lo.info()
            g = torch.Generator(device=DEV)
            g.manual_seed(1)
            b = torch.rand(m, generator=g, dtype=torch.float64, device=DEV) * 2 - 1
            b32, x, x32 = b.float(), torch.empty_like(b), torch.empty(m, dtype=torch.float32, device=DEV)
            before = hi.info()["device_bytes"]
            hi.cg_mixed(lo, b, x, rtol=RTOL, max_iterations=8)     # the workspace appears here, outside every timing
            workspace = hi.info()["device_bytes"] - before
            passes = [one_pass(hi, lo, b, a.runs) for _ in range(2)]
            spread = max(abs(passes[0][k]["ms"] - passes[1][k]["ms"]) / min(passes[0][k]["ms"], passes[1][k]["ms"]) for k in passes[0])
            N = a.iterations
            us = lambda ms: round(float(ms) / N * 1e3, 2)
            t64 = us(api.time_cg_iterations(hi.h, b, x, N, warmup=2, iters=20)[1].min())
            t32 = us(api.time_cg_iterations(lo.h, b32, x32, N, warmup=2, iters=20)[1].min())
            mix0 = api.time_cg_mixed_iterations(hi.h, lo.h, b, x, N, update_every=0, warmup=2, iters=20)[1].min()
            mix32 = api.time_cg_mixed_iterations(hi.h, lo.h, b, x, N, update_every=32, warmup=2, iters=20)[1].min()
            hb = int(ih["stream_bytes"]) + int(ih["x_bytes"]) or int(ih["alg_bytes"])
            lb = int(il["stream_bytes"]) + int(il["x_bytes"]) or int(il["alg_bytes"])
            best = {k: min(passes[0][k]["ms"], passes[1][k]["ms"]) for k in passes[0]}
            ref = passes[0]["cg_fp64"]
            r = dict(case=name, desc=desc, m=m, nnz=int(ih["nnz"]), schedule=ih["schedule_name"], rtol=RTOL, runs=a.runs, passes=passes, spread_of_two_passes=round(spread, 4),
                     speedup_over_cg_fp64={k: round(best["cg_fp64"] / v, 3) for k, v in best.items() if k != "cg_fp64"},
                     iteration_us=dict(cg_fp64=t64, cg_fp32=t32, mixed_no_update=us(mix0), mixed_update_every_32=us(mix32),
                                       update_us=round(float(mix32 - mix0) / (N // 32) * 1e3, 2), iterations_per_run=N),
                     extra_hbm=dict(low_device_bytes=int(il["device_bytes"]), workspace_bytes=int(workspace), high_device_bytes=int(before)),
                     model=dict(high_spmv_bytes=hb, low_spmv_bytes=lb, iteration_mixed_over_fp64=round(model.mixed_iteration_bytes(lb, m) / model.cg_iteration_bytes(hb, m, 8), 3),
                                measured_iteration_mixed_over_fp64=round(us(mix0) / t64, 3),
                                update_over_fp64_iteration=round(model.update_bytes(hb, m) / model.cg_iteration_bytes(hb, m, 8), 3),
                                measured_update_over_fp64_iteration=round(float(mix32 - mix0) / (N // 32) * 1e3 / t64, 3),
                                solve_mixed_over_fp64={k: round(model.mixed_over_fp64(hb, lb, m, v["iterations"], v["updates"], ref["iterations"]), 3)
                                                       for k, v in passes[0].items() if k != "cg_fp64"}))
            print(json.dumps(r), flush=True)
            rows.append(r)
        del rp, ci, va, va32, b, b32, x, x32
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
