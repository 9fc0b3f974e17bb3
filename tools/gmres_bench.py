"""spmv_hip_gmres per iteration against the multiply alone, against its bytes model and against the same GMRES composed in torch around
Handle.spmv; its time to a tolerance against spmv_hip_bicgstab's.

    python tools/gmres_bench.py [--cases web,s27,band] [--dtypes float64,float32] [--restarts 10,30] [--cycles 2] [--runs 10] [--out profiles/gmres_bench.json]

All in one process, on one GPU, on the three nonsymmetric cases of tools/bicgstab_bench.py (web, s27, band: see there).  Per case, value type
and restart R, the minimum over --runs event-timed runs of --cycles * R iterations each, divided by that count -- so an "iteration" carries
its share of the cycle's end and of the restart:
    gmres      spmv_hip_time_gmres_iterations (stop tests off; the start of a solve is outside the events)
    (a)        the multiply alone: spmv_hip_time_launches
    (b)        GMRES(R) with classical Gram-Schmidt twice in torch on device tensors around Handle.spmv on torch's stream: the projections are
               torch.mv on the stacked basis, the Hessenberg matrix stays on the device and a cycle ends with torch.linalg.lstsq on it
and gmres / (a) against the bytes model (spmv bytes + (3 jbar + 6) s m) / spmv bytes, jbar = (R + 1) / 2 the mean step of a cycle, spmv bytes =
the schedule's stream_bytes + x_bytes.  What the kernels of kernels/gmres.hpp move at step j is more than the model's 3 (j + 1) + 3 vectors:
gmres_dots j + ceil(j / G), gmres_sub_dots 2 j + 1 + ceil(j / G) (the basis is read for the subtraction and again for the dots), gmres_sub_norm
j + 2, gmres_scale 2: 4 j + 5 + 2 ceil(j / G), reported as kernel_vectors for jbar.
Time to a tolerance: wall clock around Handle.gmres and Handle.bicgstab on the same system from x = 0, rtol 1e-8 in fp64 and 1e-4 in fp32 (1e-8
is below what fp32 vectors reach), at most 3000 iterations, min of 3; a solve that does not converge is reported with its status.
check_every in {1, 2, 4, 8, 16, 32} on the smallest and the largest case at the largest restart: wall clock around spmv_hip_gmres with rtol = 0
and a fixed budget, min of 5.
A number from one box at one time: compare ratios taken in one run, not milliseconds across runs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bicgstab_bench import DEV, case, timed_runs  # noqa: E402
from spmv_amd import api, build  # noqa: E402

GROUP = 8   # kGmresGroup


def torch_loop(h, b, restart, cycles):
    """-> run(): `cycles` full cycles of GMRES(restart) from x = 0 around Handle.spmv, nothing read back by the host"""
    m = b.numel()
    V = torch.empty(restart + 1, m, dtype=b.dtype, device=DEV)
    H = torch.zeros(restart + 1, restart, dtype=b.dtype, device=DEV)
    rhs = torch.zeros(restart + 1, 1, dtype=b.dtype, device=DEV)
    x, r, w = (torch.empty_like(b) for _ in range(3))

    def run():
        x.zero_()
        r.copy_(b)
        for _ in range(cycles):
            beta = torch.linalg.vector_norm(r)
            torch.div(r, beta, out=V[0])
            H.zero_()
            for j in range(1, restart + 1):
                h.spmv(V[j - 1], w)
                basis = V[:j]
                c = torch.mv(basis, w)
                w.sub_(torch.mv(basis.t(), c))
                e = torch.mv(basis, w)
                w.sub_(torch.mv(basis.t(), e))
                hn = torch.linalg.vector_norm(w)
                H[:j, j - 1] = c + e
                H[j, j - 1] = hn
                torch.div(w, hn, out=V[j])
            rhs.zero_()
            rhs[0, 0] = beta
            y = torch.linalg.lstsq(H, rhs).solution[:, 0]
            x.add_(torch.mv(V[:restart].t(), y))
            h.spmv(x, w)
            torch.sub(b, w, out=r)
        return r
    return run


def wall(solve, repeats):
    best, out = float("inf"), None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = solve()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="web,s27,band")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--restarts", default="10,30")
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    api.load()
    names = a.cases.split(",")
    restarts = [int(v) for v in a.restarts.split(",")]
    rows = []
    for name in names:
        for dt in a.dtypes.split(","):
            dtype = getattr(torch, dt)
            desc, method, (m, n, rp, ci, va) = case(name, dtype)
            s = va.element_size()
            with api.Handle(m, n, rp, ci, va, method) as h:
                info = h.info()
                g = torch.Generator(device=DEV)
                g.manual_seed(1)
                b = torch.rand(m, generator=g, dtype=dtype, device=DEV) * 2 - 1
                x = torch.empty_like(b)
                mult = float(api.time_launches(h.h, b, x, 10, 100)[1].min())
                spmv_bytes = int(info["stream_bytes"]) + int(info["x_bytes"]) or int(info["alg_bytes"])
                rtol = 1e-8 if s == 8 else 1e-4
                t_bi, (_, bi) = wall(lambda: h.bicgstab(b, x, rtol=rtol, max_iterations=3000), 3)
                for R in restarts:
                    N = a.cycles * R
                    it = float(api.time_gmres_iterations(h.h, b, x, N, restart=R, warmup=2, iters=a.runs)[1].min()) / N
                    it_jac = float(api.time_gmres_iterations(h.h, b, x, N, restart=R, dinv=torch.ones_like(b), warmup=2, iters=a.runs)[1].min()) / N
                    jbar = (R + 1) / 2
                    moved = sum(4 * j + 5 + 2 * -(-j // GROUP) for j in range(1, R + 1)) / R
                    t_gm, (_, gm) = wall(lambda: h.gmres(b, x, restart=R, rtol=rtol, max_iterations=3000), 3)
                    r = dict(case=name, desc=desc, dtype=dt, m=m, nnz=int(info["nnz"]), schedule=info["schedule_name"], restart=R, iterations_per_run=N, runs=a.runs,
                             gmres_us=round(it * 1e3, 2), gmres_ones_dinv_us=round(it_jac * 1e3, 2), spmv_us=round(mult * 1e3, 2), gmres_over_spmv=round(it / mult, 3),
                             spmv_bytes=spmv_bytes, model_vectors=3 * jbar + 6, model_over_spmv=round((spmv_bytes + (3 * jbar + 6) * s * m) / spmv_bytes, 3),
                             kernel_vectors=round(moved, 2), kernel_model_over_spmv=round((spmv_bytes + moved * s * m) / spmv_bytes, 3),
                             to_rtol=dict(rtol=rtol, gmres_ms=round(t_gm * 1e3, 2), gmres_status=gm["status_name"], gmres_iterations=gm["iterations"],
                                          bicgstab_ms=round(t_bi * 1e3, 2), bicgstab_status=bi["status_name"], bicgstab_iterations=bi["iterations"],
                                          bicgstab_multiplies=2 * bi["iterations"], gmres_over_bicgstab=round(t_gm / t_bi, 3)))
                    if name in (names[0], names[-1]) and R == restarts[-1]:
                        budget, every = 8 * R, {}
                        for ce in (1, 2, 4, 8, 16, 32):
                            best, (_, got) = wall(lambda: api.gmres(h.h, m, rp, ci, va, b, x, R, rtol=0.0, max_iterations=budget, check_every=ce), 5)
                            every[str(ce)] = round(best / budget * 1e6, 2) if (got["status_name"], got["iterations"]) == ("max_iterations", budget) else \
                                f"{got['status_name']} at iteration {got['iterations']}"
                        r["check_every_us_per_iteration"] = every
                        r["check_every_budget"] = budget
                    rows.append(r)
                h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
                for r in rows[-len(restarts):]:
                    tb = timed_runs(torch_loop(h, b, r["restart"], a.cycles), 1, max(3, a.runs // 2)) / r["iterations_per_run"]
                    r.update(torch_us=round(tb * 1e3, 2), speedup_over_torch=round(tb * 1e3 / r["gmres_us"], 2))
                    print(json.dumps(r), flush=True)
            del rp, ci, va, b, x
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
