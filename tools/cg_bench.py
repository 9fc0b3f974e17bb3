"""spmv_hip_cg per iteration against the multiply alone and against the same loop composed in torch around Handle.spmv.

    python tools/cg_bench.py [--cases web,s27,band] [--dtypes float64,float32] [--iterations 50] [--runs 20] [--out profiles/cg_bench.json]

All in one process, on one GPU.  Matrices (symmetric, diagonal = (1 + 2^-10) * sum |off-diagonal|: positive definite, so CG applies, and with a
condition number near 2^11, so that no solve here reaches rr = 0 inside a fixed budget and ends early):
    web    the webbase-size case: 1e6 rows, a random symmetric pattern, ~3 entries per row
    s27    the 27-point stencil on a 160^3 periodic grid
    band   the config-2 band made symmetric: 1e7 rows x 33 (offsets -16 .. 16)
Per case and value type, the minimum over --runs event-timed runs of --iterations iterations each, divided by --iterations:
    cg     spmv_hip_time_cg_iterations (stop tests off; the start of a solve is outside the events)
    (a)    the multiply alone: spmv_hip_time_launches
    (b)    the same recurrence in torch on device tensors around Handle.spmv on torch's stream, alpha and beta kept as 0-dim device tensors
    (c)    loop (b) with .item() scalars: two host round trips per iteration
and cg / (a) against the bytes model (spmv bytes + 11 s m) / spmv bytes, spmv bytes = the schedule's stream_bytes + x_bytes.
check_every in {1, 4, 8, 16, 32} on the smallest and the largest case: wall clock around spmv_hip_cg with rtol = 0 and a fixed budget, min of 7;
every one of those solves must use up its budget (status max_iterations), or the tool stops.
A number from one box at one time: compare ratios taken in one run, not milliseconds across runs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from spmv_amd import api, build  # noqa: E402

DEV = "cuda:0"
M = api.SPMV_METHODS
DOMINANCE = 1.0 + 2.0 ** -10   # diagonal / sum |off-diagonal|


def _circulant(m, offs, coef, dtype):
    """rows i hold columns (i + offs) mod m, sorted, with the value of each offset; offs symmetric, coef[t] = coef of -offs[t]"""
    k = offs.numel()
    assert (m + 1) * k < 2 ** 31
    rowptr = torch.arange(0, (m + 1) * k, k, dtype=torch.int32, device=DEV)
    colidx = torch.empty(m * k, dtype=torch.int32, device=DEV)
    val = torch.empty(m * k, dtype=dtype, device=DEV)
    for r0 in range(0, m, 1 << 21):
        r1 = min(m, r0 + (1 << 21))
        rows = torch.arange(r0, r1, device=DEV)
        cols, order = torch.sort((rows[:, None] + offs[None, :]) % m, dim=1)
        colidx[r0 * k:r1 * k] = cols.reshape(-1).to(torch.int32)
        val[r0 * k:r1 * k] = coef.to(dtype)[order].reshape(-1)
    return m, m, rowptr, colidx, val


def _coefficients(offs):
    """a value per offset, equal for +o and -o, in [-1, -1/4]; the diagonal = DOMINANCE * sum |others|"""
    c = -(0.25 + 0.75 * ((offs.abs() * 7) % 11).double() / 10.0)
    c[offs == 0] = 0
    c[offs == 0] = DOMINANCE * c.abs().sum()
    return c


def case(name, dtype):
    if name == "band":
        offs = torch.arange(-16, 17, device=DEV)
        return "config-2 band made symmetric: 1e7 rows x 33", M.Method_Parallel, _circulant(10_000_000, offs, _coefficients(offs), dtype)
    if name == "s27":
        nx = 160
        offs = torch.tensor([dz * nx * nx + dy * nx + dx for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], device=DEV)
        return "27-point stencil, 160^3 periodic grid", M.Method_Parallel, _circulant(nx ** 3, offs, _coefficients(offs), dtype)
    if name == "web":
        m = 1_000_000
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        i = torch.arange(m, device=DEV)
        j = torch.randint(0, m, (m,), generator=g, device=DEV)
        keep = i != j
        i, j = i[keep], j[keep]
        key = torch.unique(torch.cat([i * m + j, j * m + i, torch.arange(m, device=DEV) * (m + 1)]))   # both triangles and the diagonal, sorted
        rows, cols = key // m, key % m
        deg = torch.bincount(rows, minlength=m) - 1
        val = torch.where(rows == cols, torch.clamp(deg[rows], min=1).double() * (0.5 * DOMINANCE), torch.full_like(rows, -0.5, dtype=torch.float64)).to(dtype)
        rowptr = torch.zeros(m + 1, dtype=torch.int32, device=DEV)
        rowptr[1:] = torch.cumsum(deg + 1, 0).to(torch.int32)
        return "webbase-size: 1e6 rows, random symmetric pattern, ~3 per row", M.Method_Balanced2, (m, m, rowptr, cols.to(torch.int32), val)
    raise SystemExit(f"unknown case {name}")


def timed_runs(run, warmup, runs):
    """min ms over `runs` calls of run(), each between two events on torch's current stream"""
    for _ in range(warmup):
        run()
    best = float("inf")
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def torch_loop(h, b, iterations, items):
    """-> run(): `iterations` CG iterations from x = 0 around Handle.spmv; items: alpha and beta through .item()"""
    x, r, p, q = torch.zeros_like(b), torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)

    def run():
        x.zero_()
        r.copy_(b)
        p.copy_(b)
        rz = torch.dot(r, r)
        if items:
            rz = rz.item()
        for _ in range(iterations):
            h.spmv(p, q)
            pq = torch.dot(p, q)
            if items:
                alpha = rz / pq.item()
                x.add_(p, alpha=alpha)
                r.add_(q, alpha=-alpha)
                rz_new = torch.dot(r, r).item()
                p.mul_(rz_new / rz).add_(r)
            else:
                alpha = rz / pq
                x.addcmul_(p, alpha)
                r.addcmul_(q, -alpha)
                rz_new = torch.dot(r, r)
                p.mul_(rz_new / rz).add_(r)
            rz = rz_new
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="web,s27,band")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    api.load()
    names = a.cases.split(",")
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
                N = a.iterations
                cg = float(api.time_cg_iterations(h.h, b, x, N, warmup=2, iters=a.runs)[1].min()) / N
                jac = torch.ones_like(b)
                cg_jac = float(api.time_cg_iterations(h.h, b, x, N, dinv=jac, warmup=2, iters=a.runs)[1].min()) / N
                mult = float(api.time_launches(h.h, b, x, 10, 100)[1].min())
                _, res = h.cg(b, x, rtol=1e-6 if s == 8 else 1e-4, max_iterations=2000)
                spmv_bytes = int(info["stream_bytes"]) + int(info["x_bytes"]) or int(info["alg_bytes"])
                r = dict(case=name, desc=desc, dtype=dt, m=m, nnz=int(info["nnz"]), schedule=info["schedule_name"], iterations_per_run=N, runs=a.runs,
                         cg_us=round(cg * 1e3, 2), cg_jacobi_us=round(cg_jac * 1e3, 2), spmv_us=round(mult * 1e3, 2), cg_over_spmv=round(cg / mult, 3),
                         spmv_bytes=spmv_bytes, model_over_spmv=round((spmv_bytes + 11 * s * m) / spmv_bytes, 3),
                         model_jacobi_over_spmv=round((spmv_bytes + 13 * s * m) / spmv_bytes, 3), cg_jacobi_over_spmv=round(cg_jac / mult, 3),
                         solve=dict(status=res["status_name"], iterations=res["iterations"], rr_over_bb=res["rr"] / res["bb"]))
                if name in (names[0], names[-1]):   # the smallest and the largest case
                    budget, every = 256, {}
                    for ce in (1, 4, 8, 16, 32):
                        best = float("inf")
                        for _ in range(7):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            _, got = api.cg(h.h, m, rp, ci, va, b, x, rtol=0.0, max_iterations=budget, check_every=ce)
                            best = min(best, time.perf_counter() - t0)
                            if (got["status_name"], got["iterations"]) != ("max_iterations", budget):
                                raise SystemExit(f"{name} {dt}: the solve ended at iteration {got['iterations']} ({got['status_name']}), not at its budget")
                        every[str(ce)] = round(best / budget * 1e6, 2)
                    r["check_every_us_per_iteration"] = every
                    r["check_every_budget"] = budget
                h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
                tb = timed_runs(torch_loop(h, b, N, False), 2, a.runs) / N
                tc = timed_runs(torch_loop(h, b, N, True), 2, a.runs) / N
                r.update(torch_device_scalars_us=round(tb * 1e3, 2), torch_item_scalars_us=round(tc * 1e3, 2), speedup_over_device_scalars=round(tb / cg, 2),
                         speedup_over_item_scalars=round(tc / cg, 2))
                print(json.dumps(r), flush=True)
                rows.append(r)
            del rp, ci, va, b, x
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
