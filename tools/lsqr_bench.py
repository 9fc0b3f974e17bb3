"""spmv_hip_lsqr per iteration against its two multiplies alone, against the bytes model and against the same loop composed in torch around
Handle.spmv and Handle.spmv_transpose.

    python tools/lsqr_bench.py [--cases web,square,band] [--dtypes float64,float32] [--iterations 30] [--runs 10] [--out profiles/lsqr_bench.json]

All in one process, on one GPU.  Matrices:
    web     a tall web-like matrix: 1e6 x 2.5e5, random columns, about 3 entries per row
    square  the config-2 band: 1e7 x 1e7, 33 entries per row (offsets -16 .. 16)
    band    a tall band: 1e7 x 5e6, 32 entries per row (row i: columns i // 2 .. i // 2 + 31, wrapped)
Per case and value type, the minimum over --runs event-timed runs of --iterations iterations each, divided by --iterations, and the spread
(max / min) of those runs:
    lsqr    spmv_hip_time_lsqr_iterations (stop tests off; the start of a solve is outside the events)
    (a)     the two multiplies alone: spmv_hip_time_launches + spmv_hip_time_transpose_launches
    (b)     the same recurrence in torch on device tensors around Handle.spmv / Handle.spmv_transpose on torch's stream, every scalar a 0-dim
            device tensor
and lsqr / (a) against the bytes model (both multiplies' bytes + (5 m + 9 n) s) / both multiplies' bytes, a multiply's bytes = its schedule's
stream_bytes + x_bytes.  check_every in {1, 4, 8, 16, 32} on the smallest and the largest case: wall clock around spmv_hip_lsqr with every
tolerance 0 and a fixed budget, min of 5; every one of those solves must use up its budget (status max_iterations), or the tool stops.
Prints one JSON line (all rows); a row per case also goes to stderr as it is finished.
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


def _band(m, n, offs, row_to_col, dtype):
    """row i holds the columns (row_to_col(i) + offs) mod n, sorted; the value of offset t is +-(1/4 + 3/4 ((7 t) mod 11) / 10), the sign by t's parity"""
    k = offs.numel()
    assert (m + 1) * k < 2 ** 31
    coef = (0.25 + 0.75 * ((offs.abs() * 7) % 11).double() / 10.0) * torch.where(offs % 2 == 0, 1.0, -1.0).double()
    rowptr = torch.arange(0, (m + 1) * k, k, dtype=torch.int32, device=DEV)
    colidx = torch.empty(m * k, dtype=torch.int32, device=DEV)
    val = torch.empty(m * k, dtype=dtype, device=DEV)
    for r0 in range(0, m, 1 << 21):
        r1 = min(m, r0 + (1 << 21))
        rows = torch.arange(r0, r1, device=DEV)
        cols, order = torch.sort((row_to_col(rows)[:, None] + offs[None, :]) % n, dim=1)
        colidx[r0 * k:r1 * k] = cols.reshape(-1).to(torch.int32)
        val[r0 * k:r1 * k] = coef.to(dtype)[order].reshape(-1)
    return m, n, rowptr, colidx, val


def case(name, dtype):
    if name == "band":
        return "tall band: 1e7 x 5e6, 32 per row", M.Method_Parallel, _band(10_000_000, 5_000_000, torch.arange(0, 32, device=DEV), lambda r: r // 2, dtype)
    if name == "square":
        return "config-2 band: 1e7 x 1e7, 33 per row", M.Method_Parallel, _band(10_000_000, 10_000_000, torch.arange(-16, 17, device=DEV), lambda r: r, dtype)
    if name == "web":
        m, n = 1_000_000, 250_000
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        i = torch.arange(m, device=DEV).repeat_interleave(3)
        j = torch.randint(0, n, (3 * m,), generator=g, device=DEV)
        key = torch.unique(i * n + j)                                   # sorted by row, then column; a repeated column drops out
        rows, cols = key // n, key % n
        val = (torch.rand(key.numel(), generator=g, dtype=torch.float64, device=DEV) * 2 - 1).to(dtype)
        rowptr = torch.zeros(m + 1, dtype=torch.int32, device=DEV)
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=m), 0).to(torch.int32)
        return "web-like: 1e6 x 2.5e5, random columns, ~3 per row", M.Method_Balanced2, (m, n, rowptr, cols.to(torch.int32), val)
    raise SystemExit(f"unknown case {name}")


def timed_runs(run, warmup, runs):
    """-> (min, max) ms over `runs` calls of run(), each between two events on torch's current stream"""
    for _ in range(warmup):
        run()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return min(times), max(times)


def torch_loop(h, b, n, iterations, damp):
    """-> run(): `iterations` LSQR iterations from x = 0 around Handle.spmv / Handle.spmv_transpose; every scalar stays a 0-dim device tensor"""
    x, v, w, qt = (torch.empty(n, dtype=b.dtype, device=DEV) for _ in range(4))
    u, q = torch.empty_like(b), torch.empty_like(b)
    dsq = torch.tensor(damp * damp, dtype=torch.float64, device=DEV)
    norm = torch.linalg.vector_norm

    def run():
        x.zero_()
        u.copy_(b)
        beta = norm(u)
        u.div_(beta)
        h.spmv_transpose(u, v)
        alpha = norm(v)
        v.div_(alpha)
        w.copy_(v)
        phibar, rhobar = beta.double(), alpha.double()
        for _ in range(iterations):
            h.spmv(v, q)
            u.mul_(-alpha).add_(q)
            beta = norm(u)
            u.div_(beta)
            h.spmv_transpose(u, qt)
            v.mul_(-beta).add_(qt)
            alpha = norm(v)
            v.div_(alpha)
            a64, b64 = alpha.double(), beta.double()
            rhobar1 = torch.sqrt(rhobar * rhobar + dsq)
            phibar = (rhobar / rhobar1) * phibar
            rho = torch.sqrt(rhobar1 * rhobar1 + b64 * b64)
            c, s = rhobar1 / rho, b64 / rho
            theta, rhobar, phi, phibar = s * a64, -(c * a64), c * phibar, s * phibar
            x.addcmul_(w, (phi / rho).to(b.dtype))
            w.mul_(-(theta / rho).to(b.dtype)).add_(v)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="web,square,band")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--damp", type=float, default=0.0)
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
                g = torch.Generator(device=DEV)
                g.manual_seed(1)
                b = torch.rand(m, generator=g, dtype=dtype, device=DEV) * 2 - 1
                x = torch.empty(n, dtype=dtype, device=DEV)
                N = a.iterations
                runs = api.time_lsqr_iterations(h.h, b, x, N, damp=a.damp, warmup=2, iters=a.runs)[1]
                lsqr, spread = float(runs.min()) / N, float(runs.max() / runs.min())
                info, tinfo = h.info(), api.get_transpose_info(h.h)
                q = torch.empty_like(b)
                mult = float(api.time_launches(h.h, x, q, 10, 50)[1].min())
                mult_t = float(api.time_transpose_launches(h.h, b, x, 10, 50)[1].min())
                both = mult + mult_t
                spmv_bytes = sum(int(i["stream_bytes"]) + int(i["x_bytes"]) or int(i["alg_bytes"]) for i in (info, tinfo))
                r = dict(case=name, desc=desc, dtype=dt, m=m, n=n, nnz=int(info["nnz"]), schedule=info["schedule_name"], transpose_schedule=tinfo["schedule_name"],
                         iterations_per_run=N, runs=a.runs, damp=a.damp, lsqr_us=round(lsqr * 1e3, 2), lsqr_spread=round(spread, 3), spmv_us=round(mult * 1e3, 2),
                         transpose_us=round(mult_t * 1e3, 2), lsqr_over_multiplies=round(lsqr / both, 3), multiplies_bytes=spmv_bytes,
                         model_over_multiplies=round((spmv_bytes + (5 * m + 9 * n) * s) / spmv_bytes, 3), vector_bytes=(5 * m + 9 * n) * s,
                         vector_kernels_us=round((lsqr - both) * 1e3, 2))
                if name in (names[0], names[-1]):   # the smallest and the largest case
                    budget, every = 128, {}
                    for ce in (1, 4, 8, 16, 32):
                        best = float("inf")
                        for _ in range(5):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            _, got = api.lsqr(h.h, m, rp, ci, va, b, x, damp=a.damp, rtol=0.0, atol=0.0, ls_tol=0.0, max_iterations=budget, check_every=ce)
                            best = min(best, time.perf_counter() - t0)
                            if (got["status_name"], got["iterations"]) != ("max_iterations", budget):
                                raise SystemExit(f"{name} {dt}: the solve ended at iteration {got['iterations']} ({got['status_name']}), not at its budget")
                        every[str(ce)] = round(best / budget * 1e6, 2)
                    r["check_every_us_per_iteration"] = every
                    r["check_every_budget"] = budget
                h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
                lo, hi = timed_runs(torch_loop(h, b, n, N, a.damp), 2, a.runs)
                r.update(torch_device_scalars_us=round(lo / N * 1e3, 2), torch_spread=round(hi / lo, 3), speedup_over_device_scalars=round(lo / N / lsqr, 2))
                print(json.dumps(r), file=sys.stderr, flush=True)
                rows.append(r)
            del rp, ci, va, b, x, q
            torch.cuda.empty_cache()
    print(json.dumps(rows), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
