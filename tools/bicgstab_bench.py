"""spmv_hip_bicgstab per iteration against two multiplies alone and against the same loop composed in torch around Handle.spmv.

    python tools/bicgstab_bench.py [--cases web,s27,band] [--dtypes float64,float32] [--iterations 50] [--runs 20] [--out profiles/bicgstab_bench.json]

All in one process, on one GPU: tools/cg_bench.py's three cases made NONSYMMETRIC (diagonal = (1 + 2^-10) * sum |off-diagonal|: strictly
diagonally dominant, so BiCGStab applies and a fixed budget is not cut short by a breakdown, with a spectrum wide enough that no solve
reaches rr = 0 inside the budget):
    web    the webbase-size case: 1e6 rows, a random pattern that is NOT symmetrised, 2 random off-diagonal entries per row, values in (-1, -1/4)
    s27    the 27-point stencil on a 160^3 periodic grid, the coefficient of offset -o 5/3 of that of +o
    band   the config-2 band: 1e7 rows x 33 (offsets -16 .. 16), likewise
Per case and value type, the minimum over --runs event-timed runs of --iterations iterations each, divided by --iterations:
    bicgstab   spmv_hip_time_bicgstab_iterations (stop tests off; the start of a solve is outside the events)
    (a)        the multiply alone: spmv_hip_time_launches; an iteration holds two
    (b)        the same recurrence in torch on device tensors around Handle.spmv on torch's stream -- the five dots of the contract, <s,s> and
               <r,r> of the stop tests among them --, alpha, omega and beta kept as 0-dim device tensors
    (c)        loop (b) with .item() scalars: five host round trips per iteration
and bicgstab / (2 (a)) against the bytes model (2 spmv bytes + 20 s m) / (2 spmv bytes), spmv bytes = the schedule's stream_bytes + x_bytes; the
20 vector passes are those of kernels/bicgstab.hpp without Dinv: bicg_rv 2, bicg_half 6 (p, v, x, r read; x, r written), bicg_ts 2, bicg_update 6,
bicg_direction 4.  With Dinv 25: y and Dinv are read and y written in bicg_half (+2; y stands for p) and bicg_direction (+2), y is read in
bicg_update (+1).
check_every in {1, 2, 4, 8, 16, 32} on the smallest and the largest case: wall clock around spmv_hip_bicgstab with rtol = 0 and a fixed budget,
min of 7; a solve that does not use up its budget (status max_iterations) is recorded as such and its time left out.
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
PASSES, PASSES_DINV = 20, 25   # vector passes of one iteration's five kernels (the docstring)


def _circulant(m, offs, coef, dtype):
    """rows i hold columns (i + offs) mod m, sorted, coef[t] the value at offset offs[t]"""
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
    """a value per offset in [-1.25, -0.1875], that of -o 5/3 of that of +o; the diagonal = DOMINANCE * sum |others|"""
    c = -(0.25 + 0.75 * ((offs.abs() * 7) % 11).double() / 10.0)
    c = torch.where(offs < 0, 1.25 * c, 0.75 * c)
    c[offs == 0] = 0
    c[offs == 0] = DOMINANCE * c.abs().sum()
    return c


def case(name, dtype):
    if name == "band":
        offs = torch.arange(-16, 17, device=DEV)
        return "config-2 band with unequal off-diagonals: 1e7 rows x 33", M.Method_Parallel, _circulant(10_000_000, offs, _coefficients(offs), dtype)
    if name == "s27":
        nx = 160
        offs = torch.tensor([dz * nx * nx + dy * nx + dx for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], device=DEV)
        return "27-point stencil with unequal +o / -o coefficients, 160^3 periodic grid", M.Method_Parallel, _circulant(nx ** 3, offs, _coefficients(offs), dtype)
    if name == "web":
        m = 1_000_000
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        i = torch.arange(m, device=DEV).repeat(2)
        j = torch.randint(0, m, (2 * m,), generator=g, device=DEV)
        keep = i != j
        key = torch.unique(torch.cat([i[keep] * m + j[keep], torch.arange(m, device=DEV) * (m + 1)]))   # the entries as drawn and the diagonal, sorted
        rows, cols = key // m, key % m
        off = -(0.25 + 0.75 * torch.rand(key.numel(), generator=g, dtype=torch.float64, device=DEV))
        off[rows == cols] = 0
        total = torch.zeros(m, dtype=torch.float64, device=DEV).index_add_(0, rows, off.abs())
        val = torch.where(rows == cols, torch.clamp(total[rows], min=1.0) * DOMINANCE, off).to(dtype)
        rowptr = torch.zeros(m + 1, dtype=torch.int32, device=DEV)
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=m), 0).to(torch.int32)
        return "webbase-size: 1e6 rows, random unsymmetrised pattern, ~3 per row", M.Method_Balanced2, (m, m, rowptr, cols.to(torch.int32), val)
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
    """-> run(): `iterations` BiCGStab iterations from x = 0 around Handle.spmv, s kept in r; items: every scalar through .item()"""
    x, r, rhat, p, v, t = (torch.empty_like(b) for _ in range(6))

    def run():
        x.zero_()
        r.copy_(b)
        rhat.copy_(b)
        p.copy_(b)
        rho = torch.dot(rhat, r)
        if items:
            rho = rho.item()
        for _ in range(iterations):
            h.spmv(p, v)
            rv = torch.dot(rhat, v)
            if items:
                alpha = rho / rv.item()
                x.add_(p, alpha=alpha)
                r.add_(v, alpha=-alpha)
                ss = torch.dot(r, r).item()                  # the half step's stop test
                h.spmv(r, t)
                omega = torch.dot(t, r).item() / torch.dot(t, t).item()
                x.add_(r, alpha=omega)
                r.add_(t, alpha=-omega)
                rho_new, rr = torch.dot(rhat, r).item(), torch.dot(r, r).item()
                p.add_(v, alpha=-omega).mul_((rho_new / rho) * (alpha / omega)).add_(r)
            else:
                alpha = rho / rv
                x.addcmul_(p, alpha)
                r.addcmul_(v, -alpha)
                ss = torch.dot(r, r)
                h.spmv(r, t)
                omega = torch.dot(t, r) / torch.dot(t, t)
                x.addcmul_(r, omega)
                r.addcmul_(t, -omega)
                rho_new, rr = torch.dot(rhat, r), torch.dot(r, r)
                p.addcmul_(v, -omega).mul_((rho_new / rho) * (alpha / omega)).add_(r)
            rho = rho_new
        return ss, rr
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
                it = float(api.time_bicgstab_iterations(h.h, b, x, N, warmup=2, iters=a.runs)[1].min()) / N
                jac = torch.ones_like(b)
                it_jac = float(api.time_bicgstab_iterations(h.h, b, x, N, dinv=jac, warmup=2, iters=a.runs)[1].min()) / N
                mult = float(api.time_launches(h.h, b, x, 10, 100)[1].min())
                _, res = h.bicgstab(b, x, rtol=1e-6 if s == 8 else 1e-4, max_iterations=2000)
                spmv_bytes = int(info["stream_bytes"]) + int(info["x_bytes"]) or int(info["alg_bytes"])
                r = dict(case=name, desc=desc, dtype=dt, m=m, nnz=int(info["nnz"]), schedule=info["schedule_name"], iterations_per_run=N, runs=a.runs,
                         bicgstab_us=round(it * 1e3, 2), bicgstab_jacobi_us=round(it_jac * 1e3, 2), spmv_us=round(mult * 1e3, 2),
                         bicgstab_over_2spmv=round(it / (2 * mult), 3), spmv_bytes=spmv_bytes,
                         model_over_2spmv=round((2 * spmv_bytes + PASSES * s * m) / (2 * spmv_bytes), 3),
                         bicgstab_jacobi_over_2spmv=round(it_jac / (2 * mult), 3),
                         model_jacobi_over_2spmv=round((2 * spmv_bytes + PASSES_DINV * s * m) / (2 * spmv_bytes), 3),
                         solve=dict(status=res["status_name"], iterations=res["iterations"], rr_over_bb=res["rr"] / res["bb"]))
                if name in (names[0], names[-1]):   # the smallest and the largest case
                    budget, every, cut = 256, {}, {}
                    for ce in (1, 2, 4, 8, 16, 32):
                        best = float("inf")
                        for _ in range(7):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            _, got = api.bicgstab(h.h, m, rp, ci, va, b, x, rtol=0.0, max_iterations=budget, check_every=ce)
                            best = min(best, time.perf_counter() - t0)
                            if (got["status_name"], got["iterations"]) != ("max_iterations", budget):
                                cut[str(ce)] = f"{got['status_name']} at iteration {got['iterations']}"
                                break
                        every[str(ce)] = None if str(ce) in cut else round(best / budget * 1e6, 2)
                    r["check_every_us_per_iteration"] = every
                    r["check_every_budget"] = budget
                    if cut:
                        r["check_every_cut_short"] = cut
                h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
                tb = timed_runs(torch_loop(h, b, N, False), 2, a.runs) / N
                tc = timed_runs(torch_loop(h, b, N, True), 2, a.runs) / N
                r.update(torch_device_scalars_us=round(tb * 1e3, 2), torch_item_scalars_us=round(tc * 1e3, 2), speedup_over_device_scalars=round(tb / it, 2),
                         speedup_over_item_scalars=round(tc / it, 2))
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
