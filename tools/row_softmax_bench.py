"""Row softmax over A's pattern (spmv_hip_row_softmax, spmv_hip_row_softmax_backward) against the torch composition and the copy floor.

    python tools/row_softmax_bench.py [--shapes 2,3o] [--iters 10] [--no-torch] [--out profiles/row_softmax_bench.json]

Forward: spmv_hip_time_row_softmax_launches (device events around every launch, min of --iters).  Backward: the same bracketing with torch
events around Handle.row_softmax_backward on torch's current stream with async on (the timing entry point takes S and Out only).
(a) the torch composition on the same box in the same process: repeat_interleave, scatter_reduce (amax, sum) and index_select over
    nnz-sized temporaries, forward and backward; its results are compared with the kernels' (max relative difference, reported).
(b) the traffic floor 2 s nnz + 4 (m + 1) bytes at the same-box copy rate of `spmv_amd/bin/gbench copy` over 2 s nnz bytes.
A number from one box at one time: compare ratios taken in one run, not milliseconds across runs."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from spmv_amd import api, build  # noqa: E402
from tools.spmm_bench import DEV, shape  # noqa: E402


def copy_rate(nbytes):
    """GB/s (read + written bytes) of a 16-byte-per-lane copy of nbytes on this box, now; None without the tool"""
    exe = os.path.join(ROOT, "spmv_amd", "bin", "gbench")
    if not os.path.exists(exe):
        return None
    r = subprocess.run([exe, "copy", str(int(nbytes)), "10"], capture_output=True, text=True, timeout=120)
    line = next((l for l in r.stdout.splitlines() if l.startswith("{")), None)
    return json.loads(line)["copy_gbps"] if line else None


def timed(fn, warmup, iters):
    """min ms of `iters` calls, each between two events on the current stream"""
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    for i in range(iters):
        ev[i].record()
        fn()
    ev[iters].record()
    torch.cuda.synchronize()
    return min(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))


def torch_forward(rp, S):
    m = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(m, device=S.device), (rp[1:] - rp[:-1]).long())
    mx = torch.full((m,), float("-inf"), dtype=S.dtype, device=S.device).scatter_reduce(0, rows, S, "amax")
    e = torch.exp(S - mx.index_select(0, rows))
    z = torch.zeros(m, dtype=S.dtype, device=S.device).scatter_reduce(0, rows, e, "sum")
    return e / z.index_select(0, rows)


def torch_backward(rp, P, G):
    m = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(m, device=P.device), (rp[1:] - rp[:-1]).long())
    d = torch.zeros(m, dtype=P.dtype, device=P.device).scatter_reduce(0, rows, P * G, "sum")
    return P * (G - d.index_select(0, rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2,3o")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    api.load()
    rows = []
    for name in a.shapes.split(","):
        desc, method, (m, n, rp, ci, va) = shape(name)
        nnz = int(rp[-1].item())
        s = va.element_size()
        lens = (rp[1:] - rp[:-1])
        long_nnz = int(lens[lens > 512].sum().item())
        floor_bytes = 2 * s * nnz + 4 * (m + 1)
        gbps = copy_rate(s * nnz)   # s nnz read + s nnz written
        with api.Handle(m, n, rp, ci, va, method) as h:
            g = torch.Generator(device=DEV)
            g.manual_seed(1)
            S = torch.rand(nnz, generator=g, dtype=va.dtype, device=DEV) * 8 - 4
            G = torch.rand(nnz, generator=g, dtype=va.dtype, device=DEV) * 2 - 1
            P = torch.empty_like(S)
            dS = torch.empty_like(S)
            before = int(h.info()["device_bytes"])
            fwd = float(api.time_row_softmax_launches(h.h, S, P, 3, a.iters)[1].min())
            tables = int(h.info()["device_bytes"]) - before
            h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
            bwd = timed(lambda: h.row_softmax_backward(P, G, dS), 3, a.iters)
            r = dict(shape=name, desc=desc, m=m, nnz=nnz, dtype=str(va.dtype).replace("torch.", ""), long_row_nnz_share=round(long_nnz / max(nnz, 1), 4),
                     table_bytes=tables, forward_ms=round(fwd, 4), backward_ms=round(bwd, 4), floor_bytes=floor_bytes,
                     forward_tb_s=round(floor_bytes / (fwd * 1e-3) / 1e12, 3), backward_tb_s=round((3 * s * nnz + 4 * (m + 1)) / (bwd * 1e-3) / 1e12, 3),
                     copy_gbps=gbps, floor_ms=None if not gbps else round(floor_bytes / (gbps * 1e9) * 1e3, 4))
            if gbps:
                r["forward_over_floor"] = round(fwd / r["floor_ms"], 2)
            if not a.no_torch:
                tf = timed(lambda: torch_forward(rp, S), 1, min(a.iters, 5))
                tb = timed(lambda: torch_backward(rp, P, G), 1, min(a.iters, 5))
                Pt, dt = torch_forward(rp, S), torch_backward(rp, P, G)
                r.update(torch_forward_ms=round(tf, 3), torch_backward_ms=round(tb, 3), forward_speedup=round(tf / fwd, 1), backward_speedup=round(tb / bwd, 1),
                         forward_max_rel_diff=float(((P - Pt).abs() / Pt).max()), backward_max_abs_diff=float((dS - dt).abs().max()))
                del Pt, dt
            print(json.dumps(r), flush=True)
            rows.append(r)
        del rp, ci, va, S, G, P, dS
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
