"""Y = A X for k right-hand sides (spmv_hip_spmm) against k separate spmv() calls, on the bench shapes.

    python tools/spmm_bench.py [--shapes 2,2-ii,3o,4] [--ks 1,2,4,8,16,32] [--iters 20] [--out profiles/spmm_bench.json]

Both sides are warm and timed with device events on the handle's stream (spmv_hip_time_spmm_launches / spmv_hip_time_launches); the
spmv side is k x the best single launch.  Bytes model of one spmm: B = 4(m+1) + P nnz (4 + s) + k s (n + m), P = ceil(k / KP) panels
(KP = 16 fp64 / 32 fp32), reported as a fraction of 8 TB/s."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from spmv_amd import api, build, synth  # noqa: E402

M = api.SPMV_METHODS
DEV = "cuda:0"
HBM = 8.0e12


def shape(name):
    f64, f32 = torch.float64, torch.float32
    if name == "2":
        return "config 2: banded, 1e7 rows x 32, fp64", M.Method_Parallel, synth.banded_device(10_000_000, 10_000_000, 32, "uniform", f64, DEV, 1)
    if name == "2-ii":
        return "config 2-ii: uniform columns, 1e7 rows x 32, fp64", M.Method_Parallel, synth.uniform_k_device(10_000_000, 10_000_000, 32, "uniform", f64, DEV, 1)
    if name == "3o":
        lens = synth.powerlaw_lengths_device(3_070_000, 76, 33000, 1.5, DEV, 1)
        return ("config 3 stand-in com-Orkut-style: power-law rows, R-MAT columns, fp64", M.Method_Balanced2,
                synth.from_row_lengths_device(lens, 3_070_000, "uniform", f64, DEV, 1, cols="rmat"))
    if name == "4":
        lens = synth.skewed_lengths_device(10_000_000, DEV, 1)
        return ("config 4: skewed rows, columns within +-4096, fp32", M.Method_SellCSigma,
                synth.from_row_lengths_device(lens, 10_000_000, "uniform", f32, DEV, 1, local=4096))
    raise SystemExit(f"unknown shape {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2,2-ii,3o,4")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    api.load()
    rows = []
    for name in a.shapes.split(","):
        desc, method, (m, n, rp, ci, va) = shape(name)
        nnz = int(rp[-1].item())
        s = va.element_size()
        kp = 16 if s == 8 else 32
        with api.Handle(m, n, rp, ci, va, method) as h:
            x = torch.rand(n, dtype=va.dtype, device=DEV)
            y = torch.empty(m, dtype=va.dtype, device=DEV)
            t1 = float(api.time_launches(h.h, x, y, 5, a.iters)[1].min())
            for k in (int(v) for v in a.ks.split(",")):
                X = torch.rand((n, k), dtype=va.dtype, device=DEV)
                Y = torch.empty((m, k), dtype=va.dtype, device=DEV)
                tk = float(api.time_spmm_launches(h.h, X, Y, 3, a.iters)[1].min())
                b = 4 * (m + 1) + math.ceil(k / kp) * nnz * (4 + s) + k * s * (n + m)
                r = dict(shape=name, desc=desc, method=method.name, m=m, n=n, nnz=nnz, dtype=str(va.dtype).replace("torch.", ""), k=k,
                         spmm_ms=round(tk, 4), spmv_x_k_ms=round(k * t1, 4), spmv_ms=round(t1, 4), ratio=round(tk / (k * t1), 3),
                         bytes_model=b, tb_s=round(b / (tk * 1e-3) / 1e12, 2), frac_8tbs=round(b / (tk * 1e-3) / HBM, 3))
                print(json.dumps(r), flush=True)
                rows.append(r)
                del X, Y
        del rp, ci, va
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
