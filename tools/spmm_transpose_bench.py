"""Y = A^T X for k right-hand sides (spmv_hip_spmm_transpose) against k separate spmv_hip_spmv_transpose calls and against spmv_hip_spmm on A,
on the bench shapes.

    python tools/spmm_transpose_bench.py [--shapes 2,2-ii,3o,4] [--ks 1,8,32] [--iters 20] [--out profiles/spmm_transpose_bench.json]

All sides are warm and timed with device events on the handle's stream (spmv_hip_time_spmm_transpose_launches, _time_transpose_launches,
_time_spmm_launches; min of --iters launches); the transpose-vector side is k x the best single launch of the same handle.  Bytes model of
one call: that of spmm on A^T, B = 4(n+1) + P nnz (4 + s) + k s (n + m), P = ceil(k / KP) panels (KP = 16 fp64 / 32 fp32)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from spmv_amd import api, build  # noqa: E402
from tools.spmm_bench import DEV, shape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2,2-ii,3o,4")
    ap.add_argument("--ks", default="1,8,32")
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
            api.prepare_transpose(h.h)
            x = torch.rand(m, dtype=va.dtype, device=DEV)
            y = torch.empty(n, dtype=va.dtype, device=DEV)
            t1 = float(api.time_transpose_launches(h.h, x, y, 5, a.iters)[1].min())
            for k in (int(v) for v in a.ks.split(",")):
                X = torch.rand((m, k), dtype=va.dtype, device=DEV)
                Y = torch.empty((n, k), dtype=va.dtype, device=DEV)
                tk = float(api.time_spmm_transpose_launches(h.h, X, Y, 3, a.iters)[1].min())
                Xa = torch.rand((n, k), dtype=va.dtype, device=DEV)
                Ya = torch.empty((m, k), dtype=va.dtype, device=DEV)
                ta = float(api.time_spmm_launches(h.h, Xa, Ya, 3, a.iters)[1].min())
                b = 4 * (n + 1) + math.ceil(k / kp) * nnz * (4 + s) + k * s * (n + m)
                r = dict(shape=name, desc=desc, method=method.name, m=m, n=n, nnz=nnz, dtype=str(va.dtype).replace("torch.", ""), k=k,
                         spmm_transpose_ms=round(tk, 4), transpose_x_k_ms=round(k * t1, 4), spmv_transpose_ms=round(t1, 4),
                         ratio_vs_k_calls=round(tk / (k * t1), 3), spmm_ms=round(ta, 4), ratio_vs_spmm=round(tk / ta, 3),
                         bytes_model=b, tb_s=round(b / (tk * 1e-3) / 1e12, 2), device_bytes=h.info()["device_bytes"])
                print(json.dumps(r), flush=True)
                rows.append(r)
                del X, Y, Xa, Ya
        del rp, ci, va
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
