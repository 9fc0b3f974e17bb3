"""Out = (U V^T) sampled on A's pattern (spmv_hip_sddmm) on the bench shapes, against its bytes model.

    python tools/sddmm_bench.py [--shapes 2,2-ii,3o,4] [--ks 1,8,32] [--iters 20] [--out profiles/sddmm_bench.json]

Warm, timed with device events on the handle's stream (spmv_hip_time_sddmm_launches; min of --iters launches).  Bytes model of one call:
B_sddmm = 4(m+1) + 4 nnz (ColIdx) + s nnz (Out) + s k (nnz + m); the nnz k s term is the gather of V rows and an UPPER bound -- L2 reuse of V
rows lowers what HBM sees.  Reported as TB/s of B_sddmm; compare with the same-box pure-read rate of spmv_amd/bin/gbench."""
import argparse
import json
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
        with api.Handle(m, n, rp, ci, va, method) as h:
            out = torch.empty(nnz, dtype=va.dtype, device=DEV)
            for k in (int(v) for v in a.ks.split(",")):
                U = torch.rand((m, k), dtype=va.dtype, device=DEV)
                V = torch.rand((n, k), dtype=va.dtype, device=DEV)
                t = float(api.time_sddmm_launches(h.h, U, V, out, 3, a.iters)[1].min())
                b = 4 * (m + 1) + 4 * nnz + s * nnz + s * k * (nnz + m)
                floor = 4 * (m + 1) + 4 * nnz + s * nnz + s * k * (n + m)   # every V row read once
                r = dict(shape=name, desc=desc, method=method.name, m=m, n=n, nnz=nnz, dtype=str(va.dtype).replace("torch.", ""), k=k,
                         sddmm_ms=round(t, 4), bytes_model=b, tb_s=round(b / (t * 1e-3) / 1e12, 2), bytes_floor=floor,
                         tb_s_floor=round(floor / (t * 1e-3) / 1e12, 2), gflops=round(2.0 * k * nnz / (t * 1e-3) / 1e9, 1))
                print(json.dumps(r), flush=True)
                rows.append(r)
                del U, V
        del rp, ci, va, out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
