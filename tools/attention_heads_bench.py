"""Multi-head sparse attention (spmv_hip_attention_heads) against H single-head calls (spmv_hip_attention) on the column slices of the same buffers.

    python tools/attention_heads_bench.py [--shapes 2,3o] [--dtypes f64,f32] [--configs 4x8,8x8,2x32] [--iters 20] [--out profiles/attention_heads_bench.json]

Heads call: spmv_hip_time_attention_heads_launches (device events around every call, min of --iters).  H calls, in the same process on the
same handle with the same Q, K, V: spmv_hip_attention on the slices, back to back between two torch events on the current stream with async
on; min of --iters.  A config HxK is H heads of k = dv = K.  The two results are compared bit for bit.
B_heads = 4 (m + 1) + 4 nnz + H s (k (m + nnz) + dv (nnz + m)) is the heads call's bytes model; the H calls pay the two index terms H times.
A number from one box at one time: compare the two columns of one run, not milliseconds across runs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from spmv_amd import api, build  # noqa: E402
from tools.row_softmax_bench import timed  # noqa: E402
from tools.spmm_bench import DEV, shape  # noqa: E402

DTYPES = {"f64": torch.float64, "f32": torch.float32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2,3o")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--configs", default="4x8,8x8,2x32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_heads_bench.json"))
    a = ap.parse_args()
    build.build()
    api.load()
    configs = [tuple(int(x) for x in c.split("x")) for c in a.configs.split(",")]
    rows = []
    for name in a.shapes.split(","):
        desc, method, (m, n, rp, ci, va0) = shape(name)
        nnz = int(rp[-1].item())
        for dt in a.dtypes.split(","):
            va = va0.to(DTYPES[dt])
            s = va.element_size()
            ibits = torch.int64 if s == 8 else torch.int32
            with api.Handle(m, n, rp, ci, va, method) as h:
                for heads, k in configs:
                    dv = k
                    scale = k ** -0.5
                    g = torch.Generator(device=DEV)
                    g.manual_seed(100 * heads + k)
                    Q, K, V = (torch.rand(shp, generator=g, dtype=va.dtype, device=DEV) * 2 - 1 for shp in ((m, heads * k), (n, heads * k), (n, heads * dv)))
                    O, O2 = (torch.empty((m, heads * dv), dtype=va.dtype, device=DEV) for _ in range(2))
                    fused = float(api.time_attention_heads_launches(h.h, heads, Q, K, V, O, scale, 3, a.iters)[1].min())
                    h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
                    slices = [(Q[:, hd * k:(hd + 1) * k], K[:, hd * k:(hd + 1) * k], V[:, hd * dv:(hd + 1) * dv], O2[:, hd * dv:(hd + 1) * dv]) for hd in range(heads)]

                    def head_by_head():
                        for q, kk, v, o in slices:
                            h.attention(q, kk, v, scale, out=o)
                    calls = timed(head_by_head, 3, a.iters)
                    torch.cuda.synchronize()
                    b = 4 * (m + 1) + 4 * nnz + heads * s * (k * (m + nnz) + dv * (nnz + m))
                    r = dict(shape=name, desc=desc.rsplit(",", 1)[0], m=m, nnz=nnz, dtype=dt, heads=heads, k=k, dv=dv, heads_ms=round(fused, 4),
                             h_calls_ms=round(calls, 4), h_calls_over_heads=round(calls / fused, 3), b_heads=b,
                             heads_tb_s=round(b / (fused * 1e-3) / 1e12, 3), same_bits=bool(torch.equal(O.view(ibits), O2.view(ibits))))
                    print(json.dumps(r), flush=True)
                    rows.append(r)
                    del Q, K, V, O, O2, slices
            del va
        del rp, ci, va0
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
