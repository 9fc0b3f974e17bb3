"""Fused sparse attention (spmv_hip_attention) against the three-call composition on the library's own kernels.

    python tools/attention_bench.py [--shapes 2,3o] [--k 8,32] [--iters 20] [--out profiles/attention_bench.json]

Fused: spmv_hip_time_attention_launches (device events around every call, min of --iters).  Composition, in the same process on the same
handle: Handle.sddmm, an in-place `* scale`, Handle.row_softmax in place, Handle.update_values(P) -- the copy and the re-permutation into the
schedule's private layouts -- and Handle.spmm, between two torch events on the current stream with async on; min of --iters.  k = dv.  The
two results are compared bit for bit.  B_att = 4 (m + 1) + 4 nnz + s (k (m + nnz) + dv (nnz + m)) is the fused call's bytes model.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2,3o")
    ap.add_argument("--k", default="8,32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.json"))
    a = ap.parse_args()
    build.build()
    api.load()
    rows = []
    for name in a.shapes.split(","):
        desc, method, (m, n, rp, ci, va) = shape(name)
        nnz = int(rp[-1].item())
        s = va.element_size()
        with api.Handle(m, n, rp, ci, va, method) as h:
            for k in (int(x) for x in a.k.split(",")):
                dv = k
                scale = k ** -0.5
                g = torch.Generator(device=DEV)
                g.manual_seed(k)
                Q, K, V = (torch.rand(shp, generator=g, dtype=va.dtype, device=DEV) * 2 - 1 for shp in ((m, k), (n, k), (n, dv)))
                O, O2, S = (torch.empty(shp, dtype=va.dtype, device=DEV) for shp in ((m, dv), (m, dv), (nnz,)))
                fused = float(api.time_attention_launches(h.h, Q, K, V, O, scale, 3, a.iters)[1].min())
                h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)

                def composed():
                    h.sddmm(Q, K, S)
                    S.mul_(scale)
                    h.row_softmax(S, S)
                    h.update_values(S)
                    h.spmm(V, O2)
                try:
                    comp = timed(composed, 3, a.iters)
                finally:
                    h.update_values(va)
                torch.cuda.synchronize()
                bytes_att = 4 * (m + 1) + 4 * nnz + s * (k * (m + nnz) + dv * (nnz + m))
                r = dict(shape=name, desc=desc, m=m, nnz=nnz, dtype=str(va.dtype).replace("torch.", ""), k=k, dv=dv, fused_ms=round(fused, 4),
                         composition_ms=round(comp, 4), composition_over_fused=round(comp / fused, 3), b_att=bytes_att,
                         fused_tb_s=round(bytes_att / (fused * 1e-3) / 1e12, 3), same_bits=bool(torch.equal(O.view(torch.int64 if s == 8 else torch.int32),
                                                                                                            O2.view(torch.int64 if s == 8 else torch.int32))))
                print(json.dumps(r), flush=True)
                rows.append(r)
                del Q, K, V, O, O2, S
        del rp, ci, va
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
