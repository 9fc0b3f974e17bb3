"""Fused sparse attention backward (spmv_hip_attention_backward) against the composed backward on the library's own kernels.

    python tools/attention_backward_bench.py [--shapes 2,3o] [--k 8,32] [--iters 20] [--out profiles/attention_backward_bench.json]

All three gradients, k = dv.  Fused: spmv_hip_time_attention_backward_launches (device events around every call, min of --iters).  Composed,
in the same process on the same handle: autograd._Attention.backward's sequence -- Handle.sddmm, `* scale`, Handle.row_softmax in place,
Handle.update_values(P), Handle.spmm_transpose, Handle.sddmm(G, V), Handle.row_softmax_backward in place, `* scale`,
Handle.update_values(dS), Handle.spmm, Handle.spmm_transpose, Handle.update_values(the handle's values) -- between two torch events on the
current stream with async on; min of --iters.  The two results are compared bit for bit.
B_bwd = 4 (m + n + 2) + 12 nnz + s (2 nnz (k + dv) + m (2 k + dv) + 4 nnz + n (k + dv)) is the fused call's bytes model: the patterns of A and
A^T and perm; a K and a V row per entry in the row pass, a Q and a G row per entry in the column pass; Q, G and dQ once; P and dS written
once and gathered once; dK and dV.
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


def bits(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2,3o")
    ap.add_argument("--k", default="8,32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_backward_bench.json"))
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
                Q, K, V, G = (torch.rand(shp, generator=g, dtype=va.dtype, device=DEV) * 2 - 1 for shp in ((m, k), (n, k), (n, dv), (m, dv)))
                fused_out = [torch.empty(shp, dtype=va.dtype, device=DEV) for shp in ((m, k), (n, k), (n, dv))]
                comp_out = [torch.empty(shp, dtype=va.dtype, device=DEV) for shp in ((m, k), (n, k), (n, dv))]
                S, dP = (torch.empty((nnz,), dtype=va.dtype, device=DEV) for _ in range(2))
                fused = float(api.time_attention_backward_launches(h.h, Q, K, V, G, *fused_out, scale=scale, warmup=3, iters=a.iters)[1].min())
                h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)

                def composed():
                    h.sddmm(Q, K, S)
                    S.mul_(scale)
                    h.row_softmax(S, S)
                    h.update_values(S)
                    h.spmm_transpose(G, comp_out[2])
                    h.sddmm(G, V, dP)
                    h.row_softmax_backward(S, dP, dP)
                    dP.mul_(scale)
                    h.update_values(dP)
                    h.spmm(K, comp_out[0])
                    h.spmm_transpose(Q, comp_out[1])
                    h.update_values(va)
                try:
                    comp = timed(composed, 3, a.iters)
                finally:
                    h.update_values(va)
                torch.cuda.synchronize()
                h.attach_stream(0, async_=False)
                b_bwd = 4 * (m + n + 2) + 12 * nnz + s * (2 * nnz * (k + dv) + m * (2 * k + dv) + 4 * nnz + n * (k + dv))
                r = dict(shape=name, desc=desc, m=m, nnz=nnz, dtype=str(va.dtype).replace("torch.", ""), k=k, dv=dv, fused_ms=round(fused, 4),
                         composed_ms=round(comp, 4), composed_over_fused=round(comp / fused, 3), b_bwd=b_bwd,
                         fused_tb_s=round(b_bwd / (fused * 1e-3) / 1e12, 3),
                         same_bits=[bool(torch.equal(bits(x), bits(y))) for x, y in zip(fused_out, comp_out)])
                print(json.dumps(r), flush=True)
                rows.append(r)
                del Q, K, V, G, fused_out, comp_out, S, dP
        del rp, ci, va
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
