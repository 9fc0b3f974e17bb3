"""Biased sparse attention (spmv_hip_attention_bias, spmv_hip_attention_bias_backward) against the no-bias heads calls and against the composition
with the bias added on the device.

    python tools/attention_bias_bench.py [--shapes 2,3o] [--configs 1x8,8x8,1x32,8x32] [--iters 10] [--out profiles/attention_bias_bench.json]

Everything runs in one process on one handle, fp64, per-head bias planes uniform in [-2, 2] on the device.  A config HxK is H heads of k = dv = K.
Forward: the bias call and the no-bias heads call by their own timers (device events around every call, min of --iters); the composition per
head -- Handle.sddmm, * scale, + B[h], Handle.row_softmax, Handle.update_values(P), Handle.spmm, and the update_values that puts the handle's
values back once at the end -- between two torch events on the current stream with async on.  Backward: the same three ways, all four outputs
wanted by the bias call, three by the no-bias call; the composition is autograd.attention(backward="composed")'s steps per head.  The bias
call's results are compared bit for bit with the composition's in the run.
Bytes model: B_att = 4 (m + 1) + 4 nnz + H s (k (m + nnz) + dv (nnz + m)) as in tools/attention_heads_bench.py; the bias adds H s nnz forward;
backward the dB store adds H s nnz more (b_bias_fwd, b_bias_bwd_extra in the rows).
A number from one box at one time: compare the columns of one run, not milliseconds across runs."""
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


def same(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2,3o")
    ap.add_argument("--configs", default="1x8,8x8,1x32,8x32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bias_bench.json"))
    a = ap.parse_args()
    build.build()
    api.load()
    configs = [tuple(int(x) for x in c.split("x")) for c in a.configs.split(",")]
    rows = []
    for name in a.shapes.split(","):
        desc, method, (m, n, rp, ci, va0) = shape(name)
        nnz = int(rp[-1].item())
        va = va0.to(torch.float64)
        s = va.element_size()
        with api.Handle(m, n, rp, ci, va, method) as h:
            for heads, k in configs:
                dv = k
                scale = k ** -0.5
                g = torch.Generator(device=DEV)
                g.manual_seed(100 * heads + k)
                Q, K, V, G = (torch.rand(shp, generator=g, dtype=va.dtype, device=DEV) * 2 - 1 for shp in ((m, heads * k), (n, heads * k), (n, heads * dv), (m, heads * dv)))
                B = torch.rand((heads, nnz), generator=g, dtype=va.dtype, device=DEV) * 4 - 2
                O, O0, Oc = (torch.empty((m, heads * dv), dtype=va.dtype, device=DEV) for _ in range(3))
                sl = [(slice(hd * k, (hd + 1) * k), slice(hd * dv, (hd + 1) * dv)) for hd in range(heads)]

                # ---- forward
                bias_ms = float(api.time_attention_bias_launches(h.h, heads, Q, K, V, B, O, scale, 2, a.iters)[1].min())
                heads_ms = float(api.time_attention_heads_launches(h.h, heads, Q, K, V, O0, scale, 2, a.iters)[1].min())
                h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)

                def composed_forward():
                    for hd, (ck, cv) in enumerate(sl):
                        S = h.sddmm(Q[:, ck], K[:, ck])
                        S.mul_(scale)
                        S.add_(B[hd])
                        P = h.row_softmax(S, out=S)
                        h.update_values(P)
                        h.spmm(V[:, cv], Oc[:, cv])
                    h.update_values(va)
                comp_ms = timed(composed_forward, 1, a.iters)
                torch.cuda.synchronize()
                fwd_same = same(O, Oc)

                # ---- backward
                dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
                dB = torch.empty_like(B)
                bias_bwd_ms = float(api.time_attention_bias_backward_launches(h.h, heads, Q, K, V, B, G, dQ, dK, dV, dB, scale, 2, a.iters)[1].min())
                dQ0, dK0, dV0 = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
                heads_bwd_ms = float(api.time_attention_heads_backward_launches(h.h, heads, Q, K, V, G, dQ0, dK0, dV0, scale, 2, a.iters)[1].min())
                h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
                cQ, cK, cV, cB = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V), torch.empty_like(B)

                def composed_backward():
                    for hd, (ck, cv) in enumerate(sl):
                        S = h.sddmm(Q[:, ck], K[:, ck])
                        S.mul_(scale)
                        S.add_(B[hd])
                        P = h.row_softmax(S, out=S)
                        h.update_values(P)
                        h.spmm_transpose(G[:, cv], cV[:, cv])
                        dP = h.sddmm(G[:, cv], V[:, cv])
                        h.row_softmax_backward(P, dP, out=cB[hd])
                        dS = torch.mul(cB[hd], scale, out=dP)
                        h.update_values(dS)
                        h.spmm(K[:, ck], cQ[:, ck])
                        h.spmm_transpose(Q[:, ck], cK[:, ck])
                    h.update_values(va)
                comp_bwd_ms = timed(composed_backward, 1, a.iters)
                torch.cuda.synchronize()
                bwd_same = same(dQ, cQ) and same(dK, cK) and same(dV, cV) and same(dB, cB)

                b_att = 4 * (m + 1) + 4 * nnz + heads * s * (k * (m + nnz) + dv * (nnz + m))
                r = dict(shape=name, desc=desc.rsplit(",", 1)[0], m=m, nnz=nnz, dtype="f64", heads=heads, k=k, dv=dv,
                         bias_ms=round(bias_ms, 4), heads_ms=round(heads_ms, 4), composed_ms=round(comp_ms, 4),
                         bias_over_heads=round(bias_ms / heads_ms, 3), composed_over_bias=round(comp_ms / bias_ms, 3),
                         bias_bwd_ms=round(bias_bwd_ms, 4), heads_bwd_ms=round(heads_bwd_ms, 4), composed_bwd_ms=round(comp_bwd_ms, 4),
                         bias_bwd_over_heads_bwd=round(bias_bwd_ms / heads_bwd_ms, 3), composed_bwd_over_bias_bwd=round(comp_bwd_ms / bias_bwd_ms, 3),
                         b_att=b_att, b_bias_fwd=b_att + heads * s * nnz, b_bias_bwd_extra=2 * heads * s * nnz,
                         bias_tb_s=round((b_att + heads * s * nnz) / (bias_ms * 1e-3) / 1e12, 3), fwd_same_bits=fwd_same, bwd_same_bits=bwd_same)
                print(json.dumps(r), flush=True)
                rows.append(r)
                del Q, K, V, G, B, O, O0, Oc, dQ, dK, dV, dB, dQ0, dK0, dV0, cQ, cK, cV, cB
                torch.cuda.empty_cache()
        del rp, ci, va0, va
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
