"""Grouped-query sparse attention (spmv_hip_attention_gqa, spmv_hip_attention_gqa_backward) against what a caller did before it existed: K and V
repeated heads / kv_heads times, the heads call, and -- backward -- the group sums of dK and dV in torch.

    python tools/attention_gqa_bench.py [--rows 10000000] [--dtypes f64,f32] [--heads 8] [--kv 8,2,1] [--k 8] [--iters 10]
                                        [--out profiles/attention_gqa_bench.json]

The pattern is config 2's band (tools/spmm_bench.py: --rows rows x 32 entries, columns within the band), no bias, k = dv = --k.  Everything of one
value type runs in one process on one handle with async on and device operands.  Per kv_heads, forward and backward (all of dQ, dK, dV):
  (a) gqa_ms            the GQA call on K (n x kv*k) and V (n x kv*dv)
  (b) expanded_ms       the heads call on K and V already repeated (the expansion and, backward, the reduction NOT timed)
      expanded_full_ms  repeat_interleave of K and V, the heads call and, backward, dK / dV summed group by group in torch -- all timed
  (c) heads_ms          kv_heads = heads only: the existing heads call on the same operands (the GQA entry point's overhead over it)
Every timing is the MEDIAN of --iters calls after 2 warm-up calls, each call between two events on the handle's stream (the library's timers
for the single calls, torch events for (b)'s sequences).  O and dQ of (a) are compared bit for bit with (b)'s in the run; dK and dV of (a) are
compared with torch's group sums by allclose only (torch's order of summation is its own).
Gathered operand bytes differ between (a) and (b): K and V are kv/heads as wide, so their footprint -- what has to stay in the caches while a
band's rows reuse it -- shrinks by that factor; the instructions and the index streams are the same.
A number from one box at one time: compare the columns of one run, not milliseconds across runs."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from spmv_amd import api, build, synth  # noqa: E402
from tools.spmm_bench import DEV  # noqa: E402

M = api.SPMV_METHODS
DTYPES = {"f64": torch.float64, "f32": torch.float32}


def bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def same(a, b):
    return bool(torch.equal(bits(a), bits(b)))


def med(ms):
    return float(statistics.median(float(x) for x in ms))


def timed_median(fn, warmup, iters):
    """median ms of `iters` calls, each between two events on the current stream"""
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    for i in range(iters):
        ev[i].record()
        fn()
    ev[iters].record()
    torch.cuda.synchronize()
    return med(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--kv", default="8,2,1")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_gqa_bench.json"))
    a = ap.parse_args()
    build.build()
    api.load()
    heads, k = a.heads, a.k
    dv, scale, W = k, k ** -0.5, 2
    rows = []
    for dname in a.dtypes.split(","):
        dt = DTYPES[dname]
        m, n, rp, ci, va = synth.banded_device(a.rows, a.rows, 32, "uniform", dt, DEV, 1)
        nnz = int(rp[-1].item())
        with api.Handle(m, n, rp, ci, va, M.Method_Parallel) as h:
            h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
            g = torch.Generator(device=DEV)
            g.manual_seed(100 * heads + k)
            Q, G = (torch.rand((m, heads * w), generator=g, dtype=dt, device=DEV) * 2 - 1 for w in (k, dv))
            O, Ob = (torch.empty((m, heads * dv), dtype=dt, device=DEV) for _ in range(2))
            dQ, dQb = torch.empty_like(Q), torch.empty_like(Q)
            for kv in (int(x) for x in a.kv.split(",")):
                gs = heads // kv
                K, V = (torch.rand((n, kv * w), generator=g, dtype=dt, device=DEV) * 2 - 1 for w in (k, dv))

                def expand(X, w):
                    return X.view(n, kv, w).repeat_interleave(gs, dim=1).reshape(n, heads * w)

                Ke, Ve = expand(K, k), expand(V, dv)
                # ---- forward
                gqa_ms = med(api.time_attention_gqa_launches(h.h, heads, kv, Q, K, V, None, O, scale, W, a.iters)[1])
                exp_ms = med(api.time_attention_heads_launches(h.h, heads, Q, Ke, Ve, Ob, scale, W, a.iters)[1])
                fwd_same = same(O, Ob)

                def expanded_forward():
                    h.attention_heads(Q, expand(K, k), expand(V, dv), heads, scale, out=Ob)
                full_ms = timed_median(expanded_forward, W, a.iters)
                heads_ms = med(api.time_attention_heads_launches(h.h, heads, Q, K, V, Ob, scale, W, a.iters)[1]) if kv == heads else None

                # ---- backward
                dK, dV = torch.empty_like(K), torch.empty_like(V)
                dKe, dVe = torch.empty_like(Ke), torch.empty_like(Ve)
                gqa_bwd_ms = med(api.time_attention_gqa_backward_launches(h.h, heads, kv, Q, K, V, None, G, dQ, dK, dV, None, scale, W, a.iters)[1])
                exp_bwd_ms = med(api.time_attention_heads_backward_launches(h.h, heads, Q, Ke, Ve, G, dQb, dKe, dVe, scale, W, a.iters)[1])
                sums = [None, None]

                def expanded_backward():
                    api.attention_heads_backward(h.h, m, rp, ci, va, heads, Q, expand(K, k), expand(V, dv), G, dQb, dKe, dVe, scale)
                    sums[0] = dKe.view(n, kv, gs, k).sum(2).reshape(n, kv * k)
                    sums[1] = dVe.view(n, kv, gs, dv).sum(2).reshape(n, kv * dv)
                full_bwd_ms = timed_median(expanded_backward, W, a.iters)
                heads_bwd_ms = med(api.time_attention_heads_backward_launches(h.h, heads, Q, K, V, G, dQb, dKe, dVe, scale, W, a.iters)[1]) if kv == heads else None
                torch.cuda.synchronize()
                bwd_same = same(dQ, dQb)
                close = bool(torch.allclose(dK, sums[0]) and torch.allclose(dV, sums[1]))

                def ratio(x, y):
                    return None if x is None or y is None else round(x / y, 3)

                def r4(x):
                    return None if x is None else round(x, 4)

                r = dict(pattern=f"banded, {m} rows x 32", m=m, nnz=nnz, dtype=dname, heads=heads, kv_heads=kv, k=k, dv=dv, iters=a.iters,
                         gqa_ms=r4(gqa_ms), expanded_ms=r4(exp_ms), expanded_full_ms=r4(full_ms), heads_ms=r4(heads_ms),
                         expanded_over_gqa=ratio(exp_ms, gqa_ms), expanded_full_over_gqa=ratio(full_ms, gqa_ms), gqa_over_heads=ratio(gqa_ms, heads_ms),
                         gqa_bwd_ms=r4(gqa_bwd_ms), expanded_bwd_ms=r4(exp_bwd_ms), expanded_full_bwd_ms=r4(full_bwd_ms), heads_bwd_ms=r4(heads_bwd_ms),
                         expanded_bwd_over_gqa_bwd=ratio(exp_bwd_ms, gqa_bwd_ms), expanded_full_bwd_over_gqa_bwd=ratio(full_bwd_ms, gqa_bwd_ms),
                         gqa_bwd_over_heads_bwd=ratio(gqa_bwd_ms, heads_bwd_ms),
                         option_attention_backward_heads=int(h.option("attention_backward_heads")), fwd_same_bits=fwd_same, dq_same_bits=bwd_same, dk_dv_close=close)
                print(json.dumps(r), flush=True)
                rows.append(r)
                del K, V, Ke, Ve, dK, dV, dKe, dVe, sums
                torch.cuda.empty_cache()
            del Q, G, O, Ob, dQ, dQb
        del rp, ci, va
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
