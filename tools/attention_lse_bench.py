"""The log-sum-exp attention calls (spmv_hip_attention_gqa_lse, spmv_hip_attention_merge, spmv_hip_attention_gqa_backward_lse) against the calls
they extend, on the shapes of tools/attention_gqa_bench.py.

    python tools/attention_lse_bench.py [--rows 10000000] [--dtypes f64,f32] [--heads 8] [--kv 8,2,1] [--k 8] [--iters 10]
                                        [--out profiles/attention_lse_bench.json]

The pattern is config 2's band (--rows rows x 32 entries), no bias, k = dv = --k; one handle per value type with async on and device operands.
Per kv_heads:
  forward   gqa_ms       spmv_hip_attention_gqa                       gqa_lse_ms      the same with L written (O compared bit for bit in the run)
  backward  gqa_bwd_ms   spmv_hip_attention_gqa_backward (all of dQ, dK, dV)
            gqa_bwd_lse_ms   spmv_hip_attention_gqa_backward_lse with the forward's own O and L (compared by allclose in the run)
  parts     the band's 32 entries per row cut into a left and a right half of 16, a handle each over the same K and V:
            parts_ms = two spmv_hip_attention_gqa_lse calls and one spmv_hip_attention_merge into the first's O and L, timed as one sequence,
            against gqa_lse_ms of the unsplit handle (the merged O compared by allclose in the run)
Once per value type:
  merge     merge_ms for m x heads*dv, against copy_ms -- torch's device copy of the same number of bytes (three m x heads*dv arrays and three
            heads x m planes: two read and one written of each) between the same events -- and the GB/s both reach: the byte bound on this box
            at this time, not a peak from a data sheet.
The existing calls are timed twice (.._ms and .._ms_again), before and after the new ones: their spread is what a difference has to exceed.
Every timing is the MEDIAN of --iters calls after 2 warm-up calls, each call between two events on the handle's stream.
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


def r4(x):
    return None if x is None else round(x, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--kv", default="8,2,1")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_lse_bench.json"))
    a = ap.parse_args()
    build.build()
    api.load()
    heads, k = a.heads, a.k
    dv, scale, W = k, k ** -0.5, 2
    rows = []
    for dname in a.dtypes.split(","):
        dt = DTYPES[dname]
        s = torch.empty((), dtype=dt).element_size()
        m, n, rp, ci, va = synth.banded_device(a.rows, a.rows, 32, "uniform", dt, DEV, 1)
        nnz = int(rp[-1].item())
        # the two halves of every row: entries 0 .. 15 and 16 .. 31 of the band, over the same columns
        rp_half = torch.arange(0, (m + 1) * 16, 16, dtype=torch.int32, device=DEV)
        halves = [ci.view(m, 32)[:, lo:lo + 16].contiguous().view(-1) for lo in (0, 16)]
        va_half = va[:m * 16].contiguous()
        stream = int(torch.cuda.current_stream().cuda_stream)
        with api.Handle(m, n, rp, ci, va, M.Method_Parallel) as h, api.Handle(m, n, rp_half, halves[0], va_half, M.Method_Parallel) as h1, \
                api.Handle(m, n, rp_half, halves[1], va_half, M.Method_Parallel) as h2:
            for x in (h, h1, h2):
                x.attach_stream(stream, async_=True)
            g = torch.Generator(device=DEV)
            g.manual_seed(100 * heads + k)
            Q, G = (torch.rand((m, heads * w), generator=g, dtype=dt, device=DEV) * 2 - 1 for w in (k, dv))
            O, Ol, O1, O2 = (torch.empty((m, heads * dv), dtype=dt, device=DEV) for _ in range(4))
            L, L1, L2 = (torch.empty((heads, m), dtype=dt, device=DEV) for _ in range(3))
            dQ, dQl = torch.empty_like(Q), torch.empty_like(Q)
            # ---- the merge against a copy of the same bytes
            h.attention_gqa_lse(Q, torch.rand((n, heads * k), generator=g, dtype=dt, device=DEV), torch.rand((n, heads * dv), generator=g, dtype=dt, device=DEV), heads, heads,
                                None, scale, out=O1, lse=L1)
            O2.copy_(O1)
            L2.copy_(L1)
            merge_ms = med(api.time_attention_merge_launches(h.h, heads, O1, L1, O2, L2, Ol, L, W, a.iters)[1])
            merge_bytes = 3 * s * (m * heads * dv + heads * m)
            src = torch.empty(merge_bytes // 2 // s, dtype=dt, device=DEV)   # a copy reads and writes: half the bytes each way
            dst = torch.empty_like(src)
            copy_ms = timed_median(lambda: dst.copy_(src), W, a.iters)
            del src, dst
            r = dict(what="merge", pattern=f"{m} rows", m=m, dtype=dname, heads=heads, dv=dv, iters=a.iters, merge_ms=r4(merge_ms), copy_ms=r4(copy_ms), bytes=merge_bytes,
                     merge_gbs=round(merge_bytes / merge_ms / 1e6, 1), copy_gbs=round(merge_bytes / copy_ms / 1e6, 1), merge_over_copy=round(merge_ms / copy_ms, 3))
            print(json.dumps(r), flush=True)
            rows.append(r)
            for kv in (int(x) for x in a.kv.split(",")):
                K, V = (torch.rand((n, kv * w), generator=g, dtype=dt, device=DEV) * 2 - 1 for w in (k, dv))
                dK, dV, dKl, dVl = torch.empty_like(K), torch.empty_like(V), torch.empty_like(K), torch.empty_like(V)
                # ---- forward: existing, new, existing again
                gqa_ms = med(api.time_attention_gqa_launches(h.h, heads, kv, Q, K, V, None, O, scale, W, a.iters)[1])
                lse_ms = med(api.time_attention_gqa_lse_launches(h.h, heads, kv, Q, K, V, None, Ol, L, scale, W, a.iters)[1])
                gqa_ms2 = med(api.time_attention_gqa_launches(h.h, heads, kv, Q, K, V, None, O, scale, W, a.iters)[1])
                fwd_same = bool(torch.equal(bits(O), bits(Ol)))

                # ---- two parts and the merge, one sequence
                def parts():
                    h1.attention_gqa_lse(Q, K, V, heads, kv, None, scale, out=O1, lse=L1)
                    h2.attention_gqa_lse(Q, K, V, heads, kv, None, scale, out=O2, lse=L2)
                    h.attention_merge(O1, L1, O2, L2, heads, out=O1, lse=L1)
                parts_ms = timed_median(parts, W, a.iters)
                parts_close = bool(torch.allclose(O1, Ol) and torch.allclose(L1, L))
                # ---- backward: existing, new, existing again
                bwd_ms = med(api.time_attention_gqa_backward_launches(h.h, heads, kv, Q, K, V, None, G, dQ, dK, dV, None, scale, W, a.iters)[1])
                bwd_lse_ms = med(api.time_attention_gqa_backward_lse_launches(h.h, heads, kv, Q, K, V, None, G, Ol, L, dQl, dKl, dVl, None, scale, W, a.iters)[1])
                bwd_ms2 = med(api.time_attention_gqa_backward_launches(h.h, heads, kv, Q, K, V, None, G, dQ, dK, dV, None, scale, W, a.iters)[1])
                torch.cuda.synchronize()
                bwd_close = bool(torch.allclose(dQ, dQl) and torch.allclose(dK, dKl) and torch.allclose(dV, dVl))
                r = dict(what="calls", pattern=f"banded, {m} rows x 32", m=m, nnz=nnz, dtype=dname, heads=heads, kv_heads=kv, k=k, dv=dv, iters=a.iters,
                         gqa_ms=r4(gqa_ms), gqa_ms_again=r4(gqa_ms2), gqa_lse_ms=r4(lse_ms), lse_over_gqa=round(lse_ms / min(gqa_ms, gqa_ms2), 3),
                         parts_ms=r4(parts_ms), parts_over_lse=round(parts_ms / lse_ms, 3),
                         gqa_bwd_ms=r4(bwd_ms), gqa_bwd_ms_again=r4(bwd_ms2), gqa_bwd_lse_ms=r4(bwd_lse_ms), bwd_lse_over_bwd=round(bwd_lse_ms / min(bwd_ms, bwd_ms2), 3),
                         option_attention_backward_heads=int(h.option("attention_backward_heads")), fwd_same_bits=fwd_same, parts_close=parts_close, bwd_close=bwd_close)
                print(json.dumps(r), flush=True)
                rows.append(r)
                del K, V, dK, dV, dKl, dVl
                torch.cuda.empty_cache()
            del Q, G, O, Ol, O1, O2, L, L1, L2, dQ, dQl
        del rp, ci, va, rp_half, halves, va_half
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
