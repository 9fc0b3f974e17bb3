"""The fused attention backward on 16-bit Q, K, V and G (spmv_hip_attention_gqa_backward_16) against the fp32 backward it widens in registers
(spmv_hip_attention_gqa_backward / _backward_lse), in the style of tools/attention_16_bench.py.

    python tools/attention_backward_16_bench.py [--rows 4000000] [--patterns banded,scattered] [--types f16,bf16] [--heads 8] [--kv 8,2] [--k 8,64]
                                                [--forms self,lse] [--iters 10] [--out profiles/attention_backward_16_bench.json]

Patterns: `banded` is config 2's band (--rows rows x 32 entries); `scattered` is 32 uniformly random columns per row (synth.uniform_k_device).  One
fp32 handle per pattern with async on and device operands, no bias, dQ, dK and dV wanted, k = dv.  form `self` is the self-normalising row pass,
`lse` the one driven by the forward's own fp32 O and L.  Per pattern, kv_heads, k, 16-bit type and form:
  a_ms      spmv_hip_attention_gqa_backward_16 with dQ, dK and dV in the 16-bit type
  b_ms      spmv_hip_attention_gqa_backward_16 with fp32 dQ, dK and dV
  c_ms      the fp32 backward on operands widened BEFORE the clock starts (timed before and after a and b: c_ms, c_ms_again)
  d_ms      what a caller with 16-bit tensors paid before: four .float() conversions (Q, K, V, G), then c, then three .to(dtype) conversions
  same_bits b's gradients against c's, bit for bit; rounded: a's gradients are c's .to(dtype), bit for bit
  a_peak_mb, d_peak_mb   peak device memory of route a and of route d, operands included: torch's peak allocation plus the handle's device_bytes
Every timing is the MEDIAN of --iters calls after 2 warm-up calls, each call between two events on the handle's stream.
A number from one box at one time: compare the columns of one run, not milliseconds across runs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from spmv_amd import api, build, synth  # noqa: E402
from tools.attention_lse_bench import bits, med, r4, timed_median  # noqa: E402
from tools.spmm_bench import DEV  # noqa: E402

M = api.SPMV_METHODS
TYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--patterns", default="banded,scattered")
    ap.add_argument("--types", default="f16,bf16")
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--kv", default="8,2")
    ap.add_argument("--k", default="8,64")
    ap.add_argument("--forms", default="self,lse")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_backward_16_bench.json"))
    a = ap.parse_args()
    build.build()
    api.load()
    heads, W = a.heads, 2
    rows = []
    mb = lambda h: round((torch.cuda.max_memory_allocated() + h.info()["device_bytes"]) / 2 ** 20, 1)
    for pname in a.patterns.split(","):
        make = synth.banded_device if pname == "banded" else synth.uniform_k_device
        m, n, rp, ci, va = make(a.rows, a.rows, 32, "uniform", torch.float32, DEV, 1)
        nnz = int(rp[-1].item())
        with api.Handle(m, n, rp, ci, va, M.Method_Parallel) as h:
            h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
            rp_, ci_, va_ = h._keep
            for k in (int(x) for x in a.k.split(",")):
                dv, scale = k, k ** -0.5
                g = torch.Generator(device=DEV)
                g.manual_seed(100 * heads + k)
                for kv in (int(x) for x in a.kv.split(",")):
                    shapes = ((m, heads * k), (n, kv * k), (n, kv * dv), (m, heads * dv))
                    for tname in a.types.split(","):
                        dt = TYPES[tname]
                        Q, K, V, G = ((torch.rand(s, generator=g, dtype=torch.float32, device=DEV) * 2 - 1).to(dt) for s in shapes)
                        O, L = h.attention_gqa_lse_16(Q, K, V, heads, kv, None, scale, out_dtype=torch.float32)   # the forward's own fp32 O and L
                        for form in a.forms.split(","):
                            OL = (O, L) if form == "lse" else (None, None)
                            g16 = [torch.empty(s, dtype=dt, device=DEV) for s in shapes[:3]]

                            def route_a():
                                api.attention_gqa_backward_16(h.h, m, rp_, ci_, va_, heads, kv, Q, K, V, None, G, *OL, *g16, None, scale)

                            def fp32_backward(ops, outs):
                                if form == "lse":
                                    api.attention_gqa_backward_lse(h.h, m, rp_, ci_, va_, heads, kv, *ops[:3], None, ops[3], O, L, *outs, None, scale)
                                else:
                                    api.attention_gqa_backward(h.h, m, rp_, ci_, va_, heads, kv, *ops[:3], None, ops[3], *outs, None, scale)

                            def route_d():
                                ops = [t.float() for t in (Q, K, V, G)]
                                outs = [torch.empty(s, dtype=torch.float32, device=DEV) for s in shapes[:3]]
                                fp32_backward(ops, outs)
                                return [o.to(dt) for o in outs]

                            route_a()   # the handle's arrays, untimed: both routes find them
                            torch.cuda.synchronize()
                            torch.cuda.reset_peak_memory_stats()
                            route_a()
                            torch.cuda.synchronize()
                            a_peak = mb(h)
                            torch.cuda.reset_peak_memory_stats()
                            got_d = route_d()
                            torch.cuda.synchronize()
                            d_peak = mb(h)
                            del got_d
                            wide = [t.float() for t in (Q, K, V, G)]
                            g32, gc = ([torch.empty(s, dtype=torch.float32, device=DEV) for s in shapes[:3]] for _ in range(2))
                            c_fn = lambda: fp32_backward(wide, gc)
                            b_fn = lambda: api.attention_gqa_backward_16(h.h, m, rp_, ci_, va_, heads, kv, Q, K, V, None, G, *OL, *g32, None, scale)
                            c_ms = timed_median(c_fn, W, a.iters)
                            a_ms = timed_median(route_a, W, a.iters)
                            b_ms = timed_median(b_fn, W, a.iters)
                            c_ms2 = timed_median(c_fn, W, a.iters)
                            same = all(bool(torch.equal(bits(x), bits(y))) for x, y in zip(g32, gc))
                            rounded = all(bool(torch.equal(x.view(torch.int16), y.to(dt).view(torch.int16))) for x, y in zip(g16, gc))
                            del wide, g32, gc
                            torch.cuda.empty_cache()
                            d_ms = timed_median(route_d, W, a.iters)
                            c = min(c_ms, c_ms2)
                            r = dict(what="calls", pattern=f"{pname}, {m} rows x 32", m=m, nnz=nnz, type=tname, form=form, heads=heads, kv_heads=kv, k=k, dv=dv, iters=a.iters,
                                     a_ms=r4(a_ms), b_ms=r4(b_ms), c_ms=r4(c_ms), c_ms_again=r4(c_ms2), d_ms=r4(d_ms), a_over_c=round(a_ms / c, 3), b_over_c=round(b_ms / c, 3),
                                     a_over_d=round(a_ms / d_ms, 3), same_bits=same, rounded=rounded, a_peak_mb=a_peak, d_peak_mb=d_peak)
                            print(json.dumps(r), flush=True)
                            rows.append(r)
                            del g16
                            torch.cuda.empty_cache()
                        del Q, K, V, G, O, L
                        torch.cuda.empty_cache()
        del rp, ci, va
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
