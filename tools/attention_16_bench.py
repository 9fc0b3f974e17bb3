"""The fused attention forward on 16-bit Q, K and V (spmv_hip_attention_gqa_lse_16) against the fp32 call it widens in registers
(spmv_hip_attention_gqa_lse), in the style of tools/attention_lse_bench.py.

    python tools/attention_16_bench.py [--rows 4000000] [--patterns banded,scattered] [--types f16,bf16] [--heads 8] [--kv 8,2] [--k 8,64]
                                       [--iters 10] [--out profiles/attention_16_bench.json]

Patterns: `banded` is config 2's band (--rows rows x 32 entries: the gathered K and V rows of neighbouring rows overlap, the caches absorb much of
the gather); `scattered` is 32 uniformly random columns per row (synth.uniform_k_device: no locality, the gather goes to HBM).  One fp32 handle per
pattern with async on and device operands, no bias, L written, k = dv.  Per pattern, kv_heads, k and 16-bit type:
  a_ms      spmv_hip_attention_gqa_lse_16 with O in the 16-bit type
  b_ms      spmv_hip_attention_gqa_lse_16 with fp32 O
  c_ms      spmv_hip_attention_gqa_lse on operands widened to fp32 BEFORE the clock starts (timed before and after a and b: c_ms, c_ms_again)
  d_ms      the three .float() conversions of Q, K and V and then c, as one sequence: what a caller with 16-bit tensors pays without the 16-bit call
  same_bits O and L of b against c, bit for bit; a_rounded: a's O is c's O .to(dtype), bit for bit
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_16_bench.json"))
    a = ap.parse_args()
    build.build()
    api.load()
    heads, W = a.heads, 2
    rows = []
    for pname in a.patterns.split(","):
        make = synth.banded_device if pname == "banded" else synth.uniform_k_device
        m, n, rp, ci, va = make(a.rows, a.rows, 32, "uniform", torch.float32, DEV, 1)
        nnz = int(rp[-1].item())
        with api.Handle(m, n, rp, ci, va, M.Method_Parallel) as h:
            h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
            for k in (int(x) for x in a.k.split(",")):
                dv, scale = k, k ** -0.5
                g = torch.Generator(device=DEV)
                g.manual_seed(100 * heads + k)
                L, Lc = torch.empty((heads, m), dtype=torch.float32, device=DEV), torch.empty((heads, m), dtype=torch.float32, device=DEV)
                O32, Oc = torch.empty((m, heads * dv), dtype=torch.float32, device=DEV), torch.empty((m, heads * dv), dtype=torch.float32, device=DEV)
                for kv in (int(x) for x in a.kv.split(",")):
                    Q0, K0, V0 = (torch.rand((r, w), generator=g, dtype=torch.float32, device=DEV) * 2 - 1 for r, w in ((m, heads * k), (n, kv * k), (n, kv * dv)))
                    for tname in a.types.split(","):
                        dt = TYPES[tname]
                        Q, K, V = Q0.to(dt), K0.to(dt), V0.to(dt)
                        Qf, Kf, Vf = Q.float(), K.float(), V.float()
                        O16 = torch.empty((m, heads * dv), dtype=dt, device=DEV)
                        c_ms = med(api.time_attention_gqa_lse_launches(h.h, heads, kv, Qf, Kf, Vf, None, Oc, Lc, scale, W, a.iters)[1])
                        a_ms = med(api.time_attention_gqa_lse_16_launches(h.h, heads, kv, Q, K, V, None, O16, L, scale, W, a.iters)[1])
                        b_ms = med(api.time_attention_gqa_lse_16_launches(h.h, heads, kv, Q, K, V, None, O32, L, scale, W, a.iters)[1])
                        c_ms2 = med(api.time_attention_gqa_lse_launches(h.h, heads, kv, Qf, Kf, Vf, None, Oc, Lc, scale, W, a.iters)[1])
                        same = bool(torch.equal(bits(O32), bits(Oc)) and torch.equal(bits(L), bits(Lc)))
                        want = Oc.to(dt)
                        a_rounded = bool(torch.equal(O16.view(torch.int16), want.view(torch.int16)))
                        del Qf, Kf, Vf, want
                        rp_, ci_, va_ = h._keep

                        def widen_and_call():
                            api.attention_gqa_lse(h.h, m, rp_, ci_, va_, heads, kv, Q.float(), K.float(), V.float(), None, Oc, Lc, scale)
                        d_ms = timed_median(widen_and_call, W, a.iters)
                        c = min(c_ms, c_ms2)
                        r = dict(what="calls", pattern=f"{pname}, {m} rows x 32", m=m, nnz=nnz, type=tname, heads=heads, kv_heads=kv, k=k, dv=dv, iters=a.iters,
                                 a_ms=r4(a_ms), b_ms=r4(b_ms), c_ms=r4(c_ms), c_ms_again=r4(c_ms2), d_ms=r4(d_ms), a_over_c=round(a_ms / c, 3), b_over_c=round(b_ms / c, 3),
                                 a_over_d=round(a_ms / d_ms, 3), same_bits=same, a_rounded=a_rounded)
                        print(json.dumps(r), flush=True)
                        rows.append(r)
                        del Q, K, V, O16
                        torch.cuda.empty_cache()
                    del Q0, K0, V0
                del L, Lc, O32, Oc
                torch.cuda.empty_cache()
        del rp, ci, va
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
