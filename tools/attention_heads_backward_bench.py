"""All heads' gradients in two passes per group of heads (spmv_hip_attention_heads_backward) against one spmv_hip_attention_backward call per head.

    python tools/attention_heads_backward_bench.py [--shapes 2,3o] [--dtypes f64,f32] [--hk 4x8,8x8,2x32] [--iters 20]
                                                   [--out profiles/attention_heads_backward_bench.json]

All three gradients, k = dv.  Per shape and value type, in one process: a handle with option "attention_backward_heads" = 0 (as many heads per
round as the memory rule allows) runs H back-to-back api.attention_backward calls on the column slices -- what autograd.attention_heads'
default backward does -- and, on the same handle and the same buffers, the heads call; a second handle with the option = 1 (H rounds of one
head) runs the heads call again.  Every timing is the minimum of --iters runs, each between two events on the handle's stream (async on).  The three gradients
of every heads call are compared bit for bit with the per-head loop's in the run.
B = rounds * (4 (m + n + 2) + 12 nnz) + H * s (2 nnz (k + dv) + m (2 k + dv) + 4 nnz + n (k + dv)) is the heads call's bytes model: B_bwd's
index terms (the patterns of A and A^T and perm) once per round, its operand terms H times.
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

OPTION = "attention_backward_heads"
DTYPES = {"f64": torch.float64, "f32": torch.float32}


def bits(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def make_handle(m, n, rp, ci, va, method, option):
    api.set_thread_option(OPTION, option)
    try:
        h = api.Handle(m, n, rp, ci, va, method)
    finally:
        api.clear_thread_options()
    h.attach_stream(int(torch.cuda.current_stream().cuda_stream), async_=True)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2,3o")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--hk", default="4x8,8x8,2x32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_heads_backward_bench.json"))
    a = ap.parse_args()
    build.build()
    api.load()
    eighth = torch.cuda.mem_get_info()[1] // 8
    cases = [tuple(int(x) for x in c.split("x")) for c in a.hk.split(",")]
    rows = []
    for name in a.shapes.split(","):
        desc, method, (m, n, rp, ci, va64) = shape(name)
        nnz = int(rp[-1].item())
        for dt in a.dtypes.split(","):
            va = va64.to(DTYPES[dt])
            s = va.element_size()
            with make_handle(m, n, rp, ci, va, method, 0) as h0, make_handle(m, n, rp, ci, va, method, 1) as h1:
                for H, k in cases:
                    dv, scale = k, k ** -0.5
                    g = torch.Generator(device=DEV)
                    g.manual_seed(100 * H + k)
                    Q, K, V, G = (torch.rand(shp, generator=g, dtype=va.dtype, device=DEV) * 2 - 1 for shp in ((m, H * k), (n, H * k), (n, H * dv), (m, H * dv)))
                    out = [torch.empty(shp, dtype=va.dtype, device=DEV) for shp in ((m, H * k), (n, H * k), (n, H * dv))]
                    lo = [torch.empty_like(o) for o in out]

                    def per_head():   # on the option-0 handle, the one the first heads call runs on
                        for hd in range(H):
                            ck, cv = slice(hd * k, (hd + 1) * k), slice(hd * dv, (hd + 1) * dv)
                            api.attention_backward(h0.h, m, rp, ci, va, Q[:, ck], K[:, ck], V[:, cv], G[:, cv], lo[0][:, ck], lo[1][:, ck], lo[2][:, cv], scale=scale)
                    loop_ms = timed(per_head, 3, a.iters)
                    for option, h in ((0, h0), (1, h1)):
                        for o in out:
                            o.fill_(float("nan"))
                        ms = timed(lambda: api.attention_heads_backward(h.h, m, rp, ci, va, H, Q, K, V, G, *out, scale=scale), 3, a.iters)
                        torch.cuda.synchronize()
                        hg = min(H, max(1, eighth // (2 * s * nnz))) if option == 0 else 1
                        rounds = -(-H // hg)
                        b = rounds * (4 * (m + n + 2) + 12 * nnz) + H * s * (2 * nnz * (k + dv) + m * (2 * k + dv) + 4 * nnz + n * (k + dv))
                        r = dict(shape=name, desc=desc, m=m, nnz=nnz, dtype=dt, heads=H, k=k, dv=dv, option=option, heads_per_round=hg, rounds=rounds,
                                 heads_ms=round(ms, 4), per_head_ms=round(loop_ms, 4), per_head_over_heads=round(loop_ms / ms, 3), bytes_model=b,
                                 heads_tb_s=round(b / (ms * 1e-3) / 1e12, 3), plane_bytes=2 * hg * s * nnz,
                                 same_bits=[bool(torch.equal(bits(x), bits(y))) for x, y in zip(out, lo)])
                        print(json.dumps(r), flush=True)
                        rows.append(r)
                    del Q, K, V, G, out, lo
                    torch.cuda.empty_cache()
            del va
            torch.cuda.empty_cache()
        del rp, ci, va64
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
