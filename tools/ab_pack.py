#!/usr/bin/env python3
"""A/B of the packed value planes (option pack_values) on BASELINE config 2 -- fp64 banded, 32 nnz per row, Method_Parallel -- in ONE process:
two handles on the same matrix, pack_values = 0 and 1, timed with time_launches in interleaved rounds; y compared bit for bit.  One JSON line.
    python tools/ab_pack.py [rows (default 10000000)] [rounds (default 5)] [launches per round (default 40)]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from spmv_amd import api, build, synth
build.build(); api.load()
dev = "cuda:0"
m = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 40
_, _, rp, ci, va = synth.banded_device(m, m, 32, "uniform", torch.float64, dev, seed=1)
g = torch.Generator(device=dev); g.manual_seed(1234)
x = torch.rand(m, generator=g, device=dev, dtype=torch.float64) * 2 - 1
hs, ys, infos = {}, {}, {}
for pack in (0, 1):
    api.set_thread_option("pack_values", pack)
    try:
        hs[pack] = api.Handle(m, m, rp, ci, va, int(api.SPMV_METHODS.Method_Parallel))
    finally:
        api.clear_thread_options()
    ys[pack] = torch.full((m,), float("nan"), dtype=torch.float64, device=dev)
    infos[pack] = hs[pack].info()
ms = {0: [], 1: []}
for r in range(rounds):
    for pack in (0, 1):
        _, t = api.time_launches(hs[pack].h, x, ys[pack], 3, iters)
        ms[pack].append(float(t.min()))
out = {"tool": "ab_pack", "m": m, "nnz": int(infos[0]["nnz"]), "lanes_per_row": infos[1]["lanes_per_row"], "rounds": rounds, "launches_per_round": iters,
       "tuned_choice": [infos[0]["tuned_choice"], infos[1]["tuned_choice"]], "packed_nnz": int(infos[1]["packed_nnz"]),
       "stream_bytes": [int(infos[0]["stream_bytes"]), int(infos[1]["stream_bytes"])], "device_bytes": [int(infos[0]["device_bytes"]), int(infos[1]["device_bytes"])],
       "ms_min_plain": [round(v, 5) for v in ms[0]], "ms_min_packed": [round(v, 5) for v in ms[1]],
       "ratio_best": round(min(ms[1]) / min(ms[0]), 4), "ratio_worst_packed_over_best_plain": round(max(ms[1]) / min(ms[0]), 4),
       "y_bit_identical": bool(torch.equal(ys[0].view(torch.int64), ys[1].view(torch.int64)))}
for h in hs.values():
    h.close()
print(json.dumps(out), flush=True)
