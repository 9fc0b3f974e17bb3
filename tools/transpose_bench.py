"""y = A^T x (spmv_hip_spmv_transpose) against y = A x (spmv()), and what building the transpose costs, on the bench shapes.

    python tools/transpose_bench.py [--shapes 2,2-ii,3o,4,27pt,rect] [--iters 20] [--out profiles/transpose_bench.json]
    python tools/transpose_bench.py --merge-trace kernel_trace.csv --out profiles/transpose_bench.json

Both multiplies are warm and timed with device events on the handle's stream (spmv_hip_time_transpose_launches / spmv_hip_time_launches;
best launch).  prepare_ms is the wall time of spmv_hip_prepare_transpose: the device transpose plus the planning and inspection of A^T.
extra_device_bytes is what the handle's device_bytes grew by.  --merge-trace reads the kernel trace of a `rocprofv3 --kernel-trace --stats`
run of this tool (same shapes, same order) and adds build_kernel_ms per shape: the summed durations of the dispatches from the shape's
first tr_hist_kernel through the tr_gather_kernel that fills val_T -- the transpose kernels, the scans between the radix passes included."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M = None
DEV = "cuda:0"


def shape(name):
    import torch
    from spmv_amd import synth
    f64, f32 = torch.float64, torch.float32
    if name == "2":
        return "config 2: banded, 1e7 rows x 32, fp64", M.Method_Parallel, synth.banded_device(10_000_000, 10_000_000, 32, "uniform", f64, DEV, 1)
    if name == "2-ii":
        return "config 2-ii: uniform columns, 1e7 rows x 32, fp64", M.Method_Parallel, synth.uniform_k_device(10_000_000, 10_000_000, 32, "uniform", f64, DEV, 1)
    if name == "3o":
        lens = synth.powerlaw_lengths_device(3_070_000, 76, 33000, 1.5, DEV, 1)
        return ("config 3 stand-in com-Orkut-style: power-law rows, R-MAT columns, fp64", M.Method_Balanced2,
                synth.from_row_lengths_device(lens, 3_070_000, "uniform", f64, DEV, 1, cols="rmat"))
    if name == "4":
        lens = synth.skewed_lengths_device(10_000_000, DEV, 1)
        return ("config 4: skewed rows, columns within +-4096, fp32", M.Method_SellCSigma,
                synth.from_row_lengths_device(lens, 10_000_000, "uniform", f32, DEV, 1, local=4096))
    if name == "27pt":
        return "27-point stencil, 215^3 periodic, fp64", M.Method_Parallel, synth.stencil27_device(215, "uniform", f64, DEV, 1)
    if name == "rect":
        return "rectangular 2e6 x 8e6, 32 uniform columns per row, fp64", M.Method_Parallel, synth.uniform_k_device(2_000_000, 8_000_000, 32, "uniform", f64, DEV, 1)
    raise SystemExit(f"unknown shape {name}")


def measure(names, iters):
    import torch
    from spmv_amd import api
    rows = []
    for name in names:
        desc, method, (m, n, rp, ci, va) = shape(name)
        nnz = int(rp[-1].item())
        with api.Handle(m, n, rp, ci, va, method) as h:
            fwd = h.info()
            x = torch.rand(n, dtype=va.dtype, device=DEV)
            y = torch.empty(m, dtype=va.dtype, device=DEV)
            t_fwd = float(api.time_launches(h.h, x, y, 5, iters)[1].min())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            api.prepare_transpose(h.h)
            prep = (time.perf_counter() - t0) * 1e3
            tinfo = api.get_transpose_info(h.h)
            xt = torch.rand(m, dtype=va.dtype, device=DEV)
            yt = torch.empty(n, dtype=va.dtype, device=DEV)
            t_tr = float(api.time_transpose_launches(h.h, xt, yt, 5, iters)[1].min())
            extra = h.info()["device_bytes"] - fwd["device_bytes"]
        r = dict(shape=name, desc=desc, method=method.name, m=m, n=n, nnz=nnz, dtype=str(va.dtype).replace("torch.", ""),
                 spmv_ms=round(t_fwd, 4), transpose_ms=round(t_tr, 4), ratio=round(t_tr / t_fwd, 3), prepare_ms=round(prep, 1),
                 create_inspect_ms=round(fwd["inspect_ms"], 1), child_inspect_ms=round(tinfo["inspect_ms"], 1),
                 schedule=fwd["schedule_name"], launch_kernels=fwd["launch_kernels"], cache_blocked=fwd["cache_blocked"],
                 t_schedule=tinfo["schedule_name"], t_launch_kernels=tinfo["launch_kernels"], t_cache_blocked=tinfo["cache_blocked"],
                 t_far_nnz=tinfo["far_nnz"], t_max_row_len=tinfo["max_row_len"], t_empty_rows=tinfo["empty_rows"],
                 t_reproducible=tinfo["reproducible"], extra_device_bytes=extra, t_device_bytes=tinfo["device_bytes"])
        print(json.dumps(r), flush=True)
        rows.append(r)
        del rp, ci, va, x, y, xt, yt
        torch.cuda.empty_cache()
    return rows


def merge_trace(rows, path):
    """build_kernel_ms per shape from a rocprofv3 kernel trace (dispatches in start order)"""
    with open(path) as f:
        ks = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    spans, cur, after_cols = [], None, False
    for k in ks:
        name = k["Kernel_Name"]
        dur = (int(k["End_Timestamp"]) - int(k["Start_Timestamp"])) * 1e-6
        if cur is None and name.startswith("spmv::tr_hist_kernel"):
            cur, after_cols = {}, False
        if cur is None:
            continue
        short = name.split("(")[0].split("<")[0].replace("void ", "").replace("spmv::", "").strip()
        cur[short] = cur.get(short, 0.0) + dur
        if short == "tr_columns_kernel":
            after_cols = True
        elif short == "tr_gather_kernel" and after_cols:
            spans.append(cur)
            cur = None
    if len(spans) != len(rows):
        raise SystemExit(f"{len(spans)} transpose builds in the trace, {len(rows)} shapes in the table")
    for r, s in zip(rows, spans):
        r["build_kernel_ms"] = round(sum(s.values()), 3)
        r["build_kernels_ms"] = {k: round(v, 3) for k, v in sorted(s.items(), key=lambda kv: -kv[1])}
        r["build_share_of_prepare"] = round(r["build_kernel_ms"] / r["prepare_ms"], 3)
    return rows


def main():
    global M
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2,2-ii,3o,4,27pt,rect")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-trace", default=None, help="kernel_trace.csv of a rocprofv3 run of this tool; merged into --out")
    a = ap.parse_args()
    if a.merge_trace:
        with open(a.out) as f:
            rows = merge_trace(json.load(f), a.merge_trace)
    else:
        from spmv_amd import api, build
        M = api.SPMV_METHODS
        build.build()
        api.load()
        rows = measure(a.shapes.split(","), a.iters)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
