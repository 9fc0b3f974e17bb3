"""Run by tests/test_gpu_lds_edges.py in a FRESH process: the 59..64 KiB band before anything has raised a kernel's LDS attribute.

ensure_lds (kernels/common.hpp) raises hipFuncAttributeMaxDynamicSharedMemorySize once per kernel instantiation and process, and the
value only grows: in a test process that has already launched a kernel with 96 KiB, a band request no longer shows what the runtime does
with static + dynamic LDS above 64 KiB under the DEFAULT attribute.  Here the requests of each value type go up from 59 to 64 KiB and
nothing larger has run before them, so no launch can lean on an earlier, larger grant.  Every case asserts the form, the error channel
and bit-exact y (test_gpu_lds_edges._run_case); prints one JSON line: kernel -> the lds_bytes values it was launched with."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import lds_edges as E
    import test_gpu_lds_edges as T
    from spmv_amd import api
    api.load()
    reached = {}
    for dt in E.DTYPES:
        for t in T.BAND_KIB:                                                  # ascending
            for case, family, target in E.line_cases():
                if case.dt != dt or target != t * E.KIB:
                    continue
                got = {}
                sell = [T.M.Method_SellCSigma]
                T._run_case(case, 300 + t, sell if family == "sell" else [m for m in E.METHODS if m not in sell], reached=got)
                assert got and all(v == {target} for v in got.values()), (case.name, target, got)
                for k, v in got.items():
                    reached.setdefault(k, set()).update(v)
    print(json.dumps({k: sorted(v) for k, v in reached.items()}))


if __name__ == "__main__":
    main()
