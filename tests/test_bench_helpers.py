"""CPU: the pure helpers of bench.py -- the three roofline fractions, the traffic lookup's keying (kernel, shape, dtype, the model's byte count and the
source hash), the column-stream accounting, the per-kernel shares, what a plain run leaves to --full and the --dump-outputs sample.  No GPU, no
library call: fake spmv_hip_info dictionaries."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _info(**kw):
    base = dict(kernel_name="csr_vector_tile_kernel", m=1000, n=1000, nnz=32000, alg_bytes=400_000, stream_bytes=300_000, x_bytes=9000, cache_blocked=0,
                x_groups=4, x_groups_staged=4, run_nnz=0, byte_nnz=0, tmpl_nnz=0, launch_kernels=["csr_vector_tile_kernel"])
    base.update(kw)
    return base


@pytest.fixture()
def fake_profiles(monkeypatch, tmp_path):
    from spmv_amd import srchash
    (tmp_path / "profiles").mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "_TRAFFIC", None)

    def write(sha, entries):
        with open(tmp_path / "profiles" / "traffic_r99.json", "w") as f:
            json.dump({"csrc_sha": sha, "entries": entries}, f)
        bench._TRAFFIC = None
    return write, srchash.csrc_sha()


def test_fractions_side_by_side_and_frac_is_the_counter_one_only_when_the_profile_matches(fake_profiles):
    write, sha = fake_profiles
    entry = {"kernel_short": "csr_vector_tile_kernel", "m": 1000, "nnz": 32000, "dtype": "f64", "model_stream_bytes": 300_000, "hbm_bytes_per_launch": 290_000.0,
             "source": "profiles/x", "kernels": [{"kernel": "csr_vector_tile_kernel", "avg_ms": 0.5, "hbm_bytes": 290_000.0}]}
    write(sha, [entry])
    rf = bench.roofline_fields(_info(), 0.001, "f64")          # 1 us launch
    assert rf["frac_source"] == "counter" and rf["traffic"] == 290_000.0
    assert rf["frac"] == rf["frac_counter"] == round(290_000 / 1e-6 / 1e9 / 8000.0, 4)
    assert rf["frac_model"] == round(300_000 / 1e-6 / 1e9 / 8000.0, 4) and rf["frac_alg"] == round(400_000 / 1e-6 / 1e9 / 8000.0, 4)
    assert rf["kernels"] == [{"kernel": "csr_vector_tile_kernel", "avg_ms_rocprof": 0.5, "share": 1.0, "hbm_bytes": 290_000.0}]
    # another matrix of the same shape (config 2 vs config 2 with holes): the model's byte count differs -> no match
    rf = bench.roofline_fields(_info(stream_bytes=330_000), 0.001, "f64")
    assert rf["frac_source"] == "model" and rf["traffic"] is None and rf["frac"] == rf["frac_model"] and rf["frac_counter"] is None
    # two matrices whose byte counts differ by less than the tolerance (the Orkut-style stand-in with R-MAT and with uniform columns): the closest entry wins
    near = dict(entry, model_stream_bytes=300_020, hbm_bytes_per_launch=310_000.0, source="profiles/near")
    write(sha, [near, entry])
    assert bench.roofline_fields(_info(), 0.001, "f64")["traffic"] == 290_000.0
    assert bench.roofline_fields(_info(stream_bytes=300_019), 0.001, "f64")["traffic"] == 310_000.0
    # a profile taken on another source tree says nothing about this run
    write("0" * 16, [entry])
    rf = bench.roofline_fields(_info(), 0.001, "f64")
    assert rf["frac_source"] == "model" and rf["traffic"] is None


def test_cache_resident_shapes_get_the_cache_level_bound(fake_profiles):
    write, sha = fake_profiles
    write(sha, [])
    small = bench.roofline_fields(_info(stream_bytes=48 << 20, alg_bytes=51 << 20), 0.027, "f64")
    assert small["cache_resident"]["level"] == "infinity_cache" and small["cache_resident"]["peak"] == bench.IC_READ_GBPS
    tiny = bench.roofline_fields(_info(stream_bytes=8 << 20, alg_bytes=9 << 20), 0.01, "f64")
    assert tiny["cache_resident"]["level"] == "l2"
    big = bench.roofline_fields(_info(stream_bytes=3 << 30, alg_bytes=4 << 30), 0.41, "f64")
    assert "cache_resident" not in big


def test_column_stream_bytes_per_nonzero():
    assert bench.column_stream_bytes(_info(run_nnz=32000)) == 0.0                       # RUN tiles: 2 B per row, nothing per entry
    assert bench.column_stream_bytes(_info(tmpl_nnz=32000)) == 0.0                      # TEMPLATE tiles likewise
    assert bench.column_stream_bytes(_info(byte_nnz=32000)) == 1.0                      # BYTE tiles
    assert bench.column_stream_bytes(_info()) == 2.0                                    # staged: 16-bit slots
    assert bench.column_stream_bytes(_info(x_groups_staged=0)) == 4.0                   # unstaged: int32 ColIdx
    assert bench.column_stream_bytes(_info(cache_blocked=1)) == 4.0                     # blocked streams: a 32-bit word per entry
    assert bench.column_stream_bytes(_info(run_nnz=16000, byte_nnz=8000)) == round((8000 * 1.0 + 8000 * 2.0) / 32000, 3)


def test_kernel_shares_list_every_launch():
    parts = [{"kernel": "csr5_group_pipe_kernel", "avg_ms": 0.41, "hbm_bytes": 2.7e9}, {"kernel": "sell_window_kernel", "avg_ms": 0.17, "hbm_bytes": 1.1e9},
             {"kernel": "csr5_fixup_kernel", "avg_ms": 0.008, "hbm_bytes": 1e7}]
    out = bench.kernel_shares(["sell_window_kernel", "csr5_group_pipe_kernel", "csr5_fixup_kernel"], parts)
    assert [k["kernel"] for k in out] == ["sell_window_kernel", "csr5_group_pipe_kernel", "csr5_fixup_kernel"]
    assert abs(sum(k["share"] for k in out) - 1.0) < 2e-3 and out[1]["share"] > 0.69
    assert bench.kernel_shares(["nat_kernel", "csr5_fixup_kernel"], None) == [{"kernel": "nat_kernel"}, {"kernel": "csr5_fixup_kernel"}]


def test_plain_run_is_lean_and_full_brings_the_rest_back():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    assert a.xchg == "halo" and a.scaling == "weak"                     # N > 1 plain: the headline exchange and leg only
    f = bench.parse(["--full"])
    assert f.full is True and f.xchg == "all" and f.scaling == "both"  # what every run measured before --full existed
    e = bench.parse(["--xchg", "bcast", "--scaling", "strong", "--dump-outputs", "out"])
    assert e.xchg == "bcast" and e.scaling == "strong" and e.dump_outputs == "out"


def test_dump_rows_is_a_fixed_seeded_sample_within_the_budget():
    assert bench.dump_rows(1000, 8) is None                              # fits: every row
    assert bench.dump_rows(10_000_000, 4) is None                        # fp32 config 2: 40 MB, every row
    rows = bench.dump_rows(10_000_000, 8)                                # fp64 config 2: 80 MB, sampled
    assert rows.size * 8 <= bench.DUMP_BYTES < 64 << 20
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < 10_000_000
    assert np.array_equal(rows, bench.dump_rows(10_000_000, 8))          # the same rows in every run
    r1 = bench.dump_rows(10_000_000, 8, world=2, rank=1)
    assert r1.size * 8 * 2 <= bench.DUMP_BYTES and not np.array_equal(r1, rows[: r1.size])


def test_dump_outputs_writes_y_in_its_dtype(tmp_path):
    import torch
    y = torch.arange(5000, dtype=torch.float64) / 7
    d = bench.dump_outputs(str(tmp_path / "o"), y)
    got = np.load(tmp_path / "o" / "y.npy")
    assert got.dtype == np.float64 and np.array_equal(got, y.numpy())
    assert d["files"]["y"] == {"dtype": "float64", "entries": 5000, "of_rows": 5000, "sampled": False}
    bench.dump_outputs(str(tmp_path / "o"), y.float(), world=2, rank=1)
    assert np.load(tmp_path / "o" / "y_rank1.npy").dtype == np.float32
