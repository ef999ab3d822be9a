"""bench.py's plain run and --dump-outputs: the plain run does only what its headline figure needs, --full adds the rest, and
the dumped arrays are what the last timed step computed (checked against the CPU oracle replaying the same seeded batches)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_plain_run_is_the_default_and_full_is_opt_in():
    bench = _bench()
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


@pytest.mark.parametrize("config", [2, 5])
def test_device_batch_generation_equals_the_host_stream(config, monkeypatch):
    """gen_batch_dev (what the timed steps merge) computes the very bits of gen_batch (bmx.synth, what the oracle replays)"""
    import torch
    bench = _bench()
    monkeypatch.setattr(bench, "CONFIG", config)
    for b, R, D in ((0, 20000, 5000), (3, 20000, 5000), (17, 10_000_000, 1 << 16), (1000, 10_000_000, 3000)):
        got = bench.gen_batch_dev(b, R, torch.device("cpu"), D=D)
        want = bench.to_dev(bench.gen_batch(b, R, D=D), torch.device("cpu"))
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(g, w), (config, b)


def test_row_sample_is_fixed_and_bounded():
    bench = _bench()
    ids = np.arange(3 * bench.DUMP_ROW_SAMPLE, dtype=np.uint64) * np.uint64(7)
    flds = np.full(len(ids), 5, np.uint32)
    a, fa = bench.row_sample(ids, flds)
    b, _ = bench.row_sample(ids, flds)
    assert len(a) == bench.DUMP_ROW_SAMPLE and np.array_equal(a, b) and np.all(np.diff(a.astype(np.int64)) > 0) and np.all(fa == 5)
    small, _ = bench.row_sample(ids[:10], flds[:10])
    assert np.array_equal(small, ids[:10])


def test_dump_outputs_writes_float64_within_the_limit(tmp_path):
    bench = _bench()
    bench.dump_outputs(str(tmp_path / "d"), {"winners": np.array([3, 1, 2], np.int32), "found": np.array([True, False])})
    w = np.load(str(tmp_path / "d" / "winners.npy"))
    assert w.dtype == np.float64 and w.tolist() == [3.0, 1.0, 2.0]
    assert np.load(str(tmp_path / "d" / "found.npy")).tolist() == [1.0, 0.0]
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "e"), {"big": np.zeros(bench.DUMP_LIMIT // 8 + 1, np.float64)})
    assert not os.path.exists(str(tmp_path / "e"))


@pytest.mark.gpu
def test_plain_bench_dumps_what_its_last_step_computed(tmp_path):
    bench = _bench()
    from bmx import synth
    from oracle.oracle import Oracle
    out = str(tmp_path / "outputs")
    env = dict(os.environ, BMX_BENCH_DETAIL=str(tmp_path / "detail.json"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert len(r.stdout.strip().splitlines()) == 1
    line = json.loads(r.stdout)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["metric"] == "CRDT field-merges/s" and line["unit"] == "merges/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["verified"] is None and line["roofline"] is None and line["cpu_baseline"] is None and "scan_config3" not in line
    arrays = {k: np.load(os.path.join(out, k + ".npy")) for k in ("winners", "row_sample_ts", "row_sample_val", "row_sample_found")}
    assert all(a.dtype == np.float64 for a in arrays.values())
    # the same three seeded batches through the oracle: the last one's winner list, then the stored rows of the sampled keys
    o = Oracle()
    try:
        o.load_rows(*synth.big_resident(bench.R_PER_GPU, seed=1, T0=bench.T0, DT=bench.DT))
        for b in range(3):
            cols = bench.gen_batch(b, bench.R_PER_GPU)
            _, win = o.merge_batch(*cols)
        assert np.array_equal(arrays["winners"], win.astype(np.float64))
        sid, sfld = bench.row_sample(cols[0], cols[1])
        assert arrays["row_sample_found"].all() and len(sid) == len(arrays["row_sample_ts"])
        for k in range(0, len(sid), 97):
            ts, val = o.get_row(int(sid[k]), int(sfld[k]))
            assert (arrays["row_sample_ts"][k], arrays["row_sample_val"][k]) == (ts, val)
    finally:
        o.close()
