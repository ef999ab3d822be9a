"""vc_sync.py — what the reconciliation sweeps of the vector-clock table cost on a 10M-row K = 3 table (20M slots of 64 bytes, 1.28 GB, load 0.5).

  python bench_micro/vc_sync.py [--out profiles/vc_sync.log] [--reps 20] [--warmup 3] [--rows 10000000]

In one process, HIP events on the table's stream (a torch stream handed to bmx_vc_set_stream), medians over the repetitions, every result checked against
numpy before its time is printed:
  * the launch that reads the same table on the parent commit: the count-only bmx_vc_scan_range of a field every row carries (k_sel_count<PredVSlotRange>
    over n_slots x 64 bytes, plus its count's way to the host);
  * bmx_vc_digest at L = 10 (LDS form) and L = 13 (global form), device memory;
  * bmx_vc_frontier;
  * bmx_vc_export_rows to device memory: everything, 8 of 1024 buckets, under the table's own frontier lowered by one in one component.
The bound of every sweep is one read of n_slots x 64 bytes; the exports read the table twice (count, write) and write 64 bytes per record.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bullet-js_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bmx  # noqa: E402
from bmx import synth  # noqa: E402

K, LOCAL = 3, 0
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(stream, fn, reps, warmup):
    """-> per-repetition milliseconds (HIP events on the table's stream around each call)"""
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(); b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.array(ms)


def fmt(ms):
    return "median %8.1f us  min %8.1f us  max %8.1f us" % (1e3 * np.median(ms), 1e3 * ms.min(), 1e3 * ms.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10_000_000)
    a = ap.parse_args()
    R = a.rows
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    ids = synth.splitmix64_np(np.arange(1, R + 1, dtype=np.uint64))          # unique keys: the loaded rows are the table
    f0 = synth.field_hash(0)
    fields = np.full(R, f0, np.uint32)
    clocks = rng.integers(0, 1000, (R, K)).astype(np.uint32)
    val = rng.integers(-(1 << 20), 1 << 20, R).astype(np.int64)
    ks = np.full(R, bmx.keyset(range(K)), np.uint32)
    state = np.full(R, bmx.VC_DENSE, np.uint32)
    dig = bmx.vc_rows_digest(ids, fields, clocks, ks, state, val)
    want_frontier = np.zeros(8, np.uint32); want_frontier[:K] = clocks.max(0)

    e = bmx.EngineVC(R + 8, K, LOCAL)                                        # (+ 8: the last chunk of the load must not trigger a growth)
    e.load_rows(ids, fields, clocks, val)
    stream = torch.cuda.Stream(device=dev)
    e.set_stream(stream.cuda_stream)
    info = e.info()
    assert info.n_rows == R
    say("table: %d slots, %.2f GB, %d rows (load %.3f), K = %d; %d timed repetitions after %d warm-ups, HIP events, medians" %
        (info.n_slots, info.table_bytes / 1e9, R, R / info.n_slots, K, a.reps, a.warmup))

    def tbs(ms, reads=1):
        return reads * info.table_bytes / (np.median(ms) * 1e-3) / 1e12

    # ---- the parent commit's sweep of the same table ----
    got = {}

    def scan():
        got["n"] = e.scan_range(f0, -(1 << 53), 1 << 53, count_only=True)
    t_scan = timed(stream, scan, a.reps, a.warmup)
    assert got["n"] == R
    scan_med = np.median(t_scan)
    say("bmx_vc_scan_range count-only (parent's sweep)  %s  (%.2f TB/s)" % (fmt(t_scan), tbs(t_scan)))

    # ---- digest ----
    d_s = torch.zeros(1 << 13, dtype=torch.int64, device=dev); d_c = torch.zeros(1 << 13, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    for L, form in ((10, "LDS form"), (13, "global form")):
        t = timed(stream, lambda: e.digest_dev(L, d_s, d_c), a.reps, a.warmup)
        sums = d_s.cpu().numpy().view(np.uint64)[:1 << L]; counts = d_c.cpu().numpy().view(np.uint64)[:1 << L]
        bk = bmx.key_bucket(ids, fields, L).astype(np.int64)
        ws = np.zeros(1 << L, np.uint64); wc = np.bincount(bk, minlength=1 << L).astype(np.uint64)
        with np.errstate(over="ignore"):
            np.add.at(ws, bk, dig)
        assert np.array_equal(sums, ws) and np.array_equal(counts, wc), "digest mismatch vs numpy"
        say("bmx_vc_digest L=%d (%s)  %s  (%.2f TB/s)  ratio to the parent's sweep: %.2f" % (L, form, fmt(t), tbs(t), np.median(t) / scan_med))

    # ---- frontier ----
    d_f = torch.zeros(8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    t = timed(stream, lambda: e.frontier_dev(d_f), a.reps, a.warmup)
    assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_frontier), "frontier mismatch vs numpy"
    say("bmx_vc_frontier  %s  (%.2f TB/s)  ratio to the parent's sweep: %.2f" % (fmt(t), tbs(t), np.median(t) / scan_med))

    # ---- exports to device memory ----
    buckets = np.arange(8) * 128 + 3
    bits = bmx.bucket_bits_of(buckets, 10)
    d_bits = torch.from_numpy(bits.view(np.int64)).to(dev)
    d_out = torch.empty(8 * R, dtype=torch.int64, device=dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    low = want_frontier.copy(); low[1] -= 1
    in_b = np.isin(bmx.key_bucket(ids, fields, 10), buckets)
    ahead = (clocks > low[:K]).any(1)
    torch.cuda.synchronize(dev)
    cases = [("everything", dict(), np.ones(R, bool)),
             ("8 of 1024 buckets", dict(log2_buckets=10, bucket_bits=d_bits), in_b),
             ("frontier lowered by one", dict(frontier=low), ahead)]
    for name, kw, m in cases:
        t = timed(stream, lambda: e.export_rows_dev(d_out, R, d_n, **kw), a.reps, a.warmup)
        n = int(d_n.item())
        assert n == int(m.sum()), (name, n, int(m.sum()))
        recs = d_out[:8 * n].cpu().numpy().view(bmx.VC_REC_DTYPE)
        got_d = bmx.vc_rows_digest(recs["id"], recs["field"], recs["clock"], recs["keyset"], recs["state"], recs["val"], summed=True)
        assert got_d == int(dig[m].sum(dtype=np.uint64)) and not recs["aux"].any(), (name, "records mismatch vs numpy")
        say("bmx_vc_export_rows %-24s %9d records  %s  (%.2f TB/s read over two sweeps)  ratio to the parent's sweep: %.2f" %
            (name, n, fmt(t), tbs(t, 2), np.median(t) / scan_med))
    e.set_stream(0)
    e.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
