"""replica_sync.py — what the reconciliation sweeps cost on the bench's config-2 table (22M-row capacity: ~44M slots, 1.4 GB; 10M rows + 3 x 1M deltas).

  python bench_micro/replica_sync.py [--out profiles/replica_sync.log] [--reps 20] [--warmup 3] [--skip-pull]

In one process, HIP events on the engine's stream (bmx_timer_*), every result checked before its time is printed:
  * bmx_digest at L = 10 (LDS form) and L = 13 (global form), device memory, against the launches that read exactly these bytes today: bmx_dump_rows with
    cap = 0 = k_sel_count<PredSlotAny> + k_sel_write<PredSlotAny, ...> (the second evaluates the same predicate over the same table and emits nothing), so one
    launch = half of that call; `rocprofv3 --kernel-trace --stats -- python bench_micro/replica_sync.py --skip-pull` gives the two kernels' own times.
  * the only way to the same number before: dump_rows() to the host + rows_digest (wall clock).
  * bmx_export_rows to device memory: everything, clock >= its 90th percentile, 8 of 1024 buckets.
  * replica.pull between two such engines that differ by one 1M-delta merge, beside shipping everything.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bullet-js_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bmx  # noqa: E402
from bmx import replica, synth  # noqa: E402
from oracle.oracle import Oracle, rows_digest  # noqa: E402

R, D, CAP = 10_000_000, 1_000_000, 22_000_000
T0 = DT = 1_000_000
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(e, fn, reps, warmup):
    """-> per-repetition milliseconds (HIP events around each call)"""
    for _ in range(warmup):
        fn()
    e.sync()
    ms = []
    for _ in range(reps):
        e.timer_start(); fn(); ms.append(e.timer_stop())
    return np.array(ms)


def fmt(ms):
    return "median %8.1f us  min %8.1f us  max %8.1f us" % (1e3 * np.median(ms), 1e3 * ms.min(), 1e3 * ms.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-pull", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = synth.big_resident(R, seed=1, T0=T0, DT=DT)
    bs = [synth.big_deltas(D, R, seed=2, T0=T0, DT=DT, insert_pct=10, unique=True, batch=b, drift=DT // 16) for b in range(4)]
    o = Oracle(); o.load_rows(*res)
    for b in bs[:3]:
        o.merge_batch(*b)
    want_digest, want_rows = o.digest(), len(o)

    e = bmx.Engine(CAP)
    e.load_rows(*res)
    for b in bs[:3]:
        e.merge_batch(*b, want_flags=False)
    info = e.info()
    say("table: %d slots, %.2f GB, %d rows (load %.3f); %d timed repetitions after %d warm-ups, HIP events" %
        (info.n_slots, info.table_bytes / 1e9, want_rows, want_rows / info.n_slots, a.reps, a.warmup))

    # ---- digest against the sweep that exists today ----
    d_s = torch.zeros(1 << 13, dtype=torch.int64, device=dev); d_c = torch.zeros(1 << 13, dtype=torch.int64, device=dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def dump0():
        e._chk(e.L.bmx_dump_rows(e.h, 0, None, None, None, None, bmx._ptr(d_n), bmx.MEM_DEVICE))
    t_dump0 = timed(e, dump0, a.reps, a.warmup)
    assert int(d_n.item()) == want_rows
    res_ms = {}
    for L in (10, 13):
        t = timed(e, lambda: e.digest_dev(L, d_s, d_c), a.reps, a.warmup)
        sums = d_s.cpu().numpy().view(np.uint64)[:1 << L]; counts = d_c.cpu().numpy().view(np.uint64)[:1 << L]
        assert int(sums.sum(dtype=np.uint64)) == want_digest and int(counts.sum()) == want_rows, "digest mismatch vs oracle"
        res_ms[L] = t
    sweep = np.median(t_dump0) / 2
    say("bmx_dump_rows(cap=0)  [k_sel_count<PredSlotAny> + k_sel_write, two sweeps]  %s  -> one sweep ~ %.1f us (%.2f TB/s)" %
        (fmt(t_dump0), 1e3 * sweep, info.table_bytes / (sweep * 1e-3) / 1e12))
    say("bmx_digest L=10 (LDS form)     %s  (%.2f TB/s)  ratio to one sweep: %.2f" %
        (fmt(res_ms[10]), info.table_bytes / (np.median(res_ms[10]) * 1e-3) / 1e12, np.median(res_ms[10]) / sweep))
    say("bmx_digest L=13 (global form)  %s  ratio to one sweep: %.2f" % (fmt(res_ms[13]), np.median(res_ms[13]) / sweep))

    # ---- the only way to the same number before ----
    t0 = time.perf_counter(); dump = e.dump_rows(); t1 = time.perf_counter(); dg = rows_digest(*dump); t2 = time.perf_counter()
    assert dg == want_digest
    t3 = time.perf_counter(); hs, _ = e.digest(10); t4 = time.perf_counter()
    assert int(hs.sum(dtype=np.uint64)) == want_digest
    say("dump_rows() to host %.1f ms + rows_digest %.1f ms = %.1f ms wall;  Engine.digest(10) to host %.3f ms wall" %
        (1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t2 - t0), 1e3 * (t4 - t3)))

    # ---- export to device memory ----
    id, f, ts, val = dump
    since = int(np.percentile(ts, 90))
    buckets = np.arange(8) * 128 + 3
    bits = bmx.bucket_bits_of(buckets, 10)
    d_bits = torch.from_numpy(bits.view(np.int64)).to(dev)
    d_out = torch.empty(4 * want_rows, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    cases = [("everything", dict(), want_rows),
             ("clock >= 90th percentile", dict(since=since), int((ts >= since).sum())),
             ("8 of 1024 buckets", dict(log2_buckets=10, bucket_bits=d_bits), int(np.isin(bmx.key_bucket(id, f, 10), buckets).sum()))]
    for nt in ("0", "1"):
        os.environ["BMX_SYNC_EXPORT_NT"] = nt          # A/B switch of the export predicate's loads (csrc/bmx_sync.inc); the default is 0
        for name, kw, want_n in cases:
            t = timed(e, lambda: e.export_rows_dev(d_out, want_rows, d_n, **kw), a.reps, a.warmup)
            assert int(d_n.item()) == want_n, (name, int(d_n.item()), want_n)
            say("bmx_export_rows %-26s %9d records  %s  [%s loads]" % (name, want_n, fmt(t), "nontemporal" if nt == "1" else "plain"))
    os.environ.pop("BMX_SYNC_EXPORT_NT")
    del d_out, dump, id, f, ts, val

    # ---- pull between two engines that differ by one merge ----
    if not a.skip_pull:
        o.merge_batch(*bs[3])
        e2 = bmx.Engine(CAP)
        e2.load_rows(*res)
        for b in bs:
            e2.merge_batch(*b, want_flags=False)
        e.sync(); e2.sync()
        t0 = time.perf_counter(); r = replica.pull(e, e2, 10); e.sync(); t1 = time.perf_counter()
        hs, hc = e.digest(10)
        assert int(hs.sum(dtype=np.uint64)) == o.digest() and int(hc.sum()) == len(o), "pull: state mismatch vs oracle"
        say("replica.pull(L=10) after one 1M-delta merge: %.2f ms wall, %d of 1024 buckets differ, %d rows shipped" %
            (1e3 * (t1 - t0), r["buckets_differing"], r["rows_shipped"]))
        # a small difference: the same pair once more, after 2000 more deltas on one side
        small = synth.big_deltas(2000, R, seed=9, T0=T0 + 4 * DT, DT=DT, insert_pct=10, unique=True)
        o.merge_batch(*small); e2.merge_batch(*small, want_flags=False)
        for L in (10, 16):
            e.sync(); e2.sync()
            t0 = time.perf_counter(); r = replica.pull(e, e2, L); e.sync(); t1 = time.perf_counter()
            say("replica.pull(L=%d) after 2000 more deltas: %.2f ms wall, %d of %d buckets differ, %d rows shipped" %
                (L, 1e3 * (t1 - t0), r["buckets_differing"], 1 << L, r["rows_shipped"]))
            hs, hc = e.digest(10)
            assert int(hs.sum(dtype=np.uint64)) == o.digest() and int(hc.sum()) == len(o), "pull: state mismatch vs oracle"
            if L == 10:                                  # the same difference again for the finer partition
                small = synth.big_deltas(2000, R, seed=10, T0=T0 + 5 * DT, DT=DT, insert_pct=10, unique=True)
                o.merge_batch(*small); e2.merge_batch(*small, want_flags=False)
        for L in (13, 16):
            e3 = bmx.Engine(CAP)
            e3.load_rows(*res)
            for b in bs[:3]:
                e3.merge_batch(*b, want_flags=False)
            e3.sync()
            t0 = time.perf_counter(); r = replica.pull(e3, e2, L); e3.sync(); t1 = time.perf_counter()
            hs, hc = e3.digest(10)
            assert int(hs.sum(dtype=np.uint64)) == o.digest() and int(hc.sum()) == len(o)
            say("replica.pull(L=%d) same pair: %.2f ms wall, %d of %d buckets differ, %d rows shipped" %
                (L, 1e3 * (t1 - t0), r["buckets_differing"], 1 << L, r["rows_shipped"]))
            e3.close()
        # shipping everything: export all of e2, merge into a fresh copy of the old state
        e3 = bmx.Engine(CAP)
        e3.load_rows(*res)
        for b in bs[:3]:
            e3.merge_batch(*b, want_flags=False)
        n2 = len(o)
        recs = torch.empty(4 * n2, dtype=torch.int64, device=dev)
        e3.sync(); torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e2.export_rows_dev(recs, n2, d_n); e2.sync()
        for off in range(0, n2, bmx.MAX_BATCH):
            e3.merge_records_dev(min(bmx.MAX_BATCH, n2 - off), recs.data_ptr() + 32 * off, bmx.INSERT_DELTA)
        e3.sync(); t1 = time.perf_counter()
        hs, _ = e3.digest(10)
        assert int(hs.sum(dtype=np.uint64)) == o.digest()
        say("shipping the full export instead (device to device, %d rows): %.2f ms wall" % (n2, 1e3 * (t1 - t0)))
        e3.close(); e2.close()
    e.close(); o.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
