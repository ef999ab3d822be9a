"""scan_aggregate.py — what an aggregate query costs beside the scan that reads the same bytes (include/bmx.h "aggregate queries").

  python bench_micro/scan_aggregate.py [--out profiles/scan_aggregate.log] [--reps 20] [--warmup 3] [--rows 100000000,10000000]

The config-3 index: R rows of an int32 `age`-like field (values 0..99), built on the device. In one process, HIP events on the engine's stream
(bmx_timer_*), device outputs, the median of the timed calls, every answer checked against torch's integer arithmetic over the same columns before its time
is printed:
  (a) bmx_scan_count over 10 % and 50 % of the values: the existing one-read-of-the-column pass, the yardstick
  (b) the single-field aggregate (count, sum, min, max of the same field) over the same ranges
  (c) "count by value": the single-field aggregate with 128 groups
  (d) a two-term aggregate whose measure is a third field, 1 % and 10 % of the rows passing term 0 (up to --probe-rows rows: the two other fields are
      loaded on that many nodes of the table)
  (e) (d) with the value-ordered view of term 0's index on
  (f) what a caller did before for (b): scan_range + get_rows to the host + a numpy sum, wall clock
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
from oracle import streams  # noqa: E402

FA, FB, FC = streams.fnv1a32("age"), streams.fnv1a32("score"), streams.fnv1a32("stock")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(e, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    e.sync()
    ms = []
    for _ in range(reps):
        e.timer_start(); fn(); ms.append(e.timer_stop())
    return np.array(ms)


def fmt(ms):
    return "median %8.1f us  min %8.1f us  max %8.1f us" % (1e3 * np.median(ms), 1e3 * ms.min(), 1e3 * ms.max())


def mix(x, k):
    """a cheap 64-bit mix on the device (torch int64 arithmetic wraps)"""
    x = x * k
    x = x ^ ((x >> 29) & 0x7FFFFFFFF)
    x = x * -0x61c8864680b583eb
    return x ^ ((x >> 32) & 0xFFFFFFFF)


def recs_of(buf, ngroups):
    return bmx.agg_results(buf.cpu().numpy()[:(ngroups + 1) * 6].view(bmx.AGG_DTYPE), ngroups)


def run(R, probe_rows, a):
    dev = torch.device("cuda", 0)
    P = min(R, probe_rows)
    e = bmx.Engine(R + 2 * P + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    age = (mix(ids, 0x2545F4914F6CDD1D) >> 8) % 100
    age = torch.where(age < 0, age + 100, age)
    score = (mix(ids[:P], 0x5851F42D4C957F2D) >> 8) % 2001 - 1000
    stock = (mix(ids[:P], 0x14057B7EF767814F) >> 8) % 100001
    ts = torch.full((R,), 5, dtype=torch.int64, device=dev)
    for f, n, v in ((FA, R, age), (FB, P, score), (FC, P, stock)):
        e.load_rows_dev(n, ids, torch.full((n,), f - (1 << 32) if f >= (1 << 31) else f, dtype=torch.int32, device=dev), ts, v.contiguous())
    e.sync()
    e.index_build(FA)
    assert e.index_size(FA) == R
    say("")
    say("== %d rows, int32 column (%.0f MB); two more fields on %d nodes; %d timed calls after %d warm-ups, HIP events, device outputs ==" %
        (R, R * 4 / 1e6, P, a.reps, a.warmup))
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_one = torch.zeros(6, dtype=torch.int64, device=dev)
    d_grp = torch.zeros(129 * 6, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    base = {}
    for name, lo, hi in (("10 %", 20, 29), ("50 %", 0, 49)):
        sel = (age >= lo) & (age <= hi)
        want = (int(sel.sum()), int(age[sel].sum()), int(age[sel].min()), int(age[sel].max()))
        ta = timed(e, lambda: e._chk(e.L.bmx_scan_count(e.h, FA, lo, hi, bmx._ptr(d_n), bmx.MEM_DEVICE)), a.reps, a.warmup)
        assert int(d_n.item()) == want[0]
        tb = timed(e, lambda: e.scan_aggregate_dev([(FA, lo, hi)], d_one, measure=FA), a.reps, a.warmup)
        r = recs_of(d_one, 0)
        assert (r.n_match, r.sum, r.min, r.max) == want and r.n == want[0], (r, want)
        base[name] = np.median(ta)
        say("(a) scan_count            %-5s %s  (%.2f TB/s)" % (name, fmt(ta), R * 4 / (np.median(ta) * 1e-3) / 1e12))
        say("(b) aggregate, one field  %-5s %s  ratio to (a): %.2f" % (name, fmt(tb), np.median(tb) / np.median(ta)))
    tc = timed(e, lambda: e.scan_aggregate_dev([(FA, 0, 99)], d_grp, group=FA, group_lo=0, ngroups=128), a.reps, a.warmup)
    g = recs_of(d_grp, 128)
    want_hist = torch.bincount(age, minlength=129).cpu().numpy()
    assert [x.n_match for x in g] == want_hist.tolist()
    tall = timed(e, lambda: e._chk(e.L.bmx_scan_count(e.h, FA, 0, 99, bmx._ptr(d_n), bmx.MEM_DEVICE)), a.reps, a.warmup)
    say("(c) count by value, 128 groups, every row   %s  ratio to scan_count over every row (%.1f us): %.2f; to (a) 50 %%: %.2f" %
        (fmt(tc), 1e3 * np.median(tall), np.median(tc) / np.median(tall), np.median(tc) / base["50 %"]))
    # (d), (e): two terms + a third field as the measure
    have = torch.zeros(R, dtype=torch.bool, device=dev); have[:P] = True
    sc = torch.zeros(R, dtype=torch.int64, device=dev); sc[:P] = score
    st = torch.zeros(R, dtype=torch.int64, device=dev); st[:P] = stock
    for view in (0, 1):
        e.index_set_ordered(FA, view)
        for name, lo, hi in (("1 %", 42, 42), ("10 %", 20, 29)):
            terms = [(FA, lo, hi), (FB, -500, 500)]
            sel = (age >= lo) & (age <= hi) & have & (sc >= -500) & (sc <= 500)
            want = (int(sel.sum()), int(st[sel].sum()))
            td = timed(e, lambda: e.scan_aggregate_dev(terms, d_one, measure=FC), a.reps, a.warmup)
            r = recs_of(d_one, 0)
            assert (r.n_match, r.sum) == want and r.n == want[0], (r, want)
            say("(%s) two terms + a third field, %-4s of the rows pass term 0, view %s  %s  (%d nodes aggregated)" %
                ("e" if view else "d", name, "on " if view else "off", fmt(td), want[0]))
    e.index_set_ordered(FA, 0)
    # (f) what a caller did before for (b)
    for name, lo, hi in (("10 %", 20, 29),):
        e.sync()
        t0 = time.perf_counter()
        got = e.scan_range(FA, lo, hi)
        _, val, found = e.get_rows(got, np.full(len(got), FA, np.uint32))
        s = int(val.sum()); t1 = time.perf_counter()
        sel = (age >= lo) & (age <= hi)
        assert s == int(age[sel].sum()) and bool(found.all())
        say("(f) scan_range + get_rows to the host + numpy sum, %s: %.1f ms wall (%d ids)" % (name, 1e3 * (t1 - t0), len(got)))
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="100000000,10000000")
    ap.add_argument("--probe-rows", type=int, default=10_000_000)
    a = ap.parse_args()
    for R in [int(x) for x in a.rows.split(",")]:
        run(R, a.probe_rows, a)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
