"""where_quantiles.py — what exact quantiles over a boolean filter (include/bmx_quant.h bmx_where_quantiles) cost beside the calls around them and beside the only
route there was before: every matching id, the measure fetched to the host, numpy.partition.

  python bench_micro/where_quantiles.py [--out profiles/where_quantiles.log] [--rows 100000000] [--reps 20] [--warmup 3] [--host-reps 3] [--limit 1100] [--no-host-route]

One table of --rows nodes (10^8; 10^7 where memory or time is short): a uniform int32 base field (0 .. 2^30: 30 bits of span, three digit passes) and an int64
measure over +-2^40 (41 bits: four digit passes over the 8-byte value scratch). In one process, HIP events on the engine's stream (bmx_timer_*), device outputs,
the median of --reps timed calls after --warmup; every answer is checked against torch over the same columns before its time is printed. At 1 / 10 / 50 %
selectivity of the base field the call is timed in four forms — the median alone (nq = 1) and 8 quantiles, each with measure = base and with the probed
measure — next to
  (a) the ungrouped bmx_where_aggregate of the same program and measure: one sweep with the same probes, a floor for pass 0;
  (b) bmx_where_top with k = 1 of the same program;
  (c) the route without this call: bmx_scan_where with ids into device memory, the ids copied down, bmx_get_rows of the measure to the host,
      numpy.partition at the eight ranks. Timed with the host's clock around the whole, --host-reps calls after one.
The expectation this tests (it asserts none of it): cost ~ (a) + digit passes x one sweep of mask + value column; nq = 8 costs little over nq = 1.
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_quantiles.log.
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bullet-js_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LINES = []
ONE = [(1, 2)]
EIGHT = [(1, 100), (1, 4), (1, 2), (3, 4), (9, 10), (95, 100), (99, 100), (999, 1000)]
CHUNK = 1 << 23          # rows per load call


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
    return "median %9.1f us  min %9.1f us  max %9.1f us  spread %.2f" % (1e3 * np.median(ms), 1e3 * ms.min(), 1e3 * ms.max(), (ms.max() - ms.min()) / np.median(ms))


def mix(x, k):
    """a cheap 64-bit mix on the device (torch int64 arithmetic wraps)"""
    x = x * k
    x = x ^ ((x >> 29) & 0x7FFFFFFFF)
    x = x * -0x61c8864680b583eb
    return x ^ ((x >> 32) & 0xFFFFFFFF)


def measure(a):
    import torch
    import bmx
    from oracle import streams

    R = a.rows
    dev = torch.device("cuda", 0)
    FU, FM = streams.fnv1a32("uniform"), streams.fnv1a32("measure")
    e = bmx.Engine(2 * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    mea = ((mix(ids, 0x5851F42D4C957F2D) >> 11) & ((1 << 41) - 1)) - (1 << 40)
    ts = torch.full((CHUNK,), 5, dtype=torch.int64, device=dev)
    for f, v in ((FU, uni), (FM, mea)):
        fld = torch.full((CHUNK,), f - (1 << 32) if f >= 1 << 31 else f, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)          # the engine loads on a stream of its own: torch's fills are done before it reads them, and nothing is freed under it
        for lo in range(0, R, CHUNK):
            m = min(CHUNK, R - lo)
            e.load_rows_dev(m, ids[lo:lo + m], fld[:m], ts[:m], v[lo:lo + m])
        e.sync()
    e.index_build(FU)
    if e.index_size(FU) != R:
        raise SystemExit("where_quantiles: the index holds %d of %d rows" % (e.index_size(FU), R))
    say("== %d rows (%.0f MB int32 base column, %.0f MB value scratch of a probed measure); %d timed calls after %d warm-ups, HIP events, device outputs ==" %
        (R, R * 4 / 1e6, R * 8 / 1e6, a.reps, a.warmup))
    d_out = torch.zeros(4 * 8, dtype=torch.int64, device=dev)
    d_res = torch.zeros(4, dtype=torch.int64, device=dev)
    d_agg = torch.zeros(6, dtype=torch.int64, device=dev)
    d_top = torch.zeros(2, dtype=torch.int64, device=dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(R, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def check(sample, qs, what):
        """the device's records against torch over the same column"""
        recs = d_out.cpu().numpy().view(bmx.QUANT_REC_DTYPE)[:len(qs)]
        res = d_res.cpu().numpy().view(bmx.QUANT_RES_DTYPE)[0]
        s = torch.sort(sample).values
        n = len(s)
        assert int(res["n"]) == n == int(res["n_match"]) and int(res["min"]) == int(s[0]) and int(res["max"]) == int(s[-1]), (what, "res")
        for r, (num, den) in zip(recs, qs):
            k = bmx.quant_rank(num, den, n)
            v = int(s[k])
            lo = int(torch.searchsorted(s, torch.tensor([v], device=dev), right=False)); hi = int(torch.searchsorted(s, torch.tensor([v], device=dev), right=True))
            assert (int(r["value"]), int(r["rank"]), int(r["n_below"]), int(r["n_equal"])) == (v, k, lo, hi - lo), (what, num, den)

    for pct in (1, 10, 50):
        hi = ((1 << 30) * pct) // 100 - 1
        prog = [[(FU, 0, hi)]]
        sel = uni <= hi
        say("-- %d %% of the base field selected (%d rows) --" % (pct, int(sel.sum())))
        t = {}
        for name, field, col in (("base", FU, uni), ("probed", FM, mea)):
            sample = col[sel]
            for qs in (ONE, EIGHT):
                t[name, len(qs)] = timed(e, lambda: e.where_quantiles_dev(FU, prog, field, qs, d_out, d_res), a.reps, a.warmup)
                check(sample, qs, "%d %% %s nq %d" % (pct, name, len(qs)))
            t[name, "agg"] = timed(e, lambda: e.where_aggregate_dev(FU, prog, d_agg, field), a.reps, a.warmup)
            agg = d_agg.cpu().numpy().view(bmx.AGG_DTYPE)[0]
            assert int(agg["n"]) == len(sample) and int(agg["min"]) == int(sample.min()) and int(agg["max"]) == int(sample.max()), "aggregate"
        t["top"] = timed(e, lambda: e.where_top_dev(FU, prog, 1, d_top, d_n[0:1]), a.reps, a.warmup)
        assert int(d_top[1].item()) == int(uni[sel].min()), "top"
        for name in ("base", "probed"):
            say("measure = %-6s  (a) where_aggregate          %s" % (name, fmt(t[name, "agg"])))
            for nq in (1, 8):
                say("                  where_quantiles nq = %d     %s  %.2f x (a)" % (nq, fmt(t[name, nq]), np.median(t[name, nq]) / np.median(t[name, "agg"])))
            say("                  nq = 8 over nq = 1: %.2f x; (quantiles nq = 1 - (a)) / digit passes (%d): %.1f us per pass" %
                (np.median(t[name, 8]) / np.median(t[name, 1]), 3 if name == "base" else 4, 1e3 * (np.median(t[name, 1]) - np.median(t[name, "agg"])) / (3 if name == "base" else 4)))
        say("                  (b) where_top k = 1          %s" % fmt(t["top"]))
        if a.no_host_route:
            continue
        for name, field, col in (("base", FU, uni), ("probed", FM, mea)):
            def route():
                e.scan_where_dev(FU, prog, d_ids, R, d_n[0:1])
                e.sync()
                m = int(d_n[0].item())
                h = d_ids[:m].cpu().numpy().view(np.uint64)
                _, val, found = e.get_rows(h, np.full(m, field, np.uint32))
                ks = sorted({bmx.quant_rank(x, y, m) for x, y in EIGHT})
                return np.partition(val, ks)[ks], bool(found.all())

            got, ok = route()
            want = torch.sort(col[sel]).values
            assert ok and [int(x) for x in got] == [int(want[k]) for k in sorted({bmx.quant_rank(x, y, len(want)) for x, y in EIGHT})], "host route"
            tf = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter(); route(); tf.append(1e3 * (time.perf_counter() - t0))
            tf = np.array(tf)
            say("measure = %-6s  (c) scan_where ids + get_rows + numpy.partition  %s  (%d calls, host clock)  where_quantiles nq = 8 is %.0f x faster" %
                (name, fmt(tf), a.host_reps, np.median(tf) / np.median(t[name, 8])))
    e.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=1100, help="seconds the measurement may take")
    ap.add_argument("--no-host-route", action="store_true", help="leave the host route (c) out")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps is 20 at least")
    if a.child:
        measure(a)
        return 0
    try:
        return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        print("where_quantiles: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
