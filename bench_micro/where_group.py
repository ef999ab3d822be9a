"""where_group.py — what a group-by over discovered values (include/bmx_group.h bmx_where_group) costs beside bmx_where_aggregate's window form of the same
program and data, and beside the only route a sparse group field had before: every matching id, the values fetched to the host, numpy.unique.

  python bench_micro/where_group.py [--out profiles/where_group.log] [--rows 100000000] [--reps 20] [--warmup 3] [--host-reps 3] [--limit 1100] [--no-host-route]

One table of --rows nodes (10^8; 10^7 where memory or time is short): a uniform int32 field (0 .. 2^30), three dense int32 fields of 5, 128 and 4096 distinct
values, and sparse int64 fields of 10^5 and 10^6 distinct keys over +-2^52 (a base field of those: the int64 column). In one process, HIP events on the
engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup; every answer is checked against torch / numpy over the same
columns before its time is printed.
  (a) group = base, all rows selected, measure = base (no probe anywhere), D = 5 / 128 / 4096 dense values: bmx_where_group (cap = 65536) next to bmx_where_aggregate with
      group_lo = 0, ngroups = D (G = 1 up to 1024 groups, the G = 2 slow form above). The window form is code this change does not touch: the yardstick, with
      its spread (max - min) / median.
  (b) base = the uniform field at 1 / 10 / 50 % selectivity, group = the 128-valued field (one probe behind the match), measure = base; again next to the
      window form.
  (c) group = base = a sparse int64 field, 10^5 and 10^6 distinct keys, cap = 2^20, next to the route without this call: bmx_scan_where with ids into device
      memory, the ids copied down, bmx_get_rows to the host, numpy.unique + bincount. Timed with the host's clock around the whole, --host-reps calls after one.
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_group.log.
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
CAP = 1 << 20          # (c): room for every key
CAP_DENSE = 65536       # (a), (b): the binding's default cap, as many groups as the window form can have


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
    return "median %9.1f us  min %9.1f us  max %9.1f us" % (1e3 * np.median(ms), 1e3 * ms.min(), 1e3 * ms.max())


def spread(ms):
    return (ms.max() - ms.min()) / np.median(ms)


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
    dense = (5, 128, 4096)
    sparse = (100_000, 1_000_000)
    FU = streams.fnv1a32("uniform")
    FD = {d: streams.fnv1a32("dense%d" % d) for d in dense}
    FS = {d: streams.fnv1a32("sparse%d" % d) for d in sparse}
    e = bmx.Engine((1 + len(dense) + len(sparse)) * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    col = {FU: uni}
    for k, d in enumerate(dense):
        col[FD[d]] = ((mix(ids, 0x5851F42D4C957F2D + 2 * k) >> 8) & 0xFFFFFFFF) % d
    for k, d in enumerate(sparse):
        j = ((mix(ids, 0x14057B7EF767814F + 2 * k) >> 8) & 0xFFFFFFFFFF) % d
        col[FS[d]] = ((mix(j + 1, 0x369DEA0F31A53F85) >> 11) & ((1 << 53) - 1)) - (1 << 52)                    # the key of bucket j: anywhere in +-2^52

    hid = ids.cpu().numpy().view(np.uint64)
    for f, v in col.items():          # through the host in chunks of 16M rows, as bench_micro/where_agg.py loads its table
        hv = v.cpu().numpy()
        for lo in range(0, R, 16_000_000):
            m = min(16_000_000, R - lo)
            e.load_rows(hid[lo:lo + m], np.full(m, f, np.uint32), np.full(m, 5, np.int64), hv[lo:lo + m])
    e.sync()
    for f in col:
        e.index_build(f)
        if e.index_size(f) != R:
            raise SystemExit("where_group: an index holds %d of %d rows" % (e.index_size(f), R))
    say("== %d rows (%.0f MB int32 column, %.0f MB int64 column); %d timed calls after %d warm-ups, HIP events, device outputs ==" % (R, R * 4 / 1e6, R * 8 / 1e6, a.reps, a.warmup))
    d_out = torch.zeros(7 * (CAP + 1), dtype=torch.int64, device=dev)
    d_res = torch.zeros(14, dtype=torch.int64, device=dev)
    d_agg = torch.zeros(6 * (4096 + 1), dtype=torch.int64, device=dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(R, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def answer():
        res = d_res.cpu().numpy().view(bmx.GROUP_RES_DTYPE)[0]
        assert int(res["flags"]) == 0, "overflow"
        recs = d_out.cpu().numpy().view(bmx.GROUP_DTYPE)[:int(res["n_groups"])]
        return recs[np.argsort(recs["key"])], res

    def check(sel, keys, vals, what):
        """the device's records against torch over the same columns: the key set, n_match and n of every key, min and max, the exact sum of a sample"""
        recs, res = answer()
        k, v = keys[sel], vals[sel]
        uk, inv, cnt = torch.unique(k, return_inverse=True, return_counts=True)
        assert np.array_equal(recs["key"], uk.cpu().numpy()), (what, "keys")
        assert np.array_equal(recs["agg"]["n_match"].astype(np.int64), cnt.cpu().numpy()) and np.array_equal(recs["agg"]["n"], recs["agg"]["n_match"]), (what, "counts")
        mn = torch.full_like(uk, (1 << 62)).scatter_reduce_(0, inv, v, "amin"); mx = torch.full_like(uk, -(1 << 62)).scatter_reduce_(0, inv, v, "amax")
        assert np.array_equal(recs["agg"]["min"], mn.cpu().numpy()) and np.array_equal(recs["agg"]["max"], mx.cpu().numpy()), (what, "min / max")
        lo = torch.zeros_like(uk).index_add_(0, inv, v & 0xFFFFFFFF).cpu().numpy(); hi = torch.zeros_like(uk).index_add_(0, inv, v >> 32).cpu().numpy()
        for i in np.linspace(0, len(recs) - 1, min(len(recs), 2000)).astype(np.int64):
            assert (int(recs[i]["agg"]["sum_hi"]) << 64) + int(recs[i]["agg"]["sum_lo"]) == (int(hi[i]) << 32) + int(lo[i]), (what, "sum", int(i))
        assert int(res["total"]["n_match"]) == int(sel.sum()) and int(res["absent"]["n_match"]) == 0, (what, "total")
        return len(recs)

    def check_window(sel, keys, vals, ng, what):
        r = d_agg.cpu().numpy().view(bmx.AGG_DTYPE)[:ng + 1]
        want_n = torch.bincount(keys[sel], minlength=ng).cpu().numpy()
        want_s = torch.zeros(ng, dtype=torch.int64, device=dev).index_add_(0, keys[sel], vals[sel]).cpu().numpy()
        assert np.array_equal(r["n_match"][:ng].astype(np.int64), want_n) and int(r["n_match"][ng]) == 0, (what, "window counts")
        assert np.array_equal(r["sum_lo"][:ng].astype(np.int64), want_s) and not r["sum_hi"][:ng].any(), (what, "window sums")

    everything = torch.ones(R, dtype=torch.bool, device=dev)
    say("-- (a) group = base, every row selected, measure = base --")
    for d in dense:
        f = FD[d]
        prog = [[(f, 0, d - 1)]]
        tw = timed(e, lambda: e.where_aggregate_dev(f, prog, d_agg, f, f, 0, d), a.reps, a.warmup)
        check_window(everything, col[f], col[f], d, "a window %d" % d)
        tg = timed(e, lambda: e.where_group_dev(f, prog, f, d_out, d_res, measure=f, cap=CAP_DENSE), a.reps, a.warmup)
        assert check(everything, col[f], col[f], "a %d" % d) == d
        say("D = %4d  where_aggregate window (G = %d) %s  spread %.2f" % (d, 1 if d <= 1024 else 2, fmt(tw), spread(tw)))
        say("          where_group                    %s  %.2f x the window form" % (fmt(tg), np.median(tg) / np.median(tw)))
    say("-- (b) base = uniform, group = the 128-valued field (probed), measure = base --")
    f = FD[128]
    for pct in (1, 10, 50):
        hi = ((1 << 30) * pct) // 100 - 1
        prog = [[(FU, 0, hi)]]
        sel = uni <= hi
        tw = timed(e, lambda: e.where_aggregate_dev(FU, prog, d_agg, FU, f, 0, 128), a.reps, a.warmup)
        check_window(sel, col[f], uni, 128, "b window %d" % pct)
        tg = timed(e, lambda: e.where_group_dev(FU, prog, f, d_out, d_res, measure=FU, cap=CAP_DENSE), a.reps, a.warmup)
        assert check(sel, col[f], uni, "b %d" % pct) == 128
        say("%2d %%  where_aggregate window (G = 1)    %s  spread %.2f" % (pct, fmt(tw), spread(tw)))
        say("      where_group                      %s  %.2f x the window form" % (fmt(tg), np.median(tg) / np.median(tw)))
    say("-- (c) group = base = a sparse int64 field over +-2^52, every row selected, measure = base, cap = 2^20 --")
    for d in sparse:
        f = FS[d]
        prog = [[(f, -(1 << 53), 1 << 53)]]
        tg = timed(e, lambda: e.where_group_dev(f, prog, f, d_out, d_res, measure=f, cap=CAP), a.reps, a.warmup)
        nk = check(everything, col[f], col[f], "c %d" % d)
        say("%7d keys  where_group                       %s" % (nk, fmt(tg)))
        if a.no_host_route:
            continue

        def route():
            e.scan_where_dev(f, prog, d_ids, R, d_n[0:1])
            e.sync()
            m = int(d_n[0].item())
            h = d_ids[:m].cpu().numpy().view(np.uint64)
            _, val, found = e.get_rows(h, np.full(m, f, np.uint32))
            uk, inv = np.unique(val, return_inverse=True)
            return uk, np.bincount(inv), bool(found.all())

        uk, cnt, ok = route()
        recs, _ = answer()
        assert ok and np.array_equal(uk, recs["key"]) and np.array_equal(cnt, recs["agg"]["n_match"].astype(np.int64)), "c route"
        tf = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter(); route(); tf.append(1e3 * (time.perf_counter() - t0))
        tf = np.array(tf)
        say("              scan_where ids + get_rows + unique %s  (%d calls, host clock)  where_group %.0f x faster" % (fmt(tf), a.host_reps, np.median(tf) / np.median(tg)))
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
    ap.add_argument("--no-host-route", action="store_true", help="leave the host route of (c) out")
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
        print("where_group: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
