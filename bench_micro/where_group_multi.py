"""where_group_multi.py — what a group-by over several fields (include/bmx_group_multi.h bmx_where_group_multi) costs beside bmx_where_group of the same
program and data, and beside the only route a tuple of keys had before: where_rows of the key fields to the host, numpy.unique(axis=0).

  python bench_micro/where_group_multi.py [--out profiles/where_group_multi.log] [--rows 100000000] [--reps 20] [--warmup 3] [--limit 1100] [--no-host-route]

One table of --rows nodes (10^8; 10^7 where memory or time is short): a base int32 field of 100 uniform values (the program `base <= pct - 1` selects pct % of
the rows, and the field can be a key), a probed int32 field of 128 values and a probed "stamp" uniform in 0 .. 2^30. In one process, HIP events on the engine's
stream (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup; every answer is checked against torch over the same columns before its
time is printed. At 1 / 10 / 50 % selectivity, measure = base:
  (a) K = 1, the identity key on the probed 128-valued field, next to bmx_where_group by that field: the same program in the same process. bmx_where_group is
      code this change does not touch: the yardstick, with its spread (max - min) / median.
  (b) K = 2, keys = the base field and the probed 128-valued field (pct x 128 tuples), next to bmx_where_group by the probed field alone: a mark with one key
      fewer, not a floor.
  (c) K = 3, keys = base, the 128-valued field and the stamp bucketed into 100 buckets (pct x 12800 tuples: 1.3 * 10^4, 1.3 * 10^5, 6.4 * 10^5), cap = 2^20,
      next to the route that existed (1 and 10 %): where_rows of the key fields to the host, then numpy.unique(axis=0) with counts; the host's clock around
      one call (at 1 % after one warm-up call).
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_group_multi.log.
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
CAP = 1 << 20           # (c): room for every tuple
CAP_DENSE = 65536       # (a), (b): the binding's default cap
NB = 100                # (c): buckets of the stamp
WIDTH = (1 << 30) // NB + 1


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
    FP, FD, FT = streams.fnv1a32("pct100"), streams.fnv1a32("dense128"), streams.fnv1a32("stamp")
    e = bmx.Engine(3 * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    col = {FP: ((mix(ids, 0x2545F4914F6CDD1D) >> 8) & 0xFFFFFFFF) % 100,
           FD: ((mix(ids, 0x5851F42D4C957F2D) >> 8) & 0xFFFFFFFF) % 128,
           FT: (mix(ids, 0x14057B7EF767814F) >> 8) & ((1 << 30) - 1)}
    hid = ids.cpu().numpy().view(np.uint64)
    for f, v in col.items():          # through the host in chunks of 16M rows, as bench_micro/where_group.py loads its table
        hv = v.cpu().numpy()
        for lo in range(0, R, 16_000_000):
            m = min(16_000_000, R - lo)
            e.load_rows(hid[lo:lo + m], np.full(m, f, np.uint32), np.full(m, 5, np.int64), hv[lo:lo + m])
    e.sync()
    e.index_build(FP)
    if e.index_size(FP) != R:
        raise SystemExit("where_group_multi: the index holds %d of %d rows" % (e.index_size(FP), R))
    say("== %d rows (%.0f MB int32 base column); %d timed calls after %d warm-ups, HIP events, device outputs ==" % (R, R * 4 / 1e6, a.reps, a.warmup))
    d_out = torch.zeros(10 * (CAP + 1), dtype=torch.int64, device=dev)
    d_out1 = torch.zeros(7 * (CAP_DENSE + 1), dtype=torch.int64, device=dev)
    d_res = torch.zeros(14, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    base, dense, bucket = col[FP], col[FD], col[FT] // WIDTH

    def check(sel, packed, what, single=False):
        """the device's records against torch over the same columns: the tuple set (packed into one word), n_match and n of every tuple, the exact sum"""
        res = d_res.cpu().numpy().view(bmx.GROUP_RES_DTYPE)[0]
        assert int(res["flags"]) == 0, (what, "overflow")
        n = int(res["n_groups"])
        if single:
            recs = d_out1.cpu().numpy().view(bmx.GROUP_DTYPE)[:n]
            got = recs["key"]
        else:
            recs = d_out.cpu().numpy().view(bmx.MGROUP_DTYPE)[:n]
            k = recs["key"]
            got = (k[:, 0] * 128 + k[:, 1]) * NB + k[:, 2] if what[0] == "c" else (k[:, 0] * 128 + k[:, 1] if what[0] == "b" else k[:, 0])
            assert (k[:, 3] == 0).all() and (what[0] == "c" or (k[:, 2] == 0).all())
        order = np.argsort(got)
        recs, got = recs[order], got[order]
        uk, inv, cnt = torch.unique(packed[sel], return_inverse=True, return_counts=True)
        assert np.array_equal(got, uk.cpu().numpy()), (what, "tuples")
        assert np.array_equal(recs["agg"]["n_match"].astype(np.int64), cnt.cpu().numpy()) and np.array_equal(recs["agg"]["n"], recs["agg"]["n_match"]), (what, "counts")
        s = torch.zeros_like(uk).index_add_(0, inv, base[sel]).cpu().numpy()
        assert np.array_equal(recs["agg"]["sum_lo"].astype(np.int64), s) and not recs["agg"]["sum_hi"].any(), (what, "sums")
        assert int(res["total"]["n_match"]) == int(sel.sum()) and int(res["absent"]["n_match"]) == 0, (what, "total")
        return n

    for pct in (1, 10, 50):
        prog = [[(FP, 0, pct - 1)]]
        sel = base < pct
        say("-- %2d %% selected (%d rows), measure = base --" % (pct, int(sel.sum())))
        tg = timed(e, lambda: e.where_group_dev(FP, prog, FD, d_out1, d_res, measure=FP, cap=CAP_DENSE), a.reps, a.warmup)
        assert check(sel, dense, "a group %d" % pct, single=True) == 128
        say("    where_group by the probed 128-valued field          %s  spread %.2f" % (fmt(tg), spread(tg)))
        t1 = timed(e, lambda: e.where_group_multi_dev(FP, prog, [FD], d_out, d_res, measure=FP, cap=CAP_DENSE), a.reps, a.warmup)
        assert check(sel, dense, "a %d" % pct) == 128
        say("(a) K = 1, the same field                               %s  %.2f x where_group" % (fmt(t1), np.median(t1) / np.median(tg)))
        t2 = timed(e, lambda: e.where_group_multi_dev(FP, prog, [FP, FD], d_out, d_res, measure=FP, cap=CAP_DENSE), a.reps, a.warmup)
        n2 = check(sel, base * 128 + dense, "b %d" % pct)
        say("(b) K = 2, base and the probed field, %6d tuples      %s  %.2f x where_group" % (n2, fmt(t2), np.median(t2) / np.median(tg)))
        keys3 = [FP, FD, (FT, 0, WIDTH)]
        t3 = timed(e, lambda: e.where_group_multi_dev(FP, prog, keys3, d_out, d_res, measure=FP, cap=CAP), a.reps, a.warmup)
        n3 = check(sel, (base * 128 + dense) * NB + bucket, "c %d" % pct)
        say("(c) K = 3, and the stamp in %d buckets, %7d tuples  %s  %.2f x where_group" % (NB, n3, fmt(t3), np.median(t3) / np.median(tg)))
        if a.no_host_route or pct > 10:
            continue

        def route():
            r = e.where_rows(FP, prog, [FP, FD, FT])
            v = r.vals.T.copy()
            v[:, 2] //= WIDTH
            return np.unique(v, axis=0, return_counts=True)

        if pct == 1:
            route()
        t0 = time.perf_counter(); ut, cnt = route(); tf = 1e3 * (time.perf_counter() - t0)
        recs = bmx.mgroup_sort(d_out.cpu().numpy().view(bmx.MGROUP_DTYPE)[:n3])
        assert np.array_equal(ut, recs["key"][:, :3]) and np.array_equal(cnt, recs["agg"]["n_match"].astype(np.int64)), "c route"
        say("    where_rows of the key fields + numpy.unique(axis=0) %9.1f ms (one call, host clock)  where_group_multi %.0f x faster" % (tf, tf / np.median(t3)))
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
        print("where_group_multi: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
