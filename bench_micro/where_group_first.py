"""where_group_first.py — what the first node per group (include/bmx_first.h bmx_where_group_first) costs beside two marks measured on entry points that were
there before it, in the same process on the same data:
  (a) bmx_where_group of the same program by the same group field with measure = the order field: it does pass 1's work (the sweep, the probes, the hash
      aggregation with both extremes) and nothing else;
  (b) the host route that existed: where_rows of the group and order fields to the host, numpy.lexsort by (group, order, id), the first row of every group,
      get_rows of the winners' fields.

  python bench_micro/where_group_first.py [--out profiles/where_group_first.log] [--rows 100000000] [--reps 20] [--warmup 3] [--limit 1100] [--no-host-route]

One table of --rows nodes (10^8; 10^7 where memory or time is short): a base int32 field of 100 uniform values (the program `base <= pct - 1` selects pct % of
the rows), a probed int32 field of 128 values (the group field) and a probed "stamp" uniform in 0 .. 2^30 (the order field, and the one projected field). In one
process, HIP events on the engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup; every answer is checked against torch
over the same columns before its time is printed (the minimum stamp per group, then the smallest id, as an unsigned number, among the rows that hold it). At
1 / 10 / 50 % selectivity: group = the probed field (two words of scratch per position), ascending and descending, and group = the base field (one word).
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. --out profiles/where_group_first.log records a run.
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
CAP = 65536             # the binding's default cap
I64MIN = -(1 << 63)


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
        raise SystemExit("where_group_first: the index holds %d of %d rows" % (e.index_size(FP), R))
    say("== %d rows (%.0f MB int32 base column); %d timed calls after %d warm-ups, HIP events, device outputs ==" % (R, R * 4 / 1e6, a.reps, a.warmup))
    d_grp = torch.zeros(7 * (CAP + 1), dtype=torch.int64, device=dev)
    d_gres = torch.zeros(14, dtype=torch.int64, device=dev)
    d_out = torch.zeros(5 * (CAP + 1), dtype=torch.int64, device=dev)
    d_val = torch.zeros(CAP, dtype=torch.int64, device=dev)
    d_res = torch.zeros(5, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    base, dense, stamp = col[FP], col[FD], col[FT]
    uid = ids ^ I64MIN                                                   # signed order of uid == unsigned order of the id

    def check(sel, key, desc, what):
        """the device's records and cells against torch over the same columns"""
        res = d_res.cpu().numpy().view(bmx.FIRST_RES_DTYPE)[0]
        assert int(res["flags"]) == 0, (what, "overflow")
        n = int(res["n_groups"])
        recs = d_out.cpu().numpy().view(bmx.FIRST_DTYPE)[:n]
        cells = d_val.cpu().numpy()[:n]
        order = np.argsort(recs["key"])
        recs, cells = recs[order], cells[order]
        uk, inv, cnt = torch.unique(key[sel], return_inverse=True, return_counts=True)
        st, u = stamp[sel], uid[sel]
        ext = torch.full_like(uk, -1 if desc else 1 << 40).scatter_reduce_(0, inv, st, "amax" if desc else "amin")
        tie = st == ext[inv]
        win = torch.full_like(uk, (1 << 63) - 1).scatter_reduce_(0, inv[tie], u[tie], "amin") ^ I64MIN
        assert np.array_equal(recs["key"], uk.cpu().numpy()), (what, "keys")
        assert np.array_equal(recs["n_match"].astype(np.int64), cnt.cpu().numpy()) and np.array_equal(recs["n"], recs["n_match"]), (what, "counts")
        assert np.array_equal(recs["val"], ext.cpu().numpy()) and np.array_equal(cells, recs["val"]), (what, "extremes and cells")
        assert np.array_equal(recs["id"], win.cpu().numpy().view(np.uint64)), (what, "winners")
        assert int(res["total"]) == int(sel.sum()) == int(res["n_ordered"]) and int(res["absent"]) == 0, (what, "totals")
        return n

    for pct in (1, 10, 50):
        prog = [[(FP, 0, pct - 1)]]
        sel = base < pct
        say("-- %2d %% selected (%d rows), order = the probed stamp, one projected field --" % (pct, int(sel.sum())))
        tg = timed(e, lambda: e.where_group_dev(FP, prog, FD, d_grp, d_gres, measure=FT, cap=CAP), a.reps, a.warmup)
        gres = d_gres.cpu().numpy().view(bmx.GROUP_RES_DTYPE)[0]
        assert int(gres["n_groups"]) == 128 and int(gres["total"]["n_match"]) == int(sel.sum())
        say("(a) where_group by the probed 128-valued field, measure = stamp   %s  spread %.2f" % (fmt(tg), spread(tg)))
        for desc in (False, True):
            tf = timed(e, lambda: e.where_group_first_dev(FP, prog, FD, FT, d_out, d_val, None, d_res, fields=(FT,), desc=desc, cap=CAP), a.reps, a.warmup)
            assert check(sel, dense, desc, "first %d %s" % (pct, desc)) == 128
            say("    where_group_first by the same field, %s           %s  %.2f x (a)" % ("descending" if desc else "ascending ", fmt(tf), np.median(tf) / np.median(tg)))
            if not desc:
                t_first = tf
        tb = timed(e, lambda: e.where_group_dev(FP, prog, FP, d_grp, d_gres, measure=FT, cap=CAP), a.reps, a.warmup)
        say("(a) where_group by the base field, measure = stamp                %s  spread %.2f" % (fmt(tb), spread(tb)))
        tf = timed(e, lambda: e.where_group_first_dev(FP, prog, FP, FT, d_out, d_val, None, d_res, fields=(FT,), cap=CAP), a.reps, a.warmup)
        assert check(sel, base, False, "first base %d" % pct) == pct
        say("    where_group_first by the base field, ascending               %s  %.2f x (a)" % (fmt(tf), np.median(tf) / np.median(tb)))
        if a.no_host_route or pct > 10:
            continue

        def route():
            r = e.where_rows(FP, prog, [FD, FT])
            o = np.lexsort((r.ids, r.vals[1], r.vals[0]))
            g = r.vals[0][o]
            head = np.ones(len(o), bool); head[1:] = g[1:] != g[:-1]
            w = r.ids[o][head]
            return g[head], w, e.get_rows(w, np.full(len(w), FT, np.uint32))[1]

        if pct == 1:
            route()
        t0 = time.perf_counter(); g, w, cells = route(); th = 1e3 * (time.perf_counter() - t0)
        e.where_group_first_dev(FP, prog, FD, FT, d_out, d_val, None, d_res, fields=(FT,), cap=CAP); e.sync()
        recs = np.sort(d_out.cpu().numpy().view(bmx.FIRST_DTYPE)[:128], order="key")
        assert np.array_equal(g, recs["key"]) and np.array_equal(w, recs["id"]) and np.array_equal(cells, recs["val"]), "the host route's winners"
        say("(b) where_rows of group + order, lexsort, get_rows of the winners  %9.1f ms (one call, host clock)  where_group_first %.0f x faster" % (th, th / np.median(t_first)))
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
    ap.add_argument("--no-host-route", action="store_true", help="leave the host route (b) out")
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
        print("where_group_first: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
