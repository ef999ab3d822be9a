"""where_group_top.py — what the first N nodes per group (include/bmx_group_top.h bmx_where_group_top) cost beside two marks measured on entry points that were
there before it, in the same process on the same data:
  (a) bmx_where_group_first of the same program, group and order field: pass 1 and round 0 are its kernels, so per = 1 should cost about the same and per = 4 /
      16 should add 2 * per - 2 sweeps of the words per position;
  (b) the host route that existed: where_rows of the group and order fields to the host, numpy.lexsort by (group, order, id), the first `per` rows of every
      group, get_rows of their fields.

  python bench_micro/where_group_top.py [--out profiles/where_group_top.log] [--rows 100000000] [--reps 20] [--warmup 3] [--limit 1100] [--no-host-route]

One table of --rows nodes (10^8; 10^7 where memory or time is short): a base int32 field of 100 uniform values (the program `base <= pct - 1` selects pct % of
the rows), a probed int32 field of 128 values (the group field) and a probed "stamp" uniform in 0 .. 2^30 (the order field, and the one projected field). In one
process, HIP events on the engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup; every answer is checked against torch
over the same columns before its time is printed (three stable sorts: id as an unsigned number, then the stamp, then the group; the first `per` of every group).
At 1 / 10 / 50 % selectivity: per = 1, 4 and 16 ascending, per = 4 descending. The GPU work is one step, the measurement, and runs in a child process under
--limit seconds: a measurement that hangs ends the script, and nothing is started behind it. --out profiles/where_group_top.log records a run.
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
        raise SystemExit("where_group_top: the index holds %d of %d rows" % (e.index_size(FP), R))
    say("== %d rows (%.0f MB int32 base column); %d timed calls after %d warm-ups, HIP events, device outputs ==" % (R, R * 4 / 1e6, a.reps, a.warmup))
    PMAX = 16
    d_first = torch.zeros(5 * (CAP + 1), dtype=torch.int64, device=dev)
    d_fres = torch.zeros(5, dtype=torch.int64, device=dev)
    d_out = torch.zeros(4 * (CAP + 1), dtype=torch.int64, device=dev)
    d_rows = torch.zeros(2 * CAP * PMAX, dtype=torch.int64, device=dev)
    d_val = torch.zeros(CAP * PMAX, dtype=torch.int64, device=dev)
    d_res = torch.zeros(6, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    base, dense, stamp = col[FP], col[FD], col[FT]
    uid = ids ^ I64MIN                                                   # signed order of uid == unsigned order of the id

    def expect(sel, desc):
        """torch over the same columns -> (keys, counts, ids (G, PMAX), stamps (G, PMAX)): the first PMAX of every group under the order"""
        k, st, u = dense[sel], stamp[sel], uid[sel]
        o = torch.argsort(u, stable=True)
        o = o[torch.argsort((-st if desc else st)[o], stable=True)]
        o = o[torch.argsort(k[o], stable=True)]
        ks = k[o]
        uk, cnt = torch.unique_consecutive(ks, return_counts=True)
        start = torch.cumsum(cnt, 0) - cnt
        assert int(cnt.min()) >= PMAX
        at = start[:, None] + torch.arange(PMAX, device=dev)[None, :]
        return uk.cpu().numpy(), cnt.cpu().numpy(), (u[o][at] ^ I64MIN).cpu().numpy().view(np.uint64), st[o][at].cpu().numpy()

    def check(want, sel_n, per, what):
        """the device's groups, rows and cells against torch's"""
        uk, cnt, wid, wst = want
        res = d_res.cpu().numpy().view(bmx.GTOP_RES_DTYPE)[0]
        assert int(res["flags"]) == 0 and int(res["per"]) == per, (what, "overflow")
        n = int(res["n_groups"])
        grps = d_out.cpu().numpy().view(bmx.GTOP_GRP_DTYPE)[:n]
        rows = d_rows.cpu().numpy().view(bmx.GTOP_ROW_DTYPE)[:n * per].reshape(n, per)
        cells = d_val.cpu().numpy()[:n * per].reshape(n, per)
        order = np.argsort(grps["key"])
        grps, rows, cells = grps[order], rows[order], cells[order]
        assert np.array_equal(grps["key"], uk), (what, "keys")
        assert np.array_equal(grps["n_match"].astype(np.int64), cnt) and np.array_equal(grps["n"], grps["n_match"]) and (grps["n_rows"] == per).all(), (what, "counts")
        assert np.array_equal(rows["id"], wid[:, :per]) and np.array_equal(rows["val"], wst[:, :per]) and np.array_equal(cells, rows["val"]), (what, "rows and cells")
        assert int(res["total"]) == sel_n == int(res["n_ordered"]) and int(res["absent"]) == 0 and int(res["n_rows"]) == n * per, (what, "totals")
        return n

    for pct in (1, 10, 50):
        prog = [[(FP, 0, pct - 1)]]
        sel = base < pct
        sel_n = int(sel.sum())
        say("-- %2d %% selected (%d rows), group = the probed 128-valued field, order = the probed stamp, one projected field --" % (pct, sel_n))
        tf = timed(e, lambda: e.where_group_first_dev(FP, prog, FD, FT, d_first, d_val, None, d_fres, fields=(FT,), cap=CAP), a.reps, a.warmup)
        fres = d_fres.cpu().numpy().view(bmx.FIRST_RES_DTYPE)[0]
        assert int(fres["n_groups"]) == 128 and int(fres["total"]) == sel_n
        say("(a) where_group_first, ascending                 %s  spread %.2f" % (fmt(tf), spread(tf)))
        want = {desc: expect(sel, desc) for desc in (False, True)}
        t_top = {}
        for per, desc in ((1, False), (4, False), (4, True), (16, False)):
            tt = timed(e, lambda: e.where_group_top_dev(FP, prog, FD, FT, per, d_out, d_rows, d_val, None, d_res, fields=(FT,), desc=desc, cap=CAP), a.reps, a.warmup)
            assert check(want[desc], sel_n, per, "top %d %d %s" % (pct, per, desc)) == 128
            say("    where_group_top per = %2d, %s           %s  %.2f x (a)  spread %.2f" % (per, "descending" if desc else "ascending ", fmt(tt), np.median(tt) / np.median(tf), spread(tt)))
            t_top[(per, desc)] = tt
        if a.no_host_route or pct > 10:
            continue

        def route(per):
            r = e.where_rows(FP, prog, [FD, FT])
            o = np.lexsort((r.ids, r.vals[1], r.vals[0]))
            g = r.vals[0][o]
            head = np.ones(len(o), bool); head[1:] = g[1:] != g[:-1]
            start = np.nonzero(head)[0]
            rank = np.arange(len(o)) - np.repeat(start, np.diff(np.append(start, len(o))))
            w = r.ids[o][rank < per]
            return g[head], w, e.get_rows(w, np.full(len(w), FT, np.uint32))[1]

        if pct == 1:
            route(4)
        for per in (4, 16):
            t0 = time.perf_counter(); g, w, cells = route(per); th = 1e3 * (time.perf_counter() - t0)
            assert np.array_equal(g, want[False][0]) and np.array_equal(w.reshape(128, per), want[False][2][:, :per]) and np.array_equal(cells.reshape(128, per), want[False][3][:, :per]), "the host route's rows"
            say("(b) where_rows of group + order, lexsort, get_rows of the first %2d    %9.1f ms (one call, host clock)  where_group_top %.0f x faster" % (
                per, th, th / np.median(t_top[(per, False)])))
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
        print("where_group_top: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
