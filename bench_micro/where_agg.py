"""where_agg.py — what an aggregate or a top-k over a boolean filter (include/bmx_where_agg.h) costs beside the count-only sweep of the same program and beside
the only route such a program had before: every matching id, their values fetched to the host, numpy.

  python bench_micro/where_agg.py [--out profiles/where_agg.log] [--rows 100000000] [--reps 20] [--warmup 3] [--host-reps 20] [--limit 1100]
                                  [--program N] [--no-host-route]

One index of --rows int32 rows (10^8; 10^7 where memory is short): a uniform base field (0 .. 2^30), a 128-valued "code" on every node, a 4-valued "role" on
three quarters of the nodes. In one process, HIP events on the engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup;
every answer is checked against torch / numpy over the same columns before its time is printed. Per program:
  (a) bmx_scan_where, count only                      — code this change does not touch: the yardstick
  (b) bmx_where_aggregate, ungrouped, measure = the base field (no probe behind the match)
  (c) ... measure = "code", a probed field
  (d) ... 128 groups by "code", measure = the base field
  (e) bmx_where_top, k = 100
  (f) the route without these calls: bmx_scan_where with ids into device memory, the ids copied down, bmx_get_rows of the base field to the host, numpy's
      sum / min / max. Timed with the host's clock around the whole (it ends in synchronous copies), --host-reps calls after one warm-up.
Programs: a one-clause two-literal AND at 1 %, 10 % and 50 % selectivity of its base literal, Example 8's shape (two positive literals and one negated probed
literal), a two-clause OR. --program N (0..4) runs one of them and --no-host-route leaves (f) out: what a kernel trace wants
(rocprofv3 --kernel-trace --stats -- python bench_micro/where_agg.py --child --program 1 --no-host-route; the averages then belong to one program).
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_agg.log.
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
K = 100
NG = 128


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

    FU, FC, FR = streams.fnv1a32("uniform"), streams.fnv1a32("code"), streams.fnv1a32("role")
    R = a.rows
    dev = torch.device("cuda", 0)
    e = bmx.Engine(3 * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    code = (mix(ids, 0x5851F42D4C957F2D) >> 8) & 127
    role = (mix(ids, 0x14057B7EF767814F) >> 8) & 3
    has_role = ((mix(ids, 0x369DEA0F31A53F85) >> 8) & 3) != 0

    def load(f, i, v):            # through the host in chunks of 16M rows, as bench_micro/scan_where.py loads its table
        i = i.cpu().numpy().view(np.uint64); v = v.cpu().numpy()
        for lo in range(0, len(i), 16_000_000):
            m = min(16_000_000, len(i) - lo)
            e.load_rows(i[lo:lo + m], np.full(m, f, np.uint32), np.full(m, 5, np.int64), v[lo:lo + m])

    load(FU, ids, uni); load(FC, ids, code); load(FR, ids[has_role], role[has_role])
    e.sync()
    e.index_build(FU)
    if e.index_size(FU) != R:
        raise SystemExit("where_agg: the index holds %d of %d rows (table: %d rows)" % (e.index_size(FU), R, e.row_count()))
    say("== %d int32 rows (%.0f MB column); %d timed calls after %d warm-ups, HIP events, device outputs; (f): %d calls after 1, host clock ==" %
        (R, R * 4 / 1e6, a.reps, a.warmup, a.host_reps))
    d_n = torch.zeros(2, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(R, dtype=torch.int64, device=dev)
    d_agg = torch.zeros(6 * (NG + 1), dtype=torch.int64, device=dev)
    d_top = torch.zeros(2 * K, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def recs(n):
        return d_agg.cpu().numpy().view(bmx.AGG_DTYPE)[:n]

    def check(r, sel, vals, what):
        """one record against the selection mask and the measure column (both fields are on every node: n == n_match)"""
        v = vals[sel]
        want = (int(sel.sum()), len(v), int(v.sum()) if len(v) else 0, int(v.min()) if len(v) else None, int(v.max()) if len(v) else None)
        got = (int(r["n_match"]), int(r["n"]), (int(r["sum_hi"]) << 64) + int(r["sum_lo"]), int(r["min"]) if r["n"] else None, int(r["max"]) if r["n"] else None)
        assert got == want, (what, got, want)

    hi30 = ((1 << 30) * 30) // 100 - 1
    progs = []
    for pct in (1, 10, 50):
        hi = ((1 << 30) * pct) // 100 - 1
        progs.append(("AND, %2d %% of the base" % pct, [[(FU, 0, hi), (FC, 24, 87)]], (uni <= hi) & (code >= 24) & (code <= 87)))
    progs.append(("Example 8 shape", [[(FC, 0, 63), (FU, 0, hi30), (FR, 0, 0, True)]], (code <= 63) & (uni <= hi30) & ~(has_role & (role == 0))))
    progs.append(("two-clause OR", [[(FC, 16, 23)], [(FC, 72, 79), (FR, 1, 2)]], ((code >= 16) & (code <= 23)) | ((code >= 72) & (code <= 79) & has_role & (role >= 1) & (role <= 2))))

    if a.program is not None:
        progs = progs[a.program:a.program + 1]
    for name, prog, sel in progs:
        M = int(sel.sum())
        say("-- %s: %d matches (%.1f %%) --" % (name, M, 100.0 * M / R))
        # (a)
        ta = timed(e, lambda: e.scan_where_dev(FU, prog, None, 0, d_n[0:1]), a.reps, a.warmup)
        assert int(d_n[0].item()) == M
        base = np.median(ta)
        say("(a) scan_where, count only           %s" % fmt(ta))
        # (b)
        tb = timed(e, lambda: e.where_aggregate_dev(FU, prog, d_agg, FU), a.reps, a.warmup)
        check(recs(1)[0], sel, uni, "b")
        say("(b) where_aggregate, measure = base  %s  %.2f x (a)" % (fmt(tb), np.median(tb) / base))
        # (c)
        tc = timed(e, lambda: e.where_aggregate_dev(FU, prog, d_agg, FC), a.reps, a.warmup)
        check(recs(1)[0], sel, code, "c")
        say("(c) where_aggregate, measure probed  %s  %.2f x (a)" % (fmt(tc), np.median(tc) / base))
        # (d)
        td = timed(e, lambda: e.where_aggregate_dev(FU, prog, d_agg, FU, FC, 0, NG), a.reps, a.warmup)
        r = recs(NG + 1)
        want_n = torch.bincount(code[sel], minlength=NG).cpu().numpy()
        want_s = torch.zeros(NG, dtype=torch.int64, device=dev).index_add_(0, code[sel], uni[sel]).cpu().numpy()
        assert np.array_equal(r["n_match"][:NG].astype(np.int64), want_n) and int(r["n_match"][NG]) == 0, "d: counts"
        assert np.array_equal(r["sum_lo"][:NG].astype(np.int64), want_s) and not r["sum_hi"][:NG].any(), "d: sums"
        say("(d) where_aggregate, 128 groups      %s  %.2f x (a)" % (fmt(td), np.median(td) / base))
        # (e)
        te = timed(e, lambda: e.where_top_dev(FU, prog, K, d_top, d_n[0:1], d_n[1:2]), a.reps, a.warmup)
        got = d_top.cpu().numpy().view(bmx.TOP_DTYPE)
        cnt = d_n.cpu().numpy()
        sv = uni[sel]
        thr = int(torch.topk(sv, K, largest=False).values.max().item())
        cand = sel & (uni <= thr)
        ci, cv = ids[cand].cpu().numpy().view(np.uint64), uni[cand].cpu().numpy()
        o = np.lexsort((ci, cv))[:K]
        assert int(cnt[0]) == K and int(cnt[1]) == M and np.array_equal(got["id"], ci[o]) and np.array_equal(got["val"], cv[o]), "e"
        say("(e) where_top, k = %d               %s  %.2f x (a)" % (K, fmt(te), np.median(te) / base))
        if a.no_host_route:
            continue
        # (f)
        def route():
            e.scan_where_dev(FU, prog, d_ids, R, d_n[0:1])
            e.sync()
            m = int(d_n[0].item())
            h = d_ids[:m].cpu().numpy().view(np.uint64)
            _, val, found = e.get_rows(h, np.full(m, FU, np.uint32))
            return m, int(val.sum()), int(val.min()), int(val.max()), bool(found.all())

        res = route()
        assert res == (M, int(sv.sum()), int(sv.min()), int(sv.max()), True), "f"
        tf = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter(); route(); tf.append(1e3 * (time.perf_counter() - t0))
        tf = np.array(tf)
        say("(f) scan_where ids + get_rows + numpy %s  (b) %.0f x, (c) %.0f x, (d) %.0f x, (e) %.0f x faster" %
            (fmt(tf), np.median(tf) / np.median(tb), np.median(tf) / np.median(tc), np.median(tf) / np.median(td), np.median(tf) / np.median(te)))
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
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=1100, help="seconds the measurement may take")
    ap.add_argument("--program", type=int, default=None, choices=range(5), help="one program only")
    ap.add_argument("--no-host-route", action="store_true", help="leave (f) out")
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
        print("where_agg: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
