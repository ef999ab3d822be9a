"""where_join_group.py — what a lookup join on the device (include/bmx_join.h bmx_where_join_group) costs beside the two calls it is made of and beside the only
route there was before: where_rows of both sides to the host and a numpy join.

  python bench_micro/where_join_group.py [--out profiles/where_join_group.log] [--rows 100000000] [--inner 10000000] [--reps 20] [--warmup 3] [--host-reps 3]
                                         [--limit 1100] [--no-host-route]

The outer side: --rows nodes (10^8; 10^7 where memory or time is short) with a uniform int32 base field (0 .. 2^30), which is also the measure, and an int64 link
field that holds the key of one of 10^6 buckets, anywhere in +-2^52. The inner side: --inner other nodes (10^7) with a uniform int32 base field, two key fields
that hold the keys of the first 10^5 and of all 10^6 buckets, and an attribute field with 200 values (a function of the node, so the nodes of one key differ
and the minimum is taken); an inner program that selects 10 % or all of them gives inner sides of 10^6 and 10^7 nodes. In one process, HIP events on the
engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup; every answer is checked against torch over the same columns
before its time is printed (the map: the minimum attribute per key; the records: count and sum of the measure per attribute; unmatched and total).
  join_group: bmx_where_join_group, records into device memory, map_cap = cap = 2^20, for every inner side x key field x outer literal at 1 / 10 / 50 %.
  (a) bmx_where_group of the outer program grouped by the probed link field (cap = 2^20): the same sweep, probes and aggregation without the lookup.
  (b) the build of bmx_where_semijoin for the same inner side: a count-only bmx_where_semijoin at 1 % less a counting bmx_scan_where of the outer program.
  (c) the host route, for the inner side of 10^6 nodes and the 10^5-key field at 1 and 10 %: where_rows of both sides (ids, key and attribute; ids, link and
      measure) to the host, the minimum attribute per key with numpy, searchsorted, bincount. Timed with the host's clock around the whole, --host-reps calls
      after one.
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_join_group.log.
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
CAP = 1 << 20
BUCKETS = 1_000_000
NATTR = 200


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


def key_of(j):
    """the key of bucket j: anywhere in +-2^52"""
    return ((mix(j + 1, 0x369DEA0F31A53F85) >> 11) & ((1 << 53) - 1)) - (1 << 52)


def measure(a):
    import torch
    import bmx
    from oracle import streams

    R, RI = a.rows, a.inner
    dev = torch.device("cuda", 0)
    sets = (100_000, 1_000_000)
    FU, FL, FI, FA = (streams.fnv1a32(s) for s in ("outer.uniform", "outer.link", "inner.uniform", "inner.attr"))
    FK = {d: streams.fnv1a32("inner.key%d" % d) for d in sets}
    e = bmx.Engine(2 * R + (2 + len(sets)) * RI + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    iids = torch.arange(R + 1, R + RI + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    lbucket = ((mix(ids, 0x14057B7EF767814F) >> 8) & 0xFFFFFFFFFF) % BUCKETS
    iuni = (mix(iids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    kbucket = {d: ((mix(iids, 0x5851F42D4C957F2D + 2 * k) >> 8) & 0xFFFFFFFFFF) % d for k, d in enumerate(sets)}
    attr = ((mix(iids, 0x27BB2EE687B0B0FD) >> 8) & 0xFFFFFFFFFF) % NATTR * 1009 - 100_000

    def load(hid, f, v):          # through the host in chunks of 16M rows, as bench_micro/where_group.py loads its table
        hv = v.cpu().numpy()
        for lo in range(0, len(hid), 16_000_000):
            m = min(16_000_000, len(hid) - lo)
            e.load_rows(hid[lo:lo + m], np.full(m, f, np.uint32), np.full(m, 5, np.int64), hv[lo:lo + m])
        print("loaded %d rows of field %08x" % (len(hid), f), flush=True)

    hid, hiid = ids.cpu().numpy().view(np.uint64), iids.cpu().numpy().view(np.uint64)
    load(hid, FU, uni); load(hid, FL, key_of(lbucket)); load(hiid, FI, iuni); load(hiid, FA, attr)
    for d in sets:
        load(hiid, FK[d], key_of(kbucket[d]))
    e.sync()
    for f, n in ((FU, R), (FI, RI)):
        e.index_build(f)
        if e.index_size(f) != n:
            raise SystemExit("where_join_group: an index holds %d of %d rows" % (e.index_size(f), n))
    say("== outer %d rows (%.0f MB int32 column), inner %d rows, %d attribute values; %d timed calls after %d warm-ups, HIP events, device outputs ==" % (R, R * 4 / 1e6, RI, NATTR, a.reps, a.warmup))
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_sres = torch.zeros(4, dtype=torch.int64, device=dev)
    d_grp = torch.zeros(7 * (CAP + 1), dtype=torch.int64, device=dev)
    d_gres = torch.zeros(14, dtype=torch.int64, device=dev)
    d_jres = torch.zeros(23, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    pcts = (1, 10, 50)
    outer = {p: ([[(FU, 0, ((1 << 30) * p) // 100 - 1)]], uni <= ((1 << 30) * p) // 100 - 1) for p in pcts}
    inner = {}
    for name, p in (("10^6", 10), ("10^7", 100)):
        hi = ((1 << 30) * p) // 100 - 1
        inner[name] = ([[(FI, 0, hi)]], iuni <= hi)

    say("-- (a) bmx_where_group of the outer program by the probed link field, measure = the base column, records into device memory --")
    floor = {}
    for p in pcts:
        prog, sel = outer[p]
        t = timed(e, lambda: e.where_group_dev(FU, prog, FL, d_grp, d_gres, measure=FU, cap=CAP), a.reps, a.warmup)
        gres = d_gres.cpu().numpy().view(bmx.GROUP_RES_DTYPE)[0]
        assert int(gres["flags"]) == 0 and int(gres["n_groups"]) == len(torch.unique(lbucket[sel])) and int(gres["total"]["n_match"]) == int(sel.sum()), ("a", p, gres)
        floor[p] = t
        say("%2d %%  where_group by the link   %s  (%d groups)" % (p, fmt(t), int(gres["n_groups"])))
    scan1 = timed(e, lambda: e.scan_where_dev(FU, outer[1][0], None, 0, d_n), a.reps, a.warmup)
    assert int(d_n.item()) == int(outer[1][1].sum())
    say(" 1 %%  scan_where, counting        %s" % fmt(scan1))

    def check(res, recs, sel, M, what):
        """M: the minimum attribute per bucket (NATTR * 1009: none)"""
        g = M[lbucket[sel]]
        inside = g < NATTR * 1009
        code = torch.div(g[inside] + 100_000, 1009, rounding_mode="floor")
        cnt = torch.bincount(code, minlength=NATTR).cpu().numpy()
        sums = torch.zeros(NATTR, dtype=torch.int64, device=dev).scatter_add_(0, code, uni[sel][inside]).cpu().numpy()      # (below 2^63: exact)
        assert int(res["flags"]) == 0 and int(res["total"]["n_match"]) == int(sel.sum()) and int(res["unmatched"]["n_match"]) == int((~inside).sum()), (what, res)
        assert int(res["absent"]["n_match"]) == 0 and int(res["n_groups"]) == int((cnt > 0).sum()), (what, res)
        recs = np.sort(recs[:int(res["n_groups"])], order="key")
        codes = (recs["key"] + 100_000) // 1009
        assert np.array_equal(codes, np.nonzero(cnt)[0]) and np.array_equal(recs["agg"]["n_match"], cnt[cnt > 0].astype(np.uint64)), what
        assert np.array_equal(recs["agg"]["sum_lo"].astype(np.int64), sums[cnt > 0]) and (recs["agg"]["sum_hi"] == 0).all(), what

    maps = {}
    for iname, (iprog, isel) in inner.items():
        say("-- inner side of %s nodes (%d selected) --" % (iname, int(isel.sum())))
        for d in sets:
            M = torch.full((BUCKETS,), NATTR * 1009, dtype=torch.int64, device=dev)
            M.scatter_reduce_(0, kbucket[d][isel], attr[isel], reduce="amin", include_self=True)
            nkeys = int((M < NATTR * 1009).sum())
            maps[(iname, d)] = M
            ts = timed(e, lambda: e.where_semijoin_dev(FU, outer[1][0], FL, FI, iprog, FK[d], None, 0, d_sres, set_cap=CAP), a.reps, a.warmup)
            sres = d_sres.cpu().numpy().view(bmx.SEMI_RES_DTYPE)[0]
            assert int(sres["flags"]) == 0 and int(sres["set_size"]) == nkeys, ("b", iname, d, sres)
            tb = np.median(ts) - np.median(scan1)
            say("map of %7d keys  (b) count-only where_semijoin at 1 %%  %s  less scan_where = the build: %9.1f us" % (nkeys, fmt(ts), 1e3 * tb))
            for p in pcts:
                prog, sel = outer[p]
                t = timed(e, lambda: e.where_join_group_dev(FU, prog, FL, FI, iprog, FK[d], FA, d_grp, d_jres, measure=FU, cap=CAP, map_cap=CAP), a.reps, a.warmup)
                res = d_jres.cpu().numpy().view(bmx.JOIN_RES_DTYPE)[0]
                assert (int(res["map_size"]), int(res["n_inner"]), int(res["n_keyed"])) == (nkeys, int(isel.sum()), int(isel.sum())), ("join", iname, d, p, res)
                check(res, d_grp[:7 * NATTR].cpu().numpy().view(bmx.GROUP_DTYPE), sel, M, ("join", iname, d, p))
                ab = np.median(floor[p]) + tb
                say("    %2d %%  where_join_group  %s  %.2f x (a) + (b) = %9.1f us  (%d groups, %d unmatched)" % (p, fmt(t), np.median(t) / ab, 1e3 * ab, int(res["n_groups"]), int(res["unmatched"]["n_match"])))

    if not a.no_host_route:
        say("-- (c) the host route: where_rows of both sides to the host, the minimum attribute per key, searchsorted, bincount; inner side 10^6, the 10^5-key field --")
        iprog, isel = inner["10^6"]
        d = 100_000
        for p in (1, 10):
            prog, sel = outer[p]
            n_in, n_out = int(isel.sum()), int(sel.sum())

            def route():
                ri = e.where_rows(FI, iprog, [FK[d], FA], cap=n_in)
                k, v = ri.vals[0], ri.vals[1]
                order = np.lexsort((v, k))
                k, v = k[order], v[order]
                first = np.ones(len(k), bool); first[1:] = k[1:] != k[:-1]
                K, V = k[first], v[first]
                ro = e.where_rows(FU, prog, [FL, FU], cap=n_out)
                at = np.minimum(np.searchsorted(K, ro.vals[0]), len(K) - 1)
                inside = K[at] == ro.vals[0]
                code = (V[at][inside] + 100_000) // 1009
                mv = ro.vals[1][inside]                                # (the two halves' sums are exact in float64)
                sums = np.bincount(code, weights=mv >> 16, minlength=NATTR).astype(np.int64) * 65536 + np.bincount(code, weights=mv & 0xFFFF, minlength=NATTR).astype(np.int64)
                return np.bincount(code, minlength=NATTR), sums, int((~inside).sum())

            t = timed(e, lambda: e.where_join_group_dev(FU, prog, FL, FI, iprog, FK[d], FA, d_grp, d_jres, measure=FU, cap=CAP, map_cap=CAP), a.reps, a.warmup)
            res = d_jres.cpu().numpy().view(bmx.JOIN_RES_DTYPE)[0]
            recs = np.sort(d_grp[:7 * NATTR].cpu().numpy().view(bmx.GROUP_DTYPE)[:int(res["n_groups"])], order="key")
            cnt, sums, un = route()
            assert np.array_equal(recs["agg"]["n_match"], cnt[cnt > 0].astype(np.uint64)) and np.array_equal(recs["agg"]["sum_lo"].astype(np.int64), sums[cnt > 0]) and un == int(res["unmatched"]["n_match"]), ("c", p)
            tf = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter(); route(); tf.append(1e3 * (time.perf_counter() - t0))
            tf = np.array(tf)
            say("%2d %%  host route %s  (%d calls, host clock)  where_join_group %s: %.0f x faster" % (p, fmt(tf), a.host_reps, fmt(t), np.median(tf) / np.median(t)))
    e.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--inner", type=int, default=10_000_000)
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
        print("where_join_group: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
