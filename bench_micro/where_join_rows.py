"""where_join_rows.py — what a join projection on the device (include/bmx_join_rows.h bmx_where_join_rows) costs beside the calls it is made of and beside the
only route there was before: where_rows of both sides to the host, the smallest inner node per key there, searchsorted, and get_rows per inner field.

  python bench_micro/where_join_rows.py [--out profiles/where_join_rows.log] [--rows 100000000] [--inner 10000000] [--reps 20] [--warmup 3] [--host-reps 3]
                                        [--limit 1100] [--no-host-route]

The table is bench_micro/where_join_group.py's: --rows outer nodes with a uniform int32 base field (0 .. 2^30) and an int64 link field that holds the key of one
of 10^6 buckets, anywhere in +-2^52; --inner other nodes with a uniform int32 base field, two key fields that hold the keys of the first 10^5 and of all 10^6
buckets, and an attribute field. An inner program that selects 10 % or all of them gives inner sides of a tenth of --inner and of --inner nodes. In one
process, HIP events on the engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup; every answer is checked against torch
over the same columns before its time is printed (the smallest unsigned id per key, the inner id of every delivered row, n_joined, the attribute of the inner
node).
  join_rows: bmx_where_join_rows, k = 2 outer fields (the link, twice) and j = 2 inner fields (the attribute and the key), no clocks, map_cap = 2^20, cap = the
      selection, left and inner join, for every inner side x key field x outer literal at 1 / 10 %.
  (a) bmx_where_rows of the outer program with k + j + 1 = 5 fields (the link, five times): the same mask pass, ranking and number of probes per row.
  (b) the build: a count-only bmx_where_semijoin at 1 % less a counting bmx_scan_where of the outer program, as where_join_group.py derives it.
  (m) the inner join's mask pass beside a counting bmx_scan_where with one more probed literal (the link, any value).
  (c) the host route, for the smaller inner side and the 10^5-key field at 1 and 10 %. Timed with the host's clock around the whole, --host-reps calls after one.
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_join_rows.log.
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
VAL_MAX = (1 << 53) - 1
BIAS = -(1 << 63)                       # x ^ BIAS on int64: the unsigned order of the ids as a signed order


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
            raise SystemExit("where_join_rows: an index holds %d of %d rows" % (e.index_size(f), n))
    say("== outer %d rows (%.0f MB int32 column), inner %d rows; %d timed calls after %d warm-ups, HIP events, device outputs ==" % (R, R * 4 / 1e6, RI, a.reps, a.warmup))
    pcts = (1, 10)
    outer = {p: ([[(FU, 0, ((1 << 30) * p) // 100 - 1)]], uni <= ((1 << 30) * p) // 100 - 1) for p in pcts}
    nsel = {p: int(outer[p][1].sum()) for p in pcts}
    inner = {}
    for name, p in (("%d" % (RI // 10), 10), ("%d" % RI, 100)):
        hi = ((1 << 30) * p) // 100 - 1
        inner[name] = ([[(FI, 0, hi)]], iuni <= hi)
    room = max(nsel.values())
    K, J = 2, 2
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_sres = torch.zeros(4, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(room + 1, dtype=torch.int64, device=dev)
    d_val = torch.zeros((K + J + 1) * room + 1, dtype=torch.int64, device=dev)
    d_in_ids = torch.zeros(room + 1, dtype=torch.int64, device=dev)
    d_in_val = torch.zeros(J * room + 1, dtype=torch.int64, device=dev)
    d_rres = torch.zeros(5, dtype=torch.int64, device=dev)
    d_jres = torch.zeros(9, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    # the inner nodes by id, for the check of the delivered attribute
    iid_sorted, iid_order = torch.sort(iids ^ BIAS)

    say("-- (a) bmx_where_rows of the outer program with %d fields (the probed link field, %d times), device outputs --" % (K + J + 1, K + J + 1))
    mark, scan, scan_l = {}, {}, {}
    for p in pcts:
        prog, sel = outer[p]
        t = timed(e, lambda: e.where_rows_dev(FU, prog, [FL] * (K + J + 1), nsel[p], d_ids, d_val, None, d_rres), a.reps, a.warmup)
        r = d_rres.cpu().numpy().view(bmx.ROWS_RES_DTYPE)[0]
        assert int(r["n_match"]) == int(r["n_out"]) == nsel[p], ("a", p, r)
        mark[p] = t
        say("%2d %%  where_rows, %d fields       %s  (%d rows)" % (p, K + J + 1, fmt(t), nsel[p]))
        scan[p] = timed(e, lambda: e.scan_where_dev(FU, prog, None, 0, d_n), a.reps, a.warmup)
        assert int(d_n.item()) == nsel[p]
        prog_l = [prog[0] + [(FL, -VAL_MAX, VAL_MAX)]]
        scan_l[p] = timed(e, lambda: e.scan_where_dev(FU, prog_l, None, 0, d_n), a.reps, a.warmup)
        assert int(d_n.item()) == nsel[p]
        say("%2d %%  scan_where, counting        %s;  with one more probed literal (the link)  %s" % (p, fmt(scan[p]), fmt(scan_l[p])))

    def check(res, p, sel, M, d, inner_join, what):
        """M: jrows-biased smallest inner id per bucket (INT64_MAX: none)"""
        n = int(res["n_out"])
        got_ids, got_in = d_ids[:n], d_in_ids[:n]
        w = M[lbucket[sel]]
        joined = w != torch.iinfo(torch.int64).max
        want_in = torch.where(joined, w ^ BIAS, torch.full_like(w, -1))
        want_ids = ids[sel]
        if inner_join:
            want_ids, want_in = want_ids[joined], want_in[joined]
        assert n == len(want_ids) == int(res["n_match"]) and int(res["n_joined"]) == int(joined.sum()) and int(res["flags"]) == 0, (what, res)
        go, wo = torch.argsort(got_ids), torch.argsort(want_ids)
        assert torch.equal(got_ids[go], want_ids[wo]) and torch.equal(got_in[go], want_in[wo]), what
        # the inner cells: the attribute and the key of the inner node
        has = got_in != -1
        at = iid_order[torch.searchsorted(iid_sorted, got_in[has] ^ BIAS)]
        assert torch.equal(d_in_val[:n][has], attr[at]) and torch.equal(d_in_val[n:2 * n][has], key_of(kbucket[d][at])), what
        assert bool((d_in_val[:n][~has] == torch.iinfo(torch.int64).min).all()), what
        assert torch.equal(d_val[:n][go], key_of(lbucket[sel])[joined if inner_join else slice(None)][wo]), what

    for iname, (iprog, isel) in inner.items():
        say("-- inner side of %s nodes (%d selected) --" % (iname, int(isel.sum())))
        for d in sets:
            M = torch.full((BUCKETS,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
            M.scatter_reduce_(0, kbucket[d][isel], (iids ^ BIAS)[isel], reduce="amin", include_self=True)
            nkeys = int((M != torch.iinfo(torch.int64).max).sum())
            ts = timed(e, lambda: e.where_semijoin_dev(FU, outer[1][0], FL, FI, iprog, FK[d], None, 0, d_sres, set_cap=CAP), a.reps, a.warmup)
            sres = d_sres.cpu().numpy().view(bmx.SEMI_RES_DTYPE)[0]
            assert int(sres["flags"]) == 0 and int(sres["set_size"]) == nkeys, ("b", iname, d, sres)
            tb = np.median(ts) - np.median(scan[1])
            say("map of %7d keys  (b) count-only where_semijoin at 1 %%  %s  less scan_where = the build: %9.1f us" % (nkeys, fmt(ts), 1e3 * tb))
            for p in pcts:
                prog, sel = outer[p]
                for inner_join in (False, True):
                    fn = lambda: e.where_join_rows_dev(FU, prog, FL, [FL] * K, FI, iprog, FK[d], [FA, FK[d]], nsel[p], d_ids, d_val, None, d_in_ids, d_in_val, None, d_jres,  # noqa: E731
                                                       inner=inner_join, map_cap=CAP)
                    t = timed(e, fn, a.reps, a.warmup)
                    res = d_jres.cpu().numpy().view(bmx.JROWS_RES_DTYPE)[0]
                    assert (int(res["map_size"]), int(res["n_inner"]), int(res["n_keyed"])) == (nkeys, int(isel.sum()), int(isel.sum())), ("join", iname, d, p, res)
                    # the columns have stride cap = nsel[p]: bring them to stride n_out for the check
                    n = int(res["n_out"])
                    if n != nsel[p]:
                        d_in_val[n:2 * n] = d_in_val[nsel[p]:nsel[p] + n].clone()
                    check(res, p, sel, M, d, inner_join, ("join", iname, d, p, inner_join))
                    ab = np.median(mark[p]) + tb
                    extra = ""
                    if inner_join:
                        tm = timed(e, lambda: e.where_join_rows_dev(FU, prog, FL, [], FI, iprog, FK[d], [], 0, None, None, None, None, None, None, d_jres, inner=True, map_cap=CAP), a.reps, a.warmup)
                        extra = "  (m) cap 0 less (b) = the mask pass: %8.1f us beside scan_where with the link literal %8.1f us" % (1e3 * (np.median(tm) - tb), 1e3 * np.median(scan_l[p]))
                    say("    %2d %%  %s join  %s  %.2f x (a) + (b) = %9.1f us  (%d rows, %d joined)%s" % (p, "inner" if inner_join else "left ", fmt(t), np.median(t) / ab, 1e3 * ab, n, int(res["n_joined"]), extra))

    if not a.no_host_route:
        say("-- (c) the host route: where_rows of both sides to the host, the smallest id per key, searchsorted, get_rows per inner field; the smaller inner side, the 10^5-key field --")
        iname = "%d" % (RI // 10)
        iprog, isel = inner[iname]
        d = 100_000
        n_in = int(isel.sum())
        for p in pcts:
            prog, sel = outer[p]

            def route():
                ri = e.where_rows(FI, iprog, [FK[d]], cap=n_in)
                k, i = ri.vals[0], ri.ids
                order = np.lexsort((i, k))
                k, i = k[order], i[order]
                first = np.ones(len(k), bool); first[1:] = k[1:] != k[:-1]
                Kk, Ii = k[first], i[first]
                ro = e.where_rows(FU, prog, [FL] * K, cap=nsel[p])
                at = np.minimum(np.searchsorted(Kk, ro.vals[0]), len(Kk) - 1)
                inside = Kk[at] == ro.vals[0]
                want = Ii[at][inside]
                cols = [e.get_rows(want, np.full(len(want), f, np.uint32))[1] for f in (FA, FK[d])]
                return ro.ids, inside, want, cols

            t = timed(e, lambda: e.where_join_rows_dev(FU, prog, FL, [FL] * K, FI, iprog, FK[d], [FA, FK[d]], nsel[p], d_ids, d_val, None, d_in_ids, d_in_val, None, d_jres, map_cap=CAP), a.reps, a.warmup)
            res = d_jres.cpu().numpy().view(bmx.JROWS_RES_DTYPE)[0]
            rid, inside, want, cols = route()
            n = int(res["n_out"])
            g_ids, g_in, g_attr = d_ids[:n].cpu().numpy().view(np.uint64), d_in_ids[:n].cpu().numpy().view(np.uint64), d_in_val[:n].cpu().numpy()
            assert np.array_equal(g_ids, rid) and int(res["n_joined"]) == int(inside.sum()) and np.array_equal(g_in[inside], want) and np.array_equal(g_attr[inside], cols[0]), ("c", p)
            tf = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter(); route(); tf.append(1e3 * (time.perf_counter() - t0))
            tf = np.array(tf)
            say("%2d %%  host route %s  (%d calls, host clock)  where_join_rows, left %s: %.0f x faster" % (p, fmt(tf), a.host_reps, fmt(t), np.median(tf) / np.median(t)))
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
        print("where_join_rows: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
