"""where_semijoin.py — what a semi-join on the device (include/bmx_semi.h bmx_where_semijoin) costs beside the two calls it is made of and beside the only route
there was before: both id lists to the host, the key and link values fetched with get_rows, numpy.unique and numpy.isin.

  python bench_micro/where_semijoin.py [--out profiles/where_semijoin.log] [--rows 100000000] [--inner 10000000] [--reps 20] [--warmup 3] [--host-reps 3]
                                       [--limit 1100] [--no-host-route]

The outer side: --rows nodes (10^8; 10^7 where memory or time is short) with a uniform int32 base field (0 .. 2^30) and an int64 link field that holds the key
of one of 2 * 10^6 buckets, anywhere in +-2^52. The inner side: --inner other nodes (10^7) with a uniform int32 base field and four key fields that hold the
keys of the first 5, 10^3, 10^5 and 10^6 buckets; an inner program that selects 1 %, 10 % or all of them gives inner sides of 10^5, 10^6 and 10^7 nodes. In one
process, HIP events on the engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup; every count is checked against torch
over the same columns before its time is printed.
  semijoin: bmx_where_semijoin, ids into device memory, set_cap = 2^20, for every inner side x key field x outer literal at 0 / 1 / 10 / 50 % (0 %: the build and the
      bare outer sweep; what a row at p % costs above it, less what (a) at p % costs above (a) at 0 %, is the walk of the set).
  (a) bmx_scan_where of the outer program with a presence literal on the link field, ids into device memory: the same sweep and the same probes without the
      set — the floor of the probe sweep, with its spread (max - min) / median.
  (b) bmx_where_group of the inner program on the key field (cap = 2^20, no measure): the same inner sweep with accumulators beside the keys.
  (c) the host route, for one inner side (10 %) and the 10^5-key field at 1 and 10 %: scan_where ids of both sides to the host, get_rows of key and link,
      numpy.unique, numpy.isin. Timed with the host's clock around the whole, --host-reps calls after one.
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_semijoin.log.
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
SET_CAP = 1 << 20
BUCKETS = 2_000_000


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


def key_of(j):
    """the key of bucket j: anywhere in +-2^52"""
    return ((mix(j + 1, 0x369DEA0F31A53F85) >> 11) & ((1 << 53) - 1)) - (1 << 52)


def measure(a):
    import torch
    import bmx
    from oracle import streams

    R, RI = a.rows, a.inner
    dev = torch.device("cuda", 0)
    sets = (5, 1000, 100_000, 1_000_000)
    FU, FL, FI = (streams.fnv1a32(s) for s in ("outer.uniform", "outer.link", "inner.uniform"))
    FK = {d: streams.fnv1a32("inner.key%d" % d) for d in sets}
    e = bmx.Engine(2 * R + (1 + len(sets)) * RI + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    iids = torch.arange(R + 1, R + RI + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    link = key_of(((mix(ids, 0x14057B7EF767814F) >> 8) & 0xFFFFFFFFFF) % BUCKETS)
    iuni = (mix(iids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    keys = {d: key_of(((mix(iids, 0x5851F42D4C957F2D + 2 * k) >> 8) & 0xFFFFFFFFFF) % d) for k, d in enumerate(sets)}

    def load(hid, f, v):          # through the host in chunks of 16M rows, as bench_micro/where_group.py loads its table
        hv = v.cpu().numpy()
        for lo in range(0, len(hid), 16_000_000):
            m = min(16_000_000, len(hid) - lo)
            e.load_rows(hid[lo:lo + m], np.full(m, f, np.uint32), np.full(m, 5, np.int64), hv[lo:lo + m])
        print("loaded %d rows of field %08x" % (len(hid), f), flush=True)

    hid, hiid = ids.cpu().numpy().view(np.uint64), iids.cpu().numpy().view(np.uint64)
    load(hid, FU, uni); load(hid, FL, link); load(hiid, FI, iuni)
    for d in sets:
        load(hiid, FK[d], keys[d])
    e.sync()
    for f, n in ((FU, R), (FI, RI)):
        e.index_build(f)
        if e.index_size(f) != n:
            raise SystemExit("where_semijoin: an index holds %d of %d rows" % (e.index_size(f), n))
    say("== outer %d rows (%.0f MB int32 column), inner %d rows; %d timed calls after %d warm-ups, HIP events, device outputs ==" % (R, R * 4 / 1e6, RI, a.reps, a.warmup))
    d_ids = torch.zeros(R, dtype=torch.int64, device=dev)
    d_res = torch.zeros(4, dtype=torch.int64, device=dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_grp = torch.zeros(7 * (SET_CAP + 1), dtype=torch.int64, device=dev)
    d_gres = torch.zeros(14, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    ALL = (-(1 << 62), 1 << 62)
    pcts = (0, 1, 10, 50)          # 0 %: the outer program selects nothing — the build and the bare outer sweep, no probe and no walk
    outer = {p: ([[(FU, 0, ((1 << 30) * p) // 100 - 1)]], uni <= ((1 << 30) * p) // 100 - 1) for p in pcts}
    inner = {}
    for name, p in (("10^5", 1), ("10^6", 10), ("10^7", 100)):
        hi = ((1 << 30) * p) // 100 - 1
        inner[name] = ([[(FI, 0, hi)]], iuni <= hi)

    say("-- (a) the floor of the probe sweep: bmx_scan_where, outer literal AND link present, ids into device memory --")
    floor = {}
    for p in pcts:
        prog = [[outer[p][0][0][0], (FL,) + ALL]]
        t = timed(e, lambda: e.scan_where_dev(FU, prog, d_ids, R, d_n), a.reps, a.warmup)
        assert int(d_n.item()) == int(outer[p][1].sum()), ("a", p)
        floor[p] = t
        say("%2d %%  scan_where + presence of the link   %s  spread %.2f  (%d ids)" % (p, fmt(t), spread(t), int(d_n.item())))

    for iname, (iprog, isel) in inner.items():
        say("-- inner side of %s nodes (%d selected) --" % (iname, int(isel.sum())))
        for d in sets:
            S = torch.unique(keys[d][isel])
            inS = torch.isin(link, S)
            tb = timed(e, lambda: e.where_group_dev(FI, iprog, FK[d], d_grp, d_gres, cap=SET_CAP), a.reps, a.warmup)
            gres = d_gres.cpu().numpy().view(bmx.GROUP_RES_DTYPE)[0]
            assert int(gres["flags"]) == 0 and int(gres["n_groups"]) == len(S) and int(gres["total"]["n_match"]) == int(isel.sum()), ("b", iname, d)
            say("set of %7d keys  (b) where_group of the inner program on the key   %s" % (len(S), fmt(tb)))
            for p in pcts:
                prog, sel = outer[p]
                t = timed(e, lambda: e.where_semijoin_dev(FU, prog, FL, FI, iprog, FK[d], d_ids, R, d_res, set_cap=SET_CAP), a.reps, a.warmup)
                res = d_res.cpu().numpy().view(bmx.SEMI_RES_DTYPE)[0]
                want = int((sel & inS).sum())
                assert (int(res["n_match"]), int(res["set_size"]), int(res["n_inner"]), int(res["flags"])) == (want, len(S), int(isel.sum()), 0), ("semijoin", iname, d, p, res)
                ab = np.median(floor[p]) + np.median(tb)
                say("    %2d %%  where_semijoin  %s  %.2f x (a) + (b) = %9.1f us  (%d ids)" % (p, fmt(t), np.median(t) / ab, 1e3 * ab, want))
            del inS

    if not a.no_host_route:
        say("-- (c) the host route: both id lists down, get_rows of key and link, numpy.unique, numpy.isin; inner side 10^6, the 10^5-key field --")
        iprog, isel = inner["10^6"]
        d = 100_000
        d_iids = torch.zeros(RI, dtype=torch.int64, device=dev)
        for p in (1, 10):
            prog, sel = outer[p]

            def route():
                e.scan_where_dev(FI, iprog, d_iids, RI, d_n); e.sync()
                hi_ = d_iids[:int(d_n.item())].cpu().numpy().view(np.uint64)
                _, kv, kf = e.get_rows(hi_, np.full(len(hi_), FK[d], np.uint32))
                S = np.unique(kv[kf.astype(bool)])
                e.scan_where_dev(FU, prog, d_ids, R, d_n); e.sync()
                ho = d_ids[:int(d_n.item())].cpu().numpy().view(np.uint64)
                _, lv, lf = e.get_rows(ho, np.full(len(ho), FL, np.uint32))
                return ho[lf.astype(bool) & np.isin(lv, S)]

            t = timed(e, lambda: e.where_semijoin_dev(FU, prog, FL, FI, iprog, FK[d], d_ids, R, d_res, set_cap=SET_CAP), a.reps, a.warmup)
            got = d_ids[:int(d_res[0].item())].cpu().numpy().view(np.uint64)
            assert np.array_equal(route(), got), ("c", p)
            tf = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter(); route(); tf.append(1e3 * (time.perf_counter() - t0))
            tf = np.array(tf)
            say("%2d %%  host route %s  (%d calls, host clock)  where_semijoin %s: %.0f x faster" % (p, fmt(tf), a.host_reps, fmt(t), np.median(tf) / np.median(t)))
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
        print("where_semijoin: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
