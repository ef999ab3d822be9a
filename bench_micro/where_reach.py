"""where_reach.py — what a graph traversal on the device (include/bmx_reach.h bmx_where_reach_from) costs beside the only route there was before, a host loop
over bmx_where_in and bmx_get_rows, and beside a mark made of the calls a traversal could be put together from.

  python bench_micro/where_reach.py [--out profiles/where_reach.log] [--rows 100000000] [--reps 20] [--warmup 3] [--host-reps 2] [--limit 1100] [--no-host-route]

The table: --rows nodes (10^8; 10^7 where memory or time is short) with a uniform int32 base field, an int64 key field (every node its own key, anywhere in
+-2^52) and an int64 link field, which is probed. Two forests live in it: one of depth 4 (4 levels of 200 000 nodes) below 10^5 seed values A, one of depth 16
(16 levels of 50 000 nodes) below 10^5 seed values B; a node of level L links to the key of a node of level L - 1 (level 0: to a seed value). Every other node's
link dangles: it is an edge node that walks the map in every round and is never reached. In one process, HIP events on the engine's stream (bmx_timer_*),
device outputs, the median of --reps timed calls after --warmup; every answer is checked (n_match, rounds, set_size, flags, and the ids against the host loop's)
before its time is printed.
  reach: bmx_where_reach_from, the edge program selects every node, ids and depths into device memory, set_cap = 2^20: forest A at max_depth 16, forest B at
      max_depth 16 and at 255 (the difference is the cost of 239 blind empty rounds).
  (a) the host loop: where_in with the current frontier, the ids down, get_rows of the key field, numpy.unique, what has been seen taken out; repeated until
      nothing new comes. Timed with the host's clock around the whole, --host-reps calls after one.
  (b) the mark: one device-mode bmx_where_rows of the edge program with the link field, plus `rounds` count-only bmx_where_in calls with a set of the final size.
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_reach.log.
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
NSEEDS = 100_000
FORESTS = {"A": (4, 200_000), "B": (16, 50_000)}       # name -> (depth, nodes per level)


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
    """the key of number j: anywhere in +-2^52"""
    return ((mix(j + 1, 0x369DEA0F31A53F85) >> 11) & ((1 << 53) - 1)) - (1 << 52)


def measure(a):
    import torch
    import bmx
    from oracle import streams

    R = a.rows
    dev = torch.device("cuda", 0)
    FU, FL, FK = (streams.fnv1a32(s) for s in ("reach.uniform", "reach.link", "reach.key"))
    e = bmx.Engine(3 * R + 1000)
    j = torch.arange(R, dtype=torch.int64, device=dev)
    ids = (j + 1) * -0x61c8864680b583eb - 0x0123456789ABCDEF                    # odd multiplier: unique mod 2^64
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    key = key_of(j)                                                             # numbers 0 .. R - 1: the nodes; R .. : values no node holds as key
    rnd = (mix(ids, 0x14057B7EF767814F) >> 8) & 0xFFFFFFFFFF
    link = key_of(2 * R + j)                                                    # dangling
    seeds, first, total = {}, {}, 0
    for name, (depth, width) in FORESTS.items():
        seeds[name] = key_of(R + len(seeds) * NSEEDS + torch.arange(NSEEDS, dtype=torch.int64, device=dev))
        first[name] = total
        for lv in range(depth):
            lo = total + lv * width
            sl = slice(lo, lo + width)
            link[sl] = seeds[name][rnd[sl] % NSEEDS] if lv == 0 else key_of(lo - width + rnd[sl] % width)
        total += depth * width
    if total > R:
        raise SystemExit("where_reach: --rows is below the %d nodes of the two forests" % total)

    def load(hid, f, v):          # through the host in chunks of 16M rows, as bench_micro/where_semijoin.py loads its table
        hv = v.cpu().numpy()
        for lo in range(0, len(hid), 16_000_000):
            m = min(16_000_000, len(hid) - lo)
            e.load_rows(hid[lo:lo + m], np.full(m, f, np.uint32), np.full(m, 5, np.int64), hv[lo:lo + m])
        print("loaded %d rows of field %08x" % (len(hid), f), flush=True)

    hid = ids.cpu().numpy().view(np.uint64)
    load(hid, FU, uni); load(hid, FL, link); load(hid, FK, key)
    del uni, rnd
    e.sync()
    e.index_build(FU)
    if e.index_size(FU) != R:
        raise SystemExit("where_reach: the index holds %d of %d rows" % (e.index_size(FU), R))
    say("== %d rows (%.0f MB int32 column), probed int64 link, %d seeds; %d timed calls after %d warm-ups, HIP events, device outputs ==" % (R, R * 4 / 1e6, NSEEDS, a.reps, a.warmup))
    EVERY = [[(FU, 0, 1 << 30)]]
    cap = max(d * w for d, w in FORESTS.values())
    d_ids = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_dep = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(5, dtype=torch.int64, device=dev)
    d_sres = torch.zeros(4, dtype=torch.int64, device=dev)
    d_rres = torch.zeros(5, dtype=torch.int64, device=dev)
    d_rows_ids = torch.zeros(R, dtype=torch.int64, device=dev)
    d_rows_val = torch.zeros(R, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def reach(name, max_depth):
        e.where_reach_from_dev(FU, EVERY, FL, FK, seeds[name], NSEEDS, d_ids, d_dep, cap, d_res, max_depth=max_depth, set_cap=SET_CAP)

    def host_loop(name):
        """the only route there was: a frontier at a time through where_in and get_rows -> (ids of the reached nodes, levels)"""
        seen = np.unique(seeds[name].cpu().numpy())
        frontier, found, levels = seen, [], 0
        while len(frontier):
            r = e.where_in(FU, EVERY, FL, frontier, cap=cap)
            got = np.setdiff1d(r.ids, np.concatenate(found)) if found else np.unique(r.ids)
            if not len(got):
                break
            found.append(got); levels += 1
            _, kv, kf = e.get_rows(got, np.full(len(got), FK, np.uint32))
            new = np.setdiff1d(np.unique(kv[kf.astype(bool)]), seen)
            seen = np.union1d(seen, new)
            frontier = new
        return (np.concatenate(found) if found else np.zeros(0, np.uint64)), levels

    t16 = {}
    for name, (depth, width) in FORESTS.items():
        n = depth * width
        say("-- forest %s: depth %d, %d nodes, set of %d --" % (name, depth, n, NSEEDS + n))
        t = timed(e, lambda: reach(name, 16), a.reps, a.warmup)
        res = d_res.cpu().numpy().view(bmx.REACH_RES_DTYPE)[0]
        assert (int(res["n_match"]), int(res["rounds"]), int(res["set_size"]), int(res["flags"]), int(res["n_seed"]), int(res["n_edges"])) == (
            n, depth, NSEEDS + n, bmx.REACH_MORE if depth == 16 else 0, NSEEDS, R), (name, res)      # (B's last level brings keys of level 16 = max_depth: MORE)
        got_ids = np.sort(d_ids[:n].cpu().numpy().view(np.uint64))
        assert np.array_equal(got_ids, np.sort(hid[first[name]:first[name] + n])), (name, "ids")
        dep = d_dep[:n].cpu().numpy()
        assert np.array_equal(np.bincount(dep, minlength=depth + 1)[1:], np.full(depth, width)), (name, "depths")
        t16[name] = t
        say("where_reach_from, max_depth 16          %s" % fmt(t))
        # (b) the mark
        tr = timed(e, lambda: e.where_rows_dev(FU, EVERY, [FL], R, d_rows_ids, d_rows_val, None, d_rres), a.reps, a.warmup)
        assert int(d_rres[0].item()) == R
        final = torch.cat([seeds[name], key[first[name]:first[name] + n]])
        ti = timed(e, lambda: e.where_in_dev(FU, EVERY, FL, final, len(final), None, 0, d_sres), a.reps, a.warmup)
        assert int(d_sres[0].item()) == n, (name, "where_in", d_sres)
        mark = np.median(tr) + depth * np.median(ti)
        say("(b) where_rows with the link             %s" % fmt(tr))
        say("(b) one count-only where_in, set of %d   %s" % (len(final), fmt(ti)))
        say("(b) mark = where_rows + %d x where_in = %9.1f us; where_reach_from is %.2f x the mark" % (depth, 1e3 * mark, np.median(t) / mark))
        if not a.no_host_route:
            ids_h, levels = host_loop(name)
            assert levels == depth and np.array_equal(np.sort(ids_h), got_ids), (name, "host loop")
            tf = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter(); host_loop(name); tf.append(1e3 * (time.perf_counter() - t0))
            tf = np.array(tf)
            say("(a) host loop  %s  (%d calls, host clock): where_reach_from is %.1f x faster" % (fmt(tf), a.host_reps, np.median(tf) / np.median(t)))
    say("-- the blind empty rounds: forest B at max_depth 255 --")
    t255 = timed(e, lambda: reach("B", 255), a.reps, a.warmup)
    res = d_res.cpu().numpy().view(bmx.REACH_RES_DTYPE)[0]
    assert (int(res["n_match"]), int(res["rounds"]), int(res["flags"])) == (16 * 50_000, 16, 0)
    say("where_reach_from, max_depth 255         %s  = %.2f x max_depth 16 (%.1f us per empty round)" % (
        fmt(t255), np.median(t255) / np.median(t16["B"]), 1e3 * (np.median(t255) - np.median(t16["B"])) / 239))
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
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--limit", type=int, default=1100, help="seconds the measurement may take")
    ap.add_argument("--no-host-route", action="store_true", help="leave the host loop (a) out")
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
        print("where_reach: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
