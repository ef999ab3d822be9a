"""watch_poll.py — what a standing query's poll (include/bmx_watch.h bmx_watch_poll) costs beside what a client does today: bmx_scan_where of the same program
again, count only and with all ids (which it would then pull over the link and diff on the host; neither of those is in these times).

  python bench_micro/watch_poll.py [--out profiles/watch_poll.log] [--rows 10000000,100000000] [--reps 20] [--warmup 3] [--deltas 1000000] [--limit 1100]

Per table size one process: an index of --rows int32 rows — a uniform base field (0 .. 2^30), a 16-valued field on every node, a 4-valued "role" on three quarters
of the nodes, loaded through the host in 16M-row chunks as bench_micro/scan_where.py loads them. HIP events on the engine's stream (bmx_timer_*), device outputs,
the median of --reps timed calls after --warmup. Two watches: a one-literal range on the base field at 10 % selectivity, and Example 8's shape from scan_where.py.
  (a) an idle poll: nothing was written since the last one;
  (b) a poll behind a merge of --deltas new values of the base field (distinct existing nodes), for the range watch;
  (c) the same for Example 8's shape.
In (b) and (c) the refresh of the index from the merge's change log is paid by whichever query comes first behind the merge, so it is timed on its own
(bmx_index_size) and the poll and the two scans follow it, the poll first on even repetitions and last on odd ones. Every poll's n_match is checked against the scan's
count of the same repetition, and entered / left against the sizes torch derives from the old and new values. Next to each baseline: the spread of its --reps calls,
(max - min) / median. The GPU work of one table size is one step in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is
started behind it. Recorded: profiles/watch_poll.log.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bullet-js_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def fmt(ms):
    ms = np.asarray(ms)
    return "median %8.1f us  min %8.1f us  max %8.1f us" % (1e3 * np.median(ms), 1e3 * ms.min(), 1e3 * ms.max())


def spread(ms):
    ms = np.asarray(ms)
    return (ms.max() - ms.min()) / np.median(ms)


def mix(x, k):
    """a cheap 64-bit mix on the device (torch int64 arithmetic wraps)"""
    x = x * k
    x = x ^ ((x >> 29) & 0x7FFFFFFFF)
    x = x * -0x61c8864680b583eb
    return x ^ ((x >> 32) & 0xFFFFFFFF)


def measure(a, R):
    import torch
    import bmx
    from oracle import streams

    FU, FS, FR = streams.fnv1a32("uniform"), streams.fnv1a32("sixteen"), streams.fnv1a32("role")
    dev = torch.device("cuda", 0)
    D = min(a.deltas, R // 2)
    e = bmx.Engine(3 * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    six = (mix(ids, 0x5851F42D4C957F2D) >> 8) & 15
    role = (mix(ids, 0x14057B7EF767814F) >> 8) & 3
    has_role = ((mix(ids, 0x369DEA0F31A53F85) >> 8) & 3) != 0

    def load(f, i, v):
        i = i.cpu().numpy().view(np.uint64); v = v.cpu().numpy()
        for lo in range(0, len(i), 16_000_000):
            m = min(16_000_000, len(i) - lo)
            e.load_rows(i[lo:lo + m], np.full(m, f, np.uint32), np.full(m, 5, np.int64), v[lo:lo + m])

    load(FU, ids, uni); load(FS, ids, six); load(FR, ids[has_role], role[has_role])
    e.sync()
    e.index_build(FU)
    if e.index_size(FU) != R:
        raise SystemExit("watch_poll: the index holds %d of %d rows (table: %d rows)" % (e.index_size(FU), R, e.row_count()))
    say("== %d int32 rows (%.0f MB column), merges of %d deltas; %d timed calls after %d warm-ups, HIP events, device outputs ==" % (R, R * 4 / 1e6, D, a.reps, a.warmup))
    hi10, hi30 = ((1 << 30) * 10) // 100 - 1, ((1 << 30) * 30) // 100 - 1
    progs = {"range, 10 %": [[(FU, 0, hi10)]], "Example 8 shape": [[(FS, 0, 7), (FU, 0, hi30), (FR, 0, 0, True)]]}
    other = (six <= 7) & ~(has_role & (role == 0))                      # Example 8's literals that the merges do not touch

    def truth(name, u):
        return (u <= hi10) if name.startswith("range") else ((u <= hi30) & other)

    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_out = torch.zeros(R, dtype=torch.int64, device=dev)
    d_ent = torch.zeros(R, dtype=torch.int64, device=dev)
    d_lft = torch.zeros(R, dtype=torch.int64, device=dev)
    d_res = torch.zeros(4, dtype=torch.int64, device=dev)
    ts = torch.zeros(D, dtype=torch.int64, device=dev)
    fld = torch.full((D,), FU if FU < (1 << 31) else FU - (1 << 32), dtype=torch.int32, device=dev)      # (the field hash as the int32 torch has)
    torch.cuda.synchronize(dev)

    def once(fn):
        e.timer_start(); fn(); return e.timer_stop()

    def res():
        e.sync()
        r = d_res.cpu().numpy()
        return int(r[0]), int(r[1]), int(r[2]), int(r[3]) & 0xFFFFFFFF

    watches = {}
    for name, prog in progs.items():
        w = watches[name] = e.watch_create(FU, prog)
        e.watch_poll_dev(w, d_ent, R, d_lft, R, d_res)
        ne, nl, nm, flags = res()
        assert flags == bmx.WATCH_RESET and ne == nm == int(truth(name, uni).sum()) and nl == 0, (name, ne, nl, nm, flags)
    # (a) idle
    for name, prog in progs.items():
        w = watches[name]
        for _ in range(a.warmup):
            e.watch_poll_dev(w, d_ent, R, d_lft, R, d_res); e.scan_where_dev(FU, prog, None, 0, d_n); e.scan_where_dev(FU, prog, d_out, R, d_n)
        e.sync()
        tp = [once(lambda: e.watch_poll_dev(w, d_ent, R, d_lft, R, d_res)) for _ in range(a.reps)]
        assert res()[:2] == (0, 0) and res()[3] == 0
        tc = [once(lambda: e.scan_where_dev(FU, prog, None, 0, d_n)) for _ in range(a.reps)]
        ti = [once(lambda: e.scan_where_dev(FU, prog, d_out, R, d_n)) for _ in range(a.reps)]
        say("(a) %-16s idle poll                 %s  (%d in the answer)" % (name, fmt(tp), res()[2]))
        say("(a) %-16s scan_where, count only    %s  spread %.3f  poll / this %.3f" % (name, fmt(tc), spread(tc), np.median(tp) / np.median(tc)))
        say("(a) %-16s scan_where, ids           %s  spread %.3f  poll / this %.3f" % (name, fmt(ti), spread(ti), np.median(tp) / np.median(ti)))
    # (b), (c) behind a merge
    stride = R // D
    step = 0
    for tag, name in (("(b)", "range, 10 %"), ("(c)", "Example 8 shape")):
        w, prog = watches[name], progs[name]
        e.watch_poll_dev(w, d_ent, R, d_lft, R, d_res); e.sync()                # committed against the column as it is now
        t = {"refresh": [], "poll": [], "count": [], "ids": []}
        changes = []
        for rep in range(-a.warmup, a.reps):
            step += 1
            idx = (torch.arange(D, dtype=torch.int64, device=dev) * stride + (step % stride)) % R            # distinct rows
            new = (mix(ids[idx], 0x2545F4914F6CDD1D + 2 * step) >> 8) & ((1 << 30) - 1)
            old_t, new_t = truth(name, uni)[idx], truth(name, new) if name.startswith("range") else ((new <= hi30) & other[idx])
            want_e, want_l = int((new_t & ~old_t).sum()), int((old_t & ~new_t).sum())
            b_id = ids[idx].contiguous(); b_val = new.contiguous(); ts.fill_(100 + step)
            uni[idx] = new
            want_m = int(truth(name, uni).sum())
            torch.cuda.synchronize(dev)
            e.merge_batch_dev(D, b_id, fld, ts, b_val)
            r_ms = once(lambda: e.index_size(FU))
            order = ("poll", "count", "ids") if rep % 2 == 0 else ("count", "ids", "poll")
            got = {}
            for what in order:
                if what == "poll":
                    got[what] = once(lambda: e.watch_poll_dev(w, d_ent, R, d_lft, R, d_res))
                    ne, nl, nm, flags = res()
                    assert (ne, nl, nm, flags) == (want_e, want_l, want_m, 0), (name, rep, ne, nl, nm, flags, want_e, want_l, want_m)
                else:
                    got[what] = once(lambda: e.scan_where_dev(FU, prog, d_out if what == "ids" else None, R if what == "ids" else 0, d_n))
                    e.sync()
                    assert int(d_n.item()) == want_m, (name, rep, what)
            if rep >= 0:
                t["refresh"].append(r_ms); changes.append(want_e + want_l)
                for what in order:
                    t[what].append(got[what])
        say("%s %-16s index refresh (index_size) %s" % (tag, name, fmt(t["refresh"])))
        say("%s %-16s poll behind the merge      %s  (%d ids entered or left per poll, of %d in the answer)" % (tag, name, fmt(t["poll"]), int(np.median(changes)), want_m))
        say("%s %-16s scan_where, count only     %s  spread %.3f  poll / this %.3f" % (tag, name, fmt(t["count"]), spread(t["count"]), np.median(t["poll"]) / np.median(t["count"])))
        say("%s %-16s scan_where, ids            %s  spread %.3f  poll / this %.3f" % (tag, name, fmt(t["ids"]), spread(t["ids"]), np.median(t["poll"]) / np.median(t["ids"])))
    e.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", default="10000000,100000000", help="table sizes, one child process each")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--deltas", type=int, default=1_000_000)
    ap.add_argument("--limit", type=int, default=1100, help="seconds the measurement of one table size may take")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps is 20 at least")
    if a.child:
        measure(a, a.child)
        return 0
    for rows in (int(x) for x in a.rows.split(",")):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(rows)] + sys.argv[1:], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print("watch_poll: the measurement of %d rows did not finish in %d s; nothing further is started" % (rows, a.limit), file=sys.stderr)
            return 124
        if rc:
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
