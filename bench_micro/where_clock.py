"""where_clock.py — what a clock literal (include/bmx_where.h BMX_LIT_CLOCK / BMX_LIT_CLOCK_TOMB) costs, and what its path costs the programs that have none.

  python bench_micro/where_clock.py --part a --parent-lib /path/to/parent/libbmx.so [--rounds 2] [--out profiles/where_clock.log]
  python bench_micro/where_clock.py --part b [--out profiles/where_clock.log]
  common: [--rows 100000000] [--reps 20] [--warmup 3] [--limit 900]

One index of --rows int32 rows (10^8). In each measuring process: HIP events on the engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls
after --warmup; every answer's count is checked against torch over the same columns before its time is printed. The helpers are bench_micro/where_diff.py's.

(a) THE GATE. Regression of the existing path: the programs of bench_micro/scan_where.py, none with a clock literal (where_diff.py part_a_child), timed with
    this tree's library and with a build of the parent commit (--parent-lib), the processes alternating --rounds times in one session. Per program: the medians
    of every process, the parent's own spread ((max - min) / median across its processes, and inside one process), and this tree's median over the parent's.
    This tree's median may exceed the parent's by no more than the parent's spread.
(b) The new path; reported, not gated. Expectations written down BEFORE the run (MARKS):
    (b2) a clock literal on a probed field selecting 1 / 10 / 50 % next to a plain literal on the same field selecting the same share: the probes are the
         same, parity expected (mark 1.10 x);
    (b3) a clock literal on the base field next to a plain literal on one probed field, same shares: both probe once per candidate (mark 1.10 x); and next to
         a value literal on the base field, which probes nothing (no mark: the price of the probe);
    (b4) the route that existed, bmx_where_rows of the field with clocks to the host plus numpy (wall clock, 3 calls), against the device form at 1 / 10 %
         (mark: the literal is at least 20 x faster).

Every measuring step runs in a child process under --limit seconds: a measurement that hangs or fails ends the script, and nothing is started behind it.
Recorded: profiles/where_clock.log."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "bullet-js_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import where_diff as wd  # noqa: E402
from where_diff import I64MAX, I64MIN, LINES, fmt, mix, say, timed  # noqa: E402

MARKS = {"clock_vs_plain_same_field": 1.10, "base_clock_vs_plain_probe": 1.10, "host_route_over_clock": 20.0}


def table(a):
    """-> (engine, fields, columns on the device): the base field "uniform" (0 .. 2^30, clock 0 .. 99 by node) on every node, the field "a" (0 .. 2^30, clock
    0 .. 99 by node, independent) on every node, a tenth of a's rows tombstoned at their clock"""
    import torch
    import bmx
    from oracle import streams

    R = a.rows
    dev = torch.device("cuda", 0)
    e = bmx.Engine(2 * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF
    col = {"uniform": (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1), "a": (mix(ids, 0x5851F42D4C957F2D) >> 8) & ((1 << 30) - 1),
           "ts_u": (mix(ids, 0x14057B7EF767814F) >> 8) % 100, "ts_a": (mix(ids, 0x369DEA0F31A53F85) >> 8) % 100}
    col["dead_a"] = ((mix(ids, 0x27BB2EE687B0B0FD) >> 8) % 10) == 0
    F = {name: streams.fnv1a32("where_clock." + name) for name in ("uniform", "a")}
    hid = ids.cpu().numpy().view(np.uint64)
    for name, ts, dead in (("uniform", "ts_u", None), ("a", "ts_a", "dead_a")):
        v = col[name].cpu().numpy().copy(); t = col[ts].cpu().numpy()
        if dead:
            v[col[dead].cpu().numpy()] = bmx.VAL_DELETED
        for lo in range(0, R, 16_000_000):
            m = min(16_000_000, R - lo)
            e.put_rows(hid[lo:lo + m], np.full(m, F[name], np.uint32), t[lo:lo + m], v[lo:lo + m])
    e.sync()
    e.index_build(F["uniform"])
    if e.index_size(F["uniform"]) != R:
        raise SystemExit("where_clock: the index holds %d of %d rows (table: %d rows)" % (e.index_size(F["uniform"]), R, e.row_count()))
    return e, F, col


def part_b_child(a):
    import torch
    import bmx

    e, F, c = table(a)
    FU, FA = F["uniform"], F["a"]
    uni, ca, tu, ta, dead = c["uniform"], c["a"], c["ts_u"], c["ts_a"], c["dead_a"]
    R = a.rows
    dev = torch.device("cuda", 0)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev); d_out = torch.zeros(R, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    say("== (b) %d int32 rows (%.0f MB column); %d timed calls after %d warm-ups, HIP events, device outputs; marks written before the run: %s ==" %
        (R, R * 4 / 1e6, a.reps, a.warmup, json.dumps(MARKS)))

    def run(prog, want):
        t = timed(e, lambda: e.scan_where_dev(FU, prog, d_out, R, d_n), a.reps, a.warmup)
        assert int(d_n.item()) == want, (prog, int(d_n.item()), want)
        return t

    def verdict(ratio, mark):
        return "%.3f x  (mark %.2f x: %s)" % (ratio, mark, "met" if ratio <= mark else "MISSED")

    live = ~dead
    for pct in (1, 10, 50):
        hi = ((1 << 30) * pct) // 100 - 1
        tp = run([[(FA, 0, hi)]], int((live & (ca <= hi)).sum()))
        tc = run([[(bmx.Clock(FA), 0, pct - 1)]], int((live & (ta <= pct - 1)).sum()))
        tt = run([[(bmx.Clock(FA, tombs=True), 0, pct - 1)]], int((ta <= pct - 1).sum()))
        tb = run([[(bmx.Clock(FU), 0, pct - 1)]], int((tu <= pct - 1).sum()))
        tv = run([[(FU, 0, hi)]], int((uni <= hi).sum()))
        say("(b2) %2d %%: plain literal on probed a            %s" % (pct, fmt(tp)))
        say("(b2) %2d %%: clock literal on probed a (data)     %s  %s" % (pct, fmt(tc), verdict(np.median(tc) / np.median(tp), MARKS["clock_vs_plain_same_field"])))
        say("(b2) %2d %%: clock literal on probed a (any state) %s  %.3f x the plain literal (selects 1 / 0.9 as many)" % (pct, fmt(tt), np.median(tt) / np.median(tp)))
        say("(b3) %2d %%: clock literal on the base field      %s  %s" % (pct, fmt(tb), verdict(np.median(tb) / np.median(tp), MARKS["base_clock_vs_plain_probe"])))
        say("(b3) %2d %%: value literal on the base field      %s  the clock literal takes %.2f x as long (one probe per candidate against none)" % (pct, fmt(tv), np.median(tb) / np.median(tv)))
    for pct in (1, 10):
        want = int((live & (ta <= pct - 1)).sum())
        tc = run([[(bmx.Clock(FA), 0, pct - 1)]], want)
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = e.where_rows(FU, [[(FU, I64MIN, I64MAX)]], [FA], with_ts=True)
            sel = r.ids[(r.vals[0] != bmx.VAL_DELETED) & (r.ts[0] <= pct - 1)]
            walls.append(time.perf_counter() - t0)
            assert len(sel) == want
            del r, sel
        wall = float(np.median(walls))
        ratio = wall * 1e3 / np.median(tc)
        say("(b4) %2d %%: where_rows of a with clocks to the host + numpy, %d matches: median %.2f s wall of 3 (%s)" % (pct, want, wall, ", ".join("%.2f" % w for w in walls)))
        say("(b4) %2d %%: the clock literal, ids on the device:  %s  the host route takes %.0f x as long  (mark %.0f x: %s)" %
            (pct, fmt(tc), ratio, MARKS["host_route_over_clock"], "met" if ratio >= MARKS["host_route_over_clock"] else "MISSED"))
    e.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


def child(a, part, lib=None):
    env = dict(os.environ)
    if lib:
        env["BMX_LIB_PATH"] = lib
    else:
        env.pop("BMX_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--rows", str(a.rows), "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--out", a.out] if a.out and part == "b" else [])
    out = subprocess.run(cmd, env=env, timeout=a.limit, stdout=subprocess.PIPE if part == "a" else None, text=True)
    if out.returncode != 0:
        raise SystemExit("where_clock: the measuring process ended with status %d; nothing further is started" % out.returncode)
    return json.loads(out.stdout.strip().splitlines()[-1]) if part == "a" else None


def part_a(a):
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("where_clock: --part a needs --parent-lib, a libbmx.so built from the parent commit")
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):
        runs["parent"].append(child(a, "a", a.parent_lib))
        runs["this"].append(child(a, "a"))
    say("== (a) %d int32 rows; programs without a clock literal; %d timed calls after %d warm-ups per process, HIP events, device outputs; %d processes of each library, alternating ==" %
        (a.rows, a.reps, a.warmup, a.rounds))
    worst = 0.0
    for name in runs["this"][0]:
        pm = [r[name][0] for r in runs["parent"]]; tm = [r[name][0] for r in runs["this"]]
        inside = max((r[name][2] - r[name][1]) / r[name][0] for r in runs["parent"])
        across = (max(pm) - min(pm)) / float(np.median(pm))
        spread = max(inside, across)
        diff = float(np.median(tm)) / float(np.median(pm)) - 1.0
        worst = max(worst, diff - spread)
        say("(a) %-30s parent %s us  this tree %s us  this/parent %+.3f  parent's spread %.3f (inside a process %.3f, across processes %.3f): %s" %
            (name, " ".join("%8.1f" % (1e3 * x) for x in pm), " ".join("%8.1f" % (1e3 * x) for x in tm), diff, spread, inside, across,
             "inside" if diff <= spread else "SLOWER BY MORE THAN THE SPREAD"))
    say("(a) verdict: %s" % ("no program is slower than the parent by more than the parent's own spread" if worst <= 0 else "a program is slower by %.3f beyond the spread" % worst))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")
    return 0 if worst <= 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b"], default="b")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds one measuring process may take")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps is 20 at least")
    if a.child:
        (wd.part_a_child if a.child == "a" else part_b_child)(a)
        return 0
    try:
        if a.part == "a":
            return part_a(a)
        child(a, "b")
        return 0
    except subprocess.TimeoutExpired:
        print("where_clock: a measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
