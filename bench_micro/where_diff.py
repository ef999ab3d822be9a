"""where_diff.py — what a field-to-field literal (include/bmx_where.h BMX_LIT_MINUS) costs, and what the pair path costs the programs that have none.

  python bench_micro/where_diff.py --part a --parent-lib /path/to/parent/libbmx.so [--rounds 2] [--out profiles/where_diff.log]
  python bench_micro/where_diff.py --part b [--out profiles/where_diff.log]
  common: [--rows 100000000] [--reps 20] [--warmup 3] [--limit 900]

One index of --rows int32 rows (10^8). In each measuring process: HIP events on the engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls
after --warmup; every answer's count is checked against torch over the same columns before its time is printed.

(a) Regression of the existing path: the programs of bench_micro/scan_where.py, none with a pair literal (the one-clause two-term program at 1 / 10 / 50 %,
    Example 8's shape and the two-clause OR, ids and count only), timed with this tree's library and with a build of the parent commit (--parent-lib: built from
    a checkout of that commit; it exports the same symbols, so this tree's binding loads it through BMX_LIB_PATH), the processes alternating --rounds times on
    the same box. Per program: the medians of every process, the parent's own repetition-to-repetition spread ((max - min) / median of the medians of its
    processes, and inside one process), and this tree's median over the parent's. A difference inside the parent's spread is no difference.
(b) The new path, against marks written down BEFORE the run (MARKS below): a pair (probed A, base) selecting 1 / 10 / 50 % against a plain one-literal probe
    of A selecting the same share (the two issue the same probes: mark 1.10 x); a pair (probed A, probed B) against a program with one plain literal on each
    (again the same probes: mark 1.10 x); and the route that existed, bmx_where_rows of both fields to the host plus numpy (wall clock, 3 calls; mark: the
    pair literal is at least 20 x faster). Reported, not gated.

Every measuring step runs in a child process under --limit seconds: a measurement that hangs or fails ends the script, and nothing is started behind it.
Recorded: profiles/where_diff.log."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bullet-js_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MARKS = {"pair_base_vs_probe": 1.10, "pair_two_probes_vs_two_literals": 1.10, "host_route_over_pair": 20.0}
LINES = []
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


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
    return "median %8.1f us  min %8.1f us  max %8.1f us" % (1e3 * np.median(ms), 1e3 * ms.min(), 1e3 * ms.max())


def mix(x, k):
    """a cheap 64-bit mix on the device (torch int64 arithmetic wraps)"""
    x = x * k
    x = x ^ ((x >> 29) & 0x7FFFFFFFF)
    x = x * -0x61c8864680b583eb
    return x ^ ((x >> 32) & 0xFFFFFFFF)


def table(a, fields):
    """-> (engine, columns on the device by name): the base field "uniform" (0 .. 2^30) on every node and the fields asked for"""
    import torch
    import bmx
    from oracle import streams

    R = a.rows
    dev = torch.device("cuda", 0)
    e = bmx.Engine((len(fields) + 1) * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    col = {"uniform": (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)}
    make = {
        "sixteen": lambda: (mix(ids, 0x5851F42D4C957F2D) >> 8) & 15,
        "role": lambda: (mix(ids, 0x14057B7EF767814F) >> 8) & 3,
        "a": lambda: col["uniform"] + ((mix(ids, 0x5851F42D4C957F2D) >> 8) % 100),            # a - uniform: 0 .. 99, uniform
        "b": lambda: col["uniform"] + ((mix(ids, 0x14057B7EF767814F) >> 8) % 100),            # a - b: -99 .. 99, triangular
    }
    has = {"role": ((mix(ids, 0x369DEA0F31A53F85) >> 8) & 3) != 0}
    F = {name: streams.fnv1a32("where_diff." + name) for name in ["uniform"] + list(fields)}

    def load(f, i, v):            # through the host in chunks of 16M rows, as bench_micro/big_index.py loads its table
        i = i.cpu().numpy().view(np.uint64); v = v.cpu().numpy()
        for lo in range(0, len(i), 16_000_000):
            m = min(16_000_000, len(i) - lo)
            e.load_rows(i[lo:lo + m], np.full(m, f, np.uint32), np.full(m, 5, np.int64), v[lo:lo + m])

    load(F["uniform"], ids, col["uniform"])
    for name in fields:
        col[name] = make[name]()
        keep = has.get(name)
        load(F[name], ids if keep is None else ids[keep], col[name] if keep is None else col[name][keep])
    e.sync()
    e.index_build(F["uniform"])
    if e.index_size(F["uniform"]) != R:
        raise SystemExit("where_diff: the index holds %d of %d rows (table: %d rows)" % (e.index_size(F["uniform"]), R, e.row_count()))
    return e, F, col, has


def part_a_child(a):
    """the programs of scan_where.py on one library; the last line printed is JSON: {program: [median, min, max] in ms}"""
    import torch
    import bmx

    e, F, c, has = table(a, ["sixteen", "role"])
    FU, FS, FR = F["uniform"], F["sixteen"], F["role"]
    uni, six, role, has_role = c["uniform"], c["sixteen"], c["role"], has["role"]
    R = a.rows
    dev = torch.device("cuda", 0)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev); d_out = torch.zeros(R, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    res = {}
    progs = []
    for pct in (1, 10, 50):
        hi = ((1 << 30) * pct) // 100 - 1
        progs.append(("one clause, two terms, %2d %%" % pct, [[(FU, 0, hi), (FS, 3, 10)]], int(((uni <= hi) & (six >= 3) & (six <= 10)).sum()), (d_out, R)))
    hi30 = ((1 << 30) * 30) // 100 - 1
    ex8 = [[(FS, 0, 7), (FU, 0, hi30), (FR, 0, 0, True)]]
    want8 = int(((six <= 7) & (uni <= hi30) & ~(has_role & (role == 0))).sum())
    or2 = [[(FS, 2, 2)], [(FS, 9, 9), (FR, 1, 2)]]
    want2 = int(((six == 2) | ((six == 9) & has_role & (role >= 1) & (role <= 2))).sum())
    for name, prog, want in (("Example 8 shape", ex8, want8), ("two-clause OR", or2, want2)):
        progs.append((name + ", ids", prog, want, (d_out, R))); progs.append((name + ", count only", prog, want, (None, 0)))
    for name, prog, want, (out, cap) in progs:
        t = timed(e, lambda: e.scan_where_dev(FU, prog, out, cap, d_n), a.reps, a.warmup)
        assert int(d_n.item()) == want, (name, int(d_n.item()), want)
        res[name] = [float(np.median(t)), float(t.min()), float(t.max())]
    e.close()
    print(json.dumps(res), flush=True)


def part_b_child(a):
    import torch
    import bmx

    e, F, c, _ = table(a, ["a", "b"])
    FU, FA, FB = F["uniform"], F["a"], F["b"]
    uni, ca, cb = c["uniform"], c["a"], c["b"]
    R = a.rows
    dev = torch.device("cuda", 0)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev); d_out = torch.zeros(R, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    say("== (b) %d int32 rows (%.0f MB column); %d timed calls after %d warm-ups, HIP events, device outputs; marks written before the run: %s ==" %
        (R, R * 4 / 1e6, a.reps, a.warmup, json.dumps(MARKS)))

    def run(prog, want, out=d_out, cap=R):
        t = timed(e, lambda: e.scan_where_dev(FU, prog, out, cap, d_n), a.reps, a.warmup)
        assert int(d_n.item()) == want, (prog, int(d_n.item()), want)
        return t

    def verdict(ratio, mark):
        return "%.3f x  (mark %.2f x: %s)" % (ratio, mark, "met" if ratio <= mark else "MISSED")

    for pct in (1, 10, 50):
        # a - uniform is 0 .. 99: the pair selects pct %; the plain literal on a selects the same share of a's own range
        hi = ((1 << 30) * pct) // 100 - 1
        tp = run([[(FA, 0, hi)]], int((ca <= hi).sum()))
        td = run([[((FA, FU), 0, pct - 1)]], int(((ca - uni) <= pct - 1).sum()))
        say("(b1) %2d %%: plain probe of a                   %s" % (pct, fmt(tp)))
        say("(b1) %2d %%: pair (probed a, base)              %s  %s" % (pct, fmt(td), verdict(np.median(td) / np.median(tp), MARKS["pair_base_vs_probe"])))
    for pct, k in ((1, -86), (10, -56), (50, 0)):
        # a - b is triangular on -99 .. 99; a - b <= k selects about pct %. The plain program probes a (a presence literal, always true) and b.
        want_d = int(((ca - cb) <= k).sum())
        hi = ((1 << 30) * pct) // 100 - 1
        tp = run([[(FA, I64MIN, I64MAX), (FB, 0, hi)]], int((cb <= hi).sum()))
        td = run([[((FA, FB), I64MIN, k)]], want_d)
        say("(b2) %2d %%: one plain literal on a and on b    %s" % (pct, fmt(tp)))
        say("(b2) %2d %%: pair (probed a, probed b), %5.1f %%  %s  %s" % (pct, 100.0 * want_d / R, fmt(td), verdict(np.median(td) / np.median(tp), MARKS["pair_two_probes_vs_two_literals"])))
    # the route that existed: both fields of every node to the host, the comparison in numpy (wall clock)
    k = -56
    want_d = int(((ca - cb) <= k).sum())
    td = run([[((FA, FB), I64MIN, k)]], want_d)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = e.where_rows(FU, [[(FU, I64MIN, I64MAX)]], [FA, FB])
        sel = r.ids[(r.vals[0] != bmx.VAL_DELETED) & (r.vals[1] != bmx.VAL_DELETED) & (r.vals[0] - r.vals[1] <= k)]
        walls.append(time.perf_counter() - t0)
        assert len(sel) == want_d
        del r, sel
    wall = float(np.median(walls))
    ratio = wall * 1e3 / np.median(td)
    say("(b3) where_rows of a and b to the host + numpy, %d matches: median %.2f s wall of 3 (%s)" % (want_d, wall, ", ".join("%.2f" % w for w in walls)))
    say("(b3) the pair literal, ids on the device:       %s  the host route takes %.0f x as long  (mark %.0f x: %s)" %
        (fmt(td), ratio, MARKS["host_route_over_pair"], "met" if ratio >= MARKS["host_route_over_pair"] else "MISSED"))
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
        raise SystemExit("where_diff: the measuring process ended with status %d; nothing further is started" % out.returncode)
    return json.loads(out.stdout.strip().splitlines()[-1]) if part == "a" else None


def part_a(a):
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("where_diff: --part a needs --parent-lib, a libbmx.so built from the parent commit")
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):
        runs["parent"].append(child(a, "a", a.parent_lib))
        runs["this"].append(child(a, "a"))
    say("== (a) %d int32 rows; programs without a pair literal; %d timed calls after %d warm-ups per process, HIP events, device outputs; %d processes of each library, alternating ==" %
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
    return 0


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
        (part_a_child if a.child == "a" else part_b_child)(a)
        return 0
    try:
        if a.part == "a":
            return part_a(a)
        child(a, "b")
        return 0
    except subprocess.TimeoutExpired:
        print("where_diff: a measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
