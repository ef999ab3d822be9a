"""where_expr.py — what a computed measure (include/bmx_expr.h: value(a) op value(b) of the selected node) costs beside the plain forms, and what its template
flag costs the plain forms.

  python bench_micro/where_expr.py --part c --parent-lib /path/to/parent/libbmx.so [--rounds 2] [--out profiles/where_expr.log]
  python bench_micro/where_expr.py --part abd [--out profiles/where_expr.log]
  common: [--rows 100000000] [--reps 20] [--warmup 3] [--limit 900]

One index of --rows int32 rows (10^8): the base field "uniform" (0 .. 2^30), "p" (0 .. 999) and "q" (0 .. 99) on every node; the selection is the base range
that holds 1 / 10 / 50 % of the rows. In each measuring process: HIP events on the engine's stream (bmx_timer_*), device outputs, the median of --reps timed
calls after --warmup; every answer (n_match, n, the exact sum in two halves, min, max, the group count, the quantiles, the two counters) is checked against
torch over the same columns before its time is printed.

(a) base * probed (uniform * p) beside the plain form with the probed field (p) as its measure: the same single probe. The plain form is timed twice, in front
    of and behind the expression: the difference of its two medians is the run-to-run spread the comparison is read against. Three forms: the flat aggregate,
    the group-by over discovered values (group q: one more probe in both), the quantiles (p50 / p95 / p99).
(b) probed * probed (p * q) beside the plain form with the measure p and one more probed presence literal on q: the same two probes.
(c) Plain-measure programs through the old entry points, this tree's library against a build of the parent commit (--parent-lib; this tree's binding loads it
    through BMX_LIB_PATH), the processes alternating --rounds times. A difference inside the parent's own spread is no difference.
(d) The route that existed: bmx_where_rows of p and q to the host plus numpy (wall clock, 3 calls) at 1 and 10 %, beside the flat aggregate of p * q.
The marks (MARKS) were written down before the run; DESIGN.md "Computed measures" holds the reasoning. Reported, not gated.

Every measuring step runs in a child process under --limit seconds: a measurement that hangs or fails ends the script, and nothing is started behind it.
Recorded: profiles/where_expr.log."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bullet-js_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from where_diff import LINES, fmt, mix, say, timed  # noqa: E402  (the same clock, the same column mix)

MARKS = {"base_x_probed_vs_plain": 1.05, "probed_x_probed_vs_two_probes": 1.05, "quantiles_base_x_probed_vs_plain": 2.0, "host_route_over_expr": 20.0}
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
QS = [(1, 2), (95, 100), (99, 100)]


def table(a):
    """-> (engine, field hashes by name, columns on the device by name)"""
    import torch
    import bmx
    from oracle import streams

    R = a.rows
    dev = torch.device("cuda", 0)
    e = bmx.Engine(3 * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    col = {"uniform": (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1),
           "p": ((mix(ids, 0x5851F42D4C957F2D) >> 8) & 0xFFFFFF) % 1000,
           "q": ((mix(ids, 0x14057B7EF767814F) >> 8) & 0xFFFFFF) % 100}
    F = {name: streams.fnv1a32("where_expr." + name) for name in col}
    i = ids.cpu().numpy().view(np.uint64)
    t0 = time.perf_counter()
    for name in ("uniform", "p", "q"):            # through the host in chunks of 16M rows, as bench_micro/big_index.py loads its table
        v = col[name].cpu().numpy()
        for lo in range(0, R, 16_000_000):
            m = min(16_000_000, R - lo)
            e.load_rows(i[lo:lo + m], np.full(m, F[name], np.uint32), np.full(m, 5, np.int64), v[lo:lo + m])
        print("where_expr: field %s loaded, %.0f s" % (name, time.perf_counter() - t0), file=sys.stderr, flush=True)
    e.sync()
    e.index_build(F["uniform"])
    if e.index_size(F["uniform"]) != R:
        raise SystemExit("where_expr: the index holds %d of %d rows (table: %d rows)" % (e.index_size(F["uniform"]), R, e.row_count()))
    return e, F, col


def agg_of(v):
    """torch's answer for the values v (int64, |v| < 2^53): (n, exact sum as a Python int, min, max)"""
    if v.numel() == 0:
        return 0, 0, I64MAX, I64MIN
    return int(v.numel()), (int((v >> 32).sum()) << 32) + int((v & 0xFFFFFFFF).sum()), int(v.min()), int(v.max())


def rec_of(h):
    """a bmx_agg of six int64 words -> (n_match, n, exact sum, min, max)"""
    w = [int(x) for x in h[:6]]
    return w[0], w[1], (w[5] << 64) + (w[4] & ((1 << 64) - 1)), w[2], w[3]


class Forms:
    """the three forms on one engine, plain (measure: a field) or computed (measure: a bmx.Expr), each into device memory and checked against torch"""

    def __init__(self, e, F, col, a):
        import torch
        self.e, self.F, self.col, self.a = e, F, col, a
        dev = torch.device("cuda", 0)
        self.d_agg = torch.zeros(6, dtype=torch.int64, device=dev); self.d_x = torch.zeros(2, dtype=torch.int64, device=dev)
        self.d_grp = torch.zeros(7 * 256, dtype=torch.int64, device=dev); self.d_gres = torch.zeros(14, dtype=torch.int64, device=dev)
        self.d_q = torch.zeros(4 * len(QS), dtype=torch.int64, device=dev); self.d_qres = torch.zeros(4, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)

    def call(self, form, clauses, measure):
        import bmx
        e, FU, FQ = self.e, self.F["uniform"], self.F["q"]
        x = isinstance(measure, bmx.Expr)
        if form == "aggregate":
            return (lambda: e.where_aggregate_expr_dev(FU, clauses, measure, self.d_agg, self.d_x)) if x else (lambda: e.where_aggregate_dev(FU, clauses, self.d_agg, measure=measure))
        if form == "group":
            return (lambda: e.where_group_expr_dev(FU, clauses, FQ, measure, self.d_grp, self.d_gres, self.d_x, cap=256)) if x else \
                   (lambda: e.where_group_dev(FU, clauses, FQ, self.d_grp, self.d_gres, measure=measure, cap=256))
        return (lambda: e.where_quantiles_expr_dev(FU, clauses, measure, QS, self.d_q, self.d_qres, self.d_x)) if x else \
               (lambda: e.where_quantiles_dev(FU, clauses, measure, QS, self.d_q, self.d_qres))

    def run(self, form, clauses, measure, sel, vals):
        """times the call, then checks what it left: sel = torch's selection mask, vals = torch's measure values of all rows"""
        import torch
        import bmx
        t = timed(self.e, self.call(form, clauses, measure), self.a.reps, self.a.warmup)
        v = vals[sel]
        n, s, mn, mx = agg_of(v)
        if isinstance(measure, bmx.Expr):
            assert self.d_x.cpu().tolist() == [0, 0], (form, self.d_x.cpu().tolist())      # every node holds p and q and every product is far inside the range
        if form == "aggregate":
            assert rec_of(self.d_agg.cpu().numpy()) == (n, n, s, mn, mx), (form, rec_of(self.d_agg.cpu().numpy()), (n, n, s, mn, mx))
        elif form == "group":
            r = self.d_gres.cpu().numpy()
            assert (int(r[0]), int(r[1])) == (int(torch.unique(self.col["q"][sel]).numel()), 0) and rec_of(r[8:14]) == (n, n, s, mn, mx), (form, r)
        else:
            sv = torch.sort(v).values
            want = [int(sv[(num * (n - 1)) // den]) for num, den in QS] if n else [0] * len(QS)
            h = self.d_q.cpu().numpy().reshape(len(QS), 4); r = self.d_qres.cpu().numpy()
            assert [int(x) for x in h[:, 0]] == want and (int(r[0]), int(r[1]), int(r[2]), int(r[3])) == (n, n, mn, mx), (form, h, r, want)
        return t


def verdict(ratio, mark, spread):
    return "%.3f x  (mark %.2f x: %s; the plain form's own spread %.3f)" % (ratio, mark, "met" if ratio <= mark else "MISSED", spread)


def part_abd_child(a):
    import bmx

    e, F, c = table(a)
    FU, FP, FQ = F["uniform"], F["p"], F["q"]
    uni, cp, cq = c["uniform"], c["p"], c["q"]
    f = Forms(e, F, c, a)
    say("== (a) (b) (d) %d int32 rows (%.0f MB column); %d timed calls after %d warm-ups, HIP events, device outputs; marks written before the run: %s ==" %
        (a.rows, a.rows * 4 / 1e6, a.reps, a.warmup, json.dumps(MARKS)))
    for pct in (1, 10, 50):
        hi = ((1 << 30) * pct) // 100 - 1
        sel = uni <= hi
        base = [[(FU, 0, hi)]]
        both = [[(FU, 0, hi), (FQ, I64MIN, I64MAX)]]            # ... and q holds data: one more probe, always true
        for form in ("aggregate", "group", "quantiles"):
            mark = MARKS["quantiles_base_x_probed_vs_plain" if form == "quantiles" else "base_x_probed_vs_plain"]
            t0 = f.run(form, base, FP, sel, cp)
            tx = f.run(form, base, bmx.Expr(FU, "*", FP), sel, uni * cp)
            t1 = f.run(form, base, FP, sel, cp)
            plain = min(np.median(t0), np.median(t1)); spread = abs(np.median(t0) - np.median(t1)) / plain
            say("(a) %2d %% %-9s plain, measure p            %s   again: %s" % (pct, form, fmt(t0), fmt(t1)))
            say("(a) %2d %% %-9s uniform * p                 %s  %s" % (pct, form, fmt(tx), verdict(np.median(tx) / plain, mark, spread)))
        for form in ("aggregate", "group"):
            t0 = f.run(form, both, FP, sel, cp)
            tx = f.run(form, base, bmx.Expr(FP, "*", FQ), sel, cp * cq)
            t1 = f.run(form, both, FP, sel, cp)
            plain = min(np.median(t0), np.median(t1)); spread = abs(np.median(t0) - np.median(t1)) / plain
            say("(b) %2d %% %-9s plain, measure p, q present %s   again: %s" % (pct, form, fmt(t0), fmt(t1)))
            say("(b) %2d %% %-9s p * q                       %s  %s" % (pct, form, fmt(tx), verdict(np.median(tx) / plain, MARKS["probed_x_probed_vs_two_probes"], spread)))
    for pct in (1, 10):
        hi = ((1 << 30) * pct) // 100 - 1
        sel = uni <= hi
        tx = f.run("aggregate", [[(FU, 0, hi)]], bmx.Expr(FP, "*", FQ), sel, cp * cq)
        want = agg_of((cp * cq)[sel])
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = e.where_rows(FU, [[(FU, 0, hi)]], [FP, FQ])
            ok = (r.vals[0] != bmx.VAL_DELETED) & (r.vals[1] != bmx.VAL_DELETED)
            v = r.vals[0][ok] * r.vals[1][ok]
            got = (len(v), (int((v >> 32).sum()) << 32) + int((v & 0xFFFFFFFF).sum()), int(v.min()), int(v.max()))
            walls.append(time.perf_counter() - t0)
            assert got == want, (got, want)
            del r, v
        wall = float(np.median(walls)); ratio = wall * 1e3 / np.median(tx)
        say("(d) %2d %%: where_rows of p and q to the host + numpy, %d matches: median %.3f s wall of 3 (%s)" % (pct, want[0], wall, ", ".join("%.3f" % w for w in walls)))
        say("(d) %2d %%: the flat aggregate of p * q:                 %s  the host route takes %.0f x as long  (mark %.0f x: %s)" %
            (pct, fmt(tx), ratio, MARKS["host_route_over_expr"], "met" if ratio >= MARKS["host_route_over_expr"] else "MISSED"))
    e.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


def part_c_child(a):
    """the plain forms on one library; the last line printed is JSON: {program: [median, min, max] in ms}. Only calls the parent exports."""
    e, F, c = table(a)
    FU, FP = F["uniform"], F["p"]
    uni, cp = c["uniform"], c["p"]
    f = Forms(e, F, c, a)
    res = {}
    for pct in (1, 10, 50):
        hi = ((1 << 30) * pct) // 100 - 1
        sel = uni <= hi
        for form in ("aggregate", "group", "quantiles"):
            for measure, vals, tag in ((FP, cp, "measure p"), (FU, uni, "measure base")):
                t = f.run(form, [[(FU, 0, hi)]], measure, sel, vals)
                res["%-9s %2d %%, %s" % (form, pct, tag)] = [float(np.median(t)), float(t.min()), float(t.max())]
    e.close()
    print(json.dumps(res), flush=True)


def child(a, part, lib=None):
    env = dict(os.environ)
    if lib:
        env["BMX_LIB_PATH"] = lib
    else:
        env.pop("BMX_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--rows", str(a.rows), "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--out", a.out] if a.out and part != "c" else [])
    out = subprocess.run(cmd, env=env, timeout=a.limit, stdout=subprocess.PIPE if part == "c" else None, text=True)
    if out.returncode != 0:
        raise SystemExit("where_expr: the measuring process ended with status %d; nothing further is started" % out.returncode)
    return json.loads(out.stdout.strip().splitlines()[-1]) if part == "c" else None


def part_c(a):
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("where_expr: --part c needs --parent-lib, a libbmx.so built from the parent commit")
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):
        runs["parent"].append(child(a, "c", a.parent_lib))
        runs["this"].append(child(a, "c"))
    say("== (c) %d int32 rows; plain measures through the old entry points; %d timed calls after %d warm-ups per process, HIP events, device outputs; %d processes of each library, alternating ==" %
        (a.rows, a.reps, a.warmup, a.rounds))
    worst = 0.0
    for name in runs["this"][0]:
        pm = [r[name][0] for r in runs["parent"]]; tm = [r[name][0] for r in runs["this"]]
        inside = max((r[name][2] - r[name][1]) / r[name][0] for r in runs["parent"])
        across = (max(pm) - min(pm)) / float(np.median(pm))
        spread = max(inside, across)
        diff = float(np.median(tm)) / float(np.median(pm)) - 1.0
        worst = max(worst, diff - spread)
        say("(c) %-32s parent %s us  this tree %s us  this/parent %+.3f  parent's spread %.3f (inside a process %.3f, across processes %.3f): %s" %
            (name, " ".join("%8.1f" % (1e3 * x) for x in pm), " ".join("%8.1f" % (1e3 * x) for x in tm), diff, spread, inside, across,
             "inside" if diff <= spread else "SLOWER BY MORE THAN THE SPREAD"))
    say("(c) verdict: %s" % ("no program is slower than the parent by more than the parent's own spread" if worst <= 0 else "a program is slower by %.3f beyond the spread" % worst))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["abd", "c"], default="abd")
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
        (part_c_child if a.child == "c" else part_abd_child)(a)
        return 0
    try:
        if a.part == "c":
            return part_c(a)
        child(a, "abd")
        return 0
    except subprocess.TimeoutExpired:
        print("where_expr: a measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
