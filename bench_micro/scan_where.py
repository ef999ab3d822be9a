"""scan_where.py — what a boolean filter (include/bmx_where.h bmx_scan_where) costs beside the AND filter and beside one count-only sweep of the column.

  python bench_micro/scan_where.py [--out profiles/scan_where.log] [--rows 100000000] [--reps 20] [--warmup 3] [--limit 900] [--only-filter]

One index of --rows int32 rows (10^8; 10^7 where memory is short): a uniform base field (0 .. 2^30), a 16-valued field on every node, a 4-valued "role" on
three quarters of the nodes. In one process, HIP events on the engine's stream (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup;
every answer's count is checked against torch over the same columns before its time is printed.
  (1) a one-clause, two-term positive program against bmx_scan_filter with the same two terms, at 1 %, 10 % and 50 % selectivity of the first term: the same
      work, so the ratio should lie inside the repetition-to-repetition spread of scan_filter itself ((max - min) / median, printed next to it)
  (2) Example 8's shape (two positive literals and one negated probed literal) and a two-clause OR, each against one count-only sweep of the column
      (bmx_scan_count), ids delivered and count only
--only-filter times scan_filter alone. For the parent commit's times on the same box, copy this script into a checkout of that commit, build it there and run
it there with --only-filter (this tree's binding does not load a library without bmx_scan_where, so BMX_LIB_PATH is no route).
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/scan_where.log.
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


def measure(a):
    import torch
    import bmx
    from oracle import streams

    FU, FS, FR = streams.fnv1a32("uniform"), streams.fnv1a32("sixteen"), streams.fnv1a32("role")
    R = a.rows
    dev = torch.device("cuda", 0)
    e = bmx.Engine(3 * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    six = (mix(ids, 0x5851F42D4C957F2D) >> 8) & 15
    role = (mix(ids, 0x14057B7EF767814F) >> 8) & 3
    has_role = ((mix(ids, 0x369DEA0F31A53F85) >> 8) & 3) != 0
    def load(f, i, v):            # through the host in chunks of 16M rows, as bench_micro/big_index.py loads its table
        i = i.cpu().numpy().view(np.uint64); v = v.cpu().numpy()
        for lo in range(0, len(i), 16_000_000):
            m = min(16_000_000, len(i) - lo)
            e.load_rows(i[lo:lo + m], np.full(m, f, np.uint32), np.full(m, 5, np.int64), v[lo:lo + m])

    load(FU, ids, uni); load(FS, ids, six); load(FR, ids[has_role], role[has_role])
    e.sync()
    e.index_build(FU)
    if e.index_size(FU) != R:
        raise SystemExit("scan_where: the index holds %d of %d rows (table: %d rows)" % (e.index_size(FU), R, e.row_count()))
    say("== %d int32 rows (%.0f MB column), %s; %d timed calls after %d warm-ups, HIP events, device outputs ==" %
        (R, R * 4 / 1e6, os.environ.get("BMX_LIB_PATH") or "this tree's library", a.reps, a.warmup))
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_out = torch.zeros(R, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def flt(terms):
        arr = (bmx.Term * len(terms))(*[bmx.Term(int(f), 0, int(lo), int(hi)) for f, lo, hi in terms])
        return lambda: e._chk(e.L.bmx_scan_filter(e.h, len(terms), arr, bmx._ptr(d_out), R, bmx._ptr(d_n), bmx.MEM_DEVICE))

    for pct in (1, 10, 50):
        hi = ((1 << 30) * pct) // 100 - 1
        terms = [(FU, 0, hi), (FS, 3, 10)]
        want = int(((uni <= hi) & (six >= 3) & (six <= 10)).sum())
        tf = timed(e, flt(terms), a.reps, a.warmup)
        assert int(d_n.item()) == want
        spread = (tf.max() - tf.min()) / np.median(tf)
        say("(1) %2d %%: scan_filter, two terms            %s  spread %.3f  (%d matches)" % (pct, fmt(tf), spread, want))
        if not a.only_filter:
            tw = timed(e, lambda: e.scan_where_dev(FU, [terms], d_out, R, d_n), a.reps, a.warmup)
            assert int(d_n.item()) == want
            say("(1) %2d %%: scan_where, one clause, same terms %s  ratio to scan_filter %.3f" % (pct, fmt(tw), np.median(tw) / np.median(tf)))
    if not a.only_filter:
        tc = timed(e, lambda: e._chk(e.L.bmx_scan_count(e.h, FU, 0, (1 << 29) - 1, bmx._ptr(d_n), bmx.MEM_DEVICE)), a.reps, a.warmup)
        assert int(d_n.item()) == int((uni < (1 << 29)).sum())
        base = np.median(tc)
        say("(2) scan_count, half of the rows              %s  (%.2f TB/s)" % (fmt(tc), R * 4 / (base * 1e-3) / 1e12))
        hi30 = ((1 << 30) * 30) // 100 - 1
        ex8 = [[(FS, 0, 7), (FU, 0, hi30), (FR, 0, 0, True)]]                 # active && age < 30 && role != admin
        want8 = int(((six <= 7) & (uni <= hi30) & ~(has_role & (role == 0))).sum())
        or2 = [[(FS, 2, 2)], [(FS, 9, 9), (FR, 1, 2)]]
        want2 = int(((six == 2) | ((six == 9) & has_role & (role >= 1) & (role <= 2))).sum())
        for name, prog, want in (("Example 8 shape", ex8, want8), ("two-clause OR", or2, want2)):
            for out, cap, what in ((d_out, R, "ids"), (None, 0, "count only")):
                t = timed(e, lambda: e.scan_where_dev(FU, prog, out, cap, d_n), a.reps, a.warmup)
                assert int(d_n.item()) == want
                say("(2) %-16s %-10s                %s  %.2f x scan_count  (%d matches)" % (name, what, fmt(t), np.median(t) / base, want))
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
    ap.add_argument("--limit", type=int, default=900, help="seconds the measurement may take")
    ap.add_argument("--only-filter", action="store_true")
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
        print("scan_where: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
