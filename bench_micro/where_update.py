"""where_update.py — what the update by query (include/bmx_update.h bmx_where_update) costs beside the two calls it is made of and beside the only route a program
had before it: bmx_scan_where ids to the host, bmx_get_rows of the source field with those ids, arithmetic on the host, bmx_merge_batch with the ids going up
again.

  python bench_micro/where_update.py [--out profiles/where_update.log] [--rows 100000000] [--reps 20] [--warmup 3] [--limit 1100]

One table of --rows nodes (10^8; 10^7 where memory or time is short): a uniform int32 base field (0 .. 2^30) and a field `price` that every node holds, a function
of the node id. Two updates at 1 and 10 % selectivity, in pages of 2^22 records along the cursor: SET status = 7 and COPY price -> last_price. Every call carries
a clock above the last one's, so every record wins and is written. In one process; every answer is checked against torch (the record's counts against the
selection, the target field of every selected node read back with bmx_where_rows) before its time is printed.
  update : where_update_dev page after page (the record comes down between two pages: the cursor is host data); HIP events on the engine's stream (bmx_timer_*)
           around all pages, the median of --reps timed runs after --warmup.
  (a)    : where_rows_dev with 0 fields (SET) or the source field (COPY) at the same selectivity: the selection and the read of the source, unchanged code.
  (b)    : merge_records_dev of the same number of records (built by torch from the same ids) into the same table, in batches of 2^22: the write, unchanged
           code. The expectation the update is held against is (a) + (b) plus one wait per page.
  host   : the route that was there before, the host's clock around the whole of it.
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_update.log.
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
CHUNK = 1 << 24          # rows per load (BMX_MAX_BATCH)
PAGE = 1 << 22


def say(s):
    print(s, flush=True)
    LINES.append(s)


def fmt(ms):
    return "median %9.1f us  min %9.1f us  max %9.1f us" % (1e3 * np.median(ms), 1e3 * ms.min(), 1e3 * ms.max())


def mix(x, k):
    """a cheap 64-bit mix on the device (torch int64 arithmetic wraps)"""
    x = x * k
    x = x ^ ((x >> 29) & 0x7FFFFFFFF)
    x = x * -0x61c8864680b583eb
    return x ^ ((x >> 32) & 0xFFFFFFFF)


def price_of(ids):
    return (mix(ids, 0x5851F42D4C957F2D) >> 8) & 0x3FFFFFFF


def i32(f):
    return f if f < (1 << 31) else f - (1 << 32)


def measure(a):
    import torch
    import bmx
    from oracle import streams

    R = a.rows
    dev = torch.device("cuda", 0)
    FU, FP, FS, FL = (streams.fnv1a32(s) for s in ("uniform", "price", "status", "last_price"))
    e = bmx.Engine(2 * R + R // 4 + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    for f, col in ((FU, uni), (FP, None)):
        for lo in range(0, R, CHUNK):
            m = min(CHUNK, R - lo)
            v = (col[lo:lo + m] if col is not None else price_of(ids[lo:lo + m])).contiguous()
            fcol = torch.full((m,), i32(f), dtype=torch.int32, device=dev)
            tcol = torch.full((m,), 5, dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)          # torch filled the columns on its own stream; the engine reads them on its own
            e.load_rows_dev(m, ids[lo:lo + m], fcol, tcol, v)
            e.sync()                             # ... and is done with them before torch reuses their memory
    e.index_build(FU)
    if e.index_size(FU) != R:
        raise SystemExit("where_update: the index holds %d of %d rows" % (e.index_size(FU), R))
    say("== %d rows (%.0f MB int32 column), price on every node; pages of %d; %d timed runs after %d warm-ups ==" % (R, R * 4 / 1e6, PAGE, a.reps, a.warmup))
    cap = R // 10 + R // 50
    d_ids = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_val = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_rres = torch.zeros(5, dtype=torch.int64, device=dev)
    d_ures = torch.zeros(9, dtype=torch.int64, device=dev)
    d_out = torch.zeros(PAGE, dtype=torch.int64, device=dev)
    d_na = torch.zeros(1, dtype=torch.int64, device=dev)
    recs = torch.zeros((cap, 4), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    clock = [100]

    def timed(fn, reps, warmup):
        for _ in range(warmup):
            fn(False)
        e.sync()
        ms = []
        for _ in range(reps):
            ms.append(fn(True))
        return np.array(ms)

    for pct in (1, 10):
        hi = ((1 << 30) * pct) // 100 - 1
        prog = [[(FU, 0, hi)]]
        sel = uni <= hi
        want = int(sel.sum().item())
        assert want <= cap
        say("-- %d %% of the rows (%d nodes, %d pages) --" % (pct, want, -(-want // PAGE)))
        for name, target, op, operand, src, nf in (("SET status = 7        ", FS, bmx.UPD_SET, 7, None, []), ("COPY price -> last_price", FL, bmx.UPD_COPY, 0, FP, [FP])):
            tot = {}

            def update(clocked):
                clock[0] += 1
                if clocked:
                    e.timer_start()
                start, sent, applied, pages = 0, 0, 0, 0
                while True:
                    e.where_update_dev(FU, prog, target, op, PAGE, d_out, d_ures, operand=operand, src=src, ts=clock[0], start=start)
                    e.sync()
                    r = d_ures.cpu().numpy().view(bmx.UPD_RES_DTYPE)[0]
                    sent += int(r["n_sent"]); applied += int(r["n_applied"]); pages += 1
                    if pages == 1:
                        tot["n_match"] = int(r["n_match"])
                    if int(r["n_match"]) - int(r["n_nosrc"]) - int(r["n_range"]) <= int(r["n_sent"]):
                        break
                    start = int(r["next_pos"])
                tot["sent"], tot["applied"], tot["pages"] = sent, applied, pages
                return e.timer_stop() if clocked else 0.0

            # the answer first: the counts, then the target field of every selected node read back
            update(False)
            assert (tot["n_match"], tot["sent"], tot["applied"]) == (want, want, want), (tot, want)
            e.where_rows_dev(FU, prog, [target], cap, d_ids, d_val, None, d_rres)
            e.sync()
            assert int(d_rres.cpu().numpy().view(bmx.ROWS_RES_DTYPE)[0]["n_out"]) == want
            assert torch.equal(torch.sort(d_ids[:want])[0], torch.sort(ids[sel])[0]), "exactly the selected nodes"
            expect = torch.full((want,), operand, dtype=torch.int64, device=dev) if op == bmx.UPD_SET else price_of(d_ids[:want])
            assert torch.equal(d_val[:want], expect), "the target field of every selected node"
            tu = timed(update, a.reps, a.warmup)
            say("   device  where_update %s %s" % (name, fmt(tu)))

            def rows(clocked):
                if clocked:
                    e.timer_start()
                e.where_rows_dev(FU, prog, nf, cap, d_ids, d_val, None, d_rres)
                return e.timer_stop() if clocked else 0.0

            ta = timed(rows, a.reps, a.warmup)
            say("   device  (a) where_rows, %d field(s)              %s" % (len(nf), fmt(ta)))
            recs[:want, 0] = d_ids[:want]; recs[:want, 1] = target; recs[:want, 3] = expect
            torch.cuda.synchronize(dev)

            def merge(clocked):
                clock[0] += 1
                recs[:want, 2] = clock[0]
                torch.cuda.synchronize(dev)
                if clocked:
                    e.timer_start()
                for lo in range(0, want, PAGE):
                    e.merge_records_dev(min(PAGE, want - lo), recs[lo:], insert_mode=bmx.INSERT_DELTA, n_applied=d_na)
                ms = e.timer_stop() if clocked else 0.0
                e.sync()
                return ms

            tb = timed(merge, a.reps, a.warmup)
            e.sync()
            say("   device  (b) merge_records of as many records    %s" % fmt(tb))
            say("           where_update / ((a) + (b)) = %.2f" % (np.median(tu) / (np.median(ta) + np.median(tb))))

            def route():
                clock[0] += 1
                h = e.scan_where(FU, prog, cap=want)
                if op == bmx.UPD_SET:
                    vals = np.full(len(h), operand, np.int64)
                else:
                    _, vals, found = e.get_rows(h, np.full(len(h), src, np.uint32))
                    h, vals = h[found], vals[found]
                applied = 0
                for lo in range(0, len(h), CHUNK):
                    k = min(CHUNK, len(h) - lo)
                    applied += len(e.merge_batch(h[lo:lo + k], np.full(k, target, np.uint32), np.full(k, clock[0], np.int64), vals[lo:lo + k], insert_mode=bmx.INSERT_DELTA, want_flags=False)[0])
                assert applied == want

            route()
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); route(); ms.append(1e3 * (time.perf_counter() - t0))
            tr = np.array(ms)
            say("   host    scan_where ids + get_rows + merge_batch %s  (host clock)  %.1f x where_update" % (fmt(tr), np.median(tr) / np.median(tu)))
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
    ap.add_argument("--limit", type=int, default=1100, help="seconds the measurement may take")
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
        print("where_update: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
