"""where_rows.py — what the row projection (include/bmx_rows.h bmx_where_rows) costs beside its floor, bmx_scan_where with ids of the same program (the same
sweep and the same id output), and beside the only route a program had before it: bmx_scan_where ids to the host, the same ids back for one bmx_get_rows per
field, the columns assembled in numpy.

  python bench_micro/where_rows.py [--out profiles/where_rows.log] [--rows 100000000] [--reps 20] [--warmup 3] [--limit 1100]

One table of --rows nodes (10^8; 10^7 where memory or time is short): a uniform int32 base field (0 .. 2^30) and eight int32 fields that every node holds, each
a function of the node id, so every delivered cell is checked on the device against the id beside it. In one process; every answer is checked (the ids against
bmx_scan_where's, in order; every value against the id's function; the record) before its time is printed.
  device : where_rows_dev with 0, 2 and 8 fields at 1 / 10 / 50 % selectivity next to scan_where_dev with ids; HIP events on the engine's stream
           (bmx_timer_*), device outputs, the median of --reps timed calls after --warmup, the spread (max - min) / median of the floor beside it. The
           2-field arm is run twice: with the first two projected fields loaded (their rows found room in the node's own 128-byte line of the table) and with
           the last two (nine rows per node want four slots: theirs were pushed into later lines, so a probe walks further).
  host   : with 2 fields, Engine.where_rows (BMX_MEM_HOST: synchronous, the columns end in numpy arrays) next to the route without this call — scan_where ids
           to the host, get_rows per field — both with the host's clock around the whole call, --reps calls after one.
The GPU work is one step, the measurement, and runs in a child process under --limit seconds: a measurement that hangs ends the script, and nothing is started
behind it. Recorded: profiles/where_rows.log.
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
NF = 8
CHUNK = 1 << 24          # rows per load (BMX_MAX_BATCH)


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


def host_timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ms.append(1e3 * (time.perf_counter() - t0))
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


def field_of(ids, k):
    """the value of projected field k on the nodes `ids` (int64 tensor or numpy array: the arithmetic wraps alike)"""
    return (mix(ids, 0x5851F42D4C957F2D + 2 * k) >> 8) & 0x3FFFFFFF


def measure(a):
    import torch
    import bmx
    from oracle import streams

    R = a.rows
    dev = torch.device("cuda", 0)
    FU = streams.fnv1a32("uniform")
    FP = [streams.fnv1a32("proj%d" % k) for k in range(NF)]
    e = bmx.Engine((1 + NF) * R + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    for f, k in [(FU, None)] + [(FP[k], k) for k in range(NF)]:
        for lo in range(0, R, CHUNK):
            m = min(CHUNK, R - lo)
            v = (uni[lo:lo + m] if k is None else field_of(ids[lo:lo + m], k)).contiguous()
            fcol = torch.full((m,), f if f < (1 << 31) else f - (1 << 32), dtype=torch.int32, device=dev)       # (the field id's 32 bits)
            tcol = torch.full((m,), 5, dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)          # torch filled the columns on its own stream; the engine reads them on its own
            e.load_rows_dev(m, ids[lo:lo + m], fcol, tcol, v)
            e.sync()                             # ... and is done with them before torch reuses their memory
    e.index_build(FU)
    if e.index_size(FU) != R:
        raise SystemExit("where_rows: the index holds %d of %d rows" % (e.index_size(FU), R))
    say("== %d rows (%.0f MB int32 column), %d projected fields on every node; %d timed calls after %d warm-ups ==" % (R, R * 4 / 1e6, NF, a.reps, a.warmup))
    cap = R // 2 + R // 50
    d_ids = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_ref = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_val = torch.zeros(NF * cap, dtype=torch.int64, device=dev)
    d_res = torch.zeros(5, dtype=torch.int64, device=dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    for pct in (1, 10, 50):
        hi = ((1 << 30) * pct) // 100 - 1
        prog = [[(FU, 0, hi)]]
        want = int((uni <= hi).sum().item())
        assert want <= cap
        say("-- %d %% of the rows (%d nodes) --" % (pct, want))
        tf = timed(e, lambda: e.scan_where_dev(FU, prog, d_ref, cap, d_n), a.reps, a.warmup)
        e.sync()
        assert int(d_n.item()) == want
        say("   device  scan_where ids (the floor)   %s  spread %.2f" % (fmt(tf), spread(tf)))
        t2 = None
        for nf, fields, tag in ((0, [], "0 fields          "), (2, FP[:2], "2 fields          "), (2, FP[NF - 2:], "the last 2 loaded "), (NF, FP, "8 fields          ")):
            first = FP.index(fields[0]) if nf else 0
            d_ids.zero_(); d_res.zero_()
            torch.cuda.synchronize(dev)
            t = timed(e, lambda: e.where_rows_dev(FU, prog, fields, cap, d_ids, d_val, None, d_res), a.reps, a.warmup)
            e.sync()
            r = d_res.cpu().numpy().view(bmx.ROWS_RES_DTYPE)[0]
            assert (int(r["n_match"]), int(r["n_out"]), int(r["next_pos"])) == (want, want, R), r
            assert torch.equal(d_ids[:want], d_ref[:want]), "the ids of bmx_scan_where, in order"
            for k in range(nf):
                assert torch.equal(d_val[k * cap:k * cap + want], field_of(d_ids[:want], first + k)), ("field", first + k)
            say("   device  where_rows %s %s  %.2f x the floor" % (tag, fmt(t), np.median(t) / np.median(tf)))
            if nf == 2 and t2 is None:
                t2 = t
        # host mode and the route without the call, two fields, the host's clock
        fields = FP[:2]
        got = {}

        def fused():
            got["r"] = e.where_rows(FU, prog, fields, cap=want)

        def route():
            h = e.scan_where(FU, prog, cap=want)
            cols = []
            for f in fields:
                _, val, found = e.get_rows(h, np.full(len(h), f, np.uint32))
                cols.append(np.where(found, val, bmx.VAL_DELETED))
            got["ids"], got["vals"] = h, np.stack(cols)

        th = host_timed(fused, a.reps)
        tr = host_timed(route, a.reps)
        assert np.array_equal(got["r"].ids, got["ids"]) and np.array_equal(got["r"].vals, got["vals"]), "the route's arrays"
        say("   host    where_rows 2 fields           %s  (host clock)" % fmt(th))
        say("   host    scan_where ids + get_rows x 2 %s  (host clock)  %.1f x the host-mode call, %.1f x the device-mode call" % (fmt(tr), np.median(tr) / np.median(th), np.median(tr) / np.median(t2)))
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
        print("where_rows: the measurement did not finish in %d s; nothing further is started" % a.limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
