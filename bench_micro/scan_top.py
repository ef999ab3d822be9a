"""scan_top.py — what an ordered top-k query costs beside the scan that reads the same bytes (include/bmx_top.h).

  python bench_micro/scan_top.py [--out profiles/scan_top.log] [--reps 20] [--warmup 3] [--rows 100000000,10000000,10000000w]

Per entry of --rows (a trailing "w": one value beyond int32 makes the index scan its int64 column): R nodes with a uniform field (0 .. 2^30) and a
1000-valued field, built on the device. In one process, HIP events on the engine's stream (bmx_timer_*), device outputs, the median of the timed calls, every
answer checked against torch over the same columns before its time is printed:
  (a) bmx_scan_count over the same range (half of the rows): the one-read-of-the-column pass, the yardstick per sweep
  (b) single-term top-100 over the uniform field, ascending and descending
  (c) the same over the 1000-valued field: the boundary lies inside a tie group that the ids decide
  (d) a two-term top-100 (the second field probed; on up to --probe-rows nodes)
  (e) today's route for (b): scan_range + get_rows to the host + numpy lexsort, wall clock (up to --host-rows rows)
The sweeps a query needs are known from its digit positions: pass 0 + digit passes + compaction.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bullet-js_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bmx  # noqa: E402
from oracle import streams  # noqa: E402

FU, FK, FP = streams.fnv1a32("uniform"), streams.fnv1a32("thousand"), streams.fnv1a32("probed")
SIGN = -(1 << 63)
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


def torch_top(val, ids, sel, k, desc):
    """the first k of the selected rows by (val, id as uint64) — val descending with desc — and their number"""
    v = val[sel]; i = ids[sel]
    key = -v if desc else v
    n = int(v.numel())
    if n > k:
        kb = torch.kthvalue(key, k).values
        below = key < kb; eq = key == kb
        need = k - int(below.sum())
        ie = i[eq]
        order = torch.argsort(ie ^ SIGN)[:need]          # signed order of id ^ 2^63 = unsigned order of id
        i = torch.cat([i[below], ie[order]]); v = torch.cat([v[below], v[eq][order]])
    i = i.cpu().numpy().view(np.uint64); v = v.cpu().numpy()
    o = np.lexsort((i, -v if desc else v))
    return i[o], v[o], n


def check(buf, cnt, want):
    wi, wv, wn = want
    c = cnt.cpu().numpy()
    assert int(c[0]) == len(wi) and int(c[1]) == wn, (c, len(wi), wn)
    recs = buf.cpu().numpy()[:2 * len(wi)].view(bmx.TOP_DTYPE)
    assert (recs["id"] == wi).all() and (recs["val"] == wv).all()


def sweeps(spread, n_elig, ties_at_boundary):
    """pass 0 + digit passes + compaction for a selection of n_elig rows whose keys spread over `spread` values"""
    if n_elig <= 4096:
        return 2
    d, left, bits = 0, n_elig, max(int(spread - 1).bit_length(), 0)
    while bits > 0 and left > 4096:
        w = min(11, bits); bits -= w; d += 1
        left = max(left >> w, ties_at_boundary)
    while left > 4096:          # id digits
        left >>= 11; d += 1
    return 2 + d


def run(R, wide, a):
    dev = torch.device("cuda", 0)
    P = min(R, a.probe_rows)
    e = bmx.Engine(2 * R + P + 1000)
    ids = torch.arange(1, R + 1, dtype=torch.int64, device=dev) * -0x61c8864680b583eb - 0x0123456789ABCDEF      # odd multiplier: unique mod 2^64
    uni = (mix(ids, 0x2545F4914F6CDD1D) >> 8) & ((1 << 30) - 1)
    tho = (mix(ids, 0x5851F42D4C957F2D) >> 8) % 1000
    tho = torch.where(tho < 0, tho + 1000, tho)
    if wide:
        uni[R // 2] = 1 << 40; tho[R // 2] = 1 << 40
    pro = (mix(ids[:P], 0x14057B7EF767814F) >> 8) & 15
    ts = torch.full((R,), 5, dtype=torch.int64, device=dev)
    for f, n, v in ((FU, R, uni), (FK, R, tho), (FP, P, pro)):
        e.load_rows_dev(n, ids, torch.full((n,), f - (1 << 32) if f >= (1 << 31) else f, dtype=torch.int32, device=dev), ts, v.contiguous())
    e.sync()
    e.index_build(FU); e.index_build(FK)
    assert e.index_size(FU) == R and e.index_size(FK) == R
    w = 8 if wide else 4
    say("")
    say("== %d rows, %s column (%.0f MB); a probed field on %d nodes; %d timed calls after %d warm-ups, HIP events, device outputs ==" %
        (R, "int64" if wide else "int32", R * w / 1e6, P, a.reps, a.warmup))
    K = 100
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_out = torch.zeros(2 * K, dtype=torch.int64, device=dev)
    d_cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    hi_u = (1 << 29) - 1
    ta = timed(e, lambda: e._chk(e.L.bmx_scan_count(e.h, FU, 0, hi_u, bmx._ptr(d_n), bmx.MEM_DEVICE)), a.reps, a.warmup)
    sel_u = (uni >= 0) & (uni <= hi_u)
    assert int(d_n.item()) == int(sel_u.sum())
    base = np.median(ta)
    say("(a) scan_count, half of the rows              %s  (%.2f TB/s)" % (fmt(ta), R * w / (base * 1e-3) / 1e12))
    for desc in (False, True):
        tb = timed(e, lambda: e.scan_top_dev([(FU, 0, hi_u)], K, d_out, d_cnt[0:1], d_cnt[1:2], desc=desc), a.reps, a.warmup)
        want = torch_top(uni, ids, sel_u, K, desc)
        check(d_out, d_cnt, want)
        ns = sweeps(1 << 29, want[2], 1)
        say("(b) top-100, uniform field, %-4s             %s  %d sweeps expected: %.2f x (a) per sweep" % ("desc" if desc else "asc", fmt(tb), ns, np.median(tb) / base / ns))
    tak = timed(e, lambda: e._chk(e.L.bmx_scan_count(e.h, FK, 0, 499, bmx._ptr(d_n), bmx.MEM_DEVICE)), a.reps, a.warmup)
    sel_k = (tho >= 0) & (tho <= 499)
    assert int(d_n.item()) == int(sel_k.sum())
    for desc in (False, True):
        tc = timed(e, lambda: e.scan_top_dev([(FK, 0, 499)], K, d_out, d_cnt[0:1], d_cnt[1:2], desc=desc), a.reps, a.warmup)
        want = torch_top(tho, ids, sel_k, K, desc)
        check(d_out, d_cnt, want)
        ns = sweeps(500, want[2], want[2] // 500)
        say("(c) top-100, 1000-valued field, %-4s         %s  %d sweeps expected: %.2f x scan_count of that column (%.1f us) per sweep" %
            ("desc" if desc else "asc", fmt(tc), ns, np.median(tc) / np.median(tak) / ns, 1e3 * np.median(tak)))
    have = torch.zeros(R, dtype=torch.bool, device=dev); have[:P] = True
    pr = torch.zeros(R, dtype=torch.int64, device=dev); pr[:P] = pro
    sel_d = sel_u & have & (pr >= 3) & (pr <= 6)
    td = timed(e, lambda: e.scan_top_dev([(FU, 0, hi_u), (FP, 3, 6)], K, d_out, d_cnt[0:1], d_cnt[1:2]), a.reps, a.warmup)
    want = torch_top(uni, ids, sel_d, K, False)
    check(d_out, d_cnt, want)
    ns = sweeps(1 << 29, want[2], 1)
    say("(d) top-100, two terms (%d nodes pass both)  %s  %d sweeps expected (pass 0 also probes %d rows)" % (want[2], fmt(td), ns, int(sel_u.sum())))
    if R <= a.host_rows:
        e.sync()
        t0 = time.perf_counter()
        got = e.scan_range(FU, 0, hi_u)
        _, val, found = e.get_rows(got, np.full(len(got), FU, np.uint32))
        o = np.lexsort((got, val))[:K]; t1 = time.perf_counter()
        wi, wv, _ = torch_top(uni, ids, sel_u, K, False)
        assert (got[o] == wi).all() and (val[o] == wv).all() and bool(found.all())
        say("(e) scan_range + get_rows to the host + numpy lexsort: %.1f ms wall (%d ids)" % (1e3 * (t1 - t0), len(got)))
    else:
        say("(e) not run at this size (--host-rows %d)" % a.host_rows)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="100000000,10000000,10000000w")
    ap.add_argument("--probe-rows", type=int, default=10_000_000)
    ap.add_argument("--host-rows", type=int, default=10_000_000)
    a = ap.parse_args()
    for spec in a.rows.split(","):
        run(int(spec.rstrip("w")), spec.endswith("w"), a)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
