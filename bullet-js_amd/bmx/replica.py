"""Replica reconciliation on top of bmx_digest / bmx_export_rows (include/bmx.h): find the key buckets in which two replicas differ and ship only those.

The reference's producer is _collectFullSyncData(since) (src/bullet-network-sync.js:592-664): everything modified since, plus every deleted entry, to
the peer that asked. Here the asking replica (`dst`) and the answering one (`src`) first compare per-bucket digests — tombstones included, so that a
deletion shows — and `src` exports the rows of the differing buckets only. The state join is the one the table already implements: per key the
lexicographic maximum of (ts, val), a tombstone being the smallest value (csrc/slot.h VAL_DELETED).

An endpoint is an Engine or a Comm. Nothing is computed here but the comparison of two digest vectors and the tombstones' clock test.
"""
import numpy as np

from . import Engine, EngineVC, INSERT_DELTA, MAX_BATCH, VAL_DELETED, VC_REC_DTYPE


def diff_buckets(dig_a, dig_b):
    """Two digests (sums, counts) of the same length 2^L -> the differing buckets as u64 bit words (bit b = word b // 64, bit b % 64; at least one word)."""
    sa, ca = (np.asarray(x, np.uint64) for x in dig_a)
    sb, cb = (np.asarray(x, np.uint64) for x in dig_b)
    if not (len(sa) == len(ca) == len(sb) == len(cb)) or len(sa) == 0 or len(sa) & (len(sa) - 1):
        raise ValueError("digests must have the same power-of-two length")
    d = (sa != sb) | (ca != cb)
    if len(d) < 64:
        d = np.concatenate([d, np.zeros(64 - len(d), bool)])
    return np.packbits(d, bitorder="little").view("<u8").astype(np.uint64)


def bucket_count(bits):
    return int(np.unpackbits(np.asarray(bits, np.uint64).view(np.uint8)).sum())


def _same_gpu(a, b):
    return isinstance(a, Engine) and isinstance(b, Engine) and a.device == b.device


def _merge_host(dst, recs):
    for o in range(0, len(recs), MAX_BATCH):
        r = recs[o:o + MAX_BATCH]
        cols = (np.ascontiguousarray(r["id"]), np.ascontiguousarray(r["field"]), np.ascontiguousarray(r["ts"]), np.ascontiguousarray(r["val"]))
        if isinstance(dst, Engine):
            dst.merge_batch(*cols, insert_mode=INSERT_DELTA, want_flags=False)
        else:
            dst.merge(*cols, insert_mode=INSERT_DELTA)


def _ship_device(dst, src, L, since, bits):
    """src's data rows of the chosen buckets -> dst, device to device: the records never leave the GPU. -> rows shipped"""
    import torch
    dev = torch.device("cuda", int(src.device))
    d_bits = torch.from_numpy(bits.view(np.int64)).to(dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    src.export_rows_dev(None, 0, d_n, since=since, log2_buckets=L, bucket_bits=d_bits)
    src.sync()
    n = int(d_n.item())
    if n == 0:
        return 0
    recs = torch.empty(4 * n, dtype=torch.int64, device=dev)          # n records of 32 bytes
    src.export_rows_dev(recs, n, d_n, since=since, log2_buckets=L, bucket_bits=d_bits)
    src.sync()                                                          # the engines run on streams of their own
    for o in range(0, n, MAX_BATCH):
        dst.merge_records_dev(min(MAX_BATCH, n - o), recs.data_ptr() + 32 * o, INSERT_DELTA)
    dst.sync()
    return n


def pull(dst, src, L=10, since=0):
    """Bring into `dst` what `src` has and `dst` lacks, for the buckets (2^L of them) whose digests differ: src's data rows with clock >= since are merged
    into dst (true last-writer-wins, BMX_INSERT_DELTA), then src's tombstones of those buckets are applied where their clock is strictly larger than
    dst's row (the merge refuses a tombstone as a value, so this part goes through get_rows / put_rows, as the host does for `deleted` sync entries).
    -> {buckets_differing, rows_shipped, tombstones_shipped, tombstones_applied}"""
    bits = diff_buckets(dst.digest(L, tombstones=True), src.digest(L, tombstones=True))
    out = {"buckets_differing": bucket_count(bits), "rows_shipped": 0, "tombstones_shipped": 0, "tombstones_applied": 0}
    if out["buckets_differing"] == 0:
        return out
    if _same_gpu(dst, src):
        out["rows_shipped"] = _ship_device(dst, src, L, since, bits)
    else:
        recs, n = src.export_rows(since=since, log2_buckets=L, bucket_bits=bits)
        _merge_host(dst, recs)
        out["rows_shipped"] = int(n)
    tomb, nt = src.export_rows(since=since, log2_buckets=L, bucket_bits=bits, only_tombstones=True)
    out["tombstones_shipped"] = int(nt)
    if nt:
        tid, tf, tts = np.ascontiguousarray(tomb["id"]), np.ascontiguousarray(tomb["field"]), np.ascontiguousarray(tomb["ts"])
        ts, _, found = dst.get_rows(tid, tf)
        keep = ~found | (tts > ts)
        k = int(keep.sum())
        if k:
            dst.put_rows(tid[keep], tf[keep], tts[keep], np.full(k, VAL_DELETED, np.int64))
        out["tombstones_applied"] = k
    return out


def reconcile(a, b, L=10, since=0):
    """pull both ways; afterwards a and b hold the join of their states. -> (pull(a <- b), pull(b <- a))"""
    return pull(a, b, L, since), pull(b, a, L, since)


# ---- the vector-clock table (include/bmx_vc_sync.h) ----

def _ship_device_vc(dst, src, L, frontier, bits):
    """src's rows of the chosen buckets -> dst, device to device: the 64-byte records never leave the GPU. -> (rows shipped, rows updated)"""
    import torch
    dev = torch.device("cuda", int(src.device))
    d_bits = torch.from_numpy(bits.view(np.int64)).to(dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    src.export_rows_dev(None, 0, d_n, frontier=frontier, log2_buckets=L, bucket_bits=d_bits)
    src.sync()
    n = int(d_n.item())
    if n == 0:
        return 0, 0
    recs = torch.empty(8 * n, dtype=torch.int64, device=dev)          # n records of 64 bytes
    src.export_rows_dev(recs, n, d_n, frontier=frontier, log2_buckets=L, bucket_bits=d_bits)
    src.sync()                                                          # the tables run on streams of their own
    updated = 0
    for o in range(0, n, MAX_BATCH):
        dst.merge_records_dev(min(MAX_BATCH, n - o), recs.data_ptr() + 64 * o, n_updated=d_n)
        dst.sync()
        updated += int(d_n.item())
    return n, updated


def pull_vc(dst, src, L=10, frontier=None):
    """Bring into `dst` (an EngineVC) what `src` has and `dst` holds differently, for the buckets (2^L of them) whose digests differ: src's rows of those
    buckets — with a frontier, only those whose clock exceeds it in some component — are merged into dst through its own resolve() (merge_records).
    Device to device when both tables are on one GPU, through host memory otherwise. -> {buckets_differing, rows_shipped, rows_updated}"""
    bits = diff_buckets(dst.digest(L), src.digest(L))
    out = {"buckets_differing": bucket_count(bits), "rows_shipped": 0, "rows_updated": 0}
    if out["buckets_differing"] == 0:
        return out
    if isinstance(dst, EngineVC) and isinstance(src, EngineVC) and dst.device == src.device:
        out["rows_shipped"], out["rows_updated"] = _ship_device_vc(dst, src, L, frontier, bits)
    else:
        recs, n = src.export_rows(frontier=frontier, log2_buckets=L, bucket_bits=bits)
        assert recs.dtype == VC_REC_DTYPE
        for o in range(0, len(recs), MAX_BATCH):
            out["rows_updated"] += len(dst.merge_records(recs[o:o + MAX_BATCH])[1])
        out["rows_shipped"] = int(n)
    return out


def reconcile_vc(a, b, L=10, rounds=3):
    """pull_vc(a <- b) then pull_vc(b <- a), round after round, until a round finds no differing bucket (at most `rounds`). The join is the reference's
    resolve(), whose first write stores {local: 2} instead of the incoming clock (src/bullet-crt.js:172-185): one round does not always equalise two tables.
    -> the per-round records [(pull_vc(a <- b), pull_vc(b <- a)), ...]; the tables are equal iff the last round's buckets_differing are both 0."""
    out = []
    for _ in range(int(rounds)):
        r = (pull_vc(a, b, L), pull_vc(b, a, L))
        out.append(r)
        if r[0]["buckets_differing"] == 0 and r[1]["buckets_differing"] == 0:
            break
    return out
