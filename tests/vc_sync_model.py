"""What the vector-clock reconciliation tests share (test_vc_sync_cabi.py, test_gpu_vc_sync.py, test_gpu_vc_sync_kernel_edges.py): the generator of two
replicas' histories, the model's rows as records, and the numpy restatements every device answer is compared with — exact equality throughout.
No GPU is touched here unless a check is handed an engine."""
import numpy as np

import bmx
from bmx import synth
from oracle.oracle import OracleVC

M64 = (1 << 64) - 1
GUARD = 8
FILL = 0x5A5A5A5A5A5A5A5A                                     # what a device vector holds before a digest writes into it
REC_ID, REC_AUX = 0xABABABABABABABAB, 0xCDCDCDCD              # what a record holds before an export writes into it
LS = (0, 1, 5, 10, 11, 16)                                    # digests asked of every table
DEVICE = "cuda"


def key_ids(rows):
    return synth.splitmix64_np(np.asarray(rows, np.uint64) + np.uint64(1))


def rand_keysets(rng, clocks, K, full=0.0):
    """random ordered subsets of the K writers; counters of the writers a clock does not name are zeroed in place"""
    n = len(clocks)
    ks = np.zeros(n, np.uint32)
    for j in range(n):
        order = rng.permutation(K)
        cnt = K if rng.random() < full else int(rng.integers(0, K + 1))
        keys = order[:cnt].tolist()
        mask = np.zeros(K, bool); mask[keys] = True
        clocks[j, ~mask] = 0
        ks[j] = bmx.keyset(keys)
    return ks


def replica_merges(seed, who, K=3, merges=3, n=400, nids=150, nfields=2):
    """The history of replica `who` (0 or 1) under `seed`: `merges` batches of n deltas over nids ids x nfields fields; every clock names a random subset of
    the K writers in random order with components 0..3; values -5..5. -> [(id, field, clocks, val, keysets)]"""
    rng = np.random.default_rng(7919 * seed + who)
    out = []
    for _ in range(merges):
        ids = key_ids(rng.integers(0, nids, n))
        fields = np.array([synth.field_hash(int(x)) for x in rng.integers(0, nfields, n)], np.uint32)
        clocks = rng.integers(0, 4, (n, K)).astype(np.uint32)
        val = rng.integers(-5, 6, n).astype(np.int64)
        ks = rand_keysets(rng, clocks, K)
        out.append((ids, fields, clocks, val, ks))
    return out


def recs_of(id, field, clocks, val, keysets, state):
    id = np.asarray(id, np.uint64)
    r = np.zeros(len(id), bmx.VC_REC_DTYPE)
    r["id"], r["field"], r["val"], r["keyset"], r["state"] = id, field, val, keysets, state
    if len(id):
        c = np.asarray(clocks, np.uint32).reshape(len(id), -1)
        r["clock"][:, :c.shape[1]] = c
    return r


def by_key(recs):
    return recs[np.lexsort((recs["field"], recs["id"]))]


def model_rows(o):
    """an OracleVC's rows as VC_REC_DTYPE records sorted by (id, field): dump_rows for the keys, get_rows for clocks, values, key sets and states"""
    id, field, _, _ = o.dump_rows()
    clocks, val, st, ks = o.get_rows(id, field)
    assert (st != bmx.VC_ABSENT).all()
    return by_key(recs_of(id, field, clocks, val, ks, st))


def merge_recs(o, recs):
    """OracleVC.merge_batch over the records' columns -> (flags, updated)"""
    return o.merge_batch(recs["id"], recs["field"], np.ascontiguousarray(recs["clock"][:, :o.K]), recs["val"], keysets=recs["keyset"])


def same(got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = got != want
    bad = np.flatnonzero(ne.reshape(len(got), int(np.prod(got.shape[1:]))).any(1)) if got.ndim > 1 else np.flatnonzero(ne)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def same_recs(got, want, what):
    assert got.dtype == bmx.VC_REC_DTYPE and want.dtype == bmx.VC_REC_DTYPE
    for col in bmx.VC_REC_DTYPE.names:
        same(got[col], want[col], (what, col))


def rows_digest(recs):
    return bmx.vc_rows_digest(recs["id"], recs["field"], recs["clock"], recs["keyset"], recs["state"], recs["val"])


def np_digest(recs, L):
    """numpy group-by: (sums, counts) per bucket of a row set"""
    d = rows_digest(recs)
    b = bmx.key_bucket(recs["id"], recs["field"], L).astype(np.int64)
    sums = np.zeros(1 << L, np.uint64); counts = np.zeros(1 << L, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(sums, b, d)
    np.add.at(counts, b, np.uint64(1))
    return sums, counts


def np_frontier(recs):
    return recs["clock"].max(0).astype(np.uint32) if len(recs) else np.zeros(8, np.uint32)


def beyond(recs, frontier, K):
    """the rows a frontier does not dominate: some clock[k] > frontier[k], k < K"""
    f = np.zeros(8, np.uint32); f[:len(frontier)] = frontier
    return (recs["clock"][:, :K] > f[:K]).any(1)


# ---- checks against an engine (GPU) ----

def _torch():
    import torch
    return torch


def check_digest(e, recs, Ls=LS):
    """digest(L) into host memory and into device vectors full of garbage, against the numpy group-by of the model's rows"""
    torch = _torch()
    for L in Ls:
        B = 1 << L
        want = np_digest(recs, L)
        sums, counts = e.digest(L)
        same(sums, want[0], ("digest sums", L)); same(counts, want[1], ("digest counts", L))
        assert int(counts.sum()) == e.row_count() == len(recs)
        ds = torch.full((B + GUARD,), FILL, dtype=torch.int64, device=DEVICE); dc = torch.full((B + GUARD,), FILL, dtype=torch.int64, device=DEVICE)
        torch.cuda.synchronize()
        e.digest_dev(L, ds, dc); e.sync()
        hs, hc = ds.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint64)
        same(hs[:B], want[0], ("digest sums, device", L)); same(hc[:B], want[1], ("digest counts, device", L))
        assert (hs[B:] == np.uint64(FILL)).all() and (hc[B:] == np.uint64(FILL)).all(), ("nothing behind 2^L is written", L)


def check_frontier(e, recs):
    torch = _torch()
    want = np_frontier(recs)
    same(e.frontier(), want, "frontier")
    d = torch.full((8 + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=DEVICE)
    torch.cuda.synchronize()
    e.frontier_dev(d); e.sync()
    h = d.cpu().numpy().view(np.uint32)
    same(h[:8], want, "frontier, device")
    assert (h[8:] == 0x5A5A5A5A).all()
    return want


def guarded(k):
    g = np.zeros(k, bmx.VC_REC_DTYPE)
    g["id"] = REC_ID; g["aux"] = REC_AUX; g["val"] = -1; g["state"] = 0x77; g["keyset"] = 0x12345678; g["clock"] = 0xEEEEEEEE
    return g


def untouched(g, what):
    same_recs(g, guarded(len(g)), (what, "nothing behind min(n, cap) is written"))


def queries(recs, K, frontier):
    """(arguments of export_rows, mask over recs of the rows they select): bucket bits, frontiers, both"""
    n = len(recs)
    out = [(dict(), np.ones(n, bool))]
    for L in (0, 5, 10, 16):
        bk = bmx.key_bucket(recs["id"], recs["field"], L)
        words = max(1, (1 << L) // 64)
        out.append((dict(log2_buckets=L, bucket_bits=np.zeros(words, np.uint64)), np.zeros(n, bool)))
        out.append((dict(log2_buckets=L, bucket_bits=np.full(words, M64, np.uint64)), np.ones(n, bool)))
        b = int(bk[n // 2]) if n else (1 << L) - 1
        out.append((dict(log2_buckets=L, bucket_bits=bmx.bucket_bits_of([b], L)), bk == b))
    frs = [np.zeros(8, np.uint32), frontier.copy()]
    for k in range(K):
        if frontier[k]:
            f = frontier.copy(); f[k] -= 1
            frs.append(f)
    for f in frs:
        out.append((dict(frontier=f), beyond(recs, f, K)))
    f = frs[-1]
    bk = bmx.key_bucket(recs["id"], recs["field"], 4)
    sel = beyond(recs, f, K)
    b = int(bk[np.flatnonzero(sel)[0]]) if sel.any() else 3
    out.append((dict(frontier=f, log2_buckets=4, bucket_bits=bmx.bucket_bits_of([b], 4)), sel & (bk == b)))
    return out


def check_export(e, recs, K, frontier, ordered=True, caps=True):
    """recs: the model's rows in the order the table holds them (ordered=True: compared record for record) or sorted by key (compared as sets).
    Every query; device-resident bucket bits; then the caps, into pageable memory, page-locked memory and device memory."""
    torch = _torch()
    fix = (lambda r: r) if ordered else by_key
    qs = queries(recs, K, frontier)
    for kw, m in qs:
        got, n = e.export_rows(**kw)
        assert n == int(m.sum()) == len(got), (kw, n, int(m.sum()))
        same_recs(fix(got), recs[m], kw)
    d_n = torch.zeros(1, dtype=torch.int64, device=DEVICE)
    bq = [q for q in qs if "bucket_bits" in q[0]]
    for kw, m in bq[2:12:3] + [bq[0], bq[-1]]:                  # device bits: one bucket at every L, nothing, and the one under a frontier
        k = int(m.sum())
        d_bits = torch.from_numpy(kw["bucket_bits"].view(np.int64).copy()).to(DEVICE)
        d_out = torch.from_numpy(guarded(k + GUARD).view(np.int64)).to(DEVICE)
        d_n.fill_(-1); torch.cuda.synchronize()
        e.export_rows_dev(d_out, k, d_n, **dict(kw, bucket_bits=d_bits)); e.sync()
        h = d_out.cpu().numpy().view(bmx.VC_REC_DTYPE)
        assert int(d_n.item()) == k, (kw, "device bits")
        same_recs(fix(h[:k]), recs[m], (kw, "device bits")); untouched(h[k:], (kw, "device bits"))
    if not caps:
        return
    n = len(recs)
    full, nn = e.export_rows()
    assert nn == n
    for cap in sorted({0, 1, n - 1, n, n + 1} - {-1}):
        k = min(n, cap)
        g = guarded(cap + GUARD)                                # pageable memory: through the staging buffer, which the ascending caps make grow
        got, nn = e.export_rows(out=g[:cap])
        assert nn == n and len(got) == k, (cap, "the count is the full one")
        same_recs(g[:k], full[:k], (cap, "pageable")); untouched(g[k:], (cap, "pageable"))
        hb = bmx.HostBuffer(64 * (cap + GUARD))                 # page-locked memory: the kernel writes the records where the caller wants them
        a = hb.array(bmx.VC_REC_DTYPE, cap + GUARD)
        a[:] = guarded(cap + GUARD)
        got, nn = e.export_rows(out=a[:cap])
        assert nn == n and len(got) == k
        same_recs(a[:k], full[:k], (cap, "page-locked")); untouched(a[k:], (cap, "page-locked"))
        del a, got; hb.close()
        d_out = torch.from_numpy(guarded(cap + GUARD).view(np.int64)).to(DEVICE)
        d_n.fill_(-1); torch.cuda.synchronize()
        e.export_rows_dev(d_out, cap, d_n); e.sync()
        h = d_out.cpu().numpy().view(bmx.VC_REC_DTYPE)
        assert int(d_n.item()) == n, (cap, "device count")
        same_recs(h[:k], full[:k], (cap, "device")); untouched(h[k:], (cap, "device"))
