"""GPU: the K-writer vector-clock path's own kernels (csrc/vc_kernels.h: k_vc_link, k_vc_resolve, k_vc_resolve_long; csrc/bmx_vc.inc: ensure(), and its
use of k_compact_winners) at their list-length, chunk, bitmap, queue, winner-block and workspace edges — batches built by construction, not drawn.

Every check is exact equality against oracle.oracle.OracleVC (the CPU restatement of the reference's resolve() for general clocks, itself pinned to the
real reference's goldens by the non-GPU suite): for EVERY merged batch the per-delta flags, the ascending `updated` list, row_count() and every touched
row read back with its key set (counters, value, sparse/dense state, key order). No tolerance, no sample.

A batch is a list of (key, member indices) and a size n (_build); every index no row names gets a key of its own. Only clocks (counters 0..3) and values
(-2..2) are random. Which path a row takes — preload, in-lane selection (at most VC_SHORT = 16 deltas) or the queue of k_vc_resolve_long —, how many
256-delta chunks it has, how many rows are queued, the workspace's cap after the engine's earlier calls, how many bitmap words a lane scans, the last lane
with work and the bitmap words two queued rows share are computed from the inputs alone (_paths) and asserted per batch, never read off the answer.
tests/test_vc_kernel_edges_model.py runs the same scenarios without a GPU: the claims, that rows were built as meant, and that every case's inputs
produce every flag value.

Two things the shapes force: {0..16} and "17 indices with stride n // 17 including 0 and n - 1" both hold index 0, so the bitmap batches come in two
layouts (a: first word, 31 / 32, the batch's end, the words beyond 16 384; b: the strided row) that follow each other; and at n = 4 097 the second
4096-delta block is the single index 4 096, so a row's other deltas always lie in another 256-delta block than its winner but in another 4096-delta block
only when the winner is index 4 096; the batch with a whole 4096-delta block of winners (n = 4 353) has the long row's other deltas in the second block."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from oracle import streams
from oracle.oracle import OracleVC

VC_SHORT, CHUNK, LONG_WGS, MIN_CAP = 16, 256, 64, 1 << 14     # vc_kernels.h VC_SHORT, the 256-delta stage of k_vc_resolve_long, VC_LONG_WGS; bmx_vc.inc ensure()
F = (streams.field_hash(0), streams.field_hash(1))
FILLER = 1 << 24                  # key numbers of the rows that fill a batch: FILLER + index
INC, CUR, HIST, CONC = bmx.FLAG_INCOMING, bmx.FLAG_CURRENT, bmx.FLAG_HISTORICAL, bmx.FLAG_CONCURRENT
ALL_FLAGS = {0, INC, CUR, CUR | HIST, CONC}
PAT32, PAT8 = 0x5A5A5A5A, 0xA5    # what a device output buffer holds before a batch writes into it


def _ids(keys):
    keys = np.asarray(keys, np.uint64)
    return streams.splitmix64_np(keys + np.uint64(1)), np.where(keys & np.uint64(1), F[1], F[0]).astype(np.uint32)


def _same(got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1)) if len(got) else []
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


# ---- batches by construction ----

def _keysets(rng, clocks):
    """random ordered subsets of the K writers (three in ten name all K), as key-set words; the counters of the writers a clock does not name are zeroed in place"""
    n, K = clocks.shape
    order = np.argsort(rng.random((n, K)), axis=1)
    cnt = np.where(rng.random(n) < 0.3, K, rng.integers(0, K + 1, n))
    ks = np.full(n, 0xFFFFFFFF, np.uint64)
    named = np.zeros((n, K), bool)
    for i in range(K):
        use = i < cnt
        w = order[:, i].astype(np.uint64)
        ks = np.where(use, (ks & np.uint64(~(0xF << (4 * i)) & 0xFFFFFFFF)) | (w << np.uint64(4 * i)), ks)
        named[np.flatnonzero(use), order[use, i]] = True
    clocks[~named] = 0
    return ks.astype(np.uint32)


def _build(rng, n, rows, K, keysets=False, load=False):
    """rows: [(key number, member indices)]. Every other index of the n is a row of its own (key FILLER + index). Clocks 0..3, values -2..2."""
    owner = np.full(n, -1, np.int64)
    for key, mem in rows:
        mem = np.asarray(mem, np.int64)
        assert len(mem) and len(np.unique(mem)) == len(mem) and mem.min() >= 0 and mem.max() < n and 0 <= key < FILLER, (key, n)
        assert (owner[mem] == -1).all(), ("two rows name one index", key)
        owner[mem] = key
    free = np.flatnonzero(owner < 0)
    owner[free] = FILLER + free
    ids, fields = _ids(owner)
    clocks = rng.integers(0, 4, (n, K)).astype(np.uint32)
    val = rng.integers(-2, 3, n).astype(np.int64)
    ks = _keysets(rng, clocks) if keysets else None
    return NS(n=n, K=K, ids=ids, fields=fields, clocks=clocks, val=val, ks=ks, load=load,
              rows=[(int(k), np.sort(np.asarray(m, np.int64))) for k, m in rows])


def _again(b, rng=None):
    """the same keys and clocks once more; with rng: under new values"""
    c = NS(**vars(b)); c.clocks = b.clocks.copy(); c.val = b.val.copy() if rng is None else rng.integers(-2, 3, b.n).astype(np.int64)
    return c


def _dominate(b, j, level=4):
    """delta j's clock names all K writers at `level`: above every drawn counter"""
    b.clocks[j] = level
    if b.ks is not None:
        b.ks[j] = bmx.keyset(range(b.K))


def _strided(r, R, m, n):
    """m indices congruent to r modulo R, from r to as near n - 1 as an even stride allows: rows with different r never meet"""
    step = ((n - 1 - r) // R) // max(m - 1, 1)
    assert step >= 1 or m == 1
    return r + R * step * np.arange(m)


def _scattered(n, mult, p=1237):
    """disjoint index sets of the sizes `mult` out of 0..n-1, each spread over the whole batch: consecutive runs of the sequence i * p mod n (p and n coprime)"""
    assert np.gcd(p, n) == 1 and sum(mult) <= n
    perm = (np.arange(n, dtype=np.int64) * p) % n
    cut = np.concatenate([[0], np.cumsum(mult)])
    return [np.sort(perm[cut[i]:cut[i + 1]]) for i in range(len(mult))]


# ---- which path every row of a batch takes (inputs only) ----

def _cap_after(sizes):
    """ensure(): the workspace holds max(n, 16384) rounded up to 256 for the largest n so far and never shrinks"""
    cap = 0
    for n in sizes:
        if n > cap:
            cap = (max(n, MIN_CAP) + 255) & ~255
    return cap


def _paths(batch, history=()):
    """history: [(n, keys)] of the engine's earlier calls in order — n: the size ensure() saw, keys: the (id, field) pairs the call left resident (None: a read)."""
    n = batch.n
    order = np.lexsort((np.arange(n), batch.fields, batch.ids))
    sid, sf = batch.ids[order], batch.fields[order]
    start = np.flatnonzero(np.concatenate([[True], (sid[1:] != sid[:-1]) | (sf[1:] != sf[:-1])]))
    end = np.concatenate([start[1:], [n]])
    resident = set()
    for _, keys in history:
        if keys is not None:
            resident |= keys
    rows = {}
    words = {}
    for s, e in zip(start.tolist(), end.tolist()):
        m = e - s
        key = (int(sid[s]), int(sf[s]))
        mem = order[s:e]                      # ascending: lexsort's last key
        path = "preload" if batch.load else "short" if m <= VC_SHORT else "long"
        rows[key] = NS(m=m, path=path, chunks=-(-m // CHUNK), members=mem, resident=key in resident)
        if path == "long":
            for w in np.unique(mem >> 5).tolist():
                words.setdefault(w, []).append(key)
    cap = _cap_after([h[0] for h in history] + [n])
    bw = cap // 32
    per = -(-bw // 256)
    last_busy = -(-bw // per) - 1
    return NS(rows=rows, Q=sum(r.path == "long" for r in rows.values()), cap=cap, bitmap_words=bw, per=per, last_busy=last_busy,
              first_idle=last_busy + 1 if last_busy < 255 else None, long_words=set(words), shared_words={w for w, k in words.items() if len(k) > 1})


def _claims(P, batch, expect):
    """the branch claims of one batch. rows: {key number: (m, path, resident)} for every row the batch was built from, exactly; and whichever of
    Q, chunks (sorted chunk counts of the queued rows), cap, per, lanes (last busy, first idle), words (bitmap words some queued row sets),
    shared ("all": every such word is set by two rows or more; "none"; a set: exactly these words are), shared_min (so many words at least are) the batch is about"""
    built = {int(k): m for k, m in batch.rows}
    for key, (m, path, res) in expect["rows"].items():
        i, f = _ids([key])
        r = P.rows[(int(i[0]), int(f[0]))]
        assert (r.m, r.path, r.resident) == (m, path, res), (key, r.m, r.path, r.resident, m, path, res)
        assert np.array_equal(r.members, built[key]), key
    assert set(expect["rows"]) == set(built), "a claim for every row the batch was built from"
    singles = sum(r.m == 1 for r in P.rows.values())
    assert len(P.rows) - singles == sum(len(m) > 1 for m in built.values()), "everything else is a row of one delta"
    if "Q" in expect:
        assert P.Q == expect["Q"], (P.Q, expect["Q"])
    if "chunks" in expect:
        assert sorted(r.chunks for r in P.rows.values() if r.path == "long") == sorted(expect["chunks"])
    for k in ("cap", "per"):
        if k in expect:
            assert getattr(P, k) == expect[k], (k, getattr(P, k), expect[k])
    if "lanes" in expect:
        assert (P.last_busy, P.first_idle) == expect["lanes"], (P.last_busy, P.first_idle, expect["lanes"])
    if "words" in expect:
        assert set(expect["words"]) <= P.long_words, (sorted(set(expect["words"]) - P.long_words))
    if expect.get("shared") == "all":
        assert P.long_words and P.shared_words == P.long_words
    if expect.get("shared") == "none":
        assert not P.shared_words
    if isinstance(expect.get("shared"), set):
        assert P.shared_words == expect["shared"], (sorted(P.shared_words), sorted(expect["shared"]))
    if "shared_min" in expect:
        assert len(P.shared_words) >= expect["shared_min"], (len(P.shared_words), expect["shared_min"])


def _expect_rows(batch, resident=()):
    path = lambda m: "preload" if batch.load else "short" if m <= VC_SHORT else "long"
    return {k: (len(m), path(len(m)), k in resident) for k, m in batch.rows}


# ---- one engine and its oracle, batch by batch ----

def _play(sc, gpu=True, dev=False):
    """every step of a scenario on a fresh engine and a fresh oracle; returns the oracle and [(batch, paths, flags, updated)] as the oracle has them.
    gpu=False: the oracle and the claims alone. dev: merges go through merge_batch_dev with pre-filled device buffers."""
    o = OracleVC(sc.K, sc.local)
    e = bmx.EngineVC(max(4096, 2 * sum(s.batch.n for s in sc.steps)), sc.K, sc.local) if gpu else None
    history, out = [], []
    try:
        for si, st in enumerate(sc.steps):
            b = st.batch
            P = _paths(b, history)
            _claims(P, b, st.expect)
            touched = set(P.rows)
            tid = np.array([k[0] for k in P.rows], np.uint64); tf = np.array([k[1] for k in P.rows], np.uint32)
            if b.load:
                o.load_rows(b.ids, b.fields, b.clocks, b.val, keysets=b.ks)
                f2 = u2 = None
                if gpu:
                    e.load_rows(b.ids, b.fields, b.clocks, b.val, keysets=b.ks)
            else:
                f2, u2 = o.merge_batch(b.ids, b.fields, b.clocks, b.val, keysets=b.ks)
                if st.check:
                    st.check(b, f2, u2)
                if gpu and dev:
                    f1, u1 = _merge_dev(e, b, len(u2))
                elif gpu:
                    f1, u1 = e.merge_batch(b.ids, b.fields, b.clocks, b.val, keysets=b.ks)
                if gpu:
                    _same(f1, f2, (sc.name, si, "flags"))
                    _same(u1, u2, (sc.name, si, "updated"))
            history.append((b.n, touched))
            if gpu:
                assert e.row_count() == len(o), (sc.name, si, e.row_count(), len(o))
                got = e.get_rows(tid, tf, with_keysets=True)
                history.append((len(tid), None))
                want = o.get_rows(tid, tf)
                for g, w, what in zip(got, want, ("clock", "value", "state", "key set")):
                    _same(g, w, (sc.name, si, what))
            out.append((b, P, f2, u2))
    finally:
        if e is not None:
            e.close()
    return o, out


def _merge_dev(e, b, n_updated):
    import torch
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(x).to(dev) for x in (b.ids.view(np.int64), b.fields.view(np.int32), b.clocks.view(np.int32).reshape(-1), b.val)]
    ks = None if b.ks is None else torch.from_numpy(b.ks.view(np.int32)).to(dev)
    upd = torch.full((b.n + 8,), PAT32, dtype=torch.int32, device=dev); nu = torch.full((1,), PAT32, dtype=torch.int64, device=dev)
    fl = torch.full((b.n + 8,), PAT8, dtype=torch.uint8, device=dev)
    e.merge_batch_dev(b.n, *t, updated=upd, n_updated=nu, flags=fl, keysets=ks)
    e.sync()
    k = int(nu.item())
    assert k == n_updated, (k, n_updated)
    upd = upd.cpu().numpy(); fl = fl.cpu().numpy()
    assert (upd[k:] == PAT32).all(), "nothing behind n_updated entries of `updated` changes"
    assert (fl[b.n:] == PAT8).all()
    return fl[:b.n], upd[:k].view(np.uint32)


def _step(batch, expect, check=None):
    return NS(batch=batch, expect=expect, check=check)


# ---- 1. short / long threshold ----

THRESHOLD_M = (1, 2, 15, 16, 17, 18, 33)


def sc_threshold(K, local, keysets):
    """n = 2049; every multiplicity on an absent key (numbers 0..6) and on a preloaded one (10..16), strided over the whole batch; then the same batch again"""
    rng = np.random.default_rng(1000 + 10 * K + keysets)
    n = 2049
    R = 2 * len(THRESHOLD_M)
    rows = [(i, _strided(i, R, m, n)) for i, m in enumerate(THRESHOLD_M)] + [(10 + i, _strided(7 + i, R, m, n)) for i, m in enumerate(THRESHOLD_M)]
    for _, mem in rows:
        assert len(mem) == 1 or len(np.unique(mem >> 8)) > 1, "every list crosses 256-delta blocks"
    pre = _build(rng, 7, [(10 + i, [i]) for i in range(7)], K, keysets, load=True)
    b = _build(rng, n, rows, K, keysets)
    res = set(range(10, 17))
    ex = dict(rows=_expect_rows(b, res), Q=6, chunks=[1] * 6, cap=MIN_CAP)
    ex2 = dict(ex, rows=_expect_rows(b, res | set(range(7))))
    assert [ex["rows"][i][1] for i in range(7)] == ["short"] * 4 + ["long"] * 3
    return NS(name="threshold K=%d%s" % (K, " keysets" if keysets else ""), K=K, local=local,
              steps=[_step(pre, dict(rows=_expect_rows(pre), Q=0)), _step(b, ex), _step(_again(b), ex2)])


# ---- 2. chunk edges ----

CHUNK_M = (255, 256, 257, 511, 512, 513, 769)


def _chunk_rows(n):
    return list(zip(range(len(CHUNK_M)), _scattered(n, CHUNK_M)))


def sc_chunks(K, local, keysets):
    """n = 4097: rows of 255 .. 769 deltas scattered over the batch, on absent keys, then (new clocks and values) on the rows that exist by then"""
    rng = np.random.default_rng(2000 + K)
    n = 4097
    rows = _chunk_rows(n)
    b1 = _build(rng, n, rows, K, keysets); b2 = _build(rng, n, rows, K, keysets)
    ex = dict(rows=_expect_rows(b1), Q=7, chunks=[1, 1, 2, 2, 2, 3, 4], cap=MIN_CAP, shared_min=128)        # all but the word of index 4096
    return NS(name="chunks K=%d%s" % (K, " keysets" if keysets else ""), K=K, local=local,
              steps=[_step(b1, ex), _step(b2, dict(ex, rows=_expect_rows(b2, set(range(7)))))])


def sc_chunk_barrier():
    """K = 3. The rows are preloaded with the clock 0 and the value 2; every delta has the clock 0 (it leaves the row alone: flags 0 or CURRENT, then
    CURRENT | HISTORICAL) except, in index order, each row's 256th [1,0,0], 257th [0,1,0], 512th [2,0,0], 513th [0,2,0] and 769th [0,0,1] where it has one.
    Each of them updates, and each is concurrent with or ahead of all before it: the final clock names every one that was applied to the state the chunk
    before it left. Of the 257-row only the 256th and the 257th delta update."""
    K, local = 3, 2
    rng = np.random.default_rng(2500)
    n = 4097
    rows = _chunk_rows(n)
    pre = _build(rng, 7, [(k, [k]) for k in range(7)], K, load=True)
    pre.clocks[:] = 0; pre.val[:] = 2
    b = _build(rng, n, rows, K)
    special = {255: [1, 0, 0], 256: [0, 1, 0], 511: [2, 0, 0], 512: [0, 2, 0], 768: [0, 0, 1]}
    crafted = {}
    for k, mem in b.rows:
        b.clocks[mem] = 0
        for p, c in special.items():
            if p < len(mem):
                b.clocks[mem[p]] = c; crafted.setdefault(k, []).append(int(mem[p]))

    def check(b, flags, upd):
        for k, mem in b.rows:
            updating = mem[(flags[mem] & (INC | CONC)) != 0].tolist()
            assert updating == crafted.get(k, []), (k, updating, crafted.get(k))
        assert set(upd.tolist()) >= {c[-1] for c in crafted.values()} and not set(upd.tolist()) & set(b.rows[0][1].tolist())

    res = set(range(7))
    return NS(name="chunk barrier", K=K, local=local,
              steps=[_step(pre, dict(rows=_expect_rows(pre), Q=0)),
                     _step(b, dict(rows=_expect_rows(b, res), Q=7, chunks=[1, 1, 2, 2, 2, 3, 4], cap=MIN_CAP), check)])


# ---- 3. bitmap geometry ----

def _geometry_batch(rng, n, layout, K, resident):
    """layout "a": {0..16}, 23..39 (across 31 / 32), the last 17 indices, and where the batch reaches that far 16384..16400 (the first word a workspace of
    16384 did not have); layout "b": i * (n // 17) for i < 16 and n - 1, and a second row on the index beside each of these (the same words, bit by bit)"""
    if layout == "a":
        rows = [(0, np.arange(17)), (1, np.arange(23, 40)), (2, np.arange(n - 17, n))]
        if n >= MIN_CAP + 34:
            rows.append((3, np.arange(MIN_CAP, MIN_CAP + 17)))
        words = {0, 1, (n - 1) >> 5, (n - 17) >> 5} | ({MIN_CAP >> 5} if n >= MIN_CAP + 34 else set())
    else:
        strided = np.concatenate([np.arange(16) * (n // 17), [n - 1]])
        rows = [(4, strided), (5, np.concatenate([strided[:16] + 1, [n - 2]]))]
        words = {0, (n - 1) >> 5}
    b = _build(rng, n, rows, K)
    ex = dict(rows=_expect_rows(b, resident), Q=len(rows), chunks=[1] * len(rows), words=words)
    if layout == "a":
        ex["shared"] = {0}                    # 0..16 and 23..31
    else:
        ex["shared_min"] = min(15, (n - 1) >> 5)
    return b, ex


GEOMETRY = {16384: dict(cap=16384, per=2, lanes=(255, None)), 16385: dict(cap=16640, per=3, lanes=(173, 174)), 65537: dict(cap=65792, per=9, lanes=(228, 229))}


def sc_geometry(sizes):
    """a fresh engine; for every size the layout a, then b. The claims follow the LARGEST size so far: the workspace never shrinks"""
    K, local = 3, 1
    rng = np.random.default_rng(3000 + sum(sizes))
    steps, resident, top = [], set(), 0
    for i, n in enumerate(sizes):
        top = max(top, n)
        for layout in ("a", "b") if len(sizes) <= 1 else ("ab"[i % 2],):
            b, ex = _geometry_batch(rng, n, layout, K, resident)
            ex.update(GEOMETRY[top] if top in GEOMETRY else dict(cap=MIN_CAP, per=2, lanes=(255, None)))
            steps.append(_step(b, ex))
            resident |= {k for k, _ in b.rows}
    return NS(name="geometry %s" % "-".join(map(str, sizes)), K=K, local=local, steps=steps)


GEOMETRY_SEQUENCE = (300, 16384, 16385, 300, 65537, 16385, 65537)      # a b a b a b a: both layouts at the regrown sizes


# ---- 4. queue depth and bitmap reuse ----

def _queue_batch(rng, Q, K, resident, extra=0):
    """Q rows of 17, row r at r, r + Q, r + 2Q, ...: every bitmap word is shared by up to 32 rows. extra: one more row, in the middle of the round robin,
    that goes on alone for `extra` deltas more"""
    R = Q + (1 if extra else 0)
    rows = [(r, r + R * np.arange(17)) for r in range(R)]
    if extra:
        r = R // 2
        rows[r] = (r, np.concatenate([rows[r][1], 17 * R + np.arange(extra)]))
    n = 17 * R + extra + 7
    b = _build(rng, n, rows, K)
    chunks = [1] * Q + ([-(-(17 + extra) // CHUNK)] if extra else [])
    return b, dict(rows=_expect_rows(b, resident), Q=R, chunks=chunks, cap=MIN_CAP, **(dict(shared_min=17 * R // 32) if extra else dict(shared="all" if R > 1 else "none")))


def sc_queue(Q, Q2, extra=0):
    K, local = 3, 0
    rng = np.random.default_rng(4000 + Q + extra)
    b1, ex1 = _queue_batch(rng, Q, K, set(), extra)
    b2, ex2 = _queue_batch(rng, Q2, K, {k for k, _ in b1.rows})
    return NS(name="queue %d%s then %d" % (Q, "+1 of %d" % (17 + extra) if extra else "", Q2), K=K, local=local, steps=[_step(b1, ex1), _step(b2, ex2), _step(_again(b2, rng), dict(ex2, rows=_expect_rows(b2, {k for k, _ in b1.rows + b2.rows})))])


QUEUE = [(1, 65), (63, 64), (64, 129), (65, 63), (128, 1), (129, 128)]


# ---- 5. where the winner sits ----

WINNER_AT = (0, 255, 256, 4095, 4096)


def _winner_rows(n, ws, wl):
    """a short row (key 0) of 9 deltas with index ws among them and a long row (key 1) of 40 with wl; all their other deltas in 256-delta blocks 3..14"""
    short = np.concatenate([[ws], 800 + 97 * np.arange(8)])
    long_ = np.concatenate([[wl], 1500 + 55 * np.arange(39)])
    for w, mem in ((ws, short), (wl, long_)):
        assert not ((mem[1:] >> 8) == (w >> 8)).any() and mem[1:].min() >= 768 and mem[1:].max() < 3840
    return [(0, short), (1, long_)]


def sc_winner(i):
    """n = 4097, both rows resident; the short row's dominating delta at WINNER_AT[i], the long row's at WINNER_AT[i + 1]; then the same batch under new values
    (the winners now find their own clock: json-identical, the value decides)"""
    K, local = 3, 1
    ws, wl = WINNER_AT[i], WINNER_AT[(i + 1) % len(WINNER_AT)]
    rng = np.random.default_rng(5000 + i)
    pre = _build(rng, 2, [(0, [0]), (1, [1])], K, load=True)       # resident: a first delta on an absent row would store {local: 2}, not its own clock
    b = _build(rng, 4097, _winner_rows(4097, ws, wl), K, keysets=bool(i & 1))
    _dominate(b, ws); _dominate(b, wl)

    def check(b, flags, upd):
        assert flags[ws] == INC and flags[wl] == INC and {ws, wl} <= set(upd.tolist())
        for w, (_, mem) in zip((ws, wl), b.rows):
            assert set(upd.tolist()) & set(mem.tolist()) == {w}
            assert (flags[mem[mem > w]] == CUR | HIST).all()

    ex = dict(rows=_expect_rows(b, {0, 1}), Q=1, chunks=[1], cap=MIN_CAP)
    return NS(name="winner short@%d long@%d" % (ws, wl), K=K, local=local,
              steps=[_step(pre, dict(rows=_expect_rows(pre), Q=0)), _step(b, ex, check), _step(_again(b, rng), ex)])


def sc_all_lose():
    """both rows are resident under a clock above every delta's: no delta of theirs updates, none is in `updated`"""
    K, local = 3, 1
    rng = np.random.default_rng(5100)
    pre = _build(rng, 2, [(0, [0]), (1, [1])], K, load=True)
    pre.clocks[:] = 4
    b = _build(rng, 4097, _winner_rows(4097, 255, 4096), K)

    def check(b, flags, upd):
        mem = np.concatenate([m for _, m in b.rows])
        assert (flags[mem] == CUR | HIST).all() and not set(upd.tolist()) & set(mem.tolist())
        assert len(upd) == b.n - len(mem), "every other delta creates its row"

    return NS(name="all lose", K=K, local=local,
              steps=[_step(pre, dict(rows=_expect_rows(pre), Q=0)), _step(b, dict(rows=_expect_rows(b, {0, 1}), Q=1, chunks=[1], cap=MIN_CAP), check)])


def sc_full_block():
    """n = 4353: every delta of the first 4096-delta block wins — 4095 new rows of one delta and, at index 2047, the dominating delta of a resident long row
    whose other 39 deltas lie in the second block"""
    K, local = 3, 1
    rng = np.random.default_rng(5200)
    w = 2047
    pre = _build(rng, 1, [(1, [0])], K, load=True)
    b = _build(rng, 4353, [(1, np.concatenate([[w], 4096 + 6 * np.arange(39)]))], K)
    _dominate(b, w)

    def check(b, flags, upd):
        assert np.array_equal(upd[:4096], np.arange(4096)) and len(upd) == b.n - 39

    return NS(name="full block", K=K, local=local,
              steps=[_step(pre, dict(rows=_expect_rows(pre), Q=0)), _step(b, dict(rows=_expect_rows(b, {1}), Q=1, chunks=[1], cap=MIN_CAP), check)])


# ---- 6. preload lists ----

PRELOAD_M = (1, 2, 16, 17, 256, 5000)


def sc_preload(keysets):
    """one load_rows call of 5300 rows in which six keys come 1 .. 5000 times (the highest index stays), then a merge over the same keys with a list of 17"""
    K, local = 3, 2
    rng = np.random.default_rng(6000 + keysets)
    n = 5300
    pre = _build(rng, n, list(zip(range(6), _scattered(n, PRELOAD_M))), K, keysets, load=True)
    m2 = (3, 17, 2, 1, 16, 40)
    b = _build(rng, 600, list(zip(range(6), _scattered(600, m2, p=7))), K, keysets)
    return NS(name="preload%s" % (" keysets" if keysets else ""), K=K, local=local,
              steps=[_step(pre, dict(rows=_expect_rows(pre), Q=0, cap=MIN_CAP)),
                     _step(b, dict(rows=_expect_rows(b, set(range(6))), Q=2, chunks=[1, 1], cap=MIN_CAP)),
                     _step(_again(b, rng), dict(rows=_expect_rows(b, set(range(6))), Q=2, chunks=[1, 1], cap=MIN_CAP))])


# ---- the scenarios by case (the model file walks this table) ----

THRESHOLD = [(1, 0, False), (1, 0, True), (3, 2, False), (3, 2, True), (8, 5, False), (8, 5, True)]
CHUNKS = [(3, 2, False), (8, 5, True)]
CASES = {
    "threshold": [lambda a=a: sc_threshold(*a) for a in THRESHOLD],
    "chunks": [lambda a=a: sc_chunks(*a) for a in CHUNKS] + [sc_chunk_barrier],
    "geometry": [lambda n=n: sc_geometry((n,)) for n in GEOMETRY] + [lambda: sc_geometry(GEOMETRY_SEQUENCE)],
    "queue": [lambda a=a: sc_queue(*a) for a in QUEUE] + [lambda: sc_queue(65, 64, extra=583)],
    "winner": [lambda i=i: sc_winner(i) for i in range(len(WINNER_AT))] + [sc_all_lose, sc_full_block],
    "preload": [lambda k=k: sc_preload(k) for k in (False, True)],
}


@pytest.mark.parametrize("K,local,keysets", THRESHOLD)
def test_lists_of_16_and_17_deltas_on_absent_and_resident_rows(K, local, keysets):
    _play(sc_threshold(K, local, keysets))


@pytest.mark.parametrize("K,local,keysets", CHUNKS)
def test_lists_of_255_to_769_deltas_at_the_256_delta_chunks(K, local, keysets):
    _play(sc_chunks(K, local, keysets))


def test_the_state_carried_from_one_chunk_to_the_next_decides_the_flags():
    _play(sc_chunk_barrier())


@pytest.mark.parametrize("n", list(GEOMETRY))
def test_bitmap_words_per_lane_on_a_fresh_engine(n):
    _play(sc_geometry((n,)))


def test_bitmap_in_a_workspace_that_regrows_twice_and_serves_smaller_batches():
    _play(sc_geometry(GEOMETRY_SEQUENCE))


@pytest.mark.parametrize("Q,Q2", QUEUE)
def test_queue_depths_around_the_64_workgroups_with_interleaved_rows(Q, Q2):
    _play(sc_queue(Q, Q2))


def test_queue_of_65_short_long_rows_and_one_of_600_between_them():
    _play(sc_queue(65, 64, extra=583))


@pytest.mark.parametrize("i", range(len(WINNER_AT)))
def test_winner_at_the_block_edges_of_resolve_and_compaction(i):
    _play(sc_winner(i))


def test_rows_whose_every_delta_loses_are_not_in_updated():
    _play(sc_all_lose())


def test_a_4096_delta_block_of_winners_with_a_long_rows_winner_among_them():
    _play(sc_full_block())


@pytest.mark.parametrize("keysets", [False, True])
def test_preload_lists_of_1_to_5000_then_a_merge(keysets):
    _play(sc_preload(keysets))


@pytest.mark.parametrize("which", ["chunks K=3", "chunks K=8 keysets", "queue 65"])
def test_device_pointer_entry_leaves_the_rest_of_its_buffers_alone(which):
    sc = {"chunks K=3": lambda: sc_chunks(3, 2, False), "chunks K=8 keysets": lambda: sc_chunks(8, 5, True), "queue 65": lambda: sc_queue(65, 63)}[which]()
    _play(sc, dev=True)
