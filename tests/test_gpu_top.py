"""GPU: ordered top-k queries with a keyset cursor (include/bmx_top.h bmx_scan_top). Every answer is compared exactly — records, n_out and n_eligible — with a
numpy model over the rows the test itself loaded: lexsort over (id, +-val) of the selected rows, the cursor applied, sliced to k.

The shapes are the smallest at which each piece can go wrong (csrc/top_kernels.h): a sweep's round is 512 lanes x 4 loads x 16 bytes = 8192 int32 rows (4096
int64 rows), a workgroup's share is four rounds = 32768 rows, the mask form (two terms and more) writes one 32-bit word per 8 (int32) or 16 (int64) lanes, the
candidate list holds 4096 rows: more eligible rows than that force digit passes, more rows of ONE value than that force id digits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
from oracle import streams
from helpers import load_golden

FA, FS, FO, FG = streams.fnv1a32("age"), streams.fnv1a32("score"), streams.fnv1a32("other"), streams.fnv1a32("grp")
VMAX = 2**53 - 1
CAND = 4096                # candidate capacity (TOP_CAND) == BMX_TOP_MAX_K
ROUND32, SHARE32 = 8192, 32768
ABSENT, DATA, TOMB = 0, 1, 2


class Model:
    """the table as the test loaded it: val[f][i], st[f][i] (ABSENT / DATA / TOMB) of node i"""

    def __init__(self, ids):
        self.ids = np.asarray(ids, np.uint64); self.N = len(self.ids); self.val = {}; self.st = {}

    def _f(self, f):
        if f not in self.val:
            self.val[f] = np.zeros(self.N, np.int64); self.st[f] = np.zeros(self.N, np.uint8)

    def set(self, f, idx, vals):
        self._f(f); self.val[f][idx] = vals; self.st[f][idx] = DATA

    def tomb(self, f, idx):
        self._f(f); self.st[f][idx] = TOMB

    def rows(self, f, ts):
        i = np.nonzero(self.st[f] == DATA)[0]
        return self.ids[i], np.full(len(i), f, np.uint32), np.full(len(i), ts, np.int64), self.val[f][i]

    def select(self, terms):
        sel = np.ones(self.N, bool)
        for f, lo, hi in terms:
            self._f(f)
            sel &= (self.st[f] == DATA) & (self.val[f] >= lo) & (self.val[f] <= hi)
        return sel

    def top(self, terms, k, desc=False, after=None):
        """-> (ids, vals of the first k eligible nodes in order, n_eligible)"""
        i = np.nonzero(self.select(terms))[0]
        ids, v = self.ids[i], self.val[terms[0][0]][i]
        key = -v if desc else v                         # |v| <= 2^53 - 1: exact
        if after is not None:
            aid, av = np.uint64(after[0]), int(after[1])
            # a cursor value anywhere in int64: compare in Python ints where the negation could overflow
            ak = -av if desc else av
            keep = np.array([(int(kk) > ak) or (int(kk) == ak and x > aid) for kk, x in zip(key, ids)], bool) if abs(av) > 2**62 else (key > ak) | ((key == ak) & (ids > aid))
            ids, v, key = ids[keep], v[keep], key[keep]
        o = np.lexsort((ids, key))[:k]
        return ids[o], v[o], len(ids)


def _check(e, m, terms, k, desc=False, after=None):
    recs, ne = e.scan_top(terms, k, desc=desc, after=after)
    wi, wv, wne = m.top(terms, k, desc, after)
    assert ne == wne, (terms, k, desc, after, ne, wne)
    assert len(recs) == min(k, wne) == len(wi), (terms, k, desc, after, len(recs), wne)
    bad = np.nonzero((recs["id"] != wi) | (recs["val"] != wv))[0]
    assert len(bad) == 0, (terms, k, desc, after, bad[:4], recs[bad[:4]], wi[bad[:4]], wv[bad[:4]])
    return recs, ne


def _ks(ne):
    return sorted({min(max(k, 1), bmx.TOP_MAX_K) for k in (1, ne - 1, ne, ne + 1, bmx.TOP_MAX_K)})


def _cursors(m, terms, desc):
    """a returned record, between two records, before everything, after everything"""
    wi, wv, ne = m.top(terms, 10**9, desc)
    if ne == 0:
        return [(0, 0), (2**64 - 1, VMAX)]
    mid = ne // 2
    big, small = 2**63 - 1, -(2**63)
    return [(int(wi[mid]), int(wv[mid])), (int(wi[mid]) + 1, int(wv[mid])), (0, int(wv[0])), (0, big if desc else small), (2**64 - 1, small if desc else big),
            (int(wi[-1]), int(wv[-1])), (int(wi[0]), int(wv[0]))]


def _engine_with(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    for f in fields:
        if (m.st[f] == DATA).any():
            e.load_rows(*m.rows(f, 5))
    return e


def _ids(n, salt=0):
    return streams.splitmix64_np(np.arange(1 + salt, n + 1 + salt, dtype=np.uint64))


# ---- sizes: the index's edges, a round and a workgroup's share +- 1 (odd sizes: the ragged last 16-byte unit), single-term and mask form ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, ROUND32 - 1, ROUND32 + 1, SHARE32 - 1, SHARE32, SHARE32 + 1])
def test_sizes_at_the_sweeps_edges(n):
    rng = np.random.default_rng(n)
    m = Model(_ids(n))
    m.set(FA, np.arange(n), rng.integers(-40, 60, n))          # ~100 values: every boundary lies inside a tie group
    m.set(FO, np.arange(n), rng.integers(0, 4, n))
    with _engine_with(m, (FA, FO)) as e:
        for terms in ([(FA, -40, 59)], [(FA, -10, 30)], [(FA, -40, 59), (FO, 1, 3)]):
            for desc in (False, True):
                ne = m.top(terms, 1, desc)[2]
                for k in _ks(ne):
                    _check(e, m, terms, k, desc)
                for cur in _cursors(m, terms, desc)[:4]:
                    _check(e, m, terms, 7, desc, cur)
        # the first and the last row of the column alone (the ragged unit's row is the last)
        for i in (0, n - 1):
            v = int(m.val[FA][i])
            got, _ = _check(e, m, [(FA, v, v)], bmx.TOP_MAX_K)
            assert m.ids[i] in got["id"]


def test_int64_column_at_its_round_and_the_mask_block():
    """the 8-byte column: a round is 4096 rows, a mask word 16 lanes; SCAN_BLOCK_ELEMS + 1 rows in the mask form"""
    for n in (4095, 4097, 8193, 16385):
        rng = np.random.default_rng(n)
        m = Model(_ids(n, 7))
        v = rng.integers(-50, 50, n); v[n // 2] = 2**40                    # one wide value: the index scans its int64 column
        m.set(FA, np.arange(n), v); m.set(FO, np.arange(n), rng.integers(0, 3, n))
        with _engine_with(m, (FA, FO)) as e:
            for terms in ([(FA, -VMAX, VMAX)], [(FA, -VMAX, VMAX), (FO, 0, 1)], [(FA, -20, 2**41), (FO, 2, 2)]):
                for desc in (False, True):
                    ne = m.top(terms, 1, desc)[2]
                    for k in _ks(ne):
                        _check(e, m, terms, k, desc)
                    for cur in _cursors(m, terms, desc)[:3]:
                        _check(e, m, terms, 100, desc, cur)


def test_empty_selections():
    n = 5000
    m = Model(_ids(n))
    m.set(FA, np.arange(n), np.arange(n) % 100); m.set(FO, np.arange(n), np.arange(n) % 7)
    with _engine_with(m, (FA, FO)) as e:
        idx = np.nonzero(m.val[FA] == 42)[0]
        e.put_rows(m.ids[idx], np.full(len(idx), FA, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), bmx.VAL_DELETED, np.int64))
        m.tomb(FA, idx)
        for terms in ([(FA, 50, 49)], [(FA, 42, 42)], [(FA, 200, 300)], [(FA, 0, 99), (FO, 5, 4)], [(FA, 0, 99), (FO, 70, 80)], [(FA, -2**63, -2**62)]):
            for desc in (False, True):
                for k in (1, 10, bmx.TOP_MAX_K):
                    recs, ne = _check(e, m, terms, k, desc)
                    assert ne == 0 and len(recs) == 0
        _check(e, m, [(FA, 0, 99)], 100, False, (2**64 - 1, 99))        # a cursor behind everything
        assert _check(e, m, [(FA, -2**63, 2**63 - 1)], bmx.TOP_MAX_K)[1] == n - len(idx), "a tombstoned term-0 row is never eligible"


@pytest.mark.parametrize("kind", ["all_equal", "two_values", "ends_of_the_domain", "around_zero"])
def test_ties_signs_and_the_bias(kind):
    rng = np.random.default_rng(5)
    if kind == "all_equal":           # candidate capacity + 1 rows of one value: nothing but id digits can tell them apart
        n = CAND + 1; v = np.full(n, 123456)
    elif kind == "two_values":        # the tie group of the larger value straddles every rank behind 3000
        n = 9000; v = np.where(np.arange(n) < 3000, -7, 11); rng.shuffle(v)
    elif kind == "ends_of_the_domain":
        n = 3 * CAND + 5; v = rng.choice(np.array([-VMAX, -VMAX + 1, -1, 0, 1, VMAX - 1, VMAX], np.int64), n)
    else:
        n = 2 * CAND + 3; v = rng.integers(-3, 4, n)
    m = Model(_ids(n, 100))
    m.set(FA, np.arange(n), v)
    with _engine_with(m, (FA,)) as e:
        T = [(FA, -VMAX, VMAX)]
        for desc in (False, True):
            for k in (1, 2, 2999, 3000, 3001, CAND - 1, CAND):
                _check(e, m, T, k, desc)
            for cur in _cursors(m, T, desc):
                _check(e, m, T, 50, desc, cur)             # a cursor whose value has more than k ties
                _check(e, m, T, CAND, desc, cur)
        if kind == "ends_of_the_domain":
            for lo, hi in ((-VMAX, -VMAX), (VMAX, VMAX), (-1, 1), (0, VMAX), (-VMAX, -1)):
                for desc in (False, True):
                    _check(e, m, [(FA, lo, hi)], CAND, desc)


def test_int32_column_then_int64_after_one_merge():
    n = 20_001
    rng = np.random.default_rng(6)
    m = Model(_ids(n, 3))
    m.set(FA, np.arange(n), rng.integers(-2**31 + 1, 2**31 - 1, n)); m.set(FO, np.arange(n), rng.integers(0, 5, n))
    cases = [([(FA, -VMAX, VMAX)], 100), ([(FA, -2**30, 2**30)], CAND), ([(FA, -VMAX, VMAX), (FO, 1, 2)], 333), ([(FA, 0, 2**40)], 1)]
    with _engine_with(m, (FA, FO)) as e:
        for t, k in cases:
            for desc in (False, True):
                _check(e, m, t, k, desc)
        wide = np.array([n // 3]); m.set(FA, wide, np.array([2**40]))
        e.merge_batch(m.ids[wide], [FA], [99], [2**40], want_flags=False)
        for t, k in cases:
            for desc in (False, True):
                _check(e, m, t, k, desc)
        got, ne = _check(e, m, [(FA, -VMAX, VMAX)], 3, True)
        assert got["val"][0] == 2**40
        e.reserve(16 * n)                                   # a growth: the index is rebuilt
        for t, k in cases:
            _check(e, m, t, k, True)


def _sparse_model(N, seed):
    """age on every node; score absent on a third; grp absent on a fifth; other on every node"""
    rng = np.random.default_rng(seed)
    m = Model(_ids(N, seed))
    allv = np.arange(N)
    m.set(FA, allv, rng.integers(0, 100, N))
    m.set(FS, allv[allv % 3 != 0], rng.integers(-100000, 100001, N)[allv % 3 != 0])
    m.set(FG, allv[allv % 5 != 0], rng.integers(-20, 1500, N)[allv % 5 != 0])
    m.set(FO, allv, rng.integers(0, 10, N))
    return m, rng


def _load_sparse(e, m, tomb_fs, tomb_fa):
    for f in (FA, FS, FG, FO):
        e.load_rows(*m.rows(f, 5))
    for f, idx in ((FS, tomb_fs), (FA, tomb_fa)):
        e.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), bmx.VAL_DELETED, np.int64))
        m.tomb(f, idx)


SPARSE_CASES = [
    ([(FA, 0, 99)], 20), ([(FA, 10, 40)], CAND), ([(FS, -500, 90000)], 100),
    ([(FA, 0, 99), (FO, 3, 3)], 500),                                   # a selective probed term
    ([(FA, 0, 99), (FO, 0, 9)], 500),                                   # an unselective one
    ([(FA, 0, 99), (FS, -10**6, 10**6)], CAND),                         # one that is absent (and tombstoned) on some nodes
    ([(FS, -50000, 50000), (FA, 20, 60), (FG, 0, 1200)], 777),          # three terms
    ([(FA, 5, 5), (FO, 0, 9), (FS, -10**6, 10**6), (FG, -20, 1500)], 64),
]


def test_terms_missing_and_tombstoned_rows():
    N = 40_000
    m, rng = _sparse_model(N, 7)
    tomb_fs = np.arange(1, N, 11); tomb_fs = tomb_fs[tomb_fs % 3 != 0]
    tomb_fa = np.arange(2, N, 97)
    with bmx.Engine(8 * N) as e:
        _load_sparse(e, m, tomb_fs, tomb_fa)
        for t, k in SPARSE_CASES:
            for desc in (False, True):
                _check(e, m, t, k, desc)
                for cur in _cursors(m, t, desc)[:3]:
                    _check(e, m, t, k, desc, cur)
        assert _check(e, m, [(FA, 0, 99)], 1)[1] == N - len(tomb_fa)


def _walk(e, m, terms, k, desc):
    """every page behind the last record of the one before -> all records"""
    want_i, want_v, total = m.top(terms, 10**9, desc)
    pages, cur, left = [], None, total
    while True:
        recs, ne = e.scan_top(terms, k, desc=desc, after=cur)
        assert ne == left and len(recs) == min(k, left), (len(pages), ne, left)
        if len(recs) == 0:
            break
        pages.append(recs); left -= len(recs); cur = recs[-1]
    got = np.concatenate(pages) if pages else np.zeros(0, bmx.TOP_DTYPE)
    assert len(got) == total and (got["id"] == want_i).all() and (got["val"] == want_v).all()
    assert len(np.unique(got["id"])) == total, "no node twice"
    return got


def _view_model(N=30_000, seed=21):
    rng = np.random.default_rng(seed)
    m = Model(_ids(N, seed))
    m.set(FA, np.arange(N), rng.integers(0, 30, N))                     # 30 values over 30 000 rows: tie groups of ~1000
    m.set(FO, np.arange(N), rng.integers(0, 3, N))
    return m, rng


def test_paging_walks_and_ties_in_the_three_view_states():
    """view of term 0's field off, on, and carrying a pending patch: identical answers, and the view's bookkeeping untouched by the top-k calls"""
    m, rng = _view_model()
    N = m.N
    walk_t = [(FA, 0, 9)]                                                # ~10 000 rows, k = 333
    ties = [([(FA, 0, 29)], 1500), ([(FA, 0, 29)], CAND), ([(FA, 3, 3)], 500), ([(FA, 0, 29), (FO, 1, 1)], 1200)]

    def run(e):
        out = [_walk(e, m, walk_t, 333, desc) for desc in (False, True)]
        for t, k in ties:
            for desc in (False, True):
                out.append(_check(e, m, t, k, desc)[0])
                out.append(_check(e, m, t, k, desc, _cursors(m, t, desc)[1])[0])
        return out

    def same(a, b):
        return len(a) == len(b) and all((x == y).all() for x, y in zip(a, b))

    with _engine_with(m, (FA, FO), 8 * N) as e:
        e.index_set_ordered(FA, 0)
        off = run(e)
        e.index_set_ordered(FA, 1)
        assert set(e.scan_range(FA, 0, 9).tolist()) == set(m.ids[m.select(walk_t)].tolist())
        assert e.index_ordered_info(FA)[1], "the view answers"
        s0 = e.index_ordered_stats(FA)
        assert same(run(e), off)
        assert e.index_ordered_stats(FA) == s0 and e.index_ordered_info(FA)[1], "the top-k calls leave the view as it was"
        assert set(e.scan_range(FA, 0, 9).tolist()) == set(m.ids[m.select(walk_t)].tolist())
        # a pending patch: new clocks on ~1 % of the field
        pick = rng.choice(N, N // 100, replace=False); nv = rng.integers(0, 30, len(pick))
        e.merge_batch(m.ids[pick], np.full(len(pick), FA, np.uint32), np.full(len(pick), 1000, np.int64), nv, want_flags=False)
        m.set(FA, pick, nv)
        patched = run(e)                                                 # (the first of them refreshes the index, which patches the view)
        s1 = e.index_ordered_stats(FA)
        assert s1["pending_keys"] > 0 and e.index_ordered_info(FA)[1], "the view carries a pending patch"
        assert same(run(e), patched)
        assert e.index_ordered_stats(FA) == s1, "the pending patch survives the top-k calls"
        assert set(e.scan_range(FA, 0, 9).tolist()) == set(m.ids[m.select(walk_t)].tolist()), "a scan behind a top-k is still right"
        assert e.index_ordered_stats(FA)["sorts"] == s1["sorts"]
        e.index_set_ordered(FA, 0)
        assert same(run(e), patched)


def test_device_memory_and_a_clean_scratch():
    N = 30_000
    m, rng = _sparse_model(N, 9)
    dev = torch.device("cuda", 0)
    FILL = 0x5A5A5A5A5A5A5A5A
    with bmx.Engine(8 * N) as e:
        _load_sparse(e, m, np.arange(1, N, 13), np.arange(2, N, 101))
        cases = [(t, k, desc) for t, k in SPARSE_CASES[:6] for desc in (False, True)]
        bufs = []
        for t, k, desc in cases:                                         # every query right behind the one before on the stream: no synchronisation in between
            out = torch.full((2 * k + 2,), FILL, dtype=torch.int64, device=dev)
            cnt = torch.full((3,), FILL, dtype=torch.int64, device=dev)
            bufs.append((out, cnt))
        torch.cuda.synchronize()
        for (t, k, desc), (out, cnt) in zip(cases, bufs):
            cur = _cursors(m, t, desc)[0]
            e.scan_top_dev(t, k, out, cnt[0:1], cnt[1:2], desc=desc, after=cur)
        e.sync()
        for (t, k, desc), (out, cnt) in zip(cases, bufs):
            cur = _cursors(m, t, desc)[0]
            wi, wv, wne = m.top(t, k, desc, cur)
            h = out.cpu().numpy(); c = cnt.cpu().numpy()
            assert int(c[0]) == len(wi) and int(c[1]) == wne and int(c[2]) == FILL
            recs = h[:2 * len(wi)].view(bmx.TOP_DTYPE)
            assert (recs["id"] == wi).all() and (recs["val"] == wv).all()
            assert (h[2 * len(wi):] == FILL).all(), "nothing behind the last record is written"
            host, hne = e.scan_top(t, k, desc=desc, after=cur)
            assert hne == wne and (host == recs).all(), "host mode and device mode agree"
        # the counts are optional
        out = torch.full((2 * 10,), FILL, dtype=torch.int64, device=dev)
        e.scan_top_dev([(FA, 0, 99)], 10, out)
        e.sync()
        wi, wv, _ = m.top([(FA, 0, 99)], 10)
        assert (out.cpu().numpy().view(bmx.TOP_DTYPE)["id"] == wi).all()


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    N = 30_000
    m, rng = _sparse_model(N, 10 + nshards)
    with bmx.Engine(8 * N) as e, bmx.Comm([0] * nshards, 8 * N) as c:
        for f in (FA, FS, FG, FO):
            e.load_rows(*m.rows(f, 5)); c.load_rows(*m.rows(f, 5))
        idx = np.arange(1, N, 13)
        tomb = (m.ids[idx], np.full(len(idx), FS, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), bmx.VAL_DELETED, np.int64))
        e.put_rows(*tomb); c.put_rows(*tomb); m.tomb(FS, idx)
        for t, k in SPARSE_CASES + [([(FA, 50, 49)], 10)]:
            for desc in (False, True):
                for cur in (None, _cursors(m, t, desc)[1]):
                    one, ne1 = e.scan_top(t, k, desc=desc, after=cur); many, ne2 = c.scan_top(t, k, desc=desc, after=cur)
                    wi, wv, wne = m.top(t, k, desc, cur)
                    assert ne1 == ne2 == wne and len(one) == len(many) == len(wi), (nshards, t, k, desc, cur)
                    assert (one == many).all() and (many["id"] == wi).all() and (many["val"] == wv).all(), (nshards, t, k, desc, cur)


# ---- the reference's dataset (oracle/gen_golden.js genQuerySeeded, restated) ----
def _nodes(N, seed):
    rng = streams.XorShift32(seed)
    ages = np.zeros(N, np.int64); scores = np.zeros(N, np.int64)
    for i in range(N):
        ages[i] = rng() % 100
        scores[i] = rng() % 200001 - 100000
    ids = np.array([streams.fnv1a32("n/k%d" % i) | (i << 32) for i in range(N)], dtype=np.uint64)
    ts = np.array([10 + (i % 7) for i in range(N)], np.int64)
    return ids, ts, ages, scores


def test_reference_dataset():
    g = load_golden("g5_query_seeded_2k.json")
    N = g["N"]
    ids, ts, ages, scores = _nodes(N, g["seed"])
    F = {"age": FA, "score": FS}
    seen = 0
    with bmx.Engine(4 * N) as e:
        e.merge_batch(np.concatenate([ids, ids]), np.concatenate([np.full(N, FA, np.uint32), np.full(N, FS, np.uint32)]), np.concatenate([ts, ts]),
                      np.concatenate([ages, scores]), want_flags=False)
        for q in g["queries"]:
            if q["op"] != "range":
                continue
            lo, hi = q["args"]
            recs, ne = e.scan_top([(F[q["field"]], lo, hi)], bmx.TOP_MAX_K)
            assert ne == q["count"] == len(recs), q["args"]
            assert sorted(recs["id"].tolist()) == sorted(int(ids[o]) for o in q["ordinals"]), q["args"]
            assert (np.diff(recs["val"]) >= 0).all(), "non-decreasing value order"
            seen += 1
    assert seen >= 5
