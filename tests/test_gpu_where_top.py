"""GPU: ordered top-k over boolean filters (include/bmx_where_agg.h bmx_where_top). Every answer is compared exactly — records in order, n_out and n_eligible —
with the numpy model of where_agg_model.py (watch_model's mask, then top_select_model's lexsort by (value, id) behind the cursor), or with bmx_scan_top where
the two calls must agree.

The shapes are the smallest at which each piece can go wrong (csrc/where_agg_kernels.h k_where_top0, csrc/top_kernels.h): E = 4 (int32 column) or 2 (int64)
values per lane and load; a mask word is 32 positions, composed by 32 / E consecutive lanes; up to 4096 eligible rows need no digit pass, 4097 do; rows of one
value are told apart by id digits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import where_agg_model as wam
from oracle import streams
from where_agg_model import DATA, Model

FB, F1, F2, F3 = (streams.fnv1a32(s) for s in ("base", "one", "two", "three"))
FO = streams.fnv1a32("other")
NOBODY = streams.fnv1a32("nobody")
I64MIN, I64MAX = wam.I64MIN, wam.I64MAX
WIDE = 2**40
EVERY = [[(NOBODY, 0, 0, True)]]            # a negated literal on a field nobody has: true for every candidate


def _engine(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    return e


def _check(e, m, clauses, k, desc=False, after=None):
    got = e.where_top(FB, clauses, k, desc, after)
    want = wam.top(m, FB, clauses, k, desc, after)
    assert got[1] == want[2], (clauses, k, desc, after, got[1], want[2])
    assert len(got[0]) == len(want[0]) and np.array_equal(got[0]["id"], want[0]) and np.array_equal(got[0]["val"], want[1]), (clauses, k, desc, after)
    return got


def _model(n, seed, wide=False, top=300):
    rng = np.random.default_rng(seed)
    m = Model(wam.node_ids(n, 100 * seed))
    m.set(FB, np.arange(n), (WIDE if wide else 0) + rng.integers(-top, top, n))
    for f, pr in ((F1, 0.9), (F2, 0.6), (F3, 0.3)):
        idx = np.nonzero(rng.random(n) < pr)[0]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
    return m


def _programs(off):
    return [
        [[(F1, 1, 3), (F2, 2, 2, True)], [(F3, 0, 2), (FB, I64MIN, off + 10)]],      # an OR with a NOT
        [[(F1, 0, 5, True)]],                                                        # negated only: the nodes without F1
        [[(FB, off - 100, off + 100, True), (F2, I64MIN, I64MAX)]],                  # a negated literal on the order field
    ]


# ---- 1. against the model ----
@pytest.mark.parametrize("wide", [False, True])
def test_against_the_model(wide):
    m = _model(9000, 3 + wide, wide)
    with _engine(m, (FB, F1, F2, F3)) as e:
        wam.tombstone(e, m, F1, np.nonzero(m.st[F1] == DATA)[0][::7]); wam.tombstone(e, m, FB, np.arange(5, m.N, 31))
        off = WIDE if wide else 0
        for p in _programs(off):
            for desc in (False, True):
                for k in (1, 7, 4096):
                    recs, ne = _check(e, m, p, k, desc)
                    assert len(recs) == min(k, ne)
        # paging with k = 7 through a whole selection: the pages concatenate to the full order, no overlap, no gap, n_eligible falls by 7 per page
        p = [[(F3, 4, 5), (F1, 2, 2, True), (FB, off - 50, off + 50)], [(FB, off + 290, I64MAX)]]
        for desc in (False, True):
            ids, vals, total = wam.top(m, FB, p, m.N, desc)
            assert 30 < total < 400
            cur, pages, left = None, [], total
            while True:
                recs, ne = _check(e, m, p, 7, desc, cur)
                assert ne == left
                if not len(recs):
                    break
                pages.append(recs); left -= len(recs)
                cur = (int(recs[-1]["id"]), int(recs[-1]["val"]))
            walked = np.concatenate(pages)
            assert left == 0 and np.array_equal(walked["id"], ids) and np.array_equal(walked["val"], vals)
            assert all(len(x) == 7 for x in pages[:-1])


# ---- 2. equality with bmx_scan_top ----
@pytest.mark.parametrize("wide", [False, True])
def test_one_positive_clause_is_scan_top(wide):
    m = _model(9000, 7 + wide, wide)
    off = WIDE if wide else 0
    with _engine(m, (FB, F1, F2, F3)) as e:
        wam.tombstone(e, m, F2, np.nonzero(m.st[F2] == DATA)[0][::5])
        for terms in ([(FB, off - 250, off + 200)], [(FB, off - 300, off + 300), (F1, 1, 4)], [(FB, off + 3, off + 9), (F1, 0, 5), (F2, 0, 3)], [(FB, I64MIN, I64MAX), (F3, 0, 5)]):
            for desc in (False, True):
                for k, after in ((5, None), (4096, None), (300, (int(m.ids[11]), int(m.val[FB][11]))), (300, (2**63, off))):
                    a_recs, a_ne = e.where_top(FB, [terms], k, desc, after)
                    b_recs, b_ne = e.scan_top(terms, k, desc, after)
                    assert a_ne == b_ne and np.array_equal(a_recs, b_recs), (terms, desc, k, after)
                    assert wam.top_equals((a_recs, a_ne), wam.top(m, FB, [terms], k, desc, after))
            assert e.where_top(FB, [terms], 5)[1] > 0


# ---- 3. beyond the candidate list ----
def test_beyond_the_candidate_list():
    """10000 rows all eligible through a negated literal: the digit passes run. 5000 rows of one value: the id passes. Exactly 4096 and 4097 eligible."""
    rng = np.random.default_rng(31)
    m = Model(wam.node_ids(10000, 5100))
    m.set(FB, np.arange(10000), rng.integers(-(2**20), 2**20, 10000))
    with _engine(m, (FB,)) as e:
        for desc in (False, True):
            for k in (1, 100, 4096):
                assert _check(e, m, EVERY, k, desc)[1] == 10000
            _check(e, m, EVERY, 4096, desc, (int(m.ids[3]), int(m.val[FB][3])))
    m = Model(wam.node_ids(5000, 5200))
    m.set(FB, np.arange(5000), np.full(5000, 77))
    m.set(F1, np.arange(5000), np.arange(5000) % 2)
    with _engine(m, (FB, F1)) as e:
        for desc in (False, True):
            assert _check(e, m, EVERY, 4096, desc)[1] == 5000
            assert _check(e, m, [[(F1, 0, 0)], [(F1, 1, 1)]], 9, desc)[1] == 5000
            _check(e, m, EVERY, 50, desc, (int(np.sort(m.ids)[450]), 77))
    for n_elig in (4096, 4097):
        m = Model(wam.node_ids(6000, 5300 + n_elig))
        m.set(FB, np.arange(6000), rng.integers(0, 50, 6000))
        m.set(F1, np.arange(n_elig), np.ones(n_elig, np.int64))         # the others have no F1
        with _engine(m, (FB, F1)) as e:
            for p in ([[(F1, 1, 1)]], [[(F1, 1, 1), (FB, 0, 20)], [(F1, 0, 0, True), (F1, I64MIN, I64MAX), (FB, 21, 49)]]):
                for desc in (False, True):
                    recs, ne = _check(e, m, p, 4096, desc)
                    assert ne == n_elig and len(recs) == 4096


# ---- 4. mask words ----
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65])
def test_mask_words(n, wide):
    """eligibility that alternates per position and per group of 32 / E lanes (8 int32 or 16 int64 lanes: 32 positions either way), read back by the passes
    behind pass 0 — with more than 4096 eligible rows elsewhere the digit passes and the compaction read every word. Here n is small, so the compaction reads
    the mask; the patterns make a wrongly composed word show as a wrong set."""
    m = Model(wam.node_ids(n, 6000 + n + 1000 * wide))
    m.set(FB, np.arange(n), (WIDE if wide else 0) + (np.arange(n) * 7) % 13)
    with _engine(m, (FB,)) as e:
        node = m.index_of(e.index_ids(FB))                              # node[pos]: the pattern is laid over POSITIONS
        pos = np.arange(n)
        E = 2 if wide else 4
        pats = {"odd": pos % 2 == 1, "even": pos % 2 == 0, "per lane": (pos // E) % 2 == 0, "per word": (pos // 32) % 2 == 1, "first": pos == 0, "last": pos == n - 1,
                "word edges": (pos % 32 == 31) | (pos % 32 == 0)}
        for name, on in pats.items():
            m.set(F1, node[on], np.ones(int(on.sum()), np.int64))
            m.set(F1, node[~on], np.zeros(int((~on).sum()), np.int64))
            e.put_rows(*m.rows(F1, 10 + list(pats).index(name)))
            for p in ([[(F1, 1, 1)]], [[(F1, 0, 0, True)]]):
                for desc in (False, True):
                    recs, ne = _check(e, m, p, 4096, desc)
                    assert ne == int(on.sum()) and set(recs["id"].tolist()) == set(m.ids[node[on]].tolist()), (n, wide, name)


def test_mask_words_behind_the_digit_passes_and_a_stale_mask():
    """9000 rows, eligibility alternating per position, per lane group and per word, more than 4096 eligible: k_top_digit and k_top_compact read the words that
    k_where_top0 composed. Then a stale mask: this large query, a scan_range on another index (it writes the same mask scratch), and a query on a smaller index."""
    n = 9000 + 13
    big = Model(wam.node_ids(n, 6500))
    big.set(FB, np.arange(n), (np.arange(n) * 11) % 1000)
    big.set(FO, np.arange(n), np.arange(n) % 50)
    small = Model(wam.node_ids(200, 6600))
    small.set(FB, np.arange(200), np.arange(200) % 9)
    small.set(F1, np.arange(0, 200, 3), np.ones(67, np.int64))
    with _engine(big, (FB, FO)) as e, _engine(small, (FB, F1)) as e2:
        node = big.index_of(e.index_ids(FB))
        pos = np.arange(n)
        for k, on in enumerate(((pos % 2 == 1) | (pos % 64 < 3), (pos // 4) % 2 == 0, ((pos // 32) % 2 == 1) | (pos % 5 == 0))):
            big.set(F1, node[on], np.ones(int(on.sum()), np.int64)); big.set(F1, node[~on], np.zeros(int((~on).sum()), np.int64))
            e.put_rows(*big.rows(F1, 20 + k))
            assert on.sum() > 4097
            for desc in (False, True):
                assert _check(e, big, [[(F1, 1, 1)]], 4096, desc)[1] == int(on.sum())
                _check(e, big, [[(F1, 1, 1)], [(FB, 0, 2)]], 100, desc, (int(big.ids[5]), 500))
        # a stale mask on one engine: a large query, a scan_range on another index, then a query on a smaller index
        FS = streams.fnv1a32("small")
        big.set(FS, np.arange(150), np.arange(150) % 4)
        e.load_rows(*big.rows(FS, 30))
        assert e.index_size(FS) == 150
        prog = [[(F1, 1, 1)], [(FO, 7, 7)]]
        for desc in (False, True):
            _check(e, big, EVERY, 4096, desc)
            assert len(e.scan_range(FO, 0, 24)) == int((big.val[FO] <= 24).sum())
            got = e.where_top(FS, prog, 4096, desc)
            want = wam.top(big, FS, prog, 4096, desc)
            assert wam.top_equals(got, want) and 0 < want[2] < 150
            _check(e, big, [[(FB, 0, 0), (F1, 1, 1)]], 4096, desc)
        # another engine, another scratch
        _check(e2, small, [[(F1, 1, 1)]], 4096); _check(e2, small, [[(F1, 1, 1, True)]], 4096)


# ---- 5. cursor ties ----
@pytest.mark.parametrize("wide", [False, True])
def test_cursor_ties(wide):
    """a cursor whose value equals a row's value: the tie is settled by id — for a program that probes and for one that does not; and cursors that name no row"""
    n = 600
    off = WIDE if wide else 0
    m = Model(wam.node_ids(n, 7700 + wide))
    m.set(FB, np.arange(n), off + np.arange(n) % 5)                     # tie groups of 120
    m.set(F1, np.arange(n), np.arange(n) % 3)
    with _engine(m, (FB, F1)) as e:
        for p in ([[(FB, off, off + 3)], [(FB, off + 4, off + 4)]], [[(F1, 0, 1)], [(F1, 2, 2, True), (FB, off + 4, I64MAX)]], EVERY):
            for desc in (False, True):
                ids, vals, total = wam.top(m, FB, p, n, desc)
                for j in (0, 1, 119, 120, 121, total - 2, total - 1):                       # existing rows: the answer starts right behind them
                    recs, ne = _check(e, m, p, 10, desc, (int(ids[j]), int(vals[j])))
                    assert ne == total - j - 1
                tie = off + 2
                group = np.sort(m.ids[(m.val[FB] == tie) & m.mask(FB, p)])
                for cid in (0, int(group[0]) - 1, int(group[0]) + 1, int(group[60]) + 1, int(group[-1]) + 1, 2**64 - 2):   # ids that no row of the value has
                    _check(e, m, p, 10, desc, (cid, tie))
                for cv in (off - 1, off + 5, -(2**53 - 1), 2**53 - 1):                      # values no row has
                    _check(e, m, p, 10, desc, (12345, cv))
