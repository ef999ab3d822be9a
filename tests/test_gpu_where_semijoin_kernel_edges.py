"""GPU: the semi-join kernels at the edges of their geometry (csrc/semi_kernels.h PredSemi / k_semi_build, csrc/select.h k_scan_mask). One mask word is 32 rows
shared by 32 / E lanes (E = 4 int32 or 2 int64 values per lane and 16-byte load), a wave holds 2048 rows, a workgroup one 8192-row block. The outer program
selects every row, so what matches is decided by the LINK alone, row by row — by POSITION in the index: the link is the base column itself (`hit` is in the set,
`miss` is not) or a probed field loaded onto chosen positions. The inner side is a second column written the same way: which positions hold which key decides
the set. Both value widths (wide: every value beyond int32, so the index scans its int64 column). The 64-slot tables (32 keys with one home, a cluster that
wraps from slot 63 to 0, absent keys that walk a whole cluster, D = set_cap and set_cap + 1, 70 keys into 64 slots) are semi_model.table_edges, whose walks
test_semi_model.py pins on the stand-in."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import semi_model as sm
import where_agg_model as wam
from oracle import streams

FB, FL, FI, FK = (streams.fnv1a32(s) for s in ("semi.edge", "semi.edge.link", "semi.edge.inner", "semi.edge.key"))
BLOCK, WAVE, WORD = 8192, 2048, 32
SIZES = [1, 3, 31, 33, 2047, 2049, 8191, 8193, 2 * 8192 + 1]
EVERY = sm.EVERY


class Column:
    """an engine whose base column the test writes by position (hit / miss), with a link field FL on every position: 500 + (p % 3) on a hit position's turn —
    see set_hits — and 7 elsewhere; every fifth position's link is absent, every tenth tombstoned"""

    def __init__(self, n, wide, salt=0):
        self.n = n
        self.miss = (2**40 if wide else 0) + 7
        self.hit = self.miss + 1
        ids = streams.splitmix64_np(np.arange(1 + 70000 + salt + n, n + 1 + 70000 + salt + n, dtype=np.uint64))
        self.e = bmx.Engine(max(8 * n, 1024))
        self.ts = 10
        self.e.load_rows(ids, np.full(n, FB, np.uint32), np.full(n, 5, np.int64), np.full(n, self.miss, np.int64))
        self.pos_ids = self.e.index_ids(FB)
        assert len(self.pos_ids) == n
        self.hits = np.zeros(n, bool)
        p = np.arange(n)
        self.linked = p % 5 != 0
        self.e.load_rows(self.pos_ids[self.linked], np.full(int(self.linked.sum()), FL, np.uint32), np.full(int(self.linked.sum()), 5, np.int64), np.full(int(self.linked.sum()), 7, np.int64))
        dead = p[(p % 10 == 3)]
        self.e.put_rows(self.pos_ids[dead], np.full(len(dead), FL, np.uint32), np.full(len(dead), 6, np.int64), np.full(len(dead), sm.EMPTY, np.int64))
        self.linked[dead] = False

    def put(self, f, rows, vals):
        self.ts += 1
        self.e.put_rows(self.pos_ids[rows], np.full(len(rows), f, np.uint32), np.full(len(rows), self.ts, np.int64), np.asarray(vals, np.int64))

    def set_hits(self, pos):
        """exactly the positions `pos` hold `hit` in the base column and, where they have a link, a link value 500 + p % 3"""
        want = np.zeros(self.n, bool); want[np.asarray(pos, np.int64)] = True
        on, off = np.nonzero(want & ~self.hits)[0], np.nonzero(~want & self.hits)[0]
        if len(on):
            self.put(FB, on, np.full(len(on), self.hit)); k = on[self.linked[on]]
            if len(k):
                self.put(FL, k, 500 + k % 3)
        if len(off):
            self.put(FB, off, np.full(len(off), self.miss)); k = off[self.linked[off]]
            if len(k):
                self.put(FL, k, np.full(len(k), 7))
        self.hits = want

    def expect(self, tag):
        hit = np.nonzero(self.hits)[0]
        lhit = hit[self.linked[hit]]
        rest, lrest = np.nonzero(~self.hits)[0], np.nonzero(~(self.hits & self.linked))[0]
        for link, values, want, anti_want in ((FB, [self.hit, self.hit - 5], hit, rest), (FL, [500, 501, 502, 9], lhit, lrest)):
            for anti, rows in ((False, want), (True, anti_want)):
                m = len(rows)
                for cap in sorted({0, 1, max(m - 1, 0), m, self.n}):
                    buf, res = sm.raw_in(self.e, FB, EVERY, link, values, anti, cap)
                    k = min(m, cap)
                    assert (int(res["n_match"]), int(res["set_size"]), int(res["n_inner"]), int(res["flags"]), int(res["reserved"])) == (m, len(values), len(values), 0, 0), (tag, link == FB, anti, cap, res)
                    assert np.array_equal(buf[:k], self.pos_ids[rows[:k]]) and (buf[k:] == sm.FILL64).all(), (tag, link == FB, anti, cap)

    def close(self):
        self.e.close()


def _patterns(n):
    words = np.arange(0, n, WORD)
    lanes = np.arange(0, n, 4)                             # a lane's 16-byte load: 4 int32 (or two loads of 2 int64)
    edges = np.arange(WAVE, n, WAVE)                       # wave boundaries; every fourth is a block boundary
    pats = {
        "none": np.zeros(0, np.int64),
        "all": np.arange(n),
        "first": np.array([0]),
        "last": np.array([n - 1]),
        "lane ends": np.unique(np.concatenate([lanes, np.minimum(lanes + 3, n - 1)])),
        "word ends": np.unique(np.concatenate([words, np.minimum(words + WORD - 1, n - 1)])),
        "wave and block boundaries": np.unique(np.concatenate([edges - 1, edges])) if len(edges) else np.array([n // 2]),
    }
    return pats


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_probe_sweep_at_the_edges(n, wide):
    c = Column(n, wide)
    try:
        for name, rows in _patterns(n).items():
            c.set_hits(rows)
            c.expect((n, name))
        assert np.array_equal(c.e.index_ids(FB), c.pos_ids), "no position moved"
    finally:
        c.close()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 5, 2049, 8193, 2 * 8192 + 3])
def test_build_sweep_at_the_edges(n, wide):
    """the inner side by position: the inner program selects the positions whose column value is `hit`; position p's key is 1000 + p from the key field and
    the column value itself when the key is the base field. Selected positions at the first and last element of a lane's load, of a wave, of a workgroup's
    round and of the index; the set must hold exactly their keys."""
    base = (2**40 if wide else 0) + 7
    ids = streams.splitmix64_np(np.arange(1 + 80000 + n, n + 1 + 80000 + n, dtype=np.uint64))
    with bmx.Engine(max(8 * n, 1024)) as e:
        e.load_rows(ids, np.full(n, FI, np.uint32), np.full(n, 5, np.int64), np.full(n, base, np.int64))
        pos_ids = e.index_ids(FI)
        p = np.arange(n)
        e.load_rows(pos_ids, np.full(n, FK, np.uint32), np.full(n, 5, np.int64), 1000 + p)
        e.load_rows(pos_ids, np.full(n, FB, np.uint32), np.full(n, 5, np.int64), p % 1000)
        e.load_rows(pos_ids, np.full(n, FL, np.uint32), np.full(n, 5, np.int64), 1000 + (p * 7) % (n + 3))          # links: a permutation-like spread over the keys
        out_pos = e.index_ids(FB)
        order = {int(i): k for k, i in enumerate(pos_ids)}
        out_p = np.array([order[int(i)] for i in out_pos])                                                            # inner position of the node at outer position k
        ts = 10
        for name, rows in _patterns(n).items():
            ts += 2
            e.put_rows(pos_ids, np.full(n, FI, np.uint32), np.full(n, ts, np.int64), np.full(n, base, np.int64))
            if len(rows):
                e.put_rows(pos_ids[rows], np.full(len(rows), FI, np.uint32), np.full(len(rows), ts + 1, np.int64), np.full(len(rows), base + 1 + rows % 2, np.int64))
            keys = 1000 + rows
            link_of = 1000 + (out_p * 7) % (n + 3)
            for anti in (False, True):
                inside = np.isin(link_of, keys)
                want = out_pos[inside != anti]
                buf, res = sm.raw_semijoin(e, FB, EVERY, FL, FI, [[(FI, base + 1, base + 2)]], FK, anti, n, max(len(rows), 1))
                assert (int(res["n_match"]), int(res["set_size"]), int(res["n_inner"]), int(res["flags"])) == (len(want), len(rows), len(rows), 0), (n, name, anti, res)
                assert np.array_equal(buf[:len(want)], want) and (buf[len(want):] == sm.FILL64).all(), (n, name, anti)
            # the key is the inner base column: the set is {base + 1, base + 2} cut to what was selected
            buf, res = sm.raw_semijoin(e, FI, EVERY, FI, FI, [[(FI, base + 1, base + 2)]], FI, False, n, 2)
            assert (int(res["n_match"]), int(res["set_size"]), int(res["n_inner"])) == (len(rows), len(np.unique(rows % 2)), len(rows)), (n, name, res)
            if len(rows) > 1:
                buf, res = sm.raw_semijoin(e, FB, EVERY, FL, FI, [[(FI, base + 1, base + 2)]], FK, False, n, len(rows) - 1)
                assert (int(res["flags"]), int(res["n_match"]), int(res["n_inner"])) == (1, 0, len(rows)) and len(rows) - 1 < int(res["set_size"]) <= len(rows) and (buf == sm.FILL64).all()


@pytest.mark.parametrize("nkeys", [1, 5, 64, 5000])
def test_many_inner_nodes_with_few_keys(nkeys):
    """10^5 inner nodes that hold nkeys keys between them (each key is met by thousands of lanes while it is being claimed and long after), and D = 5000 under
    set_cap 8192; then every lane of a wave holding the same key (positions in runs of 2048) and every lane a different one"""
    n = 100_000
    ids = streams.splitmix64_np(np.arange(1 + 300000, n + 1 + 300000, dtype=np.uint64))
    with bmx.Engine(8 * n) as e:
        e.load_rows(ids, np.full(n, FI, np.uint32), np.full(n, 5, np.int64), np.arange(n) % 50)
        pos_ids = e.index_ids(FI)
        p = np.arange(n)
        nout = 3000
        link = sm.uid(np.arange(nout) % (2 * nkeys))
        e.load_rows(pos_ids[:nout], np.full(nout, FB, np.uint32), np.full(nout, 5, np.int64), np.arange(nout))
        e.load_rows(pos_ids[:nout], np.full(nout, FL, np.uint32), np.full(nout, 5, np.int64), link)
        out_pos = e.index_ids(FB)
        order = {int(i): k for k, i in enumerate(pos_ids[:nout])}
        lk = link[np.array([order[int(i)] for i in out_pos])]
        for ts, keys in ((5, sm.uid(p % nkeys)), (6, sm.uid((p // WAVE) % nkeys))):
            e.put_rows(pos_ids, np.full(n, FK, np.uint32), np.full(n, ts, np.int64), keys)
            for anti in (False, True):
                S = np.unique(keys)
                want = out_pos[np.isin(lk, S) != anti]
                buf, res = sm.raw_semijoin(e, FB, EVERY, FL, FI, EVERY, FK, anti, nout, 8192)
                assert (int(res["n_match"]), int(res["set_size"]), int(res["n_inner"]), int(res["flags"])) == (len(want), len(S), n, 0), (nkeys, ts, anti, res)
                assert np.array_equal(buf[:len(want)], want) and (buf[len(want):] == sm.FILL64).all()


def test_table_edges():
    """set_cap <= 32 (64 slots): 32 keys that share one home, the cluster that wraps from slot 63 to 0, links to absent keys of the same homes, D = set_cap and
    set_cap + 1 (overflow: nothing written, n_match 0, plain and anti), 70 keys into 64 slots, and an exact query behind every overflow"""
    m, tombs, qs = sm.table_edges()
    assert not tombs
    with bmx.Engine(4096) as e:
        wam.load(e, m, sm.ALL_FIELDS)
        pn = sm.pos_nodes(e, m, sm.FB)
        overflows = 0
        for q in qs:
            want = sm.want_of(m, pn, q)
            overflows += want.flags
            for cap in sm.caps_of(want.n_match, m.N):
                buf, res = sm.raw_of(e, q, cap)
                bad = sm.check(buf, res, want, cap, sm.set_cap_of(q))
                assert bad is None, (q, cap, bad, want)
        assert overflows == 6
