"""GPU: the standing-query kernels at the edges of their geometry (csrc/watch_kernels.h k_watch_mask / k_watch_commit, csrc/select.h k_scan_emit): one mask word
is 32 rows shared by 32 / E lanes (E = 4 int32 or 2 int64 values per lane and load), a wave holds 2048 rows, a workgroup one 8192-row block. The program is one
literal on the base field, so the test decides row by row — by POSITION in the index — what matches: the row's value is `hit` or `miss`. Expected lists are slices
of index_ids(base), no model needed. Both value widths (wide: every value beyond int32, so the index scans its int64 column)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from oracle import streams

FB = streams.fnv1a32("watch.edge")
BLOCK, WAVE, WORD = 8192, 2048, 32
SIZES = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 2 * 8192 + 1]


def _ids(n, salt):
    return streams.splitmix64_np(np.arange(1 + salt, n + 1 + salt, dtype=np.uint64))


class Column:
    """an engine whose base column the test writes by position"""

    def __init__(self, n, wide, salt=0, extra=0):
        self.miss = (2**40 if wide else 0) + 7
        self.hit = self.miss + 1
        self.prog = [[(FB, self.hit, self.hit)]]
        self.all_ids = _ids(n + extra, 50000 + salt + n)
        self.e = bmx.Engine(max(4 * (n + extra), 1024))
        self.ts = 10
        self.e.load_rows(self.all_ids[:n], np.full(n, FB, np.uint32), np.full(n, 5, np.int64), np.full(n, self.miss, np.int64))
        self.w = self.e.watch_create(FB, self.prog)
        self.pos_ids = self.e.index_ids(FB)
        assert len(self.pos_ids) == n
        snap = self.e.watch_poll(self.w)
        assert snap.reset and (snap.n_entered, snap.n_left, snap.n_match) == (0, 0, 0)

    def put(self, pos, hit):
        pos = np.asarray(pos)
        self.ts += 1
        self.e.put_rows(self.pos_ids[pos], np.full(len(pos), FB, np.uint32), np.full(len(pos), self.ts, np.int64), np.full(len(pos), self.hit if hit else self.miss, np.int64))

    def expect(self, entered, left, n_match, tag):
        got = self.e.watch_poll(self.w)
        ent, lft = self.pos_ids[np.sort(np.asarray(entered, np.int64))], self.pos_ids[np.sort(np.asarray(left, np.int64))]
        assert (got.n_entered, got.n_left, got.n_match, got.reset, got.overflow) == (len(ent), len(lft), n_match, False, False), (tag, repr(got))
        assert np.array_equal(got.entered, ent) and np.array_equal(got.left, lft), tag

    def close(self):
        self.e.close()


def _patterns(n):
    words = np.arange(0, n, WORD)
    edges = np.arange(WAVE, n, WAVE)                       # wave boundaries; every fourth is a block boundary
    return {
        "first": np.array([0]),
        "last": np.array([n - 1]),
        "word ends": np.unique(np.concatenate([words, np.minimum(words + WORD - 1, n - 1)])),
        "wave and block boundaries": np.unique(np.concatenate([edges - 1, edges])) if len(edges) else np.array([n // 2]),
    }


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_changed_rows_at_the_edges(n, wide):
    c = Column(n, wide)
    try:
        for name, rows in _patterns(n).items():
            c.put(rows, True); c.expect(rows, [], len(rows), (n, name, "enter"))
            c.expect([], [], len(rows), (n, name, "idle"))
            c.put(rows, False); c.expect([], rows, 0, (n, name, "leave"))
            # half of them enter, are committed, then leave while the other half enters
            a, b = rows[::2], rows[1::2]
            c.put(a, True); c.expect(a, [], len(a), (n, name, "half in"))
            c.put(a, False)
            if len(b):
                c.put(b, True)
            c.expect(b, a, len(b), (n, name, "half in, half out"))
            if len(b):
                c.put(b, False); c.expect([], b, 0, (n, name, "the rest leaves"))
        assert np.array_equal(c.e.index_ids(FB), c.pos_ids), "no position moved"
    finally:
        c.close()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n,created", [(8190, 5), (30, 4)])
def test_appended_rows_read_an_empty_committed_word(n, created, wide):
    """every old row is committed as matching; the created rows share a mask word with old ones and cross into the next word (n = 30) or the next block (n = 8190):
    the bits of the committed bitmap behind the old length must read zero — a set bit would hide an entering row or invent a leaving one"""
    c = Column(n, wide, salt=7, extra=created)
    try:
        c.put(np.arange(n), True); c.expect(np.arange(n), [], n, "all in")
        new = c.all_ids[n:]
        vals = np.array([c.hit if k % 2 == 0 else c.miss for k in range(created)], np.int64)        # created: matching, not, matching, ...
        c.e.merge_batch(new, np.full(created, FB, np.uint32), np.full(created, 500, np.int64), vals, want_flags=False)
        pos_ids = c.e.index_ids(FB)
        assert np.array_equal(pos_ids[:n], c.pos_ids) and set(pos_ids[n:].tolist()) == set(new.tolist()), "appended behind the old rows"
        c.pos_ids = pos_ids; c.ts = 1000
        where = {int(i): n + k for k, i in enumerate(pos_ids[n:])}
        hit_pos = [where[int(i)] for i, v in zip(new, vals) if v == c.hit]
        miss_pos = [where[int(i)] for i, v in zip(new, vals) if v == c.miss]
        c.expect(hit_pos, [], n + len(hit_pos), "created rows enter, the others do nothing")
        c.expect([], [], n + len(hit_pos), "idle")
        c.put(hit_pos, False); c.put(miss_pos, True)
        c.expect(miss_pos, hit_pos, n + len(miss_pos), "swap")
        c.put(np.arange(n + created), False)
        c.expect([], list(range(n)) + miss_pos, 0, "all out")
    finally:
        c.close()


@pytest.mark.parametrize("wide", [False, True])
def test_a_whole_block_at_once(wide):
    """every row of three blocks enters in one poll and leaves in one poll: the emit pass streams its densest blocks (8192 matches, far above SCAN_STREAM_MIN)"""
    n = 2 * BLOCK + 1
    c = Column(n, wide, salt=3)
    try:
        rows = np.arange(n)
        c.put(rows, True); c.expect(rows, [], n, "all in")
        mid = np.arange(BLOCK, 2 * BLOCK)
        c.put(mid, False); c.expect([], mid, n - BLOCK, "the middle block out")
        c.put(mid, True); c.put(np.arange(BLOCK), False); c.expect(mid, np.arange(BLOCK), n - BLOCK, "one block in, one out")
        c.put(np.arange(BLOCK, n), False); c.expect([], np.arange(BLOCK, n), 0, "all out")
    finally:
        c.close()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("blocks", [9, 17])
def test_eight_blocks_per_workgroup(monkeypatch, blocks, wide):
    """BMX_SCAN_SUB8_BLOCKS=1: the emit pass takes eight blocks per workgroup; 9 and 17 blocks leave a last workgroup with one block. Sparse lists take its
    one-scan path, dense ones go block by block."""
    n = (blocks - 1) * BLOCK + 5
    c = Column(n, wide, salt=11)
    try:
        monkeypatch.setenv("BMX_SCAN_SUB8_BLOCKS", "1")
        sparse = np.unique(np.concatenate([np.arange(0, n, 509), np.arange(BLOCK - 1, n, BLOCK), np.arange(BLOCK, n, BLOCK), [n - 1]]))
        c.put(sparse, True); c.expect(sparse, [], len(sparse), "sparse in")
        dense = np.setdiff1d(np.arange(n), sparse)
        c.put(dense, True); c.put(sparse, False); c.expect(dense, sparse, len(dense), "dense in, sparse out")
        c.put(dense[::3], False); c.expect([], dense[::3], len(dense) - len(dense[::3]), "a third out")
        rest = np.setdiff1d(dense, dense[::3])
        c.put(rest, False); c.expect([], rest, 0, "all out")
    finally:
        c.close()
