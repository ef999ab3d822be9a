"""GPU: the row-projection kernels at the edges of their geometry (csrc/rows_kernels.h PredRowsFrom / k_rows_emit, csrc/select.h k_scan_mask): one mask word is
32 rows shared by 32 / E lanes (E = 4 int32 or 2 int64 values per lane and load), a wave holds 2048 rows, a workgroup one 8192-row block (eight of them in the
large-column form). The program is one literal on the base field, so the test decides row by row — by POSITION in the index — what matches: the row's value is
`hit` or `miss`. Two projected fields are loaded for every second and every third position (every twelfth position holds a tombstone of the second), so the
expected columns are arithmetic on positions: no model needed. Both value widths (wide: every value beyond int32, so the index scans its int64 column)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import rows_model as rm
from oracle import streams

FB, F2, F3 = (streams.fnv1a32(s) for s in ("rows.edge", "rows.edge.two", "rows.edge.three"))
BLOCK, WAVE, WORD = 8192, 2048, 32
SIZES = [1, 31, 32, 33, 2047, 2048, 2049, 8191, 8192, 8193, 2 * 8192 + 1]


class Column:
    """an engine whose base column the test writes by position; F2 on every second position (value 1000 + p, clock 3), F3 on every third (value -p, clock 4 + p % 5;
    every twelfth tombstoned at clock 50)"""

    def __init__(self, n, wide, salt=0):
        self.n = n
        self.miss = (2**40 if wide else 0) + 7
        self.hit = self.miss + 1
        self.prog = [[(FB, self.hit, self.hit)]]
        ids = streams.splitmix64_np(np.arange(1 + 90000 + salt + n, n + 1 + 90000 + salt + n, dtype=np.uint64))
        self.e = bmx.Engine(max(8 * n, 1024))
        self.ts = 10
        self.e.load_rows(ids, np.full(n, FB, np.uint32), np.full(n, 5, np.int64), np.full(n, self.miss, np.int64))
        self.pos_ids = self.e.index_ids(FB)
        assert len(self.pos_ids) == n
        p = np.arange(n)
        p2, p3, p12 = p[::2], p[::3], p[::12]
        self.e.load_rows(self.pos_ids[p2], np.full(len(p2), F2, np.uint32), np.full(len(p2), 3, np.int64), 1000 + p2)
        self.e.load_rows(self.pos_ids[p3], np.full(len(p3), F3, np.uint32), 4 + p3 % 5, -p3)
        self.e.put_rows(self.pos_ids[p12], np.full(len(p12), F3, np.uint32), np.full(len(p12), 50, np.int64), np.full(len(p12), rm.VAL_DELETED, np.int64))
        self.hits = np.zeros(n, bool)

    def set_hits(self, pos):
        """exactly the positions `pos` match"""
        want = np.zeros(self.n, bool); want[np.asarray(pos, np.int64)] = True
        for rows, v in ((np.nonzero(want & ~self.hits)[0], self.hit), (np.nonzero(~want & self.hits)[0], self.miss)):
            if len(rows):
                self.ts += 1
                self.e.put_rows(self.pos_ids[rows], np.full(len(rows), FB, np.uint32), np.full(len(rows), self.ts, np.int64), np.full(len(rows), v, np.int64))
        self.hits = want

    def expect(self, start, cap, tag):
        hit = np.nonzero(self.hits)[0]
        hit = hit[hit >= start]
        out = hit[:cap]
        ids, vals, ts, r = rm.raw_rows(self.e, FB, self.prog, [F2, F3, FB], True, start, cap)
        assert (int(r["n_match"]), int(r["n_out"]), int(r["next_pos"])) == (len(hit), len(out), int(hit[cap]) if len(hit) > cap else self.n), (tag, start, cap, r)
        assert np.array_equal(ids, self.pos_ids[out]), (tag, start, cap)
        v2 = np.where(out % 2 == 0, 1000 + out, rm.VAL_DELETED); t2 = np.where(out % 2 == 0, 3, rm.NO_CLOCK)
        v3 = np.where((out % 3 == 0) & (out % 12 != 0), -out, rm.VAL_DELETED); t3 = np.where(out % 12 == 0, 50, np.where(out % 3 == 0, 4 + out % 5, rm.NO_CLOCK))
        assert np.array_equal(vals[0], v2) and np.array_equal(ts[0], t2), (tag, start, cap, "every second position")
        assert np.array_equal(vals[1], v3) and np.array_equal(ts[1], t3), (tag, start, cap, "every third position")
        assert (vals[2] == self.hit).all() and (ts[2] >= 5).all(), (tag, start, cap, "the base field")
        # the same page without clocks: the base field comes from the column
        ids_b, vals_b, _, r_b = rm.raw_rows(self.e, FB, self.prog, [FB, F3], False, start, cap)
        assert r_b.tobytes() == r.tobytes() and np.array_equal(ids_b, ids) and (vals_b[0] == self.hit).all() and np.array_equal(vals_b[1], v3), (tag, start, cap, "no clocks")

    def close(self):
        self.e.close()


def _patterns(n):
    words = np.arange(0, n, WORD)
    edges = np.arange(WAVE, n, WAVE)                       # wave boundaries; every fourth is a block boundary
    pats = {
        "none": np.zeros(0, np.int64),
        "all": np.arange(n),
        "first": np.array([0]),
        "last": np.array([n - 1]),
        "word ends": np.unique(np.concatenate([words, np.minimum(words + WORD - 1, n - 1)])),
        "wave and block boundaries": np.unique(np.concatenate([edges - 1, edges])) if len(edges) else np.array([n // 2]),
    }
    if n > BLOCK:
        pats["a full block next to an empty one"] = np.arange(BLOCK)
        if n > 2 * BLOCK:
            pats["an empty block in front of a full one"] = np.arange(BLOCK, 2 * BLOCK)
    return pats


def _cursors(n, hits):
    """(start, cap) pairs: caps on a word, wave and block boundary of the RANKS and exactly on the last match; starts inside a word, at a word edge, at a block edge,
    at the last row — each cut at what the column has"""
    m = len(hits)
    caps = sorted({c for c in (0, 1, WORD - 1, WORD, WORD + 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, m - 1, m, m + 1, n) if 0 <= c <= n + 1})
    starts = sorted({s for s in (0, 5, WORD, WORD + 17, WAVE, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, n - 1) if 0 <= s < n})
    pairs = [(0, c) for c in caps] + [(s, n) for s in starts]
    pairs += [(s, c) for s in starts[1::2] for c in (1, WORD, m // 2)]
    return pairs


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_rows_at_the_edges(n, wide):
    c = Column(n, wide)
    try:
        for name, rows in _patterns(n).items():
            c.set_hits(rows)
            for start, cap in _cursors(n, rows):
                c.expect(start, cap, (n, name))
        assert np.array_equal(c.e.index_ids(FB), c.pos_ids), "no position moved"
    finally:
        c.close()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("blocks", [9, 17])
def test_eight_blocks_per_workgroup(monkeypatch, blocks, wide):
    """BMX_SCAN_SUB8_BLOCKS=1: the emit pass takes eight blocks per workgroup; 9 and 17 blocks leave a last workgroup with one block. Sparse selections take its
    one-scan path (at most 8192 matches in eight blocks), dense ones go block by block; the answers equal the one-block form's."""
    n = (blocks - 1) * BLOCK + 5
    c = Column(n, wide, salt=11)
    try:
        sparse = np.unique(np.concatenate([np.arange(0, n, 509), np.arange(BLOCK - 1, n, BLOCK), np.arange(BLOCK, n, BLOCK), [n - 1]]))
        dense = np.setdiff1d(np.arange(n), sparse)
        for name, rows in (("sparse", sparse), ("dense", dense), ("exactly 8192 in the first eight blocks", np.arange(0, 8 * BLOCK, 8)), ("8193 there", np.concatenate([np.arange(0, 8 * BLOCK, 8), [3]]))):
            c.set_hits(rows)
            m = len(rows)
            for start, cap in ((0, n), (0, 0), (0, 1), (0, m - 1), (0, m), (0, BLOCK), (0, 8 * BLOCK + 1), (8 * BLOCK, n), (8 * BLOCK - 1, 3), (5 * BLOCK + 17, WAVE), (n - 1, 2)):
                monkeypatch.setenv("BMX_SCAN_SUB8_BLOCKS", "1")
                c.expect(start, cap, (blocks, name, "eight blocks per workgroup"))
                monkeypatch.delenv("BMX_SCAN_SUB8_BLOCKS")
            c.expect(0, n, (blocks, name, "one block per workgroup"))
    finally:
        c.close()
