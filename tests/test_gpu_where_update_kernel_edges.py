"""GPU: the update-by-query kernels at the edges of their geometry (csrc/update_kernels.h PredUpd / k_upd_emit / k_upd_finish, csrc/select.h k_scan_mask): one
mask word is 32 rows shared by 32 / E lanes (E = 4 int32 or 2 int64 values per lane and load), a wave holds 2048 rows, a workgroup one 8192-row block (eight of
them in the large-column form). The program is one literal on the base field, so the test decides row by row — by POSITION in the index — what is selected. The
source field is absent on every third position and tombstoned on every fifth, so n_nosrc and the dense ranks disagree with the program's own count in every
block; the first and the last position of every block hold 2^53 - 1, so ADD 1 leaves the range exactly there. The expected records are arithmetic on positions.
Both value widths (wide: every base value beyond int32, so the index scans its int64 column)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import update_model as um
from oracle import streams
from update_model import ADD, COPY, SET

FB, FS, FT = (streams.fnv1a32(s) for s in ("upd.edge", "upd.edge.src", "upd.edge.target"))
BLOCK, WAVE, WORD = 8192, 2048, 32
BIG = 2**53 - 1
SIZES = [1, 63, 64, 65, 8191, 8192, 8193, 2 * 8192 + 1]


class Column:
    """an engine whose base column the test writes by position, with the source field FS and the target FT it keeps track of"""

    def __init__(self, n, wide, salt=0):
        self.n = n
        self.miss = (2**40 if wide else 0) + 7
        self.hit = self.miss + 1
        self.prog = [[(FB, self.hit, self.hit)]]
        ids = streams.splitmix64_np(np.arange(1 + 130000 + salt + n, n + 1 + 130000 + salt + n, dtype=np.uint64))
        self.e = bmx.Engine(max(8 * n, 1024))
        self.ts = 10
        self.e.load_rows(ids, np.full(n, FB, np.uint32), np.full(n, 5, np.int64), np.full(n, self.miss, np.int64))
        self.pos_ids = self.e.index_ids(FB)
        assert len(self.pos_ids) == n
        p = np.arange(n)
        self.edge = (p % BLOCK == 0) | (p % BLOCK == BLOCK - 1)
        self.absent = (p % 3 == 1) & ~self.edge
        self.tomb = (p % 5 == 2) & ~self.absent & ~self.edge
        self.src = np.where(self.edge, BIG, p + 1)
        have = np.nonzero(~self.absent)[0]
        self.e.load_rows(self.pos_ids[have], np.full(len(have), FS, np.uint32), np.full(len(have), 3, np.int64), self.src[have])
        dead = np.nonzero(self.tomb)[0]
        if len(dead):
            self.e.put_rows(self.pos_ids[dead], np.full(len(dead), FS, np.uint32), np.full(len(dead), 4, np.int64), np.full(len(dead), um.VAL_DELETED, np.int64))
        self.hits = np.zeros(n, bool)
        self.t_have = np.zeros(n, bool); self.t_val = np.zeros(n, np.int64); self.t_ts = np.zeros(n, np.int64)       # the target field, by position
        self.rows = n + len(have)

    def set_hits(self, pos):
        """exactly the positions `pos` are selected"""
        want = np.zeros(self.n, bool); want[np.asarray(pos, np.int64)] = True
        for rows, v in ((np.nonzero(want & ~self.hits)[0], self.hit), (np.nonzero(~want & self.hits)[0], self.miss)):
            if len(rows):
                self.ts += 1
                self.e.put_rows(self.pos_ids[rows], np.full(len(rows), FB, np.uint32), np.full(len(rows), self.ts, np.int64), np.full(len(rows), v, np.int64))
        self.hits = want

    def writable(self, op, start):
        sel = self.hits.copy(); sel[:start] = False
        if op == SET:
            return sel, 0, 0, np.full(self.n, 77, np.int64)
        if op == COPY:                                              # from the base column: no probe, never without source
            return sel, 0, 0, np.full(self.n, self.hit, np.int64)
        nosrc = sel & (self.absent | self.tomb)
        rng = sel & ~nosrc & self.edge
        return sel & ~nosrc & ~rng, int(nosrc.sum()), int(rng.sum()), self.src + 1

    def expect(self, op, start, cap, tag):
        """one call with a clock above every earlier one: every record sent wins"""
        self.ts += 1
        w, n_nosrc, n_range, vals = self.writable(op, start)
        wpos = np.nonzero(w)[0]
        out = wpos[:cap]
        ids, r = um.raw_update(self.e, FB, self.prog, FT, op, 77 if op == SET else (1 if op == ADD else 0), FB if op == COPY else FS, self.ts, False, start, cap)
        self.t_have[out] = True; self.t_val[out] = vals[out]; self.t_ts[out] = self.ts
        want = (len(wpos) + n_nosrc + n_range, n_nosrc, n_range, len(out), len(out), self.rows + int(self.t_have.sum()), int(wpos[cap]) if len(wpos) > cap else self.n)
        assert tuple(int(r[k]) for k in um.WORDS) == want, (tag, op, start, cap, r, want)
        assert np.array_equal(ids, self.pos_ids[out]), (tag, op, start, cap)

    def check_target(self, tag):
        ts, val, found = self.e.get_rows(self.pos_ids, np.full(self.n, FT, np.uint32))
        assert np.array_equal(found, self.t_have), tag
        assert np.array_equal(val[found], self.t_val[found]) and np.array_equal(ts[found], self.t_ts[found]), tag

    def close(self):
        self.e.close()


def _cursors(c, op):
    """(start, cap) pairs: caps around the number of writable nodes, at the block size, and at the first and last rank of the second workgroup; starts at the
    block edges and at the last row — each cut at what the column has"""
    n = c.n
    w = np.nonzero(c.writable(op, 0)[0])[0]
    m = len(w)
    k1 = int((w < BLOCK).sum())                                    # ranks k1 - 1 and k1: the last of the first workgroup and the first of the second
    k2 = int((w < 2 * BLOCK).sum())
    caps = sorted({x for x in (0, 1, m - 1, m, m + 1, BLOCK - 1, BLOCK, BLOCK + 1, k1 - 1, k1, k1 + 1, k2 - 1, k2) if 0 <= x <= n + 1})
    starts = sorted({s for s in (0, 5, WORD + 17, BLOCK - 1, BLOCK, BLOCK + 1, n - 1) if 0 <= s < n})
    return [(0, x) for x in caps] + [(s, n) for s in starts[1:]] + [(s, x) for s in starts[1::2] for x in (1, m // 2)]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_update_at_the_edges(n, wide):
    c = Column(n, wide)
    try:
        for name, rows in (("none", np.zeros(0, np.int64)), ("all", np.arange(n)), ("every other", np.arange(0, n, 2))):
            c.set_hits(rows)
            for op in (ADD, SET, COPY):
                for start, cap in (_cursors(c, op) if op == ADD else [(0, n), (0, 0), (min(BLOCK - 1, n - 1), 3)]):
                    c.expect(op, start, cap, (n, name))
            c.check_target((n, name))
        assert np.array_equal(c.e.index_ids(FB), c.pos_ids), "no position moved"
    finally:
        c.close()


@pytest.mark.parametrize("wide", [False, True])
def test_eight_blocks_per_workgroup(monkeypatch, wide):
    """BMX_SCAN_SUB8_BLOCKS=1: the emit pass takes eight blocks per workgroup; 9 blocks leave a last workgroup with one. Sparse selections take its one-scan
    path (at most 8192 writable nodes in eight blocks), dense ones go block by block; the answers equal the one-block form's."""
    n = 8 * BLOCK + 5
    c = Column(n, wide, salt=11)
    try:
        sparse = np.unique(np.concatenate([np.arange(0, n, 509), np.arange(BLOCK - 1, n, BLOCK), np.arange(BLOCK, n, BLOCK), [n - 1]]))
        for name, rows in (("sparse", sparse), ("dense", np.setdiff1d(np.arange(n), sparse)), ("all", np.arange(n))):
            c.set_hits(rows)
            m = int(c.writable(ADD, 0)[0].sum())
            for start, cap in ((0, n), (0, 0), (0, 1), (0, m - 1), (0, m), (0, BLOCK), (8 * BLOCK, n), (8 * BLOCK - 1, 3), (5 * BLOCK + 17, WAVE), (n - 1, 2)):
                monkeypatch.setenv("BMX_SCAN_SUB8_BLOCKS", "1")
                c.expect(ADD, start, cap, (name, "eight blocks per workgroup"))
                monkeypatch.delenv("BMX_SCAN_SUB8_BLOCKS")
            c.expect(ADD, 0, n, (name, "one block per workgroup"))
            monkeypatch.setenv("BMX_SCAN_SUB8_BLOCKS", "1")
            c.expect(SET, 0, n, (name, "eight blocks per workgroup"))
            monkeypatch.delenv("BMX_SCAN_SUB8_BLOCKS")
            c.check_target(name)
    finally:
        c.close()
