"""GPU: the traversal kernels at the edges of their geometry (csrc/reach_kernels.h k_reach_prepare / k_reach_round / PredReach / k_reach_emit, csrc/select.h
k_scan_mask). The prepare sweep gives a lane 16 bytes of the base column (4 int32 or 2 int64 positions), the round a lane two positions (one 16-byte load of
links, one 2-byte load of depths), the mask pass a lane sixteen depth bytes — half a mask word; a wave of the mask pass holds 1024 positions, a workgroup one
8192-position block. The edge program selects every position, so what is reached is decided by the LINK alone, position by position: a hit position p has the
link 500 + p % 3 and the key 501 + p % 3 under the seed 500, so the depths 1, 2 and 3 interleave inside one mask word; every other position's link dangles.
The link comes from the base column itself and from a probed field holding the same values. Both value widths (wide: every value beyond int32). Expected values
come from reach_model's brute force over a model whose node k is position k."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import group_model as gm
import reach_model as rm
from oracle import streams
from watch_model import Model

FB, FL, FK = (streams.fnv1a32(s) for s in ("reach.edge", "reach.edge.link", "reach.edge.key"))
BLOCK, WAVE, WORD = 8192, 2048, 32
SIZES = [1, 3, 31, 33, 2047, 2049, 8191, 8193, 2 * 8192 + 1]
EVERY = rm.EVERY


class Column:
    """an engine whose base column the test writes by position; FL mirrors the column (the same link from a probe), FK is the key"""

    def __init__(self, n, wide, salt=0):
        self.n, self.off = n, (2**40 if wide else 0)
        ids = streams.splitmix64_np(np.arange(1 + 90000 + salt + n, n + 1 + 90000 + salt + n, dtype=np.uint64))
        self.e = bmx.Engine(max(8 * n, 1024))
        self.ts = 10
        miss = np.full(n, self.off + 7, np.int64)
        self.e.load_rows(ids, np.full(n, FB, np.uint32), np.full(n, 5, np.int64), miss)
        self.pos_ids = self.e.index_ids(FB)
        assert len(self.pos_ids) == n
        self.m = Model(self.pos_ids)                     # node k of the model is position k
        p = np.arange(n)
        for f, v in ((FB, miss), (FL, miss), (FK, np.full(n, self.off + 9, np.int64))):
            if f != FB:
                self.e.load_rows(self.pos_ids, np.full(n, f, np.uint32), np.full(n, 5, np.int64), v)
            self.m.set(f, p, v)
        self.hits = np.zeros(n, bool)
        self.pn = p

    def put(self, f, rows, vals):
        self.ts += 1
        self.e.put_rows(self.pos_ids[rows], np.full(len(rows), f, np.uint32), np.full(len(rows), self.ts, np.int64), np.asarray(vals, np.int64))
        self.m.set(f, rows, vals)

    def set_hits(self, pos):
        want = np.zeros(self.n, bool); want[np.asarray(pos, np.int64)] = True
        on, off = np.nonzero(want & ~self.hits)[0], np.nonzero(~want & self.hits)[0]
        for rows, link, key in ((on, self.off + 500 + on % 3, self.off + 501 + on % 3), (off, np.full(len(off), self.off + 7), np.full(len(off), self.off + 9))):
            if len(rows):
                self.put(FB, rows, link); self.put(FL, rows, link); self.put(FK, rows, key)
        self.hits = want

    def expect(self, tag, more_caps=()):
        """-> the expectation of the deeper query (max_depth 4: every hit that can be reached)"""
        seed = [self.off + 500, self.off + 500]
        for link in (FB, FL):
            for D in (2, 4):
                q = rm.QFROM(FB, EVERY, link, FK, seed, D, 64)
                want = rm.answer(self.m, self.pn, q)
                for cap in sorted(set(rm.caps_of(want.n_match, self.n)) | {c for c in more_caps if c <= self.n}):
                    ids, dep, res = rm.raw_of(self.e, q, cap)
                    bad = rm.check(ids, dep, res, want, cap, 64)
                    assert bad is None, (tag, link == FB, D, cap, bad, want)
        return want

    def close(self):
        self.e.close()


def _patterns(n):
    words = np.arange(0, n, WORD)
    lanes = np.arange(0, n, 4)                             # a lane's 16-byte load of the prepare sweep: 4 int32 (or two loads of 2 int64)
    halves = np.arange(0, n, 16)                           # a lane's sixteen depth bytes in the mask pass
    edges = np.arange(WAVE, n, WAVE)                       # wave boundaries; every fourth is a block boundary
    return {
        "none": np.zeros(0, np.int64),
        "all": np.arange(n),
        "first": np.array([0]),
        "last": np.array([n - 1]),
        "lane ends": np.unique(np.concatenate([lanes, np.minimum(lanes + 3, n - 1), halves, np.minimum(halves + 15, n - 1)])),
        "word ends": np.unique(np.concatenate([words, np.minimum(words + WORD - 1, n - 1)])),
        "wave and block boundaries": np.unique(np.concatenate([edges - 1, edges])) if len(edges) else np.array([n // 2]),
    }


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sweeps_at_the_edges(n, wide):
    c = Column(n, wide)
    try:
        depths = set()
        for name, rows in _patterns(n).items():
            c.set_hits(rows)
            want = c.expect((n, name), (8191, 8192, 8193) if name == "all" else ())
            depths |= set(want.depth.tolist())
            assert want.n_match <= len(rows) and (name != "all" or want.n_match == n)
        assert depths == ({1, 2, 3} if n >= 3 else {1})
        assert np.array_equal(c.e.index_ids(FB), c.pos_ids), "no position moved"
    finally:
        c.close()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [8193, 2 * 8192 + 1, 8 * 8192 + 5])
def test_eight_blocks_per_workgroup(monkeypatch, n, wide):
    c = Column(n, wide, salt=7)
    try:
        monkeypatch.setenv("BMX_SCAN_SUB8_BLOCKS", "1")
        for name in ("all", "word ends", "wave and block boundaries", "last"):      # "all": more than 8192 matches in a group of eight blocks (the fall-through)
            c.set_hits(_patterns(n)[name])
            c.expect((n, name, "sub8"), (8191, 8192, 8193) if name == "all" else ())
    finally:
        c.close()


def test_walks_that_wrap_in_a_64_slot_map():
    """set_cap <= 32 (64 slots): seeds and contributed keys that share the homes 62 and 63, so inserts and the rounds' lookups walk from slot 63 to slot 0;
    links to absent values of the same homes walk a whole cluster; set_cap at K and K - 1"""
    seeds = gm.keys_with_home(62, 64, 4, start=1000)
    mid = gm.keys_with_home(63, 64, 6, start=5000, avoid=seeds)
    absent = gm.keys_with_home(62, 64, 3, start=9000, avoid=seeds + mid)
    L, K = {}, {}
    for i, s in enumerate(seeds):                                  # depth 1: four nodes below the seeds, their keys crowd slot 63 onward
        L[i] = s; K[i] = mid[i]
    for i, v in enumerate(mid[:4]):                                # depth 2, the last two keys of `mid` arrive here
        L[4 + i] = v; K[4 + i] = mid[(i + 4) % 6]
    L[8] = mid[5]; K[8] = seeds[0]                                 # depth 3, back to a seed
    for i, v in enumerate(absent):
        L[9 + i] = v; K[9 + i] = 77
    m = rm.graph(12, L, K)
    with bmx.Engine(4096) as e:
        rm.load(e, m)
        pn = rm.pos_nodes(e, m, rm.FB)
        full = rm.QFROM(rm.FB, EVERY, rm.FL, rm.FK, seeds, set_cap=32)
        want = rm.ask(e, m, full, None, pn)
        assert (want.n_match, want.rounds, want.set_size, want.flags) == (9, 3, 10, 0)
        assert "wrap" in rm.device_of(m, full)[4].tags
        for q in (dict(full, set_cap=10), dict(full, set_cap=9), dict(full, set_cap=3), dict(full, max_depth=2), full):
            rm.ask(e, m, q, None, pn)
        assert rm.answer(m, pn, dict(full, set_cap=9)).flags == rm.OVERFLOW


@pytest.mark.parametrize("nkeys", [1, 5])
def test_many_nodes_on_few_keys(nkeys):
    """10^5 nodes that hold nkeys keys between them: each key is met by thousands of lanes while it is being claimed and long after, so the minimum skips its
    atomics; half of the nodes sit below the seed, the other half below those keys and bring the same keys again one round later"""
    n = 100_000
    p = np.arange(n)
    m = Model(streams.splitmix64_np(np.arange(1 + 400000, n + 1 + 400000, dtype=np.uint64)))
    m.set(rm.FB, p, p % 50)
    m.set(rm.FL, p, np.where(p % 2 == 0, 500, rm.uid(p % nkeys)))
    m.set(rm.FK, p, rm.uid((p // 3) % nkeys))
    with bmx.Engine(8 * n) as e:
        rm.load(e, m, [rm.FB, rm.FL, rm.FK])
        pn = rm.pos_nodes(e, m, rm.FB)
        want = rm.ask(e, m, rm.QFROM(rm.FB, EVERY, rm.FL, rm.FK, [500], set_cap=64), None, pn)
        assert (want.n_match, want.set_size, want.rounds, want.flags) == (n, 1 + nkeys, 2, 0)
        rm.ask(e, m, rm.QFROM(rm.FB, EVERY, rm.FL, rm.FK, [500], 1, set_cap=64), 1000, pn)


def test_one_chain_of_200_levels_of_500():
    n = 100_000
    p = np.arange(n)
    lvl = p // 500
    m = Model(streams.splitmix64_np(np.arange(1 + 600000, n + 1 + 600000, dtype=np.uint64)))
    m.set(rm.FB, p, p % 50)
    m.set(rm.FL, p, np.where(lvl == 0, 500, 1000 + lvl - 1))
    m.set(rm.FK, p, 1000 + lvl)
    with bmx.Engine(8 * n) as e:
        rm.load(e, m, [rm.FB, rm.FL, rm.FK])
        pn = rm.pos_nodes(e, m, rm.FB)
        want = rm.ask(e, m, rm.QFROM(rm.FB, EVERY, rm.FL, rm.FK, [500], set_cap=256), None, pn)
        assert (want.n_match, want.set_size, want.rounds, want.flags) == (n, 201, 200, 0)
        want = rm.ask(e, m, rm.QFROM(rm.FB, EVERY, rm.FL, rm.FK, [500], 100, set_cap=256), None, pn)
        assert (want.n_match, want.rounds, want.flags) == (50_000, 100, rm.MORE)
