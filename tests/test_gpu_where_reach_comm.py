"""GPU: bmx_comm_where_reach and bmx_comm_where_reach_from. The same rows on 1, 2 and 4 logical shards give the ids, the depths and the record one engine
gives — in shard order: the expectation is reach_model's brute force laid out over the shards' own index positions, one shard after the other; a chain whose
consecutive nodes sit on different shards is followed to its end (a key held only on another shard than the node that links to it is found, because every
level's values are united across the shards); a union above set_cap while every shard is below it raises the flag and writes nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import reach_model as rm
import where_agg_model as wam
from reach_model import EVERY, FB, FI, FK, FL, FS, MORE, OVERFLOW


def _shard(c, g):
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    return s


def _comm_pos_nodes(c, m, base, nshards):
    """the node numbers of every shard's index positions, shard after shard: the order a sharded answer comes in"""
    parts = []
    for g in range(nshards):
        s = _shard(c, g)
        try:
            parts.append(m.index_of(s.index_ids(base)))
        finally:
            s.h = None                                                                # the communicator owns the context
    return np.concatenate(parts)


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = rm.forest()
    with bmx.Engine(16 * m.N) as e, bmx.Comm([0] * nshards, 16 * m.N) as c:
        rm.load(e, m); rm.load(c, m)
        for f, idx in tombs:
            for x in (e, c):
                x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), wam.VAL_DELETED, np.int64))
        rm.apply_tombs(m, tombs)
        c.scan_where(FB, EVERY, count_only=True)                                      # (every shard's index exists before its positions are asked for)
        pn1, pnc = rm.pos_nodes(e, m, FB), _comm_pos_nodes(c, m, FB, nshards)
        assert sorted(pn1.tolist()) == sorted(pnc.tolist())
        seen = set()
        qs = rm.forest_queries()[::4] + rm.forest_queries()[3::8]
        for k, q in enumerate(qs + [rm.as_list(m, q) for q in qs[:6]]):
            want1, wantc = rm.answer(m, pn1, q), rm.answer(m, pnc, q)
            for cap in (m.N, max(wantc.n_match // 3, 1), 0):
                one, many = rm.raw_of(e, q, cap), rm.raw_of(c, q, cap)
                assert rm.check(*one, want1, cap, q["set_cap"]) is None
                bad = rm.check(*many, wantc, cap, q["set_cap"])
                assert bad is None, (k, cap, bad, wantc)
                if not wantc.flags & OVERFLOW:
                    assert many[2].tobytes() == one[2].tobytes(), "one engine's record, byte for byte"
            seen.add((wantc.flags, wantc.n_match > 0))
        assert {(0, True), (MORE, True), (OVERFLOW, False)} <= seen, seen
        q = next(q for q in qs if rm.answer(m, pnc, q).n_match > 0)                     # (none that overflows: its set_size is a lower bound only)
        r, w =c.where_reach(FB, q["clauses"], FL, FK, FI, q["seed_clauses"], FS, max_depth=q["max_depth"], set_cap=q["set_cap"]), rm.answer(m, pnc, q)
        assert np.array_equal(r.ids, w.ids) and np.array_equal(r.depth, w.depth) and (r.n_match, r.set_size, r.rounds, r.flags) == (w.n_match, w.set_size, w.rounds, w.flags)
        r = c.where_reach_from(FB, EVERY, FL, FK, rm.uid(np.arange(5)), count_only=True)
        assert r.n_match == rm.answer(m, pnc, rm.QFROM(FB, EVERY, FL, FK, rm.uid(np.arange(5)))).n_match > 0 and len(r.ids) == 0


def test_a_chain_across_the_shards_and_a_union_that_overflows():
    n = 100
    ids = wam.node_ids(n + 1, 91000)
    L = bmx.load_library()
    owner = np.array([L.bmx_owner_of(int(x), 2) for x in ids[:n]])
    on = [np.nonzero(owner == g)[0] for g in (0, 1)]
    k = min(len(on[0]), len(on[1]), 20)
    assert k == 20
    order = np.ravel(np.column_stack([on[0][:k], on[1][:k]]))                         # consecutive nodes of the chain sit on different shards
    links = {int(x): (500 if j == 0 else 1000 + j - 1) for j, x in enumerate(order)}
    keys = {int(x): 1000 + j for j, x in enumerate(order)}
    rest = [int(x) for x in range(n) if x not in links]
    for j, x in enumerate(rest):                                                      # a star below the seed 600 with a key per node: the union of the second test
        links[x] = 600; keys[x] = 3000 + j
    m = rm.graph(n, links, keys, salt=14000, seeds=[500])
    assert np.array_equal(m.ids[:n], ids[:n])
    with bmx.Comm([0, 0], 4096) as c:
        rm.load(c, m)
        c.scan_where(FB, EVERY, count_only=True)
        pnc = _comm_pos_nodes(c, m, FB, 2)
        for q in (rm.Q(FB, EVERY, FL, FK, FI, rm.SEEDS_ALL, FS), rm.QFROM(FB, EVERY, FL, FK, [500]), rm.QFROM(FB, EVERY, FL, FK, [500], 7),
                  rm.QFROM(FB, EVERY, FK, FL, [1000 + 2 * k - 1])):
            want = rm.ask(c, m, q, None, pnc)
            assert want.n_match == (7 if q["max_depth"] == 7 else 2 * k) and want.rounds == want.n_match
        for g in range(2):                                                            # on its own, a shard gets no further than its first node
            s = _shard(c, g)
            try:
                ids_, dep, res = rm.raw_of(s, rm.QFROM(FB, EVERY, FL, FK, [500]), n)
                assert int(res["n_match"]) == (1 if g == 0 else 0)
            finally:
                s.h = None
        # every shard is below set_cap, the union is above it: 1 seed + the star's keys
        star = np.array(rest)
        per = np.bincount(owner[star], minlength=2)
        assert per.min() > 0
        set_cap = 1 + int(per.max())
        q = rm.QFROM(FB, EVERY, FL, FK, [600, 600], set_cap=set_cap)
        want = rm.answer(m, pnc, q)
        ids_, dep, res = rm.raw_of(c, q, n)
        assert rm.check(ids_, dep, res, want, n, set_cap) is None
        assert (int(res["flags"]), int(res["n_match"]), int(res["rounds"]), int(res["set_size"]), int(res["n_seed"]), int(res["n_edges"])) == (OVERFLOW, 0, 0, 1 + len(rest), 2, n)
        for g in range(2):
            s = _shard(c, g)
            try:
                assert not int(rm.raw_of(s, q, n)[2]["flags"]), "no shard overflows on its own"
            finally:
                s.h = None
        rm.ask(c, m, dict(q, set_cap=1 + len(rest)), None, pnc)                        # ... and right behind it a query that fits
        rm.ask(c, m, rm.Q(FB, EVERY, FL, FK, FI, rm.SEEDS_ALL, FS), None, pnc)
