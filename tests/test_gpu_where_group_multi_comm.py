"""GPU: bmx_comm_where_group_multi. The same rows on 1, 2 and 4 logical shards give one engine's sorted answer, byte for byte, and bmx.mgroup_merge of the
per-shard answers; a tuple held on two shards is folded into one record; a union that overflows while no single shard does raises the flag and writes nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import group_model as gm
import mgroup_model as mm
import where_agg_model as wam

F = gm._names()
FB, FK, FM, F1 = F["base"], F["key"], F["measure"], F["one"]
ALL_FIELDS = [FB, F1, F["two"], F["three"], F["four"], F["five"], FM, FK] + F["more"]


def _shard_answer(c, g, base, clauses, keys, measure, cap):
    """bmx_where_group_multi on shard g's own context"""
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    try:
        out, res = mm.raw_mgroup(s, base, clauses, keys, measure, cap)
        return out[:0 if int(res["flags"]) else int(res["n_groups"])].copy(), res
    finally:
        s.h = None                                                            # the communicator owns the context


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = gm.seeded_model(False)
    with bmx.Engine(16 * m.N) as e, bmx.Comm([0] * nshards, 16 * m.N) as c:
        for x in (e, c):
            wam.load(x, m, ALL_FIELDS)
        for f, idx in tombs.items():
            wam.tombstone(e, m, f, idx)
            c.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), wam.VAL_DELETED, np.int64))
        seen = shared = 0
        for k, (p, keys, measure) in enumerate(mm.seeded_queries()[::3]):
            for cap in (8192, 3):
                one = mm.raw_mgroup(e, FB, p, keys, measure, cap)
                many = mm.raw_mgroup(c, FB, p, keys, measure, cap)
                want = mm.answer(m, FB, p, keys, measure, cap)
                assert mm.check(*many, *want, cap) is None, (k, cap, mm.check(*many, *want, cap))
                if not int(want[1]["flags"]):
                    assert many[0].tobytes() == one[0].tobytes() and many[1].tobytes() == one[1].tobytes(), "one engine's answer, byte for byte"
                    parts = [_shard_answer(c, g, FB, p, keys, measure, cap) for g in range(nshards)]
                    merged = bmx.mgroup_merge([x[0] for x in parts])
                    assert merged.tobytes() == want[0].tobytes(), "mgroup_merge of the shards' answers"
                    assert sum(int(x[1]["total"]["n_match"]) for x in parts) == int(want[1]["total"]["n_match"])
                    seen += len(merged) >= 2
                    shared += sum(len(x[0]) for x in parts) > len(merged)
        assert seen >= 8 and (nshards == 1 or shared >= 4), "tuples held on more than one shard were folded"


def test_a_tuple_held_on_two_shards_and_a_union_that_overflows_while_no_shard_does():
    n = 600
    m = wam.Model(wam.node_ids(n, 12500))
    m.set(FB, np.arange(n), np.arange(n) % 7)
    m.set(FK, np.arange(n), (np.arange(n) // 2) * 1000003 - 3 * 10**8)        # a key per pair of nodes
    m.set(F1, np.arange(n), np.arange(n) % 2)                                 # ... and the pair's two nodes apart: every node its own tuple
    L = bmx.load_library()
    owner = np.array([L.bmx_owner_of(int(i), 2) for i in m.ids])
    per = np.bincount(owner, minlength=2)
    cap = int(per.max())
    assert 0 < per.min() and cap < n
    with bmx.Comm([0, 0], 16 * n) as c:
        wam.load(c, m, [FB, FK, F1])
        every = [[(FB, 0, 6)]]
        for g in range(2):
            recs, res = _shard_answer(c, g, FB, every, [FK, F1], FB, cap)
            assert int(res["flags"]) == 0 and len(recs) == per[g], "no single shard overflows"
        out, res = mm.raw_mgroup(c, FB, every, [FK, F1], FB, cap)
        assert mm.check(out, res, *mm.answer(m, FB, every, [FK, F1], FB, cap), cap) is None
        assert int(res["flags"]) == bmx.GROUP_OVERFLOW and int(res["n_groups"]) == n and int(res["total"]["n_match"]) == n
        g = c.where_group_multi(FB, every, [FK, F1], FB, cap=n)
        assert not g.overflow and g.n_groups == n and list(g.groups) == sorted(g.groups) and g.total.n_match == n
        assert c.where_group_multi(FB, every, [FK, F1], cap=cap).overflow
        # by the pair's key and a bucket that unites the two: 300 tuples of two nodes each, most of them with a node on either shard
        split = int(((owner[0::2] != owner[1::2])).sum())
        assert split >= 50
        keys = [FK, (F1, 0, 2)]
        parts = [_shard_answer(c, s, FB, every, keys, FB, n)[0] for s in range(2)]
        assert len(parts[0]) + len(parts[1]) == n // 2 + split
        out, res = mm.raw_mgroup(c, FB, every, keys, FB, n // 2)
        assert mm.check(out, res, *mm.answer(m, FB, every, keys, FB, n // 2), n // 2) is None
        assert int(res["n_groups"]) == n // 2 and (out["agg"]["n_match"][:n // 2] == 2).all()
