"""GPU: bmx_comm_where_group. The same rows on 1, 2 and 4 logical shards give one engine's sorted answer, byte for byte, and bmx.group_merge of the per-shard
answers; a union that overflows while no single shard does raises the flag and writes nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import group_model as gm
import where_agg_model as wam

F = gm._names()
FB, FK, FM = F["base"], F["key"], F["measure"]
ALL_FIELDS = [FB, F["one"], F["two"], F["three"], F["four"], F["five"], FM, FK] + F["more"]


def _shard_answer(c, g, base, clauses, group, measure, cap):
    """bmx_where_group on shard g's own context"""
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    try:
        out, res = gm.raw_group(s, base, clauses, group, measure, cap)
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
        seen = 0
        for k, (p, group, measure) in enumerate(gm.seeded_queries()[::3]):
            for cap in (512, 3):
                one = gm.raw_group(e, FB, p, group, measure, cap)
                many = gm.raw_group(c, FB, p, group, measure, cap)
                want = gm.answer(m, FB, p, group, measure, cap)
                assert gm.check(*many, *want, cap) is None, (k, cap, gm.check(*many, *want, cap))
                if not int(want[1]["flags"]):
                    assert many[0].tobytes() == one[0].tobytes() and many[1].tobytes() == one[1].tobytes(), "one engine's answer, byte for byte"
                    parts = [_shard_answer(c, g, FB, p, group, measure, cap) for g in range(nshards)]
                    merged = bmx.group_merge([x[0] for x in parts])
                    assert merged.tobytes() == want[0].tobytes(), "group_merge of the shards' answers"
                    assert sum(int(x[1]["total"]["n_match"]) for x in parts) == int(want[1]["total"]["n_match"])
                    seen += len(merged) >= 2
        assert seen >= 8


def test_a_union_that_overflows_while_no_shard_does():
    n = 600
    m = wam.Model(wam.node_ids(n, 12000))
    m.set(FB, np.arange(n), np.arange(n) % 7)
    m.set(FK, np.arange(n), np.arange(n) * 1000003 - 3 * 10**8)               # every node its own key
    L = bmx.load_library()
    owner = np.array([L.bmx_owner_of(int(i), 2) for i in m.ids])
    per = np.bincount(owner, minlength=2)
    cap = int(per.max())
    assert 0 < per.min() and cap < n
    with bmx.Comm([0, 0], 16 * n) as c:
        wam.load(c, m, [FB, FK])
        every = [[(FB, 0, 6)]]
        for g in range(2):
            recs, res = _shard_answer(c, g, FB, every, FK, FB, cap)
            assert int(res["flags"]) == 0 and len(recs) == per[g], "no single shard overflows"
        out, res = gm.raw_group(c, FB, every, FK, FB, cap)
        assert gm.check(out, res, *gm.answer(m, FB, every, FK, FB, cap), cap) is None
        assert int(res["flags"]) == bmx.GROUP_OVERFLOW and int(res["n_groups"]) == n and int(res["total"]["n_match"]) == n
        g = c.where_group(FB, every, FK, FB, cap=n)
        assert not g.overflow and g.n_groups == n and list(g.groups) == sorted(g.groups) and g.total.n_match == n
        assert c.where_group(FB, every, FK, cap=cap).overflow
