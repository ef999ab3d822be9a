"""GPU: bmx_comm_where_group_first. The same rows on 1, 2 and 4 logical shards give one engine's sorted answer, bit for bit, and bmx.first_merge of the per-shard
answers; a group whose winner lives on another shard than most of its members; a tie across shards decided by the id; a union that overflows while no single
shard does raises the flag and writes nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import first_model as fm
import where_agg_model as wam
from where_agg_model import Model

F = fm.names()
FB, FG, FO, F1, F2, F3, NOBODY = F["base"], F["group"], F["order"], F["one"], F["two"], F["three"], F["nobody"]
EVERY = [[(NOBODY, 0, 0, True)]]


def _shard(c, g):
    """shard g's own context as an Engine (the communicator owns it)"""
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    return s


def _shard_answer(c, g, *args):
    s = _shard(c, g)
    try:
        out, vals, ts, res = fm.raw_first(s, *args)
        d = 0 if int(res["flags"]) else int(res["n_groups"])
        return out[:d].copy(), vals[:, :d].copy(), ts[:, :d].copy(), res
    finally:
        s.h = None


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = fm.seeded_model()
    fields = [FB, F1, F2, F3, FG, FO]
    with bmx.Engine(16 * m.N) as e, bmx.Comm([0] * nshards, 16 * m.N) as c:
        for x in (e, c):
            wam.load(x, m, fields)
        for f, idx in tombs.items():
            wam.tombstone(e, m, f, idx)
            c.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), wam.VAL_DELETED, np.int64))
        for k, (p, group, order, desc) in enumerate(fm.seeded_queries(m)[::4]):
            proj = (order, FB, F1)[: k % 4]
            for cap in (64, 3):
                one = fm.raw_first(e, FB, p, group, order, proj, desc, True, cap)
                many = fm.raw_first(c, FB, p, group, order, proj, desc, True, cap)
                want = fm.answer(m, FB, p, group, order, proj, desc, cap, True)
                bad = fm.check(many, want, cap, len(proj), True)
                assert bad is None, (k, cap, bad)
                if not int(want[3]["flags"]):
                    assert _same(many, one), "one engine's answer, bit for bit"
                    parts = [_shard_answer(c, g, FB, p, group, order, proj, desc, True, cap) for g in range(nshards)]
                    recs, vals, ts = bmx.first_merge([x[:3] for x in parts], desc)
                    assert recs.tobytes() == want[0].tobytes() and np.array_equal(vals, want[1]) and np.array_equal(ts, want[2]), "first_merge of the shards' answers"
                    assert sum(int(x[3]["total"]) for x in parts) == int(want[3]["total"])


def test_winner_on_another_shard_and_a_tie_across_shards():
    L = bmx.load_library()
    ids = wam.node_ids(400, 131000)
    owner = np.array([L.bmx_owner_of(int(i), 2) for i in ids])
    a, b = ids[owner == 0][:20], ids[owner == 1][:20]
    # group 1: nine members on shard 0, the winner alone on shard 1; group 2: one tying contender on each shard; group 3: members on both, a contender on neither
    nodes = np.concatenate([a[:9], b[:1], a[9:10], b[1:2], a[10:12], b[2:3]])
    m = Model(nodes)
    n = len(nodes)
    m.set(FB, np.arange(n), np.arange(n))
    m.set(FG, np.arange(n), [1] * 10 + [2] * 2 + [3] * 3)
    m.set(FO, np.arange(12), [50 + k for k in range(9)] + [7] + [4, 4])
    m.set(F1, np.arange(n), 1000 + np.arange(n))
    with bmx.Engine(4096) as e, bmx.Comm([0, 0], 4096) as c:
        for x in (e, c):
            wam.load(x, m, [FB, FG, FO, F1])
        for desc in (False, True):
            want = fm.ask(c, m, FB, EVERY, FG, FO, (F1, FO), desc, True, 8)
            assert _same(fm.raw_first(c, FB, EVERY, FG, FO, (F1, FO), desc, True, 8), fm.raw_first(e, FB, EVERY, FG, FO, (F1, FO), desc, True, 8))
            recs, vals = want[0], want[1]
            assert recs["key"].tolist() == [1, 2, 3] and recs["n_match"].tolist() == [10, 2, 3] and recs["n"].tolist() == [10, 2, 0]
            assert int(recs[1]["id"]) == int(min(nodes[10], nodes[11])) and int(recs[2]["id"]) == fm.NO_NODE, "the tie across the shards goes to the smaller id"
            if not desc:
                assert int(recs[0]["id"]) == int(b[0]) and vals[0, 0] == 1009, "the winner and its cells come from the shard that holds one member of ten"
        for g, cnt in ((0, 9), (1, 1)):
            part = _shard_answer(c, g, FB, EVERY, FG, FO, (), False, False, 8)
            assert int(part[0][0]["n_match"]) == cnt


def test_a_union_that_overflows_while_no_shard_does():
    n = 600
    m = Model(wam.node_ids(n, 132000))
    m.set(FB, np.arange(n), np.arange(n) % 7)
    m.set(FG, np.arange(n), np.arange(n) * 1000003 - 3 * 10**8)               # every node its own key
    m.set(FO, np.arange(0, n, 2), np.arange(0, n, 2))
    L = bmx.load_library()
    owner = np.array([L.bmx_owner_of(int(i), 2) for i in m.ids])
    per = np.bincount(owner, minlength=2)
    cap = int(per.max())
    assert 0 < per.min() and cap < n
    with bmx.Comm([0, 0], 16 * n) as c:
        wam.load(c, m, [FB, FG, FO])
        every = [[(FB, 0, 6)]]
        for g in range(2):
            part = _shard_answer(c, g, FB, every, FG, FO, (FO,), False, True, cap)
            assert int(part[3]["flags"]) == 0 and len(part[0]) == per[g], "no single shard overflows"
        want = fm.ask(c, m, FB, every, FG, FO, (FO,), False, True, cap)
        assert int(want[3]["flags"]) == fm.OVERFLOW
        got = fm.raw_first(c, FB, every, FG, FO, (FO,), False, True, cap)[3]
        assert int(got["n_groups"]) == n and int(got["total"]) == n and int(got["n_ordered"]) == n // 2
        r = c.where_group_first(FB, every, FG, FO, fields=(FO,), cap=n)
        assert not r.overflow and r.n_groups == n and list(r.first) == sorted(r.first) and r.total == n and sum(v is not None for v in r.first.values()) == n // 2
        assert c.where_group_first(FB, every, FG, FO, cap=cap).overflow
