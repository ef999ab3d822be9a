"""GPU: bmx_comm_where_group_top. The same rows on 1, 2 and 4 logical shards give one engine's sorted answer, bit for bit, and bmx.gtop_merge of the per-shard
answers; a key whose ranks alternate between the shards; a tie across shards at the cut decided by the id; a union that overflows while no single shard does
raises the flag and writes nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import gtop_model as tm
import where_agg_model as wam
from where_agg_model import Model

F = tm.names()
FB, FG, FO, F1, F2, F3, NOBODY = F["base"], F["group"], F["order"], F["one"], F["two"], F["three"], F["nobody"]
EVERY = [[(NOBODY, 0, 0, True)]]


def _shard(c, g):
    """shard g's own context as an Engine (the communicator owns it)"""
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    return s


def _shard_answer(c, g, base, p, group, order, per, fields, desc, with_ts, cap):
    """-> (groups, rows (D, per), vals (nf, D, per), ts, res) of shard g alone"""
    s = _shard(c, g)
    try:
        out, rows, vals, ts, res = tm.raw_gtop(s, base, p, group, order, per, fields, desc, with_ts, cap)
        d = 0 if int(res["flags"]) else int(res["n_groups"])
        nf = len(fields)
        return out[:d].copy(), rows[:d * per].reshape(d, per).copy(), vals[:, :d * per].reshape(nf, d, per).copy(), ts[:, :d * per].reshape(nf, d, per).copy(), res
    finally:
        s.h = None


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = tm.seeded_model()
    fields = [FB, F1, F2, F3, FG, FO]
    with bmx.Engine(16 * m.N) as e, bmx.Comm([0] * nshards, 16 * m.N) as c:
        for x in (e, c):
            wam.load(x, m, fields)
        for f, idx in tombs.items():
            wam.tombstone(e, m, f, idx)
            c.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), wam.VAL_DELETED, np.int64))
        for per in tm.PERS:
            for k, (p, group, order, desc) in enumerate(tm.seeded_queries(m, per)[::6]):
                proj = (order, FB, F1)[: k % 4]
                for cap in (64, 3):
                    one = tm.raw_gtop(e, FB, p, group, order, per, proj, desc, True, cap)
                    many = tm.raw_gtop(c, FB, p, group, order, per, proj, desc, True, cap)
                    want = tm.answer(m, FB, p, group, order, per, proj, desc, cap, True)
                    bad = tm.check(many, want, cap, per, len(proj), True)
                    assert bad is None, (k, cap, bad)
                    if not int(want[4]["flags"]):
                        assert _same(many, one), "one engine's answer, bit for bit"
                        parts = [_shard_answer(c, g, FB, p, group, order, per, proj, desc, True, cap) for g in range(nshards)]
                        grps, rows, vals, ts = bmx.gtop_merge([x[:4] for x in parts], per, desc)
                        assert grps.tobytes() == want[0].tobytes() and rows.tobytes() == want[1].tobytes() and np.array_equal(vals, want[2]) and np.array_equal(ts, want[3]), "gtop_merge of the shards' answers"
                        assert sum(int(x[4]["total"]) for x in parts) == int(want[4]["total"])


def test_ranks_alternating_between_shards_and_a_tie_across_shards_at_the_cut():
    L = bmx.load_library()
    ids = np.sort(wam.node_ids(400, 141000))
    owner = np.array([L.bmx_owner_of(int(i), 2) for i in ids])
    a, b = ids[owner == 0][:20], ids[owner == 1][:20]
    # group 1: ranks 1, 3, 5, 7 on shard 0 and 2, 4, 6 on shard 1 by value; group 2: four nodes tie, two on each shard; group 3: members on both, a contender on neither
    nodes = np.concatenate([a[:4], b[:3], a[4:6], b[3:5], a[6:8], b[5:6]])
    m = Model(nodes)
    n = len(nodes)
    m.set(FB, np.arange(n), np.arange(n))
    m.set(FG, np.arange(n), [1] * 7 + [2] * 4 + [3] * 3)
    m.set(FO, np.arange(11), [10, 30, 50, 70, 20, 40, 60] + [4] * 4)
    m.set(F1, np.arange(n), 1000 + np.arange(n))
    tie = sorted(int(x) for x in nodes[7:11])
    with bmx.Engine(4096) as e, bmx.Comm([0, 0], 4096) as c:
        for x in (e, c):
            wam.load(x, m, [FB, FG, FO, F1])
        for desc in (False, True):
            for per in (2, 3, 5, 16):
                want = tm.ask(c, m, FB, EVERY, FG, FO, per, (F1, FO), desc, True, 8)
                assert _same(tm.raw_gtop(c, FB, EVERY, FG, FO, per, (F1, FO), desc, True, 8), tm.raw_gtop(e, FB, EVERY, FG, FO, per, (F1, FO), desc, True, 8))
                grps, rows, vals = want[0], want[1], want[2]
                assert grps["key"].tolist() == [1, 2, 3] and grps["n_match"].tolist() == [7, 4, 3] and grps["n"].tolist() == [7, 4, 0]
                assert rows[1]["id"][:min(per, 4)].tolist() == tie[:per], "the tie across the shards goes by the id, and the cut falls inside it"
                order = [0, 4, 1, 5, 2, 6, 3][::-1 if desc else 1][:per]
                assert rows[0]["id"][:len(order)].tolist() == [int(nodes[j]) for j in order] and vals[0, 0, :len(order)].tolist() == [1000 + j for j in order], "each row brings its shard's cells"
        for g, cnt in ((0, 4), (1, 3)):
            part = _shard_answer(c, g, FB, EVERY, FG, FO, 16, (), False, False, 8)
            assert int(part[0][0]["n"]) == cnt and int(part[0][0]["n_rows"]) == cnt


def test_a_union_that_overflows_while_no_shard_does():
    n = 600
    m = Model(wam.node_ids(n, 142000))
    m.set(FB, np.arange(n), np.arange(n) % 7)
    m.set(FG, np.arange(n), np.arange(n) * 1000003 - 3 * 10**8)               # every node its own key
    m.set(FO, np.arange(0, n, 2), np.arange(0, n, 2))
    L = bmx.load_library()
    owner = np.array([L.bmx_owner_of(int(i), 2) for i in m.ids])
    cnt = np.bincount(owner, minlength=2)
    cap = int(cnt.max())
    assert 0 < cnt.min() and cap < n
    with bmx.Comm([0, 0], 16 * n) as c:
        wam.load(c, m, [FB, FG, FO])
        every = [[(FB, 0, 6)]]
        for g in range(2):
            part = _shard_answer(c, g, FB, every, FG, FO, 2, (FO,), False, True, cap)
            assert int(part[4]["flags"]) == 0 and len(part[0]) == cnt[g], "no single shard overflows"
        want = tm.ask(c, m, FB, every, FG, FO, 2, (FO,), False, True, cap)
        assert int(want[4]["flags"]) == tm.OVERFLOW
        got = tm.raw_gtop(c, FB, every, FG, FO, 2, (FO,), False, True, cap)[4]
        assert int(got["n_groups"]) == n and int(got["total"]) == n and int(got["n_ordered"]) == n // 2 and int(got["n_rows"]) == 0
        r = c.where_group_top(FB, every, FG, FO, 2, fields=(FO,), cap=n)
        assert not r.overflow and r.n_groups == n and list(r.top) == sorted(r.top) and r.total == n and r.n_rows == n // 2 and sum(len(v) for v in r.top.values()) == n // 2
        assert c.where_group_top(FB, every, FG, FO, 2, cap=cap).overflow
