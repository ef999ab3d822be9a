"""GPU: bmx_comm_where_join_group and bmx_comm_where_map_group. The same rows on 1, 2 and 4 logical shards give the records and the result record one engine
gives, byte for byte; a key held only by inner nodes of another shard than the outer node's is found (the union of the shards' maps is what every shard looks
up); one key on two shards with different attributes takes the minimum across the shards; a union above map_cap while every shard is below it, and a record
union above cap while every shard is below it, raise their flags and write nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import join_model as jm
import where_agg_model as wam
from join_model import EVERY, FA, FB, FI, FK, FL, FM, Q, QMAP


def _load(x, m, tombs):
    wam.load(x, m, jm.ALL_FIELDS)
    for f, idx in tombs.items():
        x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), wam.VAL_DELETED, np.int64))


def _shard(c, g):
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    return s


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = jm.seeded_model()
    with bmx.Engine(16 * m.N) as e, bmx.Comm([0] * nshards, 16 * m.N) as c:
        for x in (e, c):
            _load(x, m, tombs)
        jm.apply_tombs(m, tombs)
        seen = 0
        for k, q0 in enumerate(jm.seeded_pairs()[::4]):
            for q in (q0, dict(q0, cap=3), dict(q0, map_cap=3), dict(q0, cap=3, map_cap=3)):
                want = jm.ask(c, m, q)
                one, many = jm.raw_of(e, q), jm.raw_of(c, q)
                if not int(want[1]["flags"]):
                    assert many[0].tobytes() == one[0].tobytes() and many[1].tobytes() == one[1].tobytes(), "one engine's answer, byte for byte"
                    seen += len(want[0]) > 0
            keys = jm.uid(np.arange(k, 900, 7))
            ql = QMAP(FB, q0["clauses"], q0["link"], keys, np.arange(len(keys)) % 13 - 6, q0["measure"], 32)
            jm.ask(c, m, ql)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(jm.raw_of(c, ql), jm.raw_of(e, ql)))
            jm.ask(c, m, dict(ql, cap=5))
        assert seen >= 12
        q = jm.seeded_pairs()[0]
        r = c.where_join_group(FB, q["clauses"], q["link"], FI, q["inner_clauses"], q["key"], q["attr"], measure=q["measure"], cap=1024, map_cap=1024)
        recs, res = jm.want_of(m, q)
        assert r.records.tobytes() == recs.tobytes() and (r.n_groups, r.map_size, r.n_inner, r.n_keyed, r.flags) == (len(recs), int(res["map_size"]), int(res["n_inner"]), int(res["n_keyed"]), 0)
        assert c.where_join_group(FB, q["clauses"], q["link"], FI, q["inner_clauses"], q["key"], q["attr"], map_cap=2).map_overflow
        r = c.where_map_group(FB, EVERY, FL, jm.uid(np.arange(40)), np.arange(40) % 3, measure=FM, cap=8)
        assert r.n_groups == 3 and r.records.tobytes() == jm.want_of(m, QMAP(FB, EVERY, FL, jm.uid(np.arange(40)), np.arange(40) % 3, FM, 8))[0].tobytes()


def test_keys_on_other_shards_and_unions_that_overflow():
    n = 600
    m = jm.Model(wam.node_ids(n, 77000))
    i = np.arange(n)
    L = bmx.load_library()
    owner = np.array([L.bmx_owner_of(int(x), 2) for x in m.ids])
    per = np.bincount(owner, minlength=2)
    assert 0 < per.min()
    # every node is an inner node with its own key and an outer node that links to the key of a node on the OTHER shard; the attribute: 40 values
    on0, on1 = i[owner == 0], i[owner == 1]
    other = np.where(owner == 0, on1[i % len(on1)], on0[i % len(on0)])
    m.set(FB, i, i % 7); m.set(FI, i, i % 5); m.set(FK, i, jm.uid(i)); m.set(FL, i, jm.uid(other)); m.set(FA, i, i % 40); m.set(FM, i, 3 * i - 500)
    with bmx.Comm([0, 0], 16 * n) as c:
        wam.load(c, m, [FB, FI, FK, FL, FA, FM])
        q = Q(FB, EVERY, FL, FI, EVERY, FK, FA, FM, cap=64, map_cap=n)
        recs, res = jm.ask(c, m, q)
        assert int(res["unmatched"]["n_match"]) == 0 and len(recs) == 40 and int(res["map_size"]) == n
        for g in range(2):                                                            # on its own, a shard finds none of its links
            s = _shard(c, g)
            try:
                _, r = jm.raw_of(s, q)
                assert (int(r["unmatched"]["n_match"]), int(r["n_groups"]), int(r["map_size"]), int(r["n_inner"])) == (per[g], 0, per[g], per[g])
            finally:
                s.h = None                                                            # the communicator owns the context
        # every shard is below map_cap, the union is above it
        map_cap = int(per.max())
        assert map_cap < n
        _, res = jm.ask(c, m, dict(q, map_cap=map_cap))
        out, r = jm.raw_of(c, dict(q, map_cap=map_cap))
        assert (int(r["flags"]), int(r["n_groups"]), int(r["map_size"]), int(r["n_inner"]), int(r["n_keyed"])) == (jm.MAP_OVERFLOW, 0, n, n, n)
        # ... and right behind it a query that fits
        jm.ask(c, m, dict(q, inner_clauses=[[(FI, 0, 0)]]))
        # every shard's records are below cap, their union is above it: the outer nodes of shard g link to keys whose attributes are 20 g .. 20 g + 19
        m.set(FA, i, 20 * owner[other] * 0 + 20 * (1 - owner) + i % 20)
        c.put_rows(m.ids, np.full(n, FA, np.uint32), np.full(n, 20, np.int64), m.val[FA])
        attrs_seen = [np.unique(m.val[FA][other[owner == g]]) for g in range(2)]
        assert all(len(a) == 20 for a in attrs_seen) and len(np.unique(np.concatenate(attrs_seen))) == 40
        _, res = jm.ask(c, m, dict(q, cap=20))
        assert int(res["flags"]) == jm.GROUP_OVERFLOW
        jm.ask(c, m, dict(q, cap=40))
        # one key on two shards with different attributes: the minimum across the shards, whichever shard holds it
        a, b = int(on0[0]), int(on1[0])
        for va, vb in ((-7, 900), (900, -7)):
            for node, v in ((a, va), (b, vb)):
                m.set(FK, [node], 424242); m.set(FA, [node], v)
            c.put_rows(m.ids[[a, b]], np.full(2, FK, np.uint32), np.full(2, 30 + (va > 0), np.int64), np.full(2, 424242, np.int64))
            c.put_rows(m.ids[[a, b]], np.full(2, FA, np.uint32), np.full(2, 30 + (va > 0), np.int64), np.array([va, vb], np.int64))
            m.set(FL, i[:50], 424242)
            c.put_rows(m.ids[:50], np.full(50, FL, np.uint32), np.full(50, 30 + (va > 0), np.int64), np.full(50, 424242, np.int64))
            recs, res = jm.ask(c, m, dict(q, cap=64))
            assert -7 in recs["key"] and 900 not in recs["key"] and int(res["n_keyed"]) - int(res["map_size"]) == 1
