"""GPU: bmx_comm_where_join_rows and bmx_comm_where_map_rows. The same rows on 1, 2 and 4 logical shards: the rows equal one engine's as a set, they come shard
after shard in each shard's own index order with the map being the union of the shards' maps, pages cross the shard boundaries, a key held only on another
shard than its linker is found, an inner node owned by a third shard delivers its cells, the smallest id is taken across shards, a union above map_cap while
every shard is below it raises the flag and writes nothing, and start_shard >= nshards is refused."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import join_model as jm
import join_rows_model as jrm
import where_agg_model as wam
from join_rows_model import EVERY, NO_NODE, Q, QMAP, Table

COLS = ("ids", "vals", "ts", "in_ids", "in_vals", "in_ts")


def _shard(c, g):
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    return s


def _orders(c, n, base):
    shards = [_shard(c, g) for g in range(n)]
    try:
        return [s.index_ids(base) for s in shards]
    finally:
        for s in shards:
            s.h = None                                                   # the communicator owns the contexts


def _ask(c, m, orders, q, start_shard=0):
    got, want = jrm.raw(c, q, start_shard), jrm.comm_answer(m, orders, q, start_shard)
    bad = jrm.check(got, want, q)
    assert bad is None, (bad, start_shard, {k: v for k, v in q.items() if k not in ("keys", "ids")})
    assert int(got["res"]["next_shard"]) == int(want["res"]["next_shard"])
    return got


def _rowset(g):
    return sorted((int(i),) + tuple(g["vals"][:, k].tolist()) + tuple(g["ts"][:, k].tolist()) + (int(g["in_ids"][k]),) + tuple(g["in_vals"][:, k].tolist()) + tuple(g["in_ts"][:, k].tolist())
                  for k, i in enumerate(g["ids"]))


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = jrm.seeded_model()
    with bmx.Engine(16 * m.N) as e, bmx.Comm([0] * nshards, 16 * m.N) as c:
        wam.load(e, m, jm.ALL_FIELDS); wam.load(c, m, jm.ALL_FIELDS)
        jrm.apply_tombs(m, dict(tombs), e)
        for f, idx in tombs.items():                                         # the same tombstones on the shards (the model has them already)
            c.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), m.clk[f][idx], np.full(len(idx), jrm.VAL_DELETED, np.int64))
        orders = _orders(c, nshards, jm.FB)
        sizes = [len(o) for o in orders]
        total = e.index_size(jm.FB)
        assert sum(sizes) == total and min(sizes) > 0
        seen = 0
        for k, q0 in enumerate(jrm.seeded_pairs()[::5]):
            q = dict(q0, with_ts=True, cap=total)
            got = _ask(c, m, orders, q)
            one = jrm.raw(e, q)
            r = got["res"]
            assert _rowset(got) == _rowset(one) and all(int(r[x]) == int(one["res"][x]) for x in ("n_match", "n_out", "n_joined", "map_size", "n_inner", "n_keyed", "flags"))
            assert (int(r["next_shard"]), int(r["next_pos"])) == (nshards - 1, sizes[-1])
            over = _ask(c, m, orders, dict(q, map_cap=3))
            if int(over["res"]["flags"]):
                assert (int(over["res"]["next_shard"]), int(over["res"]["next_pos"]), int(over["res"]["layout"])) == (nshards - 1, sizes[-1], int(r["layout"]))
            nm = int(r["n_match"])
            r0 = _ask(c, m, orders, dict(q, cap=0))["res"]
            assert int(r0["n_match"]) == nm
            _ask(c, m, orders, dict(q, cap=7), nshards - 1)                  # shards in front of the cursor are no candidates
            ql = jrm.as_list(m, q)
            if ql is not None:
                gl = _ask(c, m, orders, ql)
                assert all(np.array_equal(gl[x], got[x]) for x in COLS)
            if nm > 2 * nshards:                                             # pages smaller than a shard's share, across the shard boundaries
                seen += 1
                cap = max(nm // (2 * nshards) - 1, 1)
                parts, start = [], (0, 0)
                while True:
                    g = _ask(c, m, orders, dict(q, start=start[1], cap=cap), start[0])
                    assert int(g["res"]["n_match"]) == nm - sum(len(x["ids"]) for x in parts) and int(g["res"]["layout"]) == int(r["layout"])
                    parts.append(g)
                    start = (int(g["res"]["next_shard"]), int(g["res"]["next_pos"]))
                    if int(g["res"]["n_match"]) == int(g["res"]["n_out"]):
                        break
                assert start == (nshards - 1, sizes[-1]) and len(parts) == -(-nm // cap)
                assert all(np.array_equal(np.concatenate([x[name] for x in parts], axis=(0 if name.endswith("ids") else 1)), got[name]) for name in COLS)
        assert seen >= 8
        # the Python surface, and the one refusal that needs a communicator
        q = jrm.seeded_pairs()[0]
        a = c.where_join_rows(q["base"], q["clauses"], q["link"], q["fields"], q["inner_base"], q["inner_clauses"], q["key"], q["in_fields"], with_ts=True)
        w = jrm.comm_answer(m, orders, dict(q, cap=total))
        assert a.n_out == a.n_match == int(w["res"]["n_match"]) and all(np.array_equal(getattr(a, x), w[x]) for x in COLS) and (a.next_shard, a.next_pos) == (nshards - 1, sizes[-1])
        k, i, _ = jrm.inner_pairs(m, q["inner_base"], q["inner_clauses"], q["key"])
        b = c.where_map_rows(q["base"], q["clauses"], q["link"], q["fields"], k, i, q["in_fields"], cap=2, inner=True)
        assert b.n_out == 2 and b.ts is None and b.n_joined == 2 and b.n_inner == len(k)
        res = np.full(72, 0x5A, np.uint8)
        head, mid, _ = jrm.call_args(dict(q, cap=0))
        assert c.L.bmx_comm_where_join_rows(c.h, *head, *mid, nshards, 0, 0, None, None, None, None, None, None, C.c_void_p(res.ctypes.data)) == bmx.ERR_INVALID
        assert b"start_shard" in c.L.bmx_comm_last_error(c.h) and (res == 0x5A).all()
        head, mid, keep = jrm.call_args(dict(jrm.as_list(m, q), cap=0))
        assert c.L.bmx_comm_where_map_rows(c.h, *head, *mid, nshards + 3, 0, 0, None, None, None, None, None, None, C.c_void_p(res.ctypes.data)) == bmx.ERR_INVALID
        assert b"start_shard" in c.L.bmx_comm_last_error(c.h) and (res == 0x5A).all()


def test_keys_and_inner_nodes_on_other_shards():
    FB, FL, FI, FK, FX = jrm.FB, jrm.FL, jrm.FI, jrm.FK, jrm.FX
    n, S = 600, 3
    m = Table(wam.node_ids(n, 87000))
    i = np.arange(n)
    L = bmx.load_library()
    owner = np.array([L.bmx_owner_of(int(x), S) for x in m.ids])
    per = np.bincount(owner, minlength=S)
    assert per.min() > 0
    on = [i[owner == g] for g in range(S)]
    # every node is an inner node with its own key, and an outer node whose link is the key of a node on the NEXT shard
    other = np.array([on[(owner[k] + 1) % S][k % len(on[(owner[k] + 1) % S])] for k in i])
    m.set(FB, i, i % 7, 5); m.set(FI, i, i % 5, 6); m.set(FK, i, 10_000 + i, 7); m.set(FL, i, 10_000 + other, 8); m.set(FX, i[i % 4 != 0], 3 * i[i % 4 != 0] - 500, 9 + i[i % 4 != 0] % 3)
    with bmx.Comm([0] * S, 16 * n) as c:
        wam.load(c, m, [FB, FI, FK, FL, FX])
        jrm.apply_tombs(m, {FX: i[i % 8 == 1]}, c)
        orders = _orders(c, S, FB)
        q = Q(FB, EVERY, FL, [FL], FI, EVERY, FK, [FX, FK], cap=n, map_cap=n)
        got = _ask(c, m, orders, q)
        assert int(got["res"]["n_joined"]) == n and int(got["res"]["map_size"]) == n
        assert np.array_equal(got["in_ids"], m.ids[other[m.index_of(got["ids"])]]) and (owner[m.index_of(got["in_ids"])] != owner[m.index_of(got["ids"])]).all()
        kinds = {("data" if v != jrm.VAL_DELETED else ("tomb" if t != jrm.NO_CLOCK else "absent")) for v, t in zip(got["in_vals"][0].tolist(), got["in_ts"][0].tolist())}
        assert kinds == {"data", "tomb", "absent"}
        _ask(c, m, orders, dict(q, inner=True, cap=50), 1)
        for g in range(S):                                                            # on its own, a shard finds none of its links
            s = _shard(c, g)
            try:
                r = jrm.raw(s, q)["res"]
                assert (int(r["n_joined"]), int(r["n_match"]), int(r["map_size"])) == (0, per[g], per[g])
            finally:
                s.h = None
        # an inner node owned by a third shard: the list names, for the links of shard 0's nodes, nodes of shard 2 (the keys' own nodes live on shard 1)
        keys = 10_000 + other[on[0]]
        third = on[2][np.arange(len(on[0])) % len(on[2])]
        gl = _ask(c, m, orders, QMAP(FB, EVERY, FL, [FL], keys, m.ids[third], [FX, FI], cap=n))
        assert int(gl["res"]["n_joined"]) == len(on[0]) and set(owner[m.index_of(gl["in_ids"][gl["in_ids"] != np.uint64(NO_NODE)])].tolist()) == {2}
        # every shard is below map_cap, the union is above it; and right behind it a query that fits
        map_cap = int(per.max())
        over = _ask(c, m, orders, dict(q, map_cap=map_cap))
        r = over["res"]
        assert (int(r["flags"]), int(r["n_out"]), int(r["map_size"]), int(r["n_inner"]), int(r["n_keyed"])) == (jrm.MAP_OVERFLOW, 0, n, n, n)
        _ask(c, m, orders, dict(q, inner_clauses=[[(FI, 0, 0)]]))
        # one key on all three shards: the smallest id across the shards, whichever shard holds it
        trio = [int(on[g][0]) for g in range(S)]
        m.set(FK, trio, 424242, 30); m.set(FL, i[:50], 424242, 30)
        c.put_rows(m.ids[trio], np.full(S, FK, np.uint32), np.full(S, 30, np.int64), np.full(S, 424242, np.int64))
        c.put_rows(m.ids[:50], np.full(50, FL, np.uint32), np.full(50, 30, np.int64), np.full(50, 424242, np.int64))
        got = _ask(c, m, orders, q)
        hit = got["vals"][0] == 424242
        assert hit.sum() == 50 and set(got["in_ids"][hit].tolist()) == {int(m.ids[trio].min())} and int(got["res"]["n_keyed"]) - int(got["res"]["map_size"]) == 2
        while len(trio) > 1:                                                          # ... and after the smallest leaves, the next smallest
            k = int(np.argmin(m.ids[trio]))
            gone = trio.pop(k)
            c.put_rows(m.ids[[gone]], np.full(1, FK, np.uint32), np.full(1, 40, np.int64), np.full(1, jrm.VAL_DELETED, np.int64))
            m.tomb(FK, [gone], 40)
            got = _ask(c, m, orders, q)
            assert set(got["in_ids"][got["vals"][0] == 424242].tolist()) == {int(m.ids[trio].min())}
