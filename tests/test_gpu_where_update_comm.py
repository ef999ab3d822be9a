"""GPU: bmx_comm_where_update. The same rows on 1, 2 and 4 logical shards against one engine: after every call the dumps are equal bit for bit and every word of
the record is the model's, shard after shard in each shard's own index order; the cursor crosses a shard boundary, a cap runs out inside the second shard, and the
cursor ends at (nshards - 1, that shard's index size)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import rows_model as rm
import update_model as um
import where_agg_model as wam
from update_model import ADD, COPY, DELETE, SET, VAL_DELETED

F = rm.names()
FB, F1, F2, F3, NOBODY = F["base"], F["one"], F["two"], F["three"], F["nobody"]
PROG = [[(FB, 0, 6), (F1, 0, 3)], [(F2, 2, 5), (FB, 3, 11)]]


def _shard_engine(c, g):
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    return s


def _model(m, orders, start, cap, args):
    """the shards one after the other from the cursor on, each with the room that is left -> (table, summed record, ids, (next_shard, next_pos))"""
    tot = {k: 0 for k in um.WORDS}
    ids, cur, cut, nxt = [], m, False, (len(orders) - 1, len(orders[-1]))
    for g, o in enumerate(orders):
        if g < start[0]:
            continue
        cur, r, i = um.update(cur, o, *args, start=start[1] if g == start[0] else 0, cap=cap - tot["n_sent"])
        for k in ("n_match", "n_nosrc", "n_range", "n_sent", "n_applied"):
            tot[k] += r[k]
        ids.append(i)
        if not cut:
            nxt = (g, r["next_pos"])
            cut = r["n_match"] - r["n_nosrc"] - r["n_range"] > r["n_sent"]
    tot["n_rows"] = um.n_rows(cur); tot["next_pos"] = nxt[1]
    return cur, tot, np.concatenate(ids) if ids else np.zeros(0, np.uint64), nxt


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = rm.seeded_table()
    every = [FB, F1, F2, F3] + F["more"]
    with bmx.Engine(16 * m.N * len(every)) as e, bmx.Comm([0] * nshards, 16 * m.N * len(every)) as c:
        for x in (e, c):
            wam.load(x, m, every)
        for f, idx in tombs.items():
            if len(idx):
                ts = m.clk[f][idx] + 1000
                for x in (e, c):
                    x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), ts, np.full(len(idx), VAL_DELETED, np.int64))
                m.tomb(f, idx, ts)
        shards = [_shard_engine(c, g) for g in range(nshards)]
        try:
            orders = [s.index_ids(FB) for s in shards]
            sizes = [len(o) for o in orders]
            assert sum(sizes) == e.index_size(FB) and min(sizes) > 0

            def call(target, op, operand, src, ts, force, start=(0, 0), cap=None):
                nonlocal m
                args = (FB, PROG, target, op, operand, src, ts, force)
                room = sum(sizes) if cap is None else cap
                cur, want, wids, nxt = _model(m, orders, start, room, args)
                got = um.raw_update(c, *args, start=start, cap=room)
                assert um.same(got, (None, want, wids)) is None, (args[2:], start, cap, um.same(got, (None, want, wids)))
                assert (int(got[1]["next_shard"]), int(got[1]["next_pos"])) == nxt
                assert int(got[1]["layout"]) == sum(int(um.raw_update(s, FB, PROG, NOBODY, SET, 0, None, 0, cap=0)[1]["layout"]) for s in shards), "the sum of all stamps"
                # one engine holding the same rows: the same nodes in one call, whatever its own order is, when nothing is cut off
                if cap is None and start == (0, 0):
                    one = e.where_update(*args[:4], operand, src, ts, force, want_ids=True)
                    assert (one.n_match, one.n_nosrc, one.n_range, one.n_sent, one.n_applied, one.n_rows) == tuple(want[k] for k in um.WORDS[:6])
                    assert sorted(one.ids.tolist()) == sorted(wids.tolist())
                else:                                                # a page: the engine takes the route that was there before, with the nodes the model names
                    _apply_to_engine(e, m, cur, target)
                m = cur
                assert np.array_equal(um.dump_sorted(c), um.state_rows(m)), "the shards against the model"
                assert np.array_equal(um.dump_sorted(c), um.dump_sorted(e)), "the shards against one engine, bit for bit"
                assert c.row_count() == e.row_count() == um.n_rows(m)
                return got[1]

            r = call(F3, COPY, 0, F1, 3000, False)
            n = int(r["n_sent"])
            assert n > 2 * nshards and (int(r["next_shard"]), int(r["next_pos"])) == (nshards - 1, sizes[-1])
            call(F1, ADD, 1, F1, 3001, False)
            call(NOBODY, SET, 5, None, 0, False)
            call(F2, DELETE, 0, None, 3002, True)
            call(FB, ADD, 1, FB, 3003, True)
            # the cap runs out inside the second shard (or the only one); then pages across the boundaries until everything is sent
            per = [um.update(m, o, FB, PROG, F3, SET, 9, None, 4000)[1]["n_sent"] for o in orders]
            cap = per[0] + max(per[1] // 2, 1) if nshards > 1 else max(per[0] // 2, 1)
            r = call(F3, SET, 9, None, 4000, False, cap=cap)
            assert int(r["n_sent"]) == cap and int(r["next_shard"]) == min(1, nshards - 1) and int(r["next_pos"]) < sizes[int(r["next_shard"])]
            start, pages = (int(r["next_shard"]), int(r["next_pos"])), 0
            while True:
                r = call(F3, SET, 9, None, 4000, False, start=start, cap=max(min(per) // 2, 1))
                pages += 1
                if int(r["n_match"]) - int(r["n_nosrc"]) - int(r["n_range"]) <= int(r["n_sent"]):
                    break
                start = (int(r["next_shard"]), int(r["next_pos"]))
            assert pages > 1 and (int(r["next_shard"]), int(r["next_pos"])) == (nshards - 1, sizes[-1])
            # a cursor in the last shard: the shards in front of it are no candidates
            r = call(F3, SET, 11, None, 5000, False, start=(nshards - 1, 0), cap=sizes[-1])
            assert int(r["n_match"]) == um.records(m, orders[-1], FB, PROG, F3, SET, 11)[3]
            # the Python surface, and the one refusal that needs a communicator
            a = c.where_update(FB, PROG, F3, SET, 12, ts=6000, want_ids=True)
            assert a.n_sent == a.n_applied == len(a.ids) > 0 and (a.next_shard, a.next_pos) == (nshards - 1, sizes[-1])
            res = np.full(72, 0x5A, np.uint8)
            args = (*bmx._where_args(FB, PROG), *bmx._upd_args(F3, SET, 1, None, 7000, False))
            assert c.L.bmx_comm_where_update(c.h, *args, nshards, 0, 0, None, C.c_void_p(res.ctypes.data)) == bmx.ERR_INVALID
            assert b"start_shard" in c.L.bmx_comm_last_error(c.h) and (res == 0x5A).all()
        finally:
            for s in shards:
                s.h = None                                                   # the communicator owns the contexts


def _apply_to_engine(e, before, after, target):
    """what a page changed in the model's target field, stored as given on the single engine"""
    before._f(target); after._f(target)
    i = np.nonzero((before.st[target] != after.st[target]) | (before.clk[target] != after.clk[target]) | (before.val[target] != after.val[target]))[0]
    if len(i):
        e.put_rows(after.ids[i], np.full(len(i), target, np.uint32), after.clk[target][i], np.where(after.st[target][i] == um.TOMB, VAL_DELETED, after.val[target][i]))
