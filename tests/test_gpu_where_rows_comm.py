"""GPU: bmx_comm_where_rows. The same rows on 1, 2 and 4 logical shards: the union of the rows equals one engine's, the shards' rows come one shard after the
other in each shard's own index order, pages cross shard boundaries with a cap smaller than a shard's share, n_match counts from the cursor on and the cursor
ends at (nshards - 1, that shard's index size)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import rows_model as rm
import where_agg_model as wam


def _shard_engine(c, g):
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    return s


def _rowset(ids, vals, ts):
    return {(int(i),) + tuple(vals[:, k].tolist()) + tuple(ts[:, k].tolist()) for k, i in enumerate(ids)}


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = rm.seeded_table()
    F = rm.names()
    FB = F["base"]
    every = [FB, F["one"], F["two"], F["three"]] + F["more"]
    with bmx.Engine(16 * m.N * len(every)) as e, bmx.Comm([0] * nshards, 16 * m.N * len(every)) as c:
        for x in (e, c):
            wam.load(x, m, every)
        rm.apply_tombs(m, dict(tombs), e)
        for f, idx in tombs.items():                                         # the same tombstones on the shards (the model has them already)
            if len(idx):
                c.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), m.clk[f][idx], np.full(len(idx), rm.VAL_DELETED, np.int64))
        shards = [_shard_engine(c, g) for g in range(nshards)]
        try:
            orders = [s.index_ids(FB) for s in shards]
            sizes = [len(o) for o in orders]
            assert sum(sizes) == e.index_size(FB) and min(sizes) > 0
            layouts = [int(rm.raw_rows(s, FB, [[(FB, 0, 0)]], [], False, 0, 0)[3]["layout"]) for s in shards]
            seen = 0
            for k, (p, fields) in enumerate(rm.seeded_cases()[::4]):
                want = [rm.rows(m, o, FB, p, fields, True) for o in orders]                      # shard by shard, each in its own index order
                nm = sum(w[3] for w in want)
                one = rm.raw_rows(e, FB, p, fields, True, 0, e.index_size(FB))
                got = rm.raw_rows(c, FB, p, fields, True, (0, 0), nm + 1)
                r = got[3]
                assert (int(r["n_match"]), int(r["n_out"]), int(r["next_shard"]), int(r["next_pos"])) == (nm, nm, nshards - 1, sizes[-1]), (k, r)
                assert int(r["layout"]) == sum(layouts)
                assert np.array_equal(got[0], np.concatenate([w[0] for w in want])) and np.array_equal(got[1], np.concatenate([w[1] for w in want], axis=1))
                assert np.array_equal(got[2], np.concatenate([w[2] for w in want], axis=1))
                assert int(one[3]["n_match"]) == nm and _rowset(*got[:3]) == _rowset(*one[:3]), "the union of the rows equals one engine's"
                # counting alone, and counting from a cursor in a later shard
                r0 = rm.raw_rows(c, FB, p, fields, True, (0, 0), 0)[3]
                first = next((g for g in range(nshards) if want[g][3]), nshards - 1)
                assert int(r0["n_match"]) == nm and int(r0["next_shard"]) == first
                assert int(r0["next_pos"]) == (rm.rows(m, orders[first], FB, p, [], False, 0, 0)[4] if nm else sizes[-1])
                rl = rm.raw_rows(c, FB, p, fields, False, (nshards - 1, 0), 0)[3]
                assert int(rl["n_match"]) == want[-1][3] and int(rl["layout"]) == sum(layouts), "shards in front of the cursor are no candidates; every stamp counts"
                # pages smaller than a shard's share, across the shard boundaries
                if nm > 2 * nshards:
                    seen += 1
                    cap = max(min(w[3] for w in want if w[3]) // 2, 1) if nshards > 1 else 3
                    ids, vals, ts, start, pages = [], [], [], (0, 0), 0
                    while True:
                        g = rm.raw_rows(c, FB, p, fields, True, start, cap)
                        assert int(g[3]["n_match"]) == nm - sum(len(x) for x in ids) and int(g[3]["layout"]) == sum(layouts)
                        ids.append(g[0]); vals.append(g[1]); ts.append(g[2]); pages += 1
                        start = (int(g[3]["next_shard"]), int(g[3]["next_pos"]))
                        if int(g[3]["n_match"]) == int(g[3]["n_out"]):
                            break
                    assert start == (nshards - 1, sizes[-1]) and pages == -(-nm // cap)
                    assert np.array_equal(np.concatenate(ids), got[0]) and np.array_equal(np.concatenate(vals, axis=1), got[1]) and np.array_equal(np.concatenate(ts, axis=1), got[2])
            assert seen >= 8
            # the Python surface, and the one refusal that needs a communicator
            p, fields = rm.seeded_cases()[8]
            a = c.where_rows(FB, p, fields, with_ts=True)
            b = c.where_rows(FB, p, fields, cap=2, start=(0, 0))
            assert a.n_out == a.n_match and np.array_equal(a.ids[:2], b.ids) and b.vals.shape == (len(fields), min(2, a.n_match)) and b.ts is None
            res = np.full(40, 0x5A, np.uint8)
            args = (*bmx._where_args(FB, p), 0, None, 0)
            assert c.L.bmx_comm_where_rows(c.h, *args, nshards, 0, 0, None, None, None, C.c_void_p(res.ctypes.data)) == bmx.ERR_INVALID
            assert b"start_shard" in c.L.bmx_comm_last_error(c.h) and (res == 0x5A).all()
        finally:
            for s in shards:
                s.h = None                                                   # the communicator owns the contexts
