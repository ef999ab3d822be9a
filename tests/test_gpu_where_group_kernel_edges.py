"""GPU: the group-by kernels at their edges (csrc/group_kernels.h). Every layout of group_model.edge_layouts is laid out BY POSITION of the base field's index
(index_ids), so the test knows which wave, lane and workgroup meets which key; the path tags the layout is there for are asserted on the sequential stand-in of
group_model.py before the query runs, and the answer is compared exactly with the brute-force answer: keys that share a home slot (2, 3 and 5), a home in the
last slot with a walk that wraps, a walk as long as the table less one, a table with no room, two keys in one cache set and more keys than the set holds, a whole
wave on one key, 64 lanes on 64 keys, lane 0 or lane 63 alone selected, the same key in two workgroups and on both sides of a chunk border, and index sizes
around the unit, the wave, the workgroup's round and the grid's first stride with a ragged last unit — on the int32 and on the int64 column."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import group_model as gm
import where_agg_model as wam
from where_agg_model import Model

F = gm._names()
FB, FK, FM, FS, NOBODY = F["base"], F["key"], F["measure"], F["select"], F["nobody"]
EVERY = [[(NOBODY, 0, 0, True)]]
SELECTED = [[(FS, 1, 1)]]
NAMES = [lay["name"] for lay in gm.edge_layouts(False)]
assert len(gm.edge_layouts(True)) == len(NAMES)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("k", range(len(NAMES)))
def test_layout(k, wide):
    lay = gm.edge_layouts(wide)[k]
    n, cap, E = lay["n"], lay["cap"], 2 if wide else 4
    pos = np.arange(n)
    m = Model(wam.node_ids(n, 40000 + 100 * k + wide))
    m.set(FB, pos, np.full(n, 1 + (gm.WIDE if wide else 0)))
    with bmx.Engine(max(16 * n, 4096)) as e:
        wam.load(e, m, [FB])
        pos_ids = e.index_ids(FB)
        node = m.index_of(pos_ids)
        m.set(FK, node[lay["present"]], lay["keys"][lay["present"]])
        if lay["sel"].any():
            m.set(FS, node[lay["sel"]], np.ones(int(lay["sel"].sum()), np.int64))
        hm = pos % 5 != 0
        m.set(FM, node[hm], 37 * pos[hm] - 1000)
        wam.load(e, m, [FK, FS, FM])
        assert np.array_equal(e.index_ids(FB), pos_ids) and e.index_size(FB) == n
        # the paths this layout is there for, from the model, before the query
        d = gm.Device(n, E, cap, True)
        d.run(*gm.rows_of(m, FB, SELECTED, FK, FM, node))
        assert lay["tags"] <= d.tags, (lay["name"], lay["tags"] - d.tags)
        assert gm.grid(n, E) == (2 if n > 4 * gm.THREADS * gm.U * E else 1)
        for measure in (FM, None, FK):
            recs, res = gm.ask(e, m, FB, SELECTED, FK, measure, cap)
            assert int(res["total"]["n_match"]) == int(lay["sel"].sum())
            if "noroom" in lay["tags"] or ("len", 63) in lay["tags"]:
                assert int(res["flags"]) == bmx.GROUP_OVERFLOW
        gm.ask(e, m, FB, SELECTED, FK, FM, 256)                              # the query behind it, with room: the state was left clean
        if lay["base"]:
            # the keys as the base column itself: rewritten in place (a row keeps its position), grouped without a probe
            m.set(FB, node, lay["keys"])
            e.put_rows(*m.rows(FB, 50))
            assert np.array_equal(e.index_ids(FB), pos_ids)
            d = gm.Device(n, E, cap, True)
            d.run(*gm.rows_of(m, FB, EVERY, FB, FM, node))
            assert lay["tags"] <= d.tags
            for measure in (FM, FB):
                gm.ask(e, m, FB, EVERY, FB, measure, cap)
