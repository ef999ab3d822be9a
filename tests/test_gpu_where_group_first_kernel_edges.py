"""GPU: the kernels of the first node per group at their edges (csrc/first_kernels.h). Every layout of first_model.edge_layouts is laid out BY POSITION of the
base field's index (index_ids), so the test knows which wave, lane and workgroup meets which row; the path tags the layout is there for are asserted on the
sequential stand-in of first_model.py before the query runs, and the answer is compared exactly with the brute force. The layouts are group_model.edge_layouts
(keys that share a home slot, a walk that wraps, a 64-slot table with no room, two keys and more keys than ways in one cache set, a whole wave on one key, 64
lanes on 64 keys, lane 0 or lane 63 alone, index sizes 1, around the unit, the wave, a workgroup's round and the grid's first stride) with order values that tie
on every extreme, and on top of them: the winner at lane 0 and lane 63, at the first and the last index position, in the ragged last unit, the extreme value in
two workgroups, the extreme on the cached and on the bypass path, a wave whose 64 rows all tie, and the two layouts in which the smallest id belongs to a member
without an order value or to a node the program rejects — on the int32 and on the int64 column, ascending and descending."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import first_model as fm
import group_model as gm
import where_agg_model as wam
from where_agg_model import Model

F = fm.names()
FB, FG, FO, FS, NOBODY = F["base"], F["group"], F["order"], F["select"], F["nobody"]
EVERY = [[(NOBODY, 0, 0, True)]]
SELECTED = [[(FS, 1, 1)]]
COUNT = len(fm.edge_layouts(False))
assert len(fm.edge_layouts(True)) == COUNT


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("k", range(COUNT))
def test_layout(k, wide):
    lay = fm.edge_layouts(wide)[k]
    n, cap, E = lay["n"], lay["cap"], 2 if wide else 4
    m = Model(wam.node_ids(n, 60000 + 100 * k + wide))
    m.set(FB, np.arange(n), np.full(n, 1 + (gm.WIDE if wide else 0)))
    with bmx.Engine(max(16 * n, 4096)) as e:
        wam.load(e, m, [FB])
        pos_ids = e.index_ids(FB)
        node = m.index_of(pos_ids)
        sel, has_o = fm.lay_fill(m, lay, node, F)
        wam.load(e, m, [FG, FS, FO])
        assert np.array_equal(e.index_ids(FB), pos_ids) and e.index_size(FB) == n
        assert gm.grid(n, E) == (2 if n > 4 * gm.THREADS * gm.U * E else 1)
        noroom = "noroom" in lay["tags"] or ("len", 63) in lay["tags"]
        descs = (False, True) if n <= 1000 else (k % 2 == 1,)
        for desc in descs:
            # the paths this layout is there for, from the stand-in, before the query
            dev = fm.Device()
            stand = fm.device_answer(dev, m, node, n, E, cap, FB, SELECTED, FG, FO, (FO,), desc, True)
            assert lay["tags"] <= dev.tags, (lay["name"], lay["tags"] - dev.tags)
            want = fm.ask(e, m, FB, SELECTED, FG, FO, (FO,), desc, True, cap)
            assert int(want[3]["total"]) == int(sel.sum())
            if noroom:
                assert int(want[3]["flags"]) == fm.OVERFLOW
            else:
                assert fm.same_answer(stand, want)
            if lay["winner"] and not desc:
                for key, p in lay["winner"].items():
                    r = want[0][want[0]["key"] == key][0]
                    assert int(r["id"]) == int(pos_ids[p]) and int(r["val"]) == int(lay["oval"][p]), "the winner is where the layout put it"
            fm.ask(e, m, FB, SELECTED, FG, FO, (FO, FG), not desc, False, 256)                # the query behind it, with room: the state was left clean
        fm.ask(e, m, FB, SELECTED, FG, FG, (), False, False, 256)                             # order == group: one probe, one word per position
        if lay.get("base"):
            # the keys as the base column itself: rewritten in place (a row keeps its position); the group value costs no probe
            m.set(FB, node, lay["keys"])
            e.put_rows(*m.rows(FB, 50))
            assert np.array_equal(e.index_ids(FB), pos_ids)
            for desc in (False, True):
                fm.ask(e, m, FB, EVERY, FB, FO, (FO,), desc, False, cap)
                fm.ask(e, m, FB, EVERY, FB, FB, (), desc, False, cap)                         # group and order both the column: the order word records the selection
            fm.ask(e, m, FB, SELECTED, FO, FB, (), True, False, 64)                           # the order value from the column, the group value probed
