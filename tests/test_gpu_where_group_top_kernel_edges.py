"""GPU: the kernels of the first N nodes per group at their edges (csrc/gtop_kernels.h). Every layout of gtop_model.edge_layouts is laid out BY POSITION of the
base field's index (index_ids), so the test knows which wave, lane and workgroup meets which row in pass 1 and in the round kernels; the path tags the layout is
there for are asserted on the sequential stand-in of gtop_model.py before the query runs, and the answer is compared exactly with the brute force. The layouts
are first_model.edge_layouts (with per = 3), and on top of them: ranks 1 and 2 on lane 0 and on lane 63 of the round kernels, at the first and the last index
position and in the ragged last unit, ranks 1 and 2 tying in two workgroups, a wave whose 64 rows all tie with per = 16, 17 contenders with per = 16, one group
exhausted in round 2 while another runs to round 16, 64 groups on 64 lanes with the cut inside a tie, and the two layouts in which members without an order
value and nodes the program rejects sit between the ranks — on the int32 and on the int64 column, ascending and descending."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import gtop_model as tm
import group_model as gm
import where_agg_model as wam
from where_agg_model import Model

F = tm.names()
FB, FG, FO, FS, NOBODY = F["base"], F["group"], F["order"], F["select"], F["nobody"]
SELECTED = [[(FS, 1, 1)]]
COUNT = len(tm.edge_layouts(False))
assert len(tm.edge_layouts(True)) == COUNT


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("k", range(COUNT))
def test_layout(k, wide):
    lay = tm.edge_layouts(wide)[k]
    n, cap, per, E = lay["n"], lay["cap"], lay["per"], 2 if wide else 4
    m = Model(wam.node_ids(n, 40000 + 100 * k + wide))
    m.set(FB, np.arange(n), np.full(n, 1 + (gm.WIDE if wide else 0)))
    with bmx.Engine(max(16 * n, 4096)) as e:
        wam.load(e, m, [FB])
        pos_ids = e.index_ids(FB)
        node = m.index_of(pos_ids)
        sel, has_o = tm.lay_fill(m, lay, node, F)
        wam.load(e, m, [FG, FS, FO])
        assert np.array_equal(e.index_ids(FB), pos_ids) and e.index_size(FB) == n
        assert tm.round_grid(n) == (n + 2047) // 2048 and gm.grid(n, E) == (2 if n > 4 * gm.THREADS * gm.U * E else 1)
        noroom = "noroom" in lay["tags"] or ("len", 63) in lay["tags"]
        for desc in ((False, True) if n <= 1000 else (k % 2 == 1,)):
            # the paths this layout is there for, from the stand-in, before the query
            dev = tm.Device()
            stand = tm.device_answer(dev, m, node, n, E, cap, per, FB, SELECTED, FG, FO, (FO,), desc, True)
            assert lay["tags"] <= dev.first_tags and lay["gtags"] <= dev.tags, (lay["name"], lay["tags"] - dev.first_tags, lay["gtags"] - dev.tags)
            want = tm.ask(e, m, FB, SELECTED, FG, FO, per, (FO,), desc, True, cap)
            assert int(want[4]["total"]) == int(sel.sum())
            if noroom:
                assert int(want[4]["flags"]) == tm.OVERFLOW
            else:
                assert tm.same_answer(stand, want)
            if lay["ranks"] and not desc:
                for key, ps in lay["ranks"].items():
                    r = want[1][want[0]["key"] == key][0]
                    assert r["id"][:len(ps)].tolist() == [int(pos_ids[p]) for p in ps] and r["val"][:len(ps)].tolist() == [int(lay["oval"][p]) for p in ps], "the ranks are where the layout put them"
            tm.ask(e, m, FB, SELECTED, FG, FO, 2 if per != 2 else 5, (FO, FG), not desc, False, 256)      # the query behind it, with room and another per: the state was left clean
        tm.ask(e, m, FB, SELECTED, FG, FG, per, (), False, False, 256)                                    # order == group: one probe, one word per position
        if lay.get("base"):
            # the keys as the base column itself: rewritten in place (a row keeps its position); the group value costs no probe
            m.set(FB, node, lay["keys"])
            e.put_rows(*m.rows(FB, 50))
            assert np.array_equal(e.index_ids(FB), pos_ids)
            tm.ask(e, m, FB, [[(NOBODY, 0, 0, True)]], FB, FO, per, (FO,), False, False, cap)
            tm.ask(e, m, FB, [[(NOBODY, 0, 0, True)]], FB, FB, per, (), True, False, cap)                 # group and order both the column: the order word records the selection
            tm.ask(e, m, FB, SELECTED, FO, FB, per, (), True, False, 64)                                  # the order value from the column, the group value probed
