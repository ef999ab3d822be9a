"""GPU: the kernels of the group-by over several fields at their edges (csrc/mgroup_kernels.h). Every layout of mgroup_model.edge_layouts is laid out BY
POSITION of the base field's index (index_ids), so the test knows which wave, lane and workgroup meets which tuple; the path tags the layout is there for are
asserted on the sequential stand-in of mgroup_model.py before the query runs, and the answer is compared exactly with the brute-force answer: dictionary values
that share a home slot, values that share an entry of the workgroup's LDS cache of codes, a dictionary walk that wraps, one that fills the table and one that finds no room (in the first and in the last dictionary of a call),
packed words that share a home slot of the tuple table (2, 3 and 5) and that wrap, more words than one cache set holds, a whole wave on one tuple, 64 lanes on
64 tuples that share key[0], lane 0 or lane 63 alone selected, the same tuple in two workgroups, and index sizes around the unit, the wave, a workgroup's round
and the grid's first stride with a ragged last unit — on the int32 and on the int64 column."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import group_model as gm
import mgroup_model as mm
import where_agg_model as wam
from where_agg_model import Model

F = gm._names()
FB, FM, FS, NOBODY = F["base"], F["measure"], F["select"], F["nobody"]
FK = [F["key"], F["one"], F["two"], F["three"]]
EVERY = [[(NOBODY, 0, 0, True)]]
SELECTED = [[(FS, 1, 1)]]
NAMES = [lay["name"] for lay in mm.edge_layouts(False)]
assert len(mm.edge_layouts(True)) == len(NAMES)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("k", range(len(NAMES)))
def test_layout(k, wide):
    lay = mm.edge_layouts(wide)[k]
    n, cap, nk, E = lay["n"], lay["cap"], lay["nkeys"], 2 if wide else 4
    keys = FK[:nk]
    pos = np.arange(n)
    m = Model(wam.node_ids(n, 50000 + 100 * k + wide))
    m.set(FB, pos, np.full(n, 1 + (mm.WIDE if wide else 0)))
    with bmx.Engine(max(16 * n, 4096)) as e:
        wam.load(e, m, [FB])
        pos_ids = e.index_ids(FB)
        node = m.index_of(pos_ids)
        for j in range(nk):
            pr = lay["present"][:, j]
            m.set(keys[j], node[pr], lay["keys"][pr, j])
        if lay["sel"].any():
            m.set(FS, node[lay["sel"]], np.ones(int(lay["sel"].sum()), np.int64))
        hm = pos % 5 != 0
        m.set(FM, node[hm], 37 * pos[hm] - 1000)
        wam.load(e, m, keys + [FS, FM])
        assert np.array_equal(e.index_ids(FB), pos_ids) and e.index_size(FB) == n
        # the paths this layout is there for, from the model, before the query
        d = mm.Device(n, E, cap, keys, True)
        d.run(*mm.rows_of(m, FB, SELECTED, keys, FM, node))
        assert lay["tags"] <= d.tags, (lay["name"], lay["tags"] - d.tags)
        assert gm.grid(n, E) == (2 if n > 4 * gm.THREADS * gm.U * E else 1)
        noroom = any(t[0] == "dict" and t[2] == "noroom" for t in lay["tags"] if isinstance(t, tuple) and len(t) == 3)
        for measure in (FM, None, keys[0]):
            recs, res = mm.ask(e, m, FB, SELECTED, keys, measure, cap)
            assert int(res["total"]["n_match"]) == int(lay["sel"].sum())
            if noroom or (("dict", 1, "len"), 63) in lay["tags"]:
                assert int(res["flags"]) == bmx.GROUP_OVERFLOW
        mm.ask(e, m, FB, SELECTED, keys, FM, 256)                            # the query behind it, with room: the state was left clean
        mm.ask(e, m, FB, SELECTED, [(f, -5, 3) for f in keys], FM, 256)     # ... and the same layout through the division
        if lay["base"]:
            # key 0 as the base column itself: rewritten in place (a row keeps its position), read without a probe
            m.set(FB, node, lay["keys"][:, 0])
            e.put_rows(*m.rows(FB, 50))
            assert np.array_equal(e.index_ids(FB), pos_ids)
            kb = [FB] + keys[1:]
            d = mm.Device(n, E, cap, kb, True)
            d.run(*mm.rows_of(m, FB, EVERY, kb, FM, node))
            assert lay["tags"] <= d.tags
            for measure in (FM, FB):
                mm.ask(e, m, FB, EVERY, kb, measure, cap)
