"""CPU: the model of the first node per group (tests/first_model.py) against itself. The brute force on tables small enough to read; the sequential stand-in
of the three kernels against the brute force on every edge layout, with the path tags each layout is there for; five one-defect variants of the stand-in, each
exposed by the edge layouts; bmx.first_merge against the brute force on split tables; and what the seeded GPU suite relies on: every seeded program has a group
with a tie on its extreme and a group without a contender."""
import numpy as np
import pytest

import bmx
import first_model as fm
import group_model as gm
import where_agg_model as wam
from where_agg_model import Model

F = fm.names()
FB, FG, FO, FS, NOBODY = F["base"], F["group"], F["order"], F["select"], F["nobody"]
EVERY = [[(NOBODY, 0, 0, True)]]
SELECTED = [[(FS, 1, 1)]]
IDS = np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 2, 77], np.uint64)


def _tiny():
    m = Model(IDS)
    m.set(FB, np.arange(6), [1, 2, 3, 4, 5, 6])
    m.set(FG, np.arange(6), [10, 10, 10, 10, 10, -4])
    m.set(FO, [1, 2, 3, 4], [5, 5, 5, 5])
    return m


def test_brute_force_on_a_table_one_can_read():
    m = _tiny()
    recs, vals, ts, res = fm.answer(m, FB, EVERY, FG, FO, (FB, FO, NOBODY), False, 8, True)
    assert recs.tolist() == [(-4, fm.NO_NODE, fm.VAL_DELETED, 1, 0), (10, 1, 5, 5, 4)]
    assert vals.tolist() == [[fm.VAL_DELETED, 2], [fm.VAL_DELETED, 5], [fm.VAL_DELETED, fm.VAL_DELETED]] and ts.tolist() == [[-1, 5], [-1, 5], [-1, -1]]
    assert (int(res["n_groups"]), int(res["flags"]), int(res["total"]), int(res["absent"]), int(res["n_ordered"])) == (2, 0, 6, 0, 4)
    # descending: the value turns, the id does not
    recs = fm.answer(m, FB, EVERY, FG, FO, (), True, 8)[0]
    assert recs[1].tolist() == (10, 1, 5, 5, 4)
    # ids compare as unsigned numbers: 2^63 - 1 < 2^63 < 2^64 - 2
    recs = fm.answer(m, FB, [[(FB, 3, 5)]], FG, FO, (), False, 8)[0]
    assert recs.tolist() == [(10, 2**63 - 1, 5, 3, 3)]
    recs = fm.answer(m, FB, [[(FB, 4, 5)]], FG, FO, (), True, 8)[0]
    assert recs.tolist() == [(10, 2**63, 5, 2, 2)]
    # order == group: every member ties, the smallest id stands for the group
    recs = fm.answer(m, FB, EVERY, FG, FG, (), True, 8)[0]
    assert recs.tolist() == [(-4, 77, -4, 1, 1), (10, 0, 10, 5, 5)]
    # a tombstoned group value is absent; overflow keeps the totals
    m.tomb(FG, [5])
    recs, _, _, res = fm.answer(m, FB, EVERY, FG, FO, (), False, 8)
    assert len(recs) == 1 and int(res["absent"]) == 1 and fm.invariant(recs, res)
    m.set(FG, [0], [11])
    recs, _, _, res = fm.answer(m, FB, EVERY, FG, FO, (), False, 1)
    assert len(recs) == 0 and (int(res["flags"]), int(res["n_groups"]), int(res["total"]), int(res["absent"]), int(res["n_ordered"])) == (1, 2, 6, 1, 4)


def _layout_model(lay, wide, salt):
    """the layout on a table whose node i sits at index position i"""
    n = lay["n"]
    m = Model(wam.node_ids(n, 880000 + salt))
    m.set(FB, np.arange(n), np.full(n, 1 + (gm.WIDE if wide else 0)))
    fm.lay_fill(m, lay, np.arange(n), F)
    return m


def _run(dev, m, lay, wide, desc, cap=None):
    E = 2 if wide else 4
    return fm.device_answer(dev, m, np.arange(lay["n"]), lay["n"], E, cap or lay["cap"], FB, SELECTED, FG, FO, (FO, FB), desc, True)


LAYOUTS = {wide: fm.edge_layouts(wide) for wide in (False, True)}
NAMES = [lay["name"] for lay in LAYOUTS[False]]
assert len(LAYOUTS[True]) == len(NAMES)          # (the sizes in the names of the size layouts depend on the width)


@pytest.mark.parametrize("wide", [False, True])
def test_the_stand_in_equals_the_brute_force_on_every_edge_layout(wide):
    reached = set()
    for k, lay in enumerate(LAYOUTS[wide]):
        m = _layout_model(lay, wide, k)
        for desc in ((False, True) if lay["n"] <= 1000 else (k % 2 == 1,)):
            dev = fm.Device()
            got = _run(dev, m, lay, wide, desc)
            want = fm.answer(m, FB, SELECTED, FG, FO, (FO, FB), desc, lay["cap"], True)
            if int(want[3]["flags"]):
                assert int(got[3]["flags"]) == 1 and lay["cap"] < int(got[3]["n_groups"]) <= int(want[3]["n_groups"]) and got[3].tobytes()[16:] == want[3].tobytes()[16:]
            else:
                assert fm.same_answer(got, want), (lay["name"], desc)
            assert lay["tags"] <= dev.tags, (lay["name"], lay["tags"] - dev.tags)
            assert dev.idw == {}, "every id word is back at its empty state"
            reached |= dev.tags
            if lay["winner"] and not desc:
                for key, p in lay["winner"].items():
                    r = got[0][got[0]["key"] == key][0]
                    assert int(r["id"]) == int(m.ids[p]) and int(r["val"]) == int(lay["oval"][p]), lay["name"]
    assert {"hit", "bypass", "home", "walk", "wrap", "noroom", "combine", "resolve_home", "resolve_walk", "resolve_wrap", "resolve_first", "resolve_tie",
            "resolve_skip"} <= reached


def test_the_extreme_sits_on_the_cached_and_on_the_bypass_path():
    lay = [x for x in LAYOUTS[False] if x["name"] == "extreme_cached_and_bypass"][0]
    m = _layout_model(lay, False, 0)
    dev = fm.Device()
    recs = dev.run(lay["n"], 4, lay["cap"], lay["sel"], [int(k) for k in lay["keys"]], [int(v) for v in lay["oval"]], [int(x) for x in m.ids])[0]
    assert {dev.row_tags[r[5]] for r in recs} == {"hit", "bypass"}, "the winners' rows took both paths"


@pytest.mark.parametrize("defect", fm.DEFECTS)
def test_every_defect_is_exposed_by_the_edge_layouts(defect):
    exposed = []
    for wide in (False, True):
        for k, lay in enumerate(LAYOUTS[wide]):
            m = _layout_model(lay, wide, k)
            if lay["n"] > 1000:
                continue                                                        # (the large layouts are there for the sweep's geometry, not for the order)
            for desc in (False, True):
                dev = fm.Device(defect)
                if defect == "idw_not_reset":
                    _run(dev, m, lay, wide, desc, cap=1)                       # a query that overflows right in front (where the layout has two keys)
                got = _run(dev, m, lay, wide, desc, cap=256)
                if not fm.same_answer(got, fm.answer(m, FB, SELECTED, FG, FO, (FO, FB), desc, 256, True)):
                    exposed.append((lay["name"], wide, desc))
    assert exposed, defect
    if defect == "desc_flips_id":
        assert all(d for _, _, d in exposed)
    if defect == "noncontender_wins":
        assert any(name == "member_without_order_first" for name, _, _ in exposed)
    if defect == "unselected_wins":
        assert any(name == "unselected_ties" for name, _, _ in exposed)


def test_first_merge_equals_the_brute_force_on_split_tables():
    m, tombs = fm.seeded_model()
    gm.apply_tombs(m, tombs)
    fields = (FO, FB, FG, F["one"])
    prog = [[(FB, 0, 9)], [(F["one"], 2, 4, True)]]
    for nshards in (1, 2, 4, 7):
        for desc in (False, True):
            parts = []
            for g in range(nshards):
                idx = np.nonzero(m.ids % np.uint64(nshards) == g)[0]
                s = Model(m.ids[idx])
                for f in m.val:
                    s._f(f); s.val[f][:] = m.val[f][idx]; s.st[f][:] = m.st[f][idx]
                r = fm.answer(s, FB, prog, FG, FO, fields, desc, 1 << 20, True)
                parts.append((r[0], r[1], r[2]))
            recs, vals, ts = bmx.first_merge(parts, desc)
            want = fm.answer(m, FB, prog, FG, FO, fields, desc, 1 << 20, True)
            assert recs.tobytes() == want[0].tobytes() and np.array_equal(vals, want[1]) and np.array_equal(ts, want[2]), (nshards, desc)
    # a tie across shards is decided by the id, whatever the order of the lists; a shard without a contender never wins
    a = np.array([(5, 2**63, 1, 2, 1)], fm.FIRST_DTYPE); b = np.array([(5, 2**63 - 1, 1, 1, 1)], fm.FIRST_DTYPE); c = np.array([(5, fm.NO_NODE, fm.VAL_DELETED, 4, 0)], fm.FIRST_DTYPE)
    va, vb, vc = np.array([[100]]), np.array([[200]]), np.array([[fm.VAL_DELETED]])
    for lists in ([(a, va, None), (b, vb, None), (c, vc, None)], [(c, vc, None), (b, vb, None), (a, va, None)]):
        for desc in (False, True):
            recs, vals, ts = bmx.first_merge(lists, desc)
            assert recs.tolist() == [(5, 2**63 - 1, 1, 7, 2)] and vals.tolist() == [[200]] and ts is None
    assert len(bmx.first_merge([], False)[0]) == 0


def test_every_seeded_program_has_a_tie_and_a_group_without_contender():
    m, tombs = fm.seeded_model()
    gm.apply_tombs(m, tombs)
    qs = fm.seeded_queries(m)
    assert len(qs) == fm.N_PROGS and sum(d for _, _, _, d in qs) == fm.N_PROGS // 2
    for p, group, order, desc in qs:
        assert fm.has_tie_and_empty(m, FB, p, group, order, desc), p
    # the ties are not all between small ids: some seed's winner is decided among ids on both sides of 2^63
    assert (m.ids >= np.uint64(2**63)).any() and (m.ids < np.uint64(2**63)).any()
