"""CPU: the model of the first N nodes per group (tests/gtop_model.py) against itself. The brute force on a table small enough to read; the sequential stand-in
of the round kernels against the brute force on every edge layout, with the path tags each layout is there for; nine one-defect variants of the stand-in, each
exposed by the edge layouts; bmx.gtop_merge against the brute force on split tables; per = 1 against first_model.answer field for field; and what the seeded GPU
suite relies on: 60 programs per `per`, each with a tie at the cut, a short group, a group without a contender and a tie on an extreme."""
import numpy as np
import pytest

import bmx
import first_model as fm
import group_model as gm
import gtop_model as tm
import where_agg_model as wam
from where_agg_model import Model

F = tm.names()
FB, FG, FO, FS, NOBODY = F["base"], F["group"], F["order"], F["select"], F["nobody"]
EVERY = [[(NOBODY, 0, 0, True)]]
SELECTED = [[(FS, 1, 1)]]
IDS = np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 2, 77], np.uint64)


def test_the_symbols_of_the_form_exist():
    assert bmx.EXPORTS_GROUP_TOP == ["bmx_where_group_top", "bmx_comm_where_group_top"] and callable(bmx.gtop_merge)
    assert tm.GRP_DTYPE == bmx.GTOP_GRP_DTYPE and tm.ROW_DTYPE == bmx.GTOP_ROW_DTYPE and tm.RES_DTYPE == bmx.GTOP_RES_DTYPE
    assert (tm.OVERFLOW, tm.MAX_CAP, tm.MAX_PER, tm.MAX_ROWS, tm.DESC) == (bmx.GTOP_OVERFLOW, bmx.GTOP_MAX_CAP, bmx.GTOP_MAX_PER, bmx.GTOP_MAX_ROWS, bmx.GTOP_DESC)


def _tiny():
    m = Model(IDS)
    m.set(FB, np.arange(6), [1, 2, 3, 4, 5, 6])
    m.set(FG, np.arange(6), [10, 10, 10, 10, 10, -4])
    m.set(FO, [1, 2, 3, 4], [5, 5, 5, 6])
    return m


def test_brute_force_on_a_table_one_can_read():
    m = _tiny()
    grps, rows, vals, ts, res = tm.answer(m, FB, EVERY, FG, FO, 3, (FB, NOBODY), False, 8, True)
    assert grps.tolist() == [(-4, 1, 0, 0), (10, 5, 4, 3)]
    assert rows.tolist() == [[(tm.NO_NODE, tm.VAL_DELETED)] * 3, [(1, 5), (2**63 - 1, 5), (2**63, 5)]], "ids ascend as unsigned numbers: 1 < 2^63 - 1 < 2^63"
    assert vals.tolist() == [[[tm.VAL_DELETED] * 3, [2, 3, 4]], [[tm.VAL_DELETED] * 3] * 2] and ts.tolist() == [[[-1] * 3, [5, 5, 5]], [[-1] * 3] * 2]
    assert tuple(int(res[k]) for k in res.dtype.names) == (2, 0, 3, 6, 0, 4, 3)
    # descending: the value turns, the id does not
    rows = tm.answer(m, FB, EVERY, FG, FO, 3, (), True, 8)[1]
    assert rows[1].tolist() == [(2**64 - 2, 6), (1, 5), (2**63 - 1, 5)]
    # per beyond n: padding; per = 1: the first node
    grps, rows = tm.answer(m, FB, EVERY, FG, FO, 16, (), False, 8)[:2]
    assert grps[1].tolist() == (10, 5, 4, 4) and rows[1].tolist()[3:5] == [(2**64 - 2, 6), (tm.NO_NODE, tm.VAL_DELETED)]
    assert tm.answer(m, FB, EVERY, FG, FO, 1, (), False, 8)[1].tolist() == [[(tm.NO_NODE, tm.VAL_DELETED)], [(1, 5)]]
    # overflow keeps the totals and reports no rows
    m.set(FG, [0], [11])
    grps, rows, _, _, res = tm.answer(m, FB, EVERY, FG, FO, 2, (), False, 2)
    assert len(grps) == 0 and rows.shape == (0, 2) and tuple(int(res[k]) for k in res.dtype.names) == (3, 1, 2, 6, 0, 4, 0)


def _layout_model(lay, wide, salt):
    """the layout on a table whose node i sits at index position i"""
    n = lay["n"]
    m = Model(wam.node_ids(n, 770000 + salt))
    m.set(FB, np.arange(n), np.full(n, 1 + (gm.WIDE if wide else 0)))
    tm.lay_fill(m, lay, np.arange(n), F)
    return m


def _run(dev, m, lay, wide, desc, cap=None, per=None):
    E = 2 if wide else 4
    return tm.device_answer(dev, m, np.arange(lay["n"]), lay["n"], E, cap or lay["cap"], per or lay["per"], FB, SELECTED, FG, FO, (FO, FB), desc, True)


LAYOUTS = {wide: tm.edge_layouts(wide) for wide in (False, True)}
assert len(LAYOUTS[True]) == len(LAYOUTS[False])


@pytest.mark.parametrize("wide", [False, True])
def test_the_stand_in_equals_the_brute_force_on_every_edge_layout(wide):
    reached = set()
    for k, lay in enumerate(LAYOUTS[wide]):
        m = _layout_model(lay, wide, k)
        for desc in ((False, True) if lay["n"] <= 1000 else (k % 2 == 1,)):
            dev = tm.Device()
            got = _run(dev, m, lay, wide, desc)
            want = tm.answer(m, FB, SELECTED, FG, FO, lay["per"], (FO, FB), desc, lay["cap"], True)
            if int(want[4]["flags"]):
                assert int(got[4]["flags"]) == 1 and lay["cap"] < int(got[4]["n_groups"]) <= int(want[4]["n_groups"]) and got[4].tobytes()[16:] == want[4].tobytes()[16:]
            else:
                assert tm.same_answer(got, want), (lay["name"], desc)
                assert tm.invariant(got[0], got[1], got[4])
            assert lay["tags"] <= dev.first_tags, (lay["name"], lay["tags"] - dev.first_tags)
            assert lay["gtags"] <= dev.tags, (lay["name"], lay["gtags"] - dev.tags)
            assert dev.state == {} and dev.first.idw == {}, "all per-slot state is back at rest"
            reached |= dev.tags
            if lay["ranks"] and not desc:
                for key, ps in lay["ranks"].items():
                    r = got[1][got[0]["key"] == key][0]
                    assert [int(x) for x in r["id"][:len(ps)]] == [int(m.ids[p]) for p in ps] and [int(x) for x in r["val"][:len(ps)]] == [int(lay["oval"][p]) for p in ps], lay["name"]
    assert tm.TAGS <= reached


@pytest.mark.parametrize("defect", tm.DEFECTS)
def test_every_defect_is_exposed_by_the_edge_layouts(defect):
    exposed = []
    for wide in (False, True):
        for k, lay in enumerate(LAYOUTS[wide]):
            if lay["n"] > 1000:
                continue                                                        # (the large layouts are there for the sweeps' geometry, not for the order)
            m = _layout_model(lay, wide, k)
            for desc in (False, True):
                dev = tm.Device(defect)
                if defect == "state_not_reset":
                    _run(dev, m, lay, wide, not desc, cap=256)                 # a query right in front, on the same table
                got = _run(dev, m, lay, wide, desc, cap=256)
                if not tm.same_answer(got, tm.answer(m, FB, SELECTED, FG, FO, lay["per"], (FO, FB), desc, 256, True)):
                    exposed.append((lay["name"], wide, desc))
    assert exposed, defect
    names = {name for name, _, _ in exposed}
    if defect == "desc_flips_id":
        assert all(d for _, _, d in exposed)
    if defect in ("after_value_only", "after_not_strict", "ext_not_reset"):
        assert "wave_all_tie_per_16" in names or "seventeen_contenders_per_16" in names
    if defect == "exhausted_repeats":
        assert "exhausted_in_round_2_and_16_rounds" in names and "short_groups" in names
    if defect == "noncontender_wins":
        assert "member_without_order_later" in names
    if defect == "unselected_wins":
        assert "unselected_later" in names


def _split(m, nshards):
    for g in range(nshards):
        idx = np.nonzero(m.ids % np.uint64(nshards) == g)[0]
        s = Model(m.ids[idx])
        for f in m.val:
            s._f(f); s.val[f][:] = m.val[f][idx]; s.st[f][:] = m.st[f][idx]
        yield s


def test_gtop_merge_equals_the_brute_force_on_split_tables():
    m, tombs = tm.seeded_model()
    gm.apply_tombs(m, tombs)
    fields = (FO, FB, FG, F["one"])
    prog = [[(FB, 0, 9)], [(F["one"], 2, 4, True)]]
    for nshards in (1, 2, 4, 7):
        for desc in (False, True):
            for per in (1, 3, 16):
                parts = [tm.answer(s, FB, prog, FG, FO, per, fields, desc, 1 << 20, True)[:4] for s in _split(m, nshards)]
                grps, rows, vals, ts = bmx.gtop_merge(parts, per, desc)
                want = tm.answer(m, FB, prog, FG, FO, per, fields, desc, 1 << 20, True)
                assert grps.tobytes() == want[0].tobytes() and rows.tobytes() == want[1].tobytes() and np.array_equal(vals, want[2]) and np.array_equal(ts, want[3]), (nshards, desc, per)
    # a key's ranks alternate between the lists; a tie at the cut is decided by the id, whatever the order of the lists; a shard without a contender adds counts
    G, R = tm.GRP_DTYPE, tm.ROW_DTYPE
    a = (np.array([(5, 3, 2, 2)], G), np.array([[(2**63, 1), (9, 3)]], R), np.array([[[100, 300]]]), None)
    b = (np.array([(5, 2, 2, 2)], G), np.array([[(2**63 - 1, 1), (4, 2)]], R), np.array([[[200, 400]]]), None)
    c = (np.array([(5, 4, 0, 0)], G), np.array([[(tm.NO_NODE, tm.VAL_DELETED)] * 2], R), np.array([[[tm.VAL_DELETED] * 2]]), None)
    for lists in ([a, b, c], [c, b, a]):
        grps, rows, vals, ts = bmx.gtop_merge(lists, 2, False)
        assert grps.tolist() == [(5, 9, 4, 2)] and rows.tolist() == [[(2**63 - 1, 1), (2**63, 1)]] and vals.tolist() == [[[200, 100]]] and ts is None
        grps, rows, vals, ts = bmx.gtop_merge(lists, 2, True)
        assert rows.tolist() == [[(9, 3), (4, 2)]] and vals.tolist() == [[[300, 400]]]
    assert len(bmx.gtop_merge([], 3, False)[0]) == 0


def test_per_1_equals_the_first_node_per_group_field_for_field():
    m, tombs = tm.seeded_model()
    gm.apply_tombs(m, tombs)
    for k, (p, group, order, desc) in enumerate(fm.seeded_queries(m)[::3]):
        for cap in (64, 3):
            fields = (order, FB, F["one"])[: k % 4]
            grps, rows, vals, ts, res = tm.answer(m, FB, p, group, order, 1, fields, desc, cap, True)
            recs, fvals, fts, fres = fm.answer(m, FB, p, group, order, fields, desc, cap, True)
            for a, b in (("key", "key"), ("n_match", "n_match"), ("n", "n")):
                assert np.array_equal(grps[a], recs[b])
            assert np.array_equal(rows[:, 0]["id"], recs["id"]) and np.array_equal(rows[:, 0]["val"], recs["val"])
            assert np.array_equal(vals[:, :, 0], fvals) and np.array_equal(ts[:, :, 0], fts)
            for a in ("n_groups", "flags", "total", "absent", "n_ordered"):
                assert int(res[a]) == int(fres[a])
            assert int(res["n_rows"]) == int((recs["n"] > 0).sum())


@pytest.mark.parametrize("per", tm.PERS)
def test_every_seeded_program_meets_the_four_conditions(per):
    m, tombs = tm.seeded_model()
    gm.apply_tombs(m, tombs)
    qs = tm.seeded_queries(m, per)
    assert len(qs) == tm.N_PROGS == 60 and sum(d for _, _, _, d in qs) == tm.N_PROGS // 2
    for p, group, order, desc in qs:
        assert tm.conditions(m, FB, p, group, order, desc, per) == (True, True, True, True), p
    assert tm.seeded_drawn(per) >= 2 * tm.N_PROGS, "the conditions are no formality: most candidates fail them"
    assert (m.ids >= np.uint64(2**63)).any() and (m.ids < np.uint64(2**63)).any()
