"""CPU: the model the GPU tests of bmx_where_group_multi rely on (tests/mgroup_model.py). The sequential stand-in of the design (dictionaries, packed word,
cache, tuple table) is held against the brute-force answer on every edge layout, with every path tag the layouts are there for reached; the same comparison
FAILS on seven one-defect stand-ins, so the checks the GPU tests make are able to see those defects; and the seeded suite meets the conditions the GPU test
relies on, asserted here on the model alone."""
import numpy as np
import pytest

import group_model as gm
import mgroup_model as mm
import where_agg_model as wam
from where_agg_model import Model

F = gm._names()
FB, FM, FS, NOBODY = F["base"], F["measure"], F["select"], F["nobody"]
FK = [F["key"], F["one"], F["two"], F["three"]]                    # the layouts' key j is a probed field of its own
SELECTED = [[(FS, 1, 1)]]


def layout_model(lay, wide, salt=0):
    """the layout as a table whose node p sits at position p -> (model, keys)"""
    n = lay["n"]
    pos = np.arange(n)
    m = Model(wam.node_ids(n, 70000 + salt))
    m.set(FB, pos, np.full(n, 1 + (mm.WIDE if wide else 0)))
    for j in range(lay["nkeys"]):
        pr = lay["present"][:, j]
        m.set(FK[j], pos[pr], lay["keys"][pr, j])
    if lay["sel"].any():
        m.set(FS, pos[lay["sel"]], np.ones(int(lay["sel"].sum()), np.int64))
    hm = pos % 5 != 0
    m.set(FM, pos[hm], 37 * pos[hm] - 1000)
    return m, FK[:lay["nkeys"]]


def run_device(m, keys, n, E, cap, measure=FM, clauses=SELECTED, scratch=None, defect=None):
    d = mm.Device(n, E, cap, keys, measure is not None, scratch=scratch, defect=defect)
    out, res = d.run(*mm.rows_of(m, FB, clauses, keys, measure, np.arange(n)))
    return d, out, res


@pytest.mark.parametrize("wide", [False, True])
def test_the_stand_in_gives_the_brute_force_answer_on_every_layout(wide):
    E = 2 if wide else 4
    reached = set()
    for k, lay in enumerate(mm.edge_layouts(wide)):
        m, keys = layout_model(lay, wide, k)
        sc = mm.Scratch()
        for measure in (FM, None):
            d, out, res = run_device(m, keys, lay["n"], E, lay["cap"], measure, scratch=sc)
            assert lay["tags"] <= d.tags, (lay["name"], lay["tags"] - d.tags)
            assert mm.check(out, res, *mm.answer(m, FB, SELECTED, keys, measure, lay["cap"]), lay["cap"]) is None, lay["name"]
            assert sc.empty(), "every query leaves its scratch empty for the next"
            reached |= d.tags
    for j in (0, 1):
        assert {("dict", j, "home"), ("dict", j, "walk") if j == 0 else ("dict", j, "wrap")} <= reached
    assert {("dict", 0, "noroom"), ("dict", 2, "noroom"), (("dict", 1, "len"), 63), "home", "walk", "wrap", "hit", "bypass", ("len", 4),
            ("dcache", "hit"), ("dcache", "claim"), ("dcache", "taken")} <= reached


def test_packing():
    assert (mm.shift_for(1), mm.shift_for(32), mm.shift_for(33), mm.shift_for(mm.MAX_CAP4), mm.shift_for(mm.MAX_CAP)) == (6, 6, 7, 15, 21)
    assert 4 * mm.shift_for(mm.MAX_CAP4) <= 63 and 3 * mm.shift_for(mm.MAX_CAP) <= 63 and 4 * mm.shift_for(mm.MAX_CAP4 + 1) > 63, "the header's cap rule"
    vals = mm.values_by_home(64)
    assert [gm.home(v, 64) for v in vals] == list(range(64))
    for a, b in mm.pairs_with_home(21, 64, 5):
        assert gm.home(a | (b << 6), 64) == 21


def test_bucket_is_floor_division():
    assert [mm.bucket(v, 0, 10) for v in (-11, -10, -1, 0, 9, 10)] == [-2, -1, -1, 0, 0, 1]
    assert mm.bucket(-mm.BIG, mm.BIG, mm.BIG) == -2 and mm.bucket(mm.BIG, -mm.BIG, mm.BIG) == 2 and mm.bucket(-mm.BIG, mm.BIG, 1) == -2 * mm.BIG
    assert mm.bucket(5, 7, 1) == -2 and mm.bucket(-1, 0, mm.BIG) == -1 and mm.bucket(0, 1, 2) == -1


def _defect_table():
    """300 nodes by position: key A in -20..19 (negative values that are and are not multiples of the width), key B 0..2 missing on every seventh node,
    key C equal to B's neighbour — tuples that differ in key[1] only, and a key[0] that several tuples share"""
    n = 300
    pos = np.arange(n)
    m = Model(wam.node_ids(n, 4242))
    m.set(FB, pos, np.full(n, 1))
    m.set(FK[0], pos, (pos % 40) - 20)
    pr = pos % 7 != 0
    m.set(FK[1], pos[pr], (pos[pr] * 3) % 5)
    m.set(FS, pos, np.ones(n, np.int64))
    m.set(FM, pos, 11 * pos - 900)
    return m, n


CASES = {
    # defect -> (keys, cap): a query on which the defect changes the answer
    "overlap": ([FK[0], FK[1]], 64),
    "trunc": ([(FK[0], 0, 8), FK[1]], 64),
    "absent_in_group": ([(FK[0], 0, 8), FK[1]], 64),
    "sort_key0": ([(FK[0], 0, 8), FK[1]], 64),
    "write_on_overflow": ([FK[0], FK[1]], 8),
    "write_behind": ([(FK[0], 0, 8), FK[1]], 64),
}


@pytest.mark.parametrize("defect", sorted(CASES))
def test_the_checks_see_a_one_defect_stand_in(defect):
    m, n = _defect_table()
    keys, cap = CASES[defect]
    want = mm.answer(m, FB, SELECTED, keys, FM, cap)
    _, out, res = run_device(m, keys, n, 4, cap)
    assert mm.check(out, res, *want, cap) is None, "the stand-in without a defect passes"
    _, out, res = run_device(m, keys, n, 4, cap, defect=defect)
    assert mm.check(out, res, *want, cap) is not None, defect


def test_five_queries_in_a_row_see_a_stale_dictionary():
    """disjoint value sets of cap - 2 values each: with dictionaries that are not emptied behind a query the third one finds no room"""
    cap, n = 32, 300
    pos = np.arange(n)
    for defect in (None, "stale_dict"):
        sc = mm.Scratch()
        bad = []
        for q in range(5):
            m = Model(wam.node_ids(n, 900 + q))
            m.set(FB, pos, np.full(n, 1)); m.set(FS, pos, np.ones(n, np.int64))
            m.set(FK[0], pos, 1000 * q + pos % (cap - 2)); m.set(FK[1], pos, np.full(n, q))
            _, out, res = run_device(m, FK[:2], n, 4, cap, scratch=sc, defect=defect)
            bad.append(mm.check(out, res, *mm.answer(m, FB, SELECTED, FK[:2], FM, cap), cap) is not None)
        assert any(bad) == (defect is not None), (defect, bad)
        assert not bad[0] and (defect is None or True in bad[:3]), "a stale dictionary overflows by the third query"


def test_merge_restated_in_numpy():
    import bmx
    a = np.zeros(3, bmx.MGROUP_DTYPE); b = np.zeros(2, bmx.MGROUP_DTYPE)
    a["key"][:, :2] = [[1, 5], [1, -5], [-2, 0]]; a["agg"]["n_match"] = [1, 2, 3]; a["agg"]["n"] = [1, 2, 3]; a["agg"]["min"] = [4, 5, 6]; a["agg"]["max"] = [4, 5, 6]
    a["agg"]["sum_lo"] = [4, 10, 18]
    b["key"][:, :2] = [[1, -5], [0, 0]]; b["agg"]["n_match"] = [7, 1]; b["agg"]["n"] = [7, 1]; b["agg"]["min"] = [-1, 0]; b["agg"]["max"] = [9, 0]
    b["agg"]["sum_lo"] = [(1 << 64) - 3, 0]; b["agg"]["sum_hi"] = [-1, 0]
    u = bmx.mgroup_merge([a, b, np.zeros(0, bmx.MGROUP_DTYPE)])
    assert u["key"][:, :2].tolist() == [[-2, 0], [0, 0], [1, -5], [1, 5]], "lexicographic, signed"
    r = u[2]["agg"]
    assert (int(r["n_match"]), int(r["min"]), int(r["max"]), int(r["sum_lo"]), int(r["sum_hi"])) == (9, -1, 9, 7, 0)
    assert mm.sort_records(u).tobytes() == bmx.mgroup_sort(u).tobytes() == u.tobytes()
    g = bmx.MultiGroupResult(np.zeros((), bmx.GROUP_RES_DTYPE), u, 2)
    assert g.n_groups == 0 and not g.groups


def test_the_seeded_suite_meets_its_conditions():
    m, tombs = gm.seeded_model()
    gm.apply_tombs(m, tombs)
    qs = mm.seeded_queries()
    assert len(qs) == 60
    nothing = tuples2 = absent = multi_bucket = 0
    for p, keys, measure in qs:
        recs, res = mm.answer(m, FB, p, keys, measure, 1 << 14)
        assert int(res["flags"]) == 0 and mm.invariant(recs, res)
        nothing += int(res["total"]["n_match"]) == 0
        tuples2 += len(recs) >= 2
        absent += int(res["absent"]["n_match"]) > 0
        multi_bucket += len(keys) >= 2 and mm.buckets_in(keys) >= 1
    assert nothing <= 6, "at most 10 % select nothing"
    assert tuples2 >= 30, "at least half give two tuples or more"
    assert absent >= 30, "at least half have a non-empty absent"
    assert multi_bucket >= 20, "at least a third use two or more keys with a bucket on one of them"
