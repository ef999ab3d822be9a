"""CPU: the model of the group-by over discovered values (group_model.py) against brute force, every layout of the edge suite against the sequential stand-in
engine with every path tag reached, the checks shown to fail on stand-ins that carry one defect each, and the conditions the seeded GPU suite relies on."""
import numpy as np
import pytest

import group_model as gm
import where_agg_model as wam
from where_agg_model import DATA, Model


def _layout_rows(lay):
    n = lay["n"]
    gk = [int(k) if p else None for k, p in zip(lay["keys"], lay["present"])]
    mv = [int(37 * i - 1000) if i % 5 else None for i in range(n)]
    return lay["sel"], gk, mv


def _layout_want(lay, measured=True):
    """brute force over the layout: numpy.unique + where_agg_model.record"""
    n = lay["n"]
    sel, pres, keys = lay["sel"], lay["present"], lay["keys"]
    mv = np.array([37 * i - 1000 for i in range(n)], np.int64); hm = np.arange(n) % 5 != 0

    def rec(rows):
        return wam.record(int(rows.sum()), mv[rows & hm] if measured else None)

    res = np.zeros((), gm.GROUP_RES_DTYPE)
    res["absent"] = rec(sel & ~pres); res["total"] = rec(sel)
    u = np.unique(keys[sel & pres])
    res["n_groups"] = len(u)
    if len(u) > lay["cap"]:
        res["flags"] = gm.OVERFLOW
        return np.zeros(0, gm.GROUP_DTYPE), res
    out = np.zeros(len(u), gm.GROUP_DTYPE)
    for i, k in enumerate(u):
        out[i]["key"] = k; out[i]["agg"] = rec(sel & pres & (keys == k))
    return out, res


def test_arithmetic_restated_twice():
    keys = np.concatenate([[0, 1, -1, gm.BIG, -gm.BIG, 2**31, -2**31, 2**32 + 5], np.random.default_rng(1).integers(-gm.BIG, gm.BIG, 500)])
    assert [gm.mix(k) for k in keys] == gm.mix_np(keys).tolist()
    assert [gm.cache_set(k) for k in keys] == gm.cache_set_np(keys).tolist()
    assert gm.mix(0) == 0 and gm.mix(1) == 0xb456bcfc34c2cb2c                          # MurmurHash3 fmix64(1)
    assert [gm.slots_for(c) for c in (1, 8, 32, 33, 1024, 1025, gm.MAX_CAP)] == [64, 64, 64, 128, 2048, 4096, 1 << 21]
    # Fibonacci hashing: an arithmetic progression of 512 values inside one 2^32 block never puts more than WAYS keys into one set, whatever its stride
    for start, step in ((0, 1), (5000, 1), (gm.WIDE, 1), (0, 3600), (7, 1024), (1700000000, 86400), (-gm.BIG, 1)):
        sets = gm.cache_set_np(start + step * np.arange(512, dtype=np.int64))
        assert np.bincount(sets, minlength=gm.SETS).max() <= gm.WAYS, (start, step)
    assert gm.grid(32768, 4) == 1 and gm.grid(32769, 4) == 2 and gm.grid(16385, 2) == 2 and gm.grid(10**9, 4) == 512
    wg, wave, lane, step = gm.place(np.array([0, 3, 4, 255, 256, 8191, 8192, 16384, 32768]), 32769, 4)
    assert wg.tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 0] and lane.tolist() == [0, 0, 1, 63, 0, 63, 0, 0, 0] and wave.tolist() == [0, 0, 0, 0, 1, 7, 0, 0, 0]


def test_walks_do_not_depend_on_the_order():
    rng = np.random.default_rng(3)
    ks = gm.keys_with_home(40, 64, 7) + gm.keys_with_home(63, 64, 3) + [int(k) for k in rng.integers(-gm.BIG, gm.BIG, 20)]
    tags0, table0 = gm.walk(ks, 64)
    for _ in range(5):
        order = [ks[i] for i in rng.permutation(len(ks))]
        tags, table = gm.walk(order, 64)
        assert set(table) == set(table0), "the occupied slots are the same whoever comes first"
    same = gm.keys_with_home(40, 64, 7)
    for _ in range(3):
        tags, _ = gm.walk([same[i] for i in rng.permutation(7)], 64)
        assert sorted(t[1] if len(t) > 1 else 0 for t in tags.values()) == list(range(7))
    tags, _ = gm.walk(gm.keys_with_home(63, 64, 2), 64)
    assert sorted(tags.values()) == [("home",), ("wrap", 1)]
    tags, _ = gm.walk(gm.keys_with_home(5, 64, 65), 64)
    assert list(tags.values()).count(("noroom",)) == 1 and ("wrap", 63) in tags.values()


@pytest.mark.parametrize("wide", [False, True])
def test_model_against_brute_force_on_the_seeded_table(wide):
    m, tombs = gm.seeded_model(wide)
    gm.apply_tombs(m, tombs)
    F = gm._names()
    pos_nodes = np.nonzero(m.st[F["base"]] != 0)[0][::-1]                 # some position order: the stand-in needs one, the answer does not depend on it
    qs = gm.seeded_queries()
    for k in range(0, len(qs), 7):
        p, group, measure = qs[k]
        for cap in (4, 400):
            want = gm.answer(m, F["base"], p, group, measure, cap)
            d = gm.Device(len(pos_nodes), 2 if wide else 4, cap, measure is not None)
            got = d.run(*gm.rows_of(m, F["base"], p, group, measure, pos_nodes))
            assert gm.check(*got, *want, cap) is None, (k, cap, gm.check(*got, *want, cap))
            if not int(want[1]["flags"]):
                assert gm.invariant(*want)


@pytest.mark.parametrize("wide", [False, True])
def test_edge_suite_on_the_stand_in_reaches_every_path(wide):
    reached = set()
    for lay in gm.edge_layouts(wide):
        d = gm.Device(lay["n"], 2 if wide else 4, lay["cap"], True)
        got = d.run(*_layout_rows(lay))
        want = _layout_want(lay)
        assert gm.check(*got, *want, lay["cap"]) is None, (lay["name"], gm.check(*got, *want, lay["cap"]))
        assert lay["tags"] <= d.tags, (lay["name"], lay["tags"] - d.tags)
        reached |= d.tags
        if lay["name"] == "set_overflows":
            assert len({lay["keys"][p] for p, t in d.row_tags.items() if t == "bypass"}) == 2, "six keys in a set of four ways: two of them bypass"
        if lay["name"] == "walk_slots_less_one":
            assert d.claims == 64 and not d.overflow and int(got[1]["flags"]) == gm.OVERFLOW, "64 keys fill 64 slots: more than cap, yet every walk found room"
        if lay["name"].startswith("size_") and lay["n"] > 4 * gm.THREADS * gm.U * (2 if wide else 4):
            assert gm.grid(lay["n"], 2 if wide else 4) == 2
    assert {"hit", "bypass", "home", "walk", "wrap", "noroom", ("len", 1), ("len", 63)} <= reached


@pytest.mark.parametrize("defect,layout", [("drop_bypass", "set_overflows"), ("lose_wrap", "wrap"), ("absent_in_group", "size_257"), ("unsorted", "lanes_on_64_keys")])
def test_the_checks_fail_on_a_wrong_answer(defect, layout):
    lay = [x for x in gm.edge_layouts(False) if x["name"] == layout][0]
    if defect == "absent_in_group":
        lay["keys"] = lay["keys"] % 7                                    # key 0 exists: the folded rows hide inside a real group
    want = _layout_want(lay)
    good = gm.Device(lay["n"], 4, lay["cap"], True).run(*_layout_rows(lay))
    assert gm.check(*good, *want, lay["cap"]) is None
    bad = gm.Device(lay["n"], 4, lay["cap"], True, defect=defect).run(*_layout_rows(lay))
    assert gm.check(*bad, *want, lay["cap"]) is not None, defect
    # an answer that writes on overflow, and one that writes behind its last record
    over = [x for x in gm.edge_layouts(False) if x["name"] == "no_room"][0]
    w = _layout_want(over)
    g = gm.Device(over["n"], 4, over["cap"], True).run(*_layout_rows(over))
    assert gm.check(*g, *w, over["cap"]) is None
    g[0][2]["key"] = 1
    assert gm.check(*g, *w, over["cap"]) is not None
    good[0][lay["cap"]]["key"] = 1
    assert gm.check(*good, *want, lay["cap"]) is not None


def test_the_seeded_suite_selects_groups_and_absent_rows():
    """what test_gpu_where_group.py's seeded run relies on, asserted on the model alone: a GPU test cannot pass by selecting nothing"""
    for wide in (False, True):
        m, tombs = gm.seeded_model(wide)
        gm.apply_tombs(m, tombs)
        F = gm._names()
        qs = gm.seeded_queries()
        assert len(qs) == gm.N_PROGS >= 60
        assert {q[1] == F["base"] for q in qs} == {True, False} and any(q[1] == F["key"] for q in qs) and {q[2] for q in qs} == {None, F["base"], F["measure"]}
        empty = rich = over = 0
        for p, group, measure in qs:
            recs, res = gm.answer(m, F["base"], p, group, measure, 4096)
            empty += int(res["total"]["n_match"]) == 0
            rich += len(recs) >= 2 and int(res["absent"]["n_match"]) > 0
            if measure == F["measure"] and len(recs):
                over += int(res["total"]["n"]) < int(res["total"]["n_match"])
        assert empty <= len(qs) // 10, empty
        assert rich >= len(qs) // 2, rich
        assert over >= 5, "measure rows absent and tombstoned: n < n_match"
        for f in ("one", "two", "three", "key", "measure"):
            assert set(np.unique(m.st[F[f]])) == {0, 1, 2}, "the fields in all three states"
        keys = m.val[F["key"]][m.st[F["key"]] == DATA]
        assert {0, 1, -1, gm.BIG, -gm.BIG} <= set(keys.tolist()) and (keys < 0).any() and (keys > 0).any()


def test_group_merge_is_the_fold_by_key():
    import bmx
    assert bmx.GROUP_DTYPE == gm.GROUP_DTYPE and bmx.GROUP_RES_DTYPE == gm.GROUP_RES_DTYPE
    m, tombs = gm.seeded_model(False)
    gm.apply_tombs(m, tombs)
    F = gm._names()
    p = [[(F["base"], 0, 11)]]
    whole, _ = gm.answer(m, F["base"], p, F["key"], F["measure"], 4096)
    parts = []
    for g in range(3):                                                   # the nodes dealt over three "shards"
        sub = Model(m.ids)
        for f in m.val:
            sub.val[f] = m.val[f].copy(); sub.st[f] = np.where(np.arange(m.N) % 3 == g, m.st[f], 0).astype(np.uint8)
        parts.append(gm.answer(sub, F["base"], p, F["key"], F["measure"], 4096)[0])
    assert len(whole) > 200 and all(0 < len(x) < len(whole) for x in parts)
    merged = bmx.group_merge(parts)
    assert merged.tobytes() == whole.tobytes()
    assert len(bmx.group_merge([])) == 0 and bmx.group_merge([parts[0]]).tobytes() == parts[0].tobytes()
