"""CPU: the model of the semi-joins against itself (tests/semi_model.py). The sequential stand-in of the kernels (Device: build / insert, probe, finish on the
group table's home and walk) gives the brute-force answer (numpy.unique + numpy.isin) on every edge layout the GPU tests run, with every path of the insert
reached; stand-ins with one defect each are caught by the same check(); and the seeded suite's 60 query pairs select what they are there to select."""
import numpy as np
import pytest

import semi_model as sm


def _layouts():
    for name, m, tombs, qs in sm.edge_layouts():
        sm.apply_tombs(m, tombs)
        yield name, m, qs


def test_the_stand_in_gives_the_brute_force_answer_on_every_layout():
    tags = set()
    overflows = fits = 0
    for name, m, qs in _layouts():
        pn = np.arange(m.N)
        for q in qs:
            want = sm.want_of(m, pn, q)
            for cap in sm.caps_of(want.n_match, m.N):
                buf, res, d = sm.device_of(m, q, cap)
                assert sm.check(buf, res, want, cap, sm.set_cap_of(q)) is None, (name, q, cap, sm.check(buf, res, want, cap, sm.set_cap_of(q)))
                assert d.table == [sm.EMPTY] * d.slots and (d.claims, d.n_inner, d.overflow) == (0, 0, 0), "finish leaves the scratch clean"
                tags |= {t[0] for t in d.tags}
            overflows += want.flags; fits += 1 - want.flags
    assert tags == {"present", "home", "walk", "wrap", "giveup", "skipped"}, tags
    assert overflows >= 6 and fits >= 60


def test_anti_is_the_exact_complement_inside_the_outer_selection():
    for name, m, qs in _layouts():
        pn = np.arange(m.N)
        for q in qs:
            if q["anti"]:
                continue
            a, b = sm.want_of(m, pn, q), sm.want_of(m, pn, dict(q, anti=True))
            if a.flags:
                assert b.flags and (a.n_match, b.n_match) == (0, 0)
                continue
            outer = m.ids[m.mask(q["base"], q["clauses"])]
            assert len(np.intersect1d(a.ids, b.ids)) == 0 and np.array_equal(np.sort(np.concatenate([a.ids, b.ids])), np.sort(outer)), (name, q)


def test_table_walks_of_the_edge_layout():
    """the table-edge layout really is what its text says: 32 keys with one home give walks 0..31; the wrapping cluster passes slot 63; a probe of the absent
    key with the cluster's home sees every one of its words"""
    m, _, qs = sm.table_edges()
    _, _, d = sm.device_of(m, qs[0])
    assert sorted(t[1] for t in d.tags if t[0] == "walk") == list(range(1, 32)) and d.tags.count(("home",)) == 1
    _, _, d = sm.device_of(m, qs[2])
    assert sum(t[0] == "wrap" for t in d.tags) == 4 and d.slots == 64
    dev = sm.Device(6)
    wrap = sm.keys_with_home(62, 64, 7, start=10**6)
    dev.insert_list(wrap[:6])
    assert [dev.table[s] != sm.EMPTY for s in (61, 62, 63, 0, 1, 2, 3, 4)] == [False, True, True, True, True, True, True, False]
    assert not dev.has(wrap[6]) and all(dev.has(k) for k in wrap[:6])


@pytest.mark.parametrize("defect", sm.DEFECTS)
def test_a_stand_in_with_one_defect_is_caught(defect):
    caught = 0
    for name, m, qs in _layouts():
        pn = np.arange(m.N)
        for q in qs:
            want = sm.want_of(m, pn, q)
            for cap in sm.caps_of(want.n_match, m.N):
                buf, res, _ = sm.device_of(m, q, cap, defect)
                caught += sm.check(buf, res, want, cap, sm.set_cap_of(q)) is not None
    assert caught >= 1, defect


def test_a_tombstoned_key_is_no_key():
    """the truth tables have no tombstoned key, so the defect above needs a layout of its own: a key row that was tombstoned keeps its old value in the slot"""
    m = sm.Model(sm.wam.node_ids(40, 65000))
    i = np.arange(40)
    m.set(sm.FB, i, i); m.set(sm.FL, i, i % 4); m.set(sm.FI, i[:4], i[:4]); m.set(sm.FK, i[:4], i[:4])
    m.tomb(sm.FK, [2])
    q = sm.Q(sm.FB, sm.EVERY, sm.FL, sm.FI, sm.EVERY, sm.FK)
    want = sm.want_of(m, i, q)
    assert (want.n_match, want.set_size, want.n_inner) == (30, 3, 4)
    buf, res, _ = sm.device_of(m, q)
    assert sm.check(buf, res, want, m.N, 64) is None
    buf, res, _ = sm.device_of(m, q, defect="tomb_key")
    assert sm.check(buf, res, want, m.N, 64) is not None


def test_the_seeded_pairs_select_what_they_are_there_for():
    m, tombs = sm.seeded_model()
    sm.apply_tombs(m, tombs)
    pairs = sm.seeded_pairs()
    assert len(pairs) == 60
    nothing = both_sides = no_link = 0
    for outer, link, inner, key, anti in pairs:
        S, n_inner = sm.inner_set(m, sm.FI, inner, key)
        sel = m.mask(sm.FB, outer)
        have = m.st[link] == sm.DATA
        inside = have & np.isin(m.val[link], S)
        nothing += sm.selected(m, sm.FB, outer, link, S, anti).sum() == 0
        both_sides += bool((sel & inside).any() and (sel & have & ~inside).any())
        no_link += bool((sel & (m.st[link] == sm.ABSENT)).any() or (sel & (m.st[link] == sm.TOMB)).any())
        assert len(S) <= 1024, "the suite's set_cap"
    assert nothing <= 6, nothing
    assert both_sides >= 30, both_sides
    assert no_link >= 15, no_link


def test_the_result_object():
    import bmx
    res = np.zeros((), bmx.SEMI_RES_DTYPE)
    res["n_match"] = 5; res["set_size"] = 3; res["n_inner"] = 9
    ids = np.arange(10, dtype=np.uint64)
    r = bmx.SemiResult(res, ids, 4)
    assert (r.n_match, r.set_size, r.n_inner, r.overflow, r.ids.tolist()) == (5, 3, 9, False, [0, 1, 2, 3])
    res["flags"] = bmx.SEMI_OVERFLOW; res["n_match"] = 0; res["set_size"] = 70
    r = bmx.SemiResult(res, ids, 4)
    assert r.overflow and r.set_size == 70 and len(r.ids) == 0
    c = bmx.SemiRes(); c.n_match = 2; c.n_inner = 1
    assert bmx.SemiResult(c, ids, 8).ids.tolist() == [0, 1] and bmx.SemiResult(c, None, 0).n_match == 2
