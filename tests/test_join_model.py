"""CPU: the model of the lookup joins against itself (tests/join_model.py). The sequential stand-in of the kernels (Device: build / insert, sweep, finish on the
group table's home and walk, with group_model's LDS cache) gives the brute-force answer on every edge layout the GPU tests run, with every path reached;
stand-ins with one defect each are caught by the same check(); and the seeded suite's 60 program pairs select what they are there to select."""
import numpy as np
import pytest

import join_model as jm


def _layouts():
    for name, m, tombs, qs in jm.edge_layouts():
        jm.apply_tombs(m, tombs)
        yield name, m, qs


def _cases():
    for name, m, qs in _layouts():
        for q0 in qs:
            for q in jm.variants(m, q0):
                yield name, m, q
            if q0["kind"] == "join":
                ql = jm.as_list(m, q0)
                if ql is not None:
                    yield name + " (as a list)", m, ql


def test_the_stand_in_gives_the_brute_force_answer_on_every_layout():
    tags = set()
    flags = {0: 0, 1: 0, 2: 0}
    for name, m, q in _cases():
        want = jm.want_of(m, q)
        out, res, d = jm.device_of(m, q)
        bad = jm.check(out, res, *want, q["cap"], jm.map_cap_of(q))
        assert bad is None, (name, q, bad)
        assert d.keys == [jm.EMPTY] * d.slots and d.vals == [jm.NO_ATTR] * d.slots and (d.claims, d.n_inner, d.n_keyed, d.overflow) == (0, 0, 0, 0), "finish leaves the scratch clean"
        tags |= {t[0] if isinstance(t, tuple) else t for t in d.tags}
        flags[int(want[1]["flags"])] += 1
    assert tags == {"present", "claim", "walk", "wrap", "giveup", "lowered", "min_skipped", "skipped", "grouped", "absent", "unmatched", "bypass"}, tags
    assert flags[0] >= 100 and flags[1] >= 20 and flags[2] >= 20, flags


def test_the_list_form_is_the_program_form_on_the_same_pairs():
    seen = 0
    for name, m, qs in _layouts():
        for q in qs:
            ql = jm.as_list(m, q) if q["kind"] == "join" else None
            if ql is None:
                continue
            a, b = jm.want_of(m, dict(q, map_cap=1 << 12)), jm.want_of(m, ql)
            assert a[0].tobytes() == b[0].tobytes()
            for k in ("n_groups", "map_size", "n_keyed", "absent", "unmatched", "total"):
                assert np.asarray(a[1][k]).tobytes() == np.asarray(b[1][k]).tobytes(), (name, k)
            seen += 1
    assert seen >= 30


def test_table_walks_of_the_edge_layout():
    """the table-edge layout really is what its text says: 32 keys with one home give walks 1..31; the wrapping cluster passes slot 63; a lookup of the absent
    key with the cluster's home sees every one of its words; 70 keys into 64 slots give up"""
    m, _, qs = jm.table_edges()
    _, _, d = jm.device_of(m, qs[0])
    assert sorted(t[1] for t in d.tags if isinstance(t, tuple)) == list(range(1, 32)) and "claim" in d.tags and d.slots == 64
    _, _, d = jm.device_of(m, qs[1])
    assert "wrap" in d.tags and d.slots == 64
    dev = jm.Device(6)
    wrap = jm.keys_with_home(62, 64, 7, start=10**6)
    dev.insert_list(wrap[:6], range(6))
    assert [dev.keys[s] != jm.EMPTY for s in (61, 62, 63, 0, 1, 2, 3, 4)] == [False, True, True, True, True, True, True, False]
    assert dev._walk(wrap[6], False) is None and [dev.vals[dev._walk(k, False)] for k in wrap[:6]] == list(range(6))
    _, res, d = jm.device_of(m, qs[4])
    assert "giveup" in d.tags and int(res["flags"]) == jm.MAP_OVERFLOW and int(res["n_keyed"]) == 70


def test_the_minimum_is_independent_of_order():
    rng = np.random.default_rng(5)
    keys, vals = rng.integers(0, 9, 200), rng.integers(-50, 50, 200)
    vals[rng.random(200) < 0.3] = jm.NO_ATTR
    K, V, _, _ = jm.list_map(keys, vals)
    for _ in range(3):
        p = rng.permutation(200)
        d = jm.Device(200)
        d.insert_list(keys[p], vals[p])
        got = {d.keys[s]: d.vals[s] for s in range(d.slots) if d.keys[s] != jm.EMPTY}
        assert got == dict(zip(K.tolist(), V.tolist()))


@pytest.mark.parametrize("defect", jm.DEFECTS)
def test_a_stand_in_with_one_defect_is_caught(defect):
    caught = 0
    for name, m, q in _cases():
        want = jm.want_of(m, q)
        out, res, _ = jm.device_of(m, q, defect)
        caught += jm.check(out, res, *want, q["cap"], jm.map_cap_of(q)) is not None
    assert caught >= 1, defect


def test_the_seeded_pairs_select_what_they_are_there_for():
    m, tombs = jm.seeded_model()
    jm.apply_tombs(m, tombs)
    pairs = jm.seeded_pairs()
    assert len(pairs) == 60
    nothing = all_three = shared = 0
    for q in pairs:
        k, v, _ = jm.inner_pairs(m, q["inner_base"], q["inner_clauses"], q["key"], q["attr"])
        K, V = jm.unite(k, v)
        assert len(K) <= q["map_cap"], "the suite's map_cap"
        sel, un, ab, gr, attr = jm.destinations(m, q["base"], q["clauses"], q["link"], K, V)
        assert len(np.unique(attr[gr])) <= q["cap"], "the suite's cap"
        nothing += sel.sum() == 0
        all_three += bool(un.any() and ab.any() and gr.any())
        # a key held by two inner nodes with different attributes
        order = np.lexsort((v, k))
        ks, vs = k[order], v[order]
        shared += bool(((ks[1:] == ks[:-1]) & (vs[1:] != vs[:-1]) & (vs[1:] != jm.NO_ATTR)).any())
    assert nothing <= 6, nothing
    assert all_three >= 30, all_three
    assert shared >= 15, shared


def test_the_result_object():
    import bmx
    res = np.zeros((), bmx.JOIN_RES_DTYPE)
    res["n_groups"] = 2; res["map_size"] = 3; res["n_inner"] = 9; res["n_keyed"] = 5
    recs = np.zeros(4, bmx.GROUP_DTYPE); recs["key"] = [4, 8, 0, 0]
    r = bmx.JoinResult(res, recs)
    assert (r.n_groups, r.map_size, r.n_inner, r.n_keyed, r.map_overflow, r.group_overflow, list(r.groups)) == (2, 3, 9, 5, False, False, [4, 8])
    res["flags"] = bmx.JOIN_GROUP_OVERFLOW; res["n_groups"] = 70
    r = bmx.JoinResult(res, recs)
    assert r.group_overflow and not r.map_overflow and r.n_groups == 70 and len(r.records) == 0
    c = bmx.JoinRes(); c.n_groups = 1; c.flags = bmx.JOIN_MAP_OVERFLOW
    assert bmx.JoinResult(c, recs).map_overflow and len(bmx.JoinResult(c, recs).records) == 0
    assert jm.JOIN_RES_DTYPE == bmx.JOIN_RES_DTYPE and (jm.MAP_OVERFLOW, jm.GROUP_OVERFLOW, jm.MAX_MAP) == (bmx.JOIN_MAP_OVERFLOW, bmx.JOIN_GROUP_OVERFLOW, bmx.JOIN_MAX_MAP)
