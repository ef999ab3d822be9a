"""CPU: the numpy model of the join projection (tests/join_rows_model.py) against plain Python loops, and its sequential stand-in of the map against the brute
force: the carried word keeps the unsigned order of the ids, the smallest unsigned id wins whatever the order of insertion, walks wrap, a stand-in that
compares the ids as signed numbers is noticed."""
import itertools

import numpy as np

import join_rows_model as jrm
from join_rows_model import DATA, FB, FI, FK, FL, FX, FY, F1, F2, NO_NODE, NOBODY

IDS = [0, 1, 2**63 - 1, 2**63, 2**64 - 2]


def test_the_carried_word_keeps_the_unsigned_order():
    words = [jrm.word_of(i) for i in IDS]
    assert words == sorted(words) and all(-(1 << 63) <= w < (1 << 63) for w in words)
    assert [jrm.id_of(w) for w in words] == IDS
    assert jrm.word_of(NO_NODE) == jrm.NO_ATTR and jrm.id_of(jrm.NO_ATTR) == NO_NODE, "the reserved id is the word of an unlowered slot"
    assert jrm.word_of(0) == jrm.INT64_MIN and jrm.word_of(2**63) == 0


def test_the_smallest_unsigned_id_wins_in_any_order():
    for perm in itertools.permutations(IDS[1:]):
        d = jrm.MapDevice(4)
        d.insert_list([7] * len(perm), perm)
        assert d.find(7) == 1 and d.claims == 1 and d.fits()
    d = jrm.MapDevice(4)
    d.insert_list([7, 7, 7], [2**63, 2**64 - 2, 2**63 - 1])
    assert d.find(7) == 2**63 - 1 and "lowered" in d.tags
    s = jrm.MapDevice(4, signed=True)
    s.insert_list([7, 7, 7], [2**63, 2**64 - 2, 2**63 - 1])
    assert s.find(7) == 2**63, "the signed defect picks the id with the top bit set"
    K, I, n_inner, n_keyed = jrm.list_map([7, 7, 7], np.array([2**63, 2**64 - 2, 2**63 - 1], np.uint64))
    assert K.tolist() == [7] and I.tolist() == [2**63 - 1] and (n_inner, n_keyed) == (3, 3)


def test_the_list_skips_what_the_header_says():
    keys = [jrm.VAL_MAX, jrm.VAL_MAX + 1, -jrm.VAL_MAX, -jrm.VAL_MAX - 1, jrm.INT64_MIN, 3, 3, 0]
    ids = [5, 6, 7, 8, 9, NO_NODE, 11, 0]
    K, I, n_inner, n_keyed = jrm.list_map(keys, np.array(ids, np.uint64))
    assert K.tolist() == [-jrm.VAL_MAX, 0, 3, jrm.VAL_MAX] and I.tolist() == [7, 0, 11, 5] and n_inner == n_keyed == 4
    d = jrm.MapDevice(len(keys))
    d.insert_list(keys, ids)
    assert d.pairs() == list(zip(K.tolist(), I.tolist())) and d.counted == 4 and "skipped" in d.tags


def test_walks_that_wrap():
    wrap = jrm.keys_with_home(62, 64, 7, start=10**6)
    same = jrm.keys_with_home(5, 64, 33)
    d = jrm.MapDevice(32)
    assert d.slots == 64
    d.insert_list(wrap[:6], range(100, 106))
    assert "wrap" in d.tags and ("walk", 5) in d.tags
    assert [d.find(k) for k in wrap] == [100, 101, 102, 103, 104, 105, NO_NODE], "a link to an absent key walks the cluster to its empty word"
    d = jrm.MapDevice(32)
    d.insert_list(same[:32] + same[:32], list(range(64, 0, -1)))
    assert d.fits() and d.claims == 32 and [d.find(k) for k in same] == list(range(32, 0, -1)) + [NO_NODE]
    d = jrm.MapDevice(32)
    d.insert_list(list(range(1000, 1070)), range(70))
    assert not d.fits()


def _loops(m, order, q):
    """answer() as plain loops over the index positions"""
    K, I, _, _ = jrm.map_of(m, q)
    M = dict(zip(K.tolist(), I.tolist()))
    node = {int(i): k for k, i in enumerate(m.ids.tolist())}
    sel = m.mask(q["base"], q["clauses"])
    rows, n_match, next_pos = [], 0, len(order)
    for pos, i in enumerate(order.tolist()):
        k = node[i]
        if pos < q["start"] or not sel[k]:
            continue
        iid = M.get(int(m.val[q["link"]][k]), NO_NODE) if m.st[q["link"]][k] == DATA else NO_NODE
        if q["inner"] and iid == NO_NODE:
            continue
        if n_match == q["cap"]:
            next_pos = pos
        n_match += 1
        if len(rows) < q["cap"]:
            rows.append((k, iid))

    def cell(f, k):
        if k is None or m.st[f][k] == jrm.ABSENT:
            return jrm.VAL_DELETED, jrm.NO_CLOCK
        return (int(m.val[f][k]) if m.st[f][k] == DATA else jrm.VAL_DELETED), int(m.clk[f][k])

    out = [(int(m.ids[k]), iid, [cell(f, k) for f in q["fields"]], [cell(f, node.get(iid)) for f in q["in_fields"]]) for k, iid in rows]
    return out, n_match, next_pos


def test_answer_against_plain_loops():
    m, tombs, ow, iw = jrm.truth_table()
    jrm.apply_tombs(m, tombs)
    order = m.ids[np.nonzero(m.st[FB] != jrm.ABSENT)[0]][::-1].copy()           # some order of the outer index
    sel, inner = [[(FB, 1, 1)]], [[(FI, 1, 3)]]
    kinds = set()
    for clauses, inn, start, cap in itertools.product((sel, jrm.EVERY, [[(FB, 1, 1), (F1, 0, 3)], [(F2, 0, 10**6, True)]]), (False, True), (0, 17), (0, 1, 5, 1000)):
        for q in (jrm.Q(FB, clauses, FL, [F1, F2, FB, FL], FI, inner, FK, [FX, FY, FK, FI, NOBODY], True, inn, start, cap),
                  jrm.QMAP(FB, clauses, FL, [F2], [100, 101, 101, 5047, 103], [int(m.ids[3]), 77, int(m.ids[9]), int(m.ids[1]), NO_NODE], [FX, FY], True, inn, start, cap)):
            want = jrm.answer(m, order, q)
            rows, n_match, next_pos = _loops(m, order, q)
            r = want["res"]
            assert (int(r["n_match"]), int(r["n_out"]), int(r["next_pos"])) == (n_match, len(rows), next_pos)
            assert int(r["n_joined"]) == sum(iid != NO_NODE for _, iid, _, _ in rows)
            assert want["ids"].tolist() == [x[0] for x in rows] and want["in_ids"].tolist() == [x[1] for x in rows]
            for k in range(len(q["fields"])):
                assert list(zip(want["vals"][k].tolist(), want["ts"][k].tolist())) == [x[2][k] for x in rows]
            for k in range(len(q["in_fields"])):
                cells = list(zip(want["in_vals"][k].tolist(), want["in_ts"][k].tolist()))
                assert cells == [x[3][k] for x in rows]
                kinds |= {"data" if v != jrm.VAL_DELETED else ("tomb" if t != jrm.NO_CLOCK else "absent") for v, t in cells}
            if inn:
                assert int(r["n_joined"]) == int(r["n_out"])
    assert kinds == {"data", "tomb", "absent"}
    # the map of the program: four nodes per key, the smallest id each; 105 is held by tombstones only
    K, I, n_inner, n_keyed = jrm.inner_map(m, FI, inner, FK)
    assert K.tolist() == [100, 101, 102, 103, 104] and n_inner == 24 + 8 and n_keyed == 20
    for k, i in zip(K.tolist(), I.tolist()):
        assert i == min(int(x) for x in m.ids[:24][(m.val[FK][:24] == k) & (m.st[FK][:24] == DATA)])
    # an overflow: nothing but the record
    q = jrm.Q(FB, sel, FL, [F1], FI, inner, FK, [FX], map_cap=4)
    w = jrm.answer(m, order, q)
    assert int(w["res"]["flags"]) == jrm.MAP_OVERFLOW and len(w["ids"]) == 0 and int(w["res"]["next_pos"]) == len(order) and int(w["res"]["n_match"]) == 0


def test_check_notices_a_signed_minimum():
    ids = np.array(IDS + [5], np.uint64)
    m = jrm.Table(ids)
    m.set(FI, np.arange(5), 1); m.set(FK, np.arange(5), 42); m.set(FX, np.arange(5), 10 + np.arange(5))
    m.set(FB, [5], 1); m.set(FL, [5], 42)
    q = jrm.Q(FB, jrm.EVERY, FL, [], FI, jrm.EVERY, FK, [FX])
    want = jrm.answer(m, ids[5:], q)
    assert want["in_ids"].tolist() == [0] and want["in_vals"].tolist() == [[10]]
    q1 = jrm.Q(FB, jrm.EVERY, FL, [], FI, [[(FX, 11, 14)]], FK, [FX])
    want = jrm.answer(m, ids[5:], q1)
    assert want["in_ids"].tolist() == [1]
    q2 = jrm.Q(FB, jrm.EVERY, FL, [], FI, [[(FX, 12, 14)]], FK, [FX])
    want = jrm.answer(m, ids[5:], q2)
    assert want["in_ids"].tolist() == [2**63 - 1], "2^63 - 1 is below 2^63 and 2^64 - 2 as unsigned numbers"
    s = jrm.MapDevice(4, signed=True)
    s.insert_list([42] * 3, IDS[2:])
    got = dict(want, in_ids=np.array([s.find(42)], np.uint64), res=want["res"].copy())
    got["res"]["layout"] = 1
    assert jrm.check(got, want, q2)[0] == "in_ids"
    ok = dict(want, res=got["res"])
    assert jrm.check(ok, want, q2) is None
