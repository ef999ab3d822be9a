"""GPU: lookup joins (include/bmx_join.h bmx_where_join_group, bmx_where_map_group). Every answer is compared exactly with join_model's brute force — the inner
selection, the minimum attribute of each present key, the three destinations of every selected outer node: every byte of the records and of the result record,
and the fill pattern behind out[D] (on either overflow: in the whole buffer).

The tables are the smallest on which each rule can go wrong (join_model.edge_layouts, which test_join_model.py runs through a sequential stand-in of the
kernels): the truth table of {outer selected or not} x {link in M with attribute, in M without, not in M, tombstone, absent} x {measure data, tombstone, absent}
on both column widths of both sides; link, key, attribute and measure from the column, from a field the program probes and from a field it does not name;
attr_field == key_field; one base field on both sides; keys and attributes 0, +-1, +-(2^53 - 1); empty and keyless inner sides; every query also with
cap = D and D - 1, map_cap = K and K - 1 and both at once, and as the list form of its own pairs. The seeded suite has more than one 8192-row block."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import group_model as gm
import join_model as jm
import semi_model as sm
import where_agg_model as wam
from join_model import EVERY, F1, F2, FA, FB, FI, FK, FL, FM, Q, QMAP

LAYOUTS = {name: (m, tombs, qs) for name, m, tombs, qs in jm.edge_layouts() if name not in ("table edges", "cache bypass")}   # (those: the kernel-edges test)


def _engine(m, tombs, fields=jm.ALL_FIELDS, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    for f, idx in tombs.items():
        wam.tombstone(e, m, f, idx)
    return e


@pytest.fixture(scope="module")
def seeded():
    m, tombs = jm.seeded_model()
    with _engine(m, tombs, cap=16 * m.N) as e:
        yield e, m


# ---- 1. the edge layouts ----
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_edge_layouts(name):
    m, tombs, qs = LAYOUTS[name]
    with _engine(m, dict(tombs)) as e:
        seen = set()
        for q0 in qs:
            for q in jm.variants(m, q0):
                recs, res = jm.ask(e, m, q)
                seen.add((int(res["flags"]), len(recs) > 0, int(res["absent"]["n_match"]) > 0, int(res["unmatched"]["n_match"]) > 0))
                assert int(res["flags"]) or jm.invariant(recs, res)
            ql = jm.as_list(m, q0) if q0["kind"] == "join" else None
            if ql is not None:
                # the list form with the inner side's pairs (duplicates included) is the same query
                jm.ask(e, m, ql)
                (o1, r1), (o2, r2) = jm.raw_of(e, dict(q0, map_cap=4096)), jm.raw_of(e, ql)
                assert o1.tobytes() == o2.tobytes() and all(r1[k].tobytes() == r2[k].tobytes() for k in ("n_groups", "map_size", "n_keyed", "absent", "unmatched", "total")), (name, q0)
        assert {0, jm.MAP_OVERFLOW, jm.GROUP_OVERFLOW} <= {s[0] for s in seen}
        if name != "base links":
            assert (0, True, True, True) in seen, "all three destinations in one answer"


# ---- 2. the seeded suite ----
def test_seeded_pairs(seeded):
    """the 60 pairs of join_model.seeded_pairs (test_join_model.py asserts what they select), every fourth with an overflowing query directly in front of it
    (the map, the records, both in turn): an overflowing query leaves the scratch clean for the next"""
    e, m = seeded
    for k, q in enumerate(jm.seeded_pairs()):
        if k % 4 == 2:
            small = (dict(q, map_cap=4), dict(q, cap=2), dict(q, map_cap=4, cap=2))[(k // 4) % 3]
            _, res = jm.ask(e, m, small)
            assert int(res["flags"]) or int(res["n_groups"]) <= 2
        recs, res = jm.ask(e, m, q)
        assert not int(res["flags"]) and jm.invariant(recs, res)
        assert int(res["total"]["n_match"]) == e.scan_where(FB, q["clauses"], count_only=True)
    q = jm.seeded_pairs()[0]
    r = e.where_join_group(FB, q["clauses"], q["link"], FI, q["inner_clauses"], q["key"], q["attr"], measure=q["measure"], cap=1024, map_cap=1024)
    recs, res = jm.want_of(m, q)
    assert r.records.tobytes() == recs.tobytes() and (r.n_groups, r.map_size, r.n_inner, r.n_keyed, r.flags) == (len(recs), int(res["map_size"]), int(res["n_inner"]), int(res["n_keyed"]), 0)
    assert r.total.n_match == int(res["total"]["n_match"]) and r.unmatched.n_match == int(res["unmatched"]["n_match"]) and r.absent.n_match == int(res["absent"]["n_match"])
    keys, vals = jm.uid(np.arange(0, 800, 3)), np.arange(0, 800, 3) % 11
    r = e.where_map_group(FB, EVERY, FL, keys, vals, measure=FM, cap=16)
    recs, res = jm.want_of(m, QMAP(FB, EVERY, FL, keys, vals, FM, 16))
    assert r.records.tobytes() == recs.tobytes() and r.n_groups == 11 and r.map_size == len(keys) == r.n_inner == r.n_keyed
    assert e.where_map_group(FB, EVERY, FL, keys, vals, cap=10).group_overflow and e.where_join_group(FB, EVERY, FL, FI, EVERY, FK, FA, map_cap=5).map_overflow


# ---- 3. device memory ----
def test_device_memory_back_to_back(seeded):
    """device mode into poisoned buffers: five queries enqueued back to back (a deep one, one whose cap is exactly D, a map overflow, the list form with device
    lists, a group overflow), one synchronisation at the end; the answers are the model's, and nothing is written where nothing belongs"""
    e, m = seeded
    dev = torch.device("cuda", 0)
    outer, inner = [[(FB, 5, 80)], [(F1, 0, 1, True), (FB, 90, 99)]], [[(FI, 0, 150)]]
    keys = np.concatenate([jm.uid(np.arange(0, 900, 3)), [jm.INT64_MIN, jm.VAL_MAX + 1], jm.uid(np.arange(0, 30, 3))]).astype(np.int64)
    vals = np.concatenate([np.arange(300) % 17 - 4, [1, 2], [jm.INT64_MAX] * 5 + [-9] * 5]).astype(np.int64)
    base = Q(FB, outer, FL, FI, inner, FK, FA, FM, cap=512, map_cap=1024)
    D = len(jm.want_of(m, base)[0])
    assert D > 3
    jobs = [base, dict(base, cap=D), dict(base, map_cap=16), QMAP(FB, outer, FL, keys, vals, FM, 64), dict(base, cap=D - 1, measure=None)]
    outs = [torch.full((56 * (q["cap"] + 1),), jm.FILL, dtype=torch.uint8, device=dev) for q in jobs]
    ress = [torch.full((184,), jm.FILL, dtype=torch.uint8, device=dev) for _ in jobs]
    dk, dv = torch.from_numpy(keys).to(dev), torch.from_numpy(vals).to(dev)
    for q, o, r in zip(jobs, outs, ress):
        if q["kind"] == "map":
            e.where_map_group_dev(FB, outer, FL, dk, dv, len(keys), o, r, measure=q["measure"], cap=q["cap"])
        else:
            e.where_join_group_dev(FB, outer, FL, FI, inner, FK, FA, o, r, measure=q["measure"], cap=q["cap"], map_cap=q["map_cap"])
    e.sync()
    flags = []
    for q, o, r in zip(jobs, outs, ress):
        want = jm.want_of(m, q)
        res = r.cpu().numpy().view(jm.JOIN_RES_DTYPE)[0]
        bad = jm.check(o.cpu().numpy().view(jm.GROUP_DTYPE), res, *want, q["cap"], jm.map_cap_of(q), host=False)
        assert bad is None, (q, bad, want[1])
        flags.append(int(res["flags"]))
    assert flags == [0, 0, jm.MAP_OVERFLOW, 0, jm.GROUP_OVERFLOW]
    assert (dk.cpu().numpy() == keys).all() and (dv.cpu().numpy() == vals).all()
    jm.ask(e, m, base)                                     # the scratch is clean behind the overflows: host mode right after


# ---- 4. the group table and the key table are shared with, or next to, older queries ----
def test_interleaved_with_where_group_and_semijoin(seeded):
    e, m = seeded
    q = Q(FB, [[(FB, 0, 60)]], FL, FI, [[(FI, 10, 150)]], FK, FA, FM, cap=512, map_cap=1024)
    outer, inner = q["clauses"], q["inner_clauses"]
    pn = sm.pos_nodes(e, m, FB)

    def older():
        gm.ask(e, m, FB, outer, F1, FM, cap=64)
        gm.ask(e, m, FB, outer, FL, None, cap=4)                      # where_group overflows
        sm.ask_semijoin(e, m, FB, outer, FL, FI, inner, FK, False, set_cap=1024, pn=pn)
        sm.ask_semijoin(e, m, FB, outer, FL, FI, inner, FK, True, cap=10, set_cap=4, pn=pn)   # the semi-join overflows

    older()
    for small in (q, dict(q, cap=2), dict(q, map_cap=4), dict(q, cap=2, map_cap=4), q):
        jm.ask(e, m, small)
        older()
    jm.ask(e, m, q)


# ---- 5. map sizes: a smaller map_cap behind a larger one ----
def test_a_smaller_map_cap_uses_the_head_of_a_larger_clean_table():
    n = 6000
    m = jm.Model(wam.node_ids(n, 76000))
    i = np.arange(n)
    m.set(FB, i, i % 100); m.set(FI, i, i); m.set(FK, i[:5000], jm.uid(i[:5000])); m.set(FK, i[5000:], jm.uid(i[5000:] % 7)); m.set(FL, i, jm.uid((i * 7) % 5500))
    m.set(FA, i, (i * 13) % 40 - 20); m.set(FM, i, i - 3000)
    with _engine(m, {}) as e:
        for map_cap, hi in ((8192, 4999), (8, 5006), (8, 5008), (4999, 4999), (5000, 4999), (1 << 17, 5999), (64, 40), (7, 5999)):
            for cap in (64, 8):
                _, res = jm.ask(e, m, Q(FB, EVERY, FL, FI, [[(FI, 5000 if map_cap == 8 else 0, hi)]], FK, FA, FM, cap=cap, map_cap=map_cap))
                assert bool(int(res["flags"]) & jm.MAP_OVERFLOW) == (map_cap in (4999, 7))
        _, res = jm.ask(e, m, QMAP(FB, EVERY, FL, jm.uid(np.arange(3000)), np.arange(3000) % 9, FM, cap=16))
        assert int(res["map_size"]) == 3000 and int(res["n_groups"]) == 9


# ---- 6. a living table ----
def test_a_living_table():
    """after a merge that moves keys, attributes and links and creates nodes, after a growth, with tombstones, with a value-ordered view on the base fields (left
    as it was), behind a deferred compaction, and after both indexes have switched to their int64 columns"""
    rng = np.random.default_rng(79)
    m, tombs = jm.seeded_model()
    N = m.N
    progs = [Q(FB, [[(FB, 10, 70)]], FL, FI, [[(FI, 20, 120)]], FK, FA, FM, 512, 2048),
             Q(FB, [[(F1, 0, 4), (FB, 0, 50)], [(F2, 9, 9)]], FL, FI, [[(FI, 0, 199), (F1, 3, 9)]], FK, FA, None, 512, 2048),
             Q(FB, EVERY, FB, FI, [[(FI, 0, 60)]], FI, FA, FB, 512, 2048)]
    dev = torch.device("cuda", 0)

    def ask(e):
        out = []
        for q in progs:
            recs, res = jm.ask(e, m, q)
            assert not int(res["flags"])
            out.append(recs.tobytes() + res.tobytes())
        return out

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.asarray(vals, np.int64), want_flags=False)
        m.set(f, idx, vals)

    with _engine(m, tombs, cap=8 * N) as e:
        first = ask(e)
        live = np.nonzero(m.st[FB] == jm.DATA)[0]
        idx = live[::3]; merge(e, FL, idx, jm.uid(rng.integers(0, 1000, len(idx))), 100)                 # links move, and appear where there was none
        idx = np.nonzero(m.st[FI] == jm.DATA)[0][::2]; merge(e, FK, idx, jm.uid(rng.integers(700, 1000, len(idx))), 100)   # keys move into the dangling range
        idx = np.nonzero(m.st[FI] == jm.DATA)[0][1::3]; merge(e, FA, idx, rng.integers(-50, 50, len(idx)), 100)             # attributes move
        idx = live[1::5]; merge(e, FB, idx, rng.integers(0, 100, len(idx)), 100)
        second = ask(e)
        assert all(a != b for a, b in zip(first, second))
        e.reserve(32 * N)                                                                               # growth
        assert ask(e) == second
        wam.tombstone(e, m, FL, np.nonzero(m.st[FL] == jm.DATA)[0][::9], ts=200)
        wam.tombstone(e, m, FK, np.nonzero(m.st[FK] == jm.DATA)[0][::7], ts=200)
        wam.tombstone(e, m, FA, np.nonzero(m.st[FA] == jm.DATA)[0][::5], ts=200)
        wam.tombstone(e, m, FI, np.nonzero(m.st[FI] == jm.DATA)[0][5::40], ts=200)
        third = ask(e)
        assert third != second
        # value-ordered views on both base fields: the same answers, and the views' counters untouched
        for f in (FB, FI):
            e.index_set_ordered(f, 1)
            e.scan_range(f, 2, 9)
            assert e.index_ordered_info(f)[1], "the view answers"
        s0 = [e.index_ordered_stats(f) for f in (FB, FI)]
        assert ask(e) == third
        assert [e.index_ordered_stats(f) for f in (FB, FI)] == s0 and all(e.index_ordered_info(f)[1] for f in (FB, FI)), "the calls leave the views as they were"
        for f in (FB, FI):
            e.index_set_ordered(f, 0)
        # deferred compaction (switched on explicitly): a device batch large enough to defer, asked right behind it
        e.set_deferred(True)
        nb = 65_536
        fields = np.array([FB, FL, FI, FK, F1, F2, FA, FM], np.uint32)                                   # 8 x N distinct (node, field) keys >= nb
        keys = rng.permutation(len(fields) * N)[:nb]
        kn, kf = keys % N, fields[keys // N]
        kv = np.where(kf == FB, rng.integers(0, 100, nb), np.where(kf == FI, rng.integers(0, 200, nb), np.where((kf == FL) | (kf == FK), jm.uid(rng.integers(0, 1000, nb)), rng.integers(0, 10, nb)))).astype(np.int64)
        cols = (torch.from_numpy(m.ids[kn].view(np.int64)).to(dev), torch.from_numpy(kf.view(np.int32)).to(dev),
                torch.full((nb,), 300, dtype=torch.int64, device=dev), torch.from_numpy(kv).to(dev))
        applied = torch.zeros(nb, dtype=torch.int32, device=dev); n_applied = torch.zeros(1, dtype=torch.int64, device=dev)
        d0 = e.deferred_counts()[0]
        e.merge_batch_dev(nb, *cols, bmx.INSERT_REFERENCE, applied=applied, n_applied=n_applied)
        for f in fields:
            m.set(int(f), kn[kf == f], kv[kf == f])
        jm.ask(e, m, progs[0])
        assert e.deferred_counts()[0] == d0 + 1 and int(n_applied.item()) == nb
        ask(e)
        # base values beyond int32 on either side: each index switches to its int64 column
        merge(e, FI, [7], [jm.WIDE], 2000)
        ask(e)
        merge(e, FB, [9, 11], [jm.WIDE, -(2**35)], 2000)
        ask(e)
        recs, res = jm.ask(e, m, Q(FB, [[(FB, 2**39, jm.INT64_MAX)]], FB, FI, [[(FI, 2**39, jm.INT64_MAX)]], FI, FI, FB))
        assert (len(recs), int(recs[0]["key"]), int(res["map_size"]), int(res["n_inner"]), int(res["total"]["n_match"])) == (1, jm.WIDE, 1, 1, 1)
