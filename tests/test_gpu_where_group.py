"""GPU: group-by over discovered values (include/bmx_group.h bmx_where_group). Every answer is compared exactly with group_model.answer — numpy.unique over the
rows the test itself loaded: the key set, all 48 bytes of every record, absent, total, n_groups, flags, the sorted order in host mode, the fill pattern behind the
last record and, on overflow, in the whole buffer.

The shapes are the smallest at which each piece can go wrong (csrc/group_kernels.h): the LDS cache holds 1024 keys per workgroup (256 sets of 4 ways), the table
has max(64, next power of two >= 2 * cap) slots, one round of a workgroup is 8192 int32 rows or 4096 int64 rows. A base value >= 2^31 forces the int64 column."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import group_model as gm
import where_agg_model as wam
from where_agg_model import DATA, Model

F = gm._names()
FB, F1, F2, FM, FK, NOBODY = F["base"], F["one"], F["two"], F["measure"], F["key"], F["nobody"]
ALL_FIELDS = [FB, F1, F2, F["three"], F["four"], F["five"], FM, FK] + F["more"]
EVERY = [[(NOBODY, 0, 0, True)]]            # a negated literal on a field nobody has: true for every candidate
BIG, WIDE = gm.BIG, gm.WIDE


def _engine(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    return e


# ---- 1. seeded programs ----
@pytest.mark.parametrize("wide", [False, True])
def test_seeded_programs(wide):
    """the 60 programs of group_model.seeded_queries (test_group_model.py asserts that they select groups and absent rows), each with room for every key and
    every fourth also with cap = 4 directly in front of it: an overflowing query leaves the state clean for the next"""
    m, tombs = gm.seeded_model(wide)
    with bmx.Engine(16 * m.N) as e:
        wam.load(e, m, ALL_FIELDS)
        for f, idx in tombs.items():
            wam.tombstone(e, m, f, idx)
        assert e.index_size(FB) == m.N
        groups = overflows = 0
        for k, (p, group, measure) in enumerate(gm.seeded_queries()):
            if k % 4 == 2:
                _, res = gm.ask(e, m, FB, p, group, measure, cap=4)
                overflows += int(res["flags"])
            recs, res = gm.ask(e, m, FB, p, group, measure, cap=512)
            assert int(res["total"]["n_match"]) == e.scan_where(FB, p, count_only=True), (k, p)
            assert int(res["flags"]) == 0
            groups += len(recs) >= 2
        assert groups >= 30 and overflows >= 5


# ---- 2. cardinalities ----
@pytest.mark.parametrize("d", [1, 2, 64, gm.CACHE - 1, gm.CACHE, gm.CACHE + 1, 5000])
def test_cardinalities(d):
    """d distinct keys, sparse over both signs, grouped by a probed field and (as int32 values) by the base field itself; the measure is the other one"""
    n = max(2 * d + 7, 600)
    rng = np.random.default_rng(d)
    m = Model(wam.node_ids(n, 100 + d))
    small = (rng.permutation(d)[np.arange(n) % d] - d // 2) * 40009                     # |.| < 2^31: the base column stays narrow
    m.set(FB, np.arange(n), small)
    m.set(FK, np.arange(n), small.astype(np.int64) * 44000101 + 1)                      # the same partition over +-2^53
    cap = 8192 if d > 2048 else 2048
    with _engine(m, (FB, FK)) as e:
        for group, measure in ((FK, FB), (FB, FK), (FK, None)):
            recs, res = gm.ask(e, m, FB, EVERY, group, measure, cap)
            assert len(recs) == d and int(res["absent"]["n_match"]) == 0 and int(res["total"]["n_match"]) == n
        half = [[(FB, 0, 2**31)]]
        recs, _ = gm.ask(e, m, FB, half, FK, FB, cap)
        assert len(recs) == d - d // 2


# ---- 3. the key values ----
@pytest.mark.parametrize("wide", [False, True])
def test_key_values(wide):
    keys = np.array([0, 1, -1, BIG, -BIG, 2**31, -(2**31), 2**32, -(2**32) - 1, 5, -5, 2**52], np.int64)
    n = 5 * len(keys)
    m = Model(wam.node_ids(n, 7000))
    if wide:
        m.set(FB, np.arange(n), keys[np.arange(n) % len(keys)])                         # the keys are the base column: int64
    else:
        m.set(FB, np.arange(n), np.arange(n))
    m.set(FK, np.arange(n), keys[np.arange(n) % len(keys)])
    m.set(FM, np.arange(n), keys[(np.arange(n) * 5 + 1) % len(keys)])
    with _engine(m, (FB, FK, FM)) as e:
        for group in (FK, FB):
            for measure in (None, FM, FK):
                recs, res = gm.ask(e, m, FB, EVERY, group, measure, 64)
                assert len(recs) == (len(keys) if group == FK or wide else n)
        recs, _ = gm.ask(e, m, FB, [[(FK, -BIG, -1)]], FK, FM, 8)
        assert recs["key"].tolist() == sorted(int(k) for k in keys if k < 0), "negative keys sort in front"
        recs, _ = gm.ask(e, m, FB, [[(FK, 1, BIG)]], FK, FM, 8)
        assert (recs["key"] > 0).all()


# ---- 4. absence ----
def test_absent_groups_and_measures():
    n = 700
    m = Model(wam.node_ids(n, 7700))
    m.set(FB, np.arange(n), np.arange(n) % 9)
    m.set(FK, np.arange(0, n, 2), np.arange(0, n, 2) % 5)
    m.set(FM, np.arange(0, n, 3), np.arange(0, n, 3) - 300)
    with _engine(m, (FB, FK, FM)) as e:
        wam.tombstone(e, m, FM, np.arange(0, n, 6)); wam.tombstone(e, m, FK, np.arange(0, n, 8))
        # a group field nobody has, and one that is tombstoned wherever it exists: every selected node is absent
        for p in (EVERY, [[(FB, 2, 5)]]):
            recs, res = gm.ask(e, m, FB, p, NOBODY, FM, 8)
            assert int(res["n_groups"]) == 0 and res["absent"].tobytes() == res["total"].tobytes() and int(res["total"]["n_match"]) > 0
        recs, res = gm.ask(e, m, FB, EVERY, FK, FM, 8)
        assert 0 < int(res["total"]["n"]) < int(res["total"]["n_match"]) and 0 < int(res["absent"]["n"]) < int(res["absent"]["n_match"])
        assert all(int(r["agg"]["n"]) < int(r["agg"]["n_match"]) for r in recs), "measure rows absent and tombstoned: n < n_match"
        recs, res = gm.ask(e, m, FB, EVERY, FK, NOBODY, 8)
        assert int(res["total"]["n"]) == 0 and int(res["total"]["min"]) == wam.I64MAX
        # nothing selected
        recs, res = gm.ask(e, m, FB, [[(FB, 100, 200)]], FK, FM, 8)
        assert int(res["n_groups"]) == 0 and int(res["total"]["n_match"]) == 0
        wam.tombstone(e, m, FK, np.nonzero(m.st[FK] == DATA)[0])
        recs, res = gm.ask(e, m, FB, EVERY, FK, FM, 8)
        assert int(res["n_groups"]) == 0 and res["absent"].tobytes() == res["total"].tobytes()


# ---- 5. overflow ----
@pytest.mark.parametrize("cap", [8, 1024])
def test_overflow(cap):
    """D = cap, cap + 1, slots and slots + 1 distinct keys: the flag, n_groups above cap, the buffer untouched, absent and total exact — and the very next query
    with enough room is exact, because the last kernel cleaned the state"""
    slots = gm.slots_for(cap)
    assert slots == (64 if cap == 8 else 2048)
    n = 2 * (slots + 1) + 50
    m = Model(wam.node_ids(n, 5000 + cap))
    m.set(FB, np.arange(n), np.arange(n))
    m.set(FK, np.arange(0, n - 50), (np.arange(n - 50) // 2) * 1000003 - 10**9)         # key j on rows 2j, 2j + 1; the last 50 rows have none
    m.set(FM, np.arange(n), 7 * np.arange(n) - 1000)
    with _engine(m, (FB, FK, FM)) as e:
        for d in (cap, cap + 1, slots, slots + 1, cap - 1):
            p = [[(FB, 0, 2 * d - 1)], [(FB, n - 50, n)]]                               # the first d keys and the rows without one
            recs, res = gm.ask(e, m, FB, p, FK, FM, cap)
            assert int(res["flags"]) == (bmx.GROUP_OVERFLOW if d > cap else 0) and int(res["absent"]["n_match"]) == 50, d
            recs, res = gm.ask(e, m, FB, p, FK, FM, slots + 1)                          # room for all of them (a larger table: scratch growth)
            assert len(recs) == d and int(res["flags"]) == 0
        g = e.where_group(FB, [[(FB, 0, 5)]], FK, FM, cap=cap)
        assert list(g.groups) == [-10**9, 1000003 - 10**9, 2000006 - 10**9] and g.groups[-10**9].n_match == 2 and not g.overflow
        assert e.where_group(FB, EVERY, FK, cap=cap).overflow


def test_a_larger_cap_after_a_smaller_one_and_back():
    n = 3000
    m = Model(wam.node_ids(n, 6100))
    m.set(FB, np.arange(n), np.arange(n) % 50)
    m.set(FK, np.arange(n), (np.arange(n) % 1500) * 99991 - 7 * 10**7)
    with _engine(m, (FB, FK)) as e:
        for cap in (8, 2000, 8, 70000, 1500, 1, 1499):
            recs, res = gm.ask(e, m, FB, EVERY, FK, FB, cap)
            assert (len(recs) == 1500) == (cap >= 1500)
            recs, _ = gm.ask(e, m, FB, [[(FB, 3, 3)]], FB, FK, cap)
            assert recs["key"].tolist() == [3]


# ---- 6. device memory ----
def test_device_memory_back_to_back():
    """device mode: the answers equal host mode as sets of whole records; three queries enqueued back to back (deep, overflowing, empty selection) with one
    synchronisation at the end"""
    n = 8192 + 700
    rng = np.random.default_rng(31)
    m = Model(wam.node_ids(n, 6600))
    m.set(FB, np.arange(n), rng.integers(0, 2000, n))
    idx = np.nonzero(rng.random(n) < 0.8)[0]; m.set(FK, idx, rng.integers(-BIG, BIG, 3000)[rng.integers(0, 3000, len(idx))])
    idx = np.nonzero(rng.random(n) < 0.6)[0]; m.set(FM, idx, rng.integers(-WIDE, WIDE, len(idx)))
    deep = [[(FB, 100, 1800)], [(FM, 0, WIDE, True), (FB, 0, 50)]]
    dev = torch.device("cuda", 0)
    queries = [(deep, FK, FM, 4096), (deep, FK, FM, 16), ([[(FB, 5000, 6000)]], FK, FM, 16), (deep, FB, None, 4096)]
    with _engine(m, (FB, FK, FM)) as e:
        wam.tombstone(e, m, FK, np.nonzero(m.st[FK] == DATA)[0][::10])
        host = [gm.ask(e, m, FB, p, g, me, cap) for p, g, me, cap in queries]
        assert len(host[0][0]) > gm.CACHE and int(host[1][1]["flags"]) == 1 and int(host[2][1]["total"]["n_match"]) == 0
        outs = [torch.full((7 * (cap + 1),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev) for _, _, _, cap in queries]
        ress = [torch.full((14,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev) for _ in queries]
        for (p, g, me, cap), o, r in zip(queries, outs, ress):
            e.where_group_dev(FB, p, g, o, r, measure=me, cap=cap)
        e.sync()
        for (p, g, me, cap), o, r, h in zip(queries, outs, ress, host):
            res = r.cpu().numpy().view(gm.GROUP_RES_DTYPE)[0]
            recs = o.cpu().numpy().view(gm.GROUP_DTYPE)
            assert gm.check(recs, res, *gm.answer(m, FB, p, g, me, cap), cap, host=False) is None, gm.check(recs, res, *gm.answer(m, FB, p, g, me, cap), cap, host=False)
            d = 0 if int(res["flags"]) else int(res["n_groups"])
            assert {x.tobytes() for x in recs[:d]} == {x.tobytes() for x in h[0]}, "the same set of whole records as in host mode"
            assert res.tobytes()[16:] == h[1].tobytes()[16:] and int(res["flags"]) == int(h[1]["flags"])


# ---- 7. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(77)
    N0, EXTRA = 8192 + 5, 300
    m = Model(wam.node_ids(N0 + EXTRA, 9900))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 12, N0))
    pool = rng.integers(-BIG, BIG, 40)
    for f, pr in ((F1, 0.9), (FK, 0.7), (FM, 0.8)):
        idx = old[rng.random(N0) < pr]
        m.set(f, idx, pool[rng.integers(0, 40, len(idx))] if f == FK else rng.integers(0, 6, len(idx)))
    progs = [[[(F1, 1, 3), (FB, 2, 9)]], [[(F1, 0, 1)], [(FM, 4, 5), (FB, 0, 5)]], [[(FB, 3, 3, True), (F1, 0, 5, True)], [(FB, 0, 1)]]]
    dev = torch.device("cuda", 0)

    def ask(e):
        out = []
        for p in progs:
            out += [gm.ask(e, m, FB, p, FK, FM, 64)[0], gm.ask(e, m, FB, p, FB, FK, 64)[0], gm.ask(e, m, FB, p, F1, None, 8)[0]]
        return out

    def same(a, b):
        return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), vals, want_flags=False)
        m.set(f, idx, vals)

    with _engine(m, (FB, F1, FK, FM), 8 * (N0 + EXTRA)) as e:
        first = ask(e)
        assert all(len(a) >= 2 for a in first)
        # a merge that changes group values, base rows, and creates rows
        idx = old[::3]; merge(e, FK, idx, pool[rng.integers(0, 40, len(idx))] + 1, 100)
        idx = old[1::5]; merge(e, FB, idx, rng.integers(0, 12, len(idx)), 100)
        new = np.arange(N0, N0 + EXTRA)
        merge(e, FB, new, rng.integers(0, 12, EXTRA), 101)
        merge(e, FK, new[::2], pool[rng.integers(0, 40, len(new[::2]))], 101)
        merge(e, F1, new, rng.integers(0, 6, EXTRA), 101)
        second = ask(e)
        assert e.index_size(FB) == N0 + EXTRA and not same(first, second)
        # growth
        e.reserve(32 * (N0 + EXTRA))
        assert same(ask(e), second)
        # tombstones on group, measure and base rows
        wam.tombstone(e, m, FK, np.nonzero(m.st[FK] == DATA)[0][::9], ts=200)
        wam.tombstone(e, m, FM, np.nonzero(m.st[FM] == DATA)[0][::7], ts=200)
        wam.tombstone(e, m, FB, np.concatenate([old[5::40], new[1::7]]), ts=200)
        third = ask(e)
        assert not same(third, second)
        # the index dropped and built again
        e.index_drop(FB)
        assert same(ask(e), third)
        # a value-ordered view on the base field: the same answers, and the view's counters untouched
        e.index_set_ordered(FB, 1)
        assert set(e.scan_range(FB, 2, 9).tolist()) == set(m.ids[m.mask(FB, [[(FB, 2, 9)]])].tolist())
        assert e.index_ordered_info(FB)[1], "the view answers"
        s0 = e.index_ordered_stats(FB)
        assert same(ask(e), third)
        assert e.index_ordered_stats(FB) == s0 and e.index_ordered_info(FB)[1], "the calls leave the view as it was"
        e.index_set_ordered(FB, 0)
        # deferred compaction (switched on explicitly): a device batch large enough to defer, asked right behind it
        e.set_deferred(True)
        nb = 65_536
        fields = np.array([FB, F1, FK, FM, F2, F["three"], F["four"], F["five"]], np.uint32)      # 8 x N0 distinct (node, field) keys >= nb
        keys = rng.permutation(len(fields) * N0)[:nb]
        kn, kf = keys % N0, fields[keys // N0]
        kv = np.where(kf == FB, rng.integers(0, 12, nb), np.where(kf == FK, pool[rng.integers(0, 40, nb)] - 1, rng.integers(0, 6, nb))).astype(np.int64)
        cols = (torch.from_numpy(m.ids[kn].view(np.int64)).to(dev), torch.from_numpy(kf.view(np.int32)).to(dev),
                torch.full((nb,), 300, dtype=torch.int64, device=dev), torch.from_numpy(kv).to(dev))
        applied = torch.zeros(nb, dtype=torch.int32, device=dev); n_applied = torch.zeros(1, dtype=torch.int64, device=dev)
        d0 = e.deferred_counts()[0]
        e.merge_batch_dev(nb, *cols, bmx.INSERT_REFERENCE, applied=applied, n_applied=n_applied)
        for f in fields:
            m.set(int(f), kn[kf == f], kv[kf == f])
        gm.ask(e, m, FB, progs[1], FK, FM, 256)
        assert e.deferred_counts()[0] == d0 + 1 and int(n_applied.item()) == nb
        ask(e)
        # a base value beyond int32: the index switches to its int64 column
        merge(e, FB, [7, N0 + 3], np.array([WIDE, -(2**35)]), 2000)
        ask(e)
        recs, _ = gm.ask(e, m, FB, [[(FB, 2**39, wam.I64MAX)], [(FB, wam.I64MIN, -(2**33))]], FB, FB, 8)
        assert recs["key"].tolist() == [-(2**35), WIDE]
