"""GPU: group-by over several fields (include/bmx_group_multi.h bmx_where_group_multi). Every answer is compared exactly with mgroup_model.answer — the tuples
through Python dicts, the sums as Python ints, // for the buckets, over the rows the test itself loaded: the tuple set, all 80 bytes of every record, absent,
total, n_groups, flags, the lexicographic order in host mode, the fill pattern behind the last record and, on overflow, in the whole buffer.

The shapes are the smallest at which each piece can go wrong (csrc/mgroup_kernels.h): a dictionary and the tuple table have max(64, next power of two >=
2 * cap) slots, the packed word gives each key log2 slots bits, one round of a workgroup is 8192 int32 rows or 4096 int64 rows. A base value >= 2^31 forces the
int64 column."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import group_model as gm
import mgroup_model as mm
import where_agg_model as wam
from where_agg_model import DATA, Model

F = gm._names()
FB, F1, F2, F3, FM, FK, NOBODY = F["base"], F["one"], F["two"], F["three"], F["measure"], F["key"], F["nobody"]
ALL_FIELDS = [FB, F1, F2, F3, F["four"], F["five"], FM, FK] + F["more"]
EVERY = [[(NOBODY, 0, 0, True)]]            # a negated literal on a field nobody has: true for every candidate
BIG, WIDE = mm.BIG, mm.WIDE


def _engine(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    return e


@pytest.fixture(scope="module")
def seeded():
    """the seeded tables (narrow, wide) with their tombstones applied, built once and left unchanged -> {wide: (model, {field: tombstoned nodes})}"""
    out = {}
    for wide in (False, True):
        m, tombs = gm.seeded_model(wide)
        gm.apply_tombs(m, tombs)
        out[wide] = (m, tombs)
    return out


def _load_seeded(e, m, tombs):
    """the model's data rows, then its tombstones as rows of their own"""
    wam.load(e, m, ALL_FIELDS)
    for f, idx in tombs.items():
        e.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), wam.VAL_DELETED, np.int64))


# ---- 1. one identity key is bmx_where_group ----
@pytest.mark.parametrize("wide", [False, True])
def test_one_identity_key_equals_where_group(seeded, wide):
    m, tombs = seeded[wide]
    with bmx.Engine(16 * m.N) as e:
        _load_seeded(e, m, tombs)
        seen = 0
        for p, group, measure in gm.seeded_queries()[::5]:
            for cap in (512, 3):
                one, r1 = gm.raw_group(e, FB, p, group, measure, cap)
                many, rm = mm.raw_mgroup(e, FB, p, [group], measure, cap)
                assert rm.tobytes() == r1.tobytes(), "the result record, byte for byte"
                assert np.array_equal(many["key"][:, 0], one["key"]) and many["agg"].tobytes() == one["agg"].tobytes(), "key[0] = key, the same 48 bytes"
                d = 0 if int(r1["flags"]) else int(r1["n_groups"])
                assert (many["key"][:d, 1:] == 0).all() and (many[d:].view(np.uint8) == mm.FILL).all()
                seen += d >= 2
        assert seen >= 6


# ---- 2. the three cell states over two keys, x the measure ----
@pytest.mark.parametrize("wide", [False, True])
def test_truth_table_of_two_keys(wide):
    n = 9 * 40
    i = np.arange(n)
    m = Model(wam.node_ids(n, 300 + wide))
    m.set(FB, i, i % 6 + (WIDE if wide else 0))
    a, b = i % 3, (i // 3) % 3                                   # 0: absent, 1: data, 2: data, then tombstoned
    m.set(F1, i[a > 0], (i[a > 0] // 9) % 4 - 1)
    m.set(F2, i[b > 0], (i[b > 0] // 9) % 3 * 1000)
    m.set(FM, i[i % 4 != 1], 5 * i[i % 4 != 1] - 700)
    with _engine(m, (FB, F1, F2, FM)) as e:
        wam.tombstone(e, m, F1, i[a == 2]); wam.tombstone(e, m, F2, i[b == 2]); wam.tombstone(e, m, FM, i[i % 8 == 3])
        for measure in (None, FB, FM):
            recs, res = mm.ask(e, m, FB, EVERY, [F1, F2], measure, 64)
            assert int(res["total"]["n_match"]) == n and int(res["absent"]["n_match"]) == n - n // 9, "only the (data, data) cell of the table lands in a record"
            assert len(recs) == 12
            recs, res = mm.ask(e, m, FB, [[(F1, 0, 5)], [(F2, 0, 0, True)]], [F2, F1, FB], measure, 64)
            assert int(res["absent"]["n_match"]) > 0 and len(recs) >= 2


# ---- 3. where a key comes from ----
@pytest.mark.parametrize("wide", [False, True])
def test_keys_from_the_column_a_program_field_and_an_unnamed_field(wide):
    n = 700
    i = np.arange(n)
    m = Model(wam.node_ids(n, 310 + wide))
    m.set(FB, i, (i % 9) * 7 - 20 + (WIDE if wide else 0))
    m.set(F1, i[i % 5 != 0], i[i % 5 != 0] % 4)
    m.set(FK, i[i % 7 != 0], (i[i % 7 != 0] % 6) * (BIG // 5) - BIG)
    m.set(FM, i, i - 350)
    prog = [[(F1, 1, 3), (FB, -20 + (WIDE if wide else 0), 22 + (WIDE if wide else 0))], [(F1, 0, 0)]]
    with _engine(m, (FB, F1, FK, FM)) as e:
        for keys in ([FB, F1], [F1, FB], [FK, FB], [FB, FK, F1], [FK], [F1], [FB], [FB, FB], [FK, F1, FB, FM]):
            for measure in (None, FM, FB):
                recs, res = mm.ask(e, m, FB, prog, keys, measure, 512)
                assert len(recs) >= 2
        g = e.where_group_multi(FB, prog, [F1, FB], FM, cap=512)
        assert list(g.groups) == sorted(g.groups) and all(len(t) == 2 for t in g.groups) and g.n_groups == len(g.groups) and not g.overflow


# ---- 4. tuples that differ in exactly one position ----
@pytest.mark.parametrize("nk", [2, 3, 4])
def test_tuples_that_differ_in_one_position(nk):
    fields = [F1, F2, F3, FK][:nk]
    tuples = [tuple([7] * nk)] + [tuple(7 if j != d else v for j in range(nk)) for d in range(nk) for v in (8, -7, 7 + 2**32, BIG)]
    n = 6 * len(tuples)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 320 + nk))
    m.set(FB, i, i % 11)
    for j, f in enumerate(fields):
        m.set(f, i, np.array([t[j] for t in tuples], np.int64)[i % len(tuples)])
    with _engine(m, [FB] + fields) as e:
        recs, res = mm.ask(e, m, FB, EVERY, fields, FB, 64)
        assert len(recs) == len(tuples) and (recs["agg"]["n_match"] == 6).all()
        assert sorted(tuple(int(v) for v in r["key"][:nk]) for r in recs) == sorted(tuples)


# ---- 5. buckets ----
def test_buckets():
    vals = np.array([-21, -20, -19, -11, -10, -1, 0, 1, 9, 10, 19, 20, BIG, -BIG, BIG - 1, 1 - BIG, 2**31, -(2**31) - 1], np.int64)
    n = 4 * len(vals)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 330))
    m.set(FB, i, i % 5)
    m.set(FK, i, vals[i % len(vals)])
    m.set(FM, i, 3 * i - 50)
    with _engine(m, (FB, FK, FM)) as e:
        for keys in ([(FK, 0, 10)],                                  # negative differences that are and are not multiples of the width
                     [(FK, 5, 10)], [(FK, -20, 10)],
                     [(FK, 7, 1)], [(FK, -BIG, 1)], [(FK, BIG, 1)],   # width 1 with an origin: no division
                     [(FK, 0, BIG)], [(FK, 1, BIG)], [(FK, -1, BIG)],  # the widest bucket
                     [(FK, BIG, BIG)], [(FK, -BIG, BIG)],              # +-(2^53 - 1) with the opposite origin
                     [(FK, BIG, 2)], [(FK, -BIG, 3)],
                     [(FK, 0, 10), (FK, 0, 100)],                      # one field at two widths
                     [(FK, 0, 1), (FK, -3, 7), FB, (FB, 1, 2)]):
            recs, res = mm.ask(e, m, FB, EVERY, keys, FM, 256)
            assert int(res["absent"]["n_match"]) == 0 and int(res["total"]["n_match"]) == n
        g = e.where_group_multi(FB, EVERY, [(FK, 0, 10)], cap=64)
        assert g.groups[(-3,)].n_match == 4 and g.groups[(-2,)].n_match == 12 and g.groups[(-1,)].n_match == 8, "floor, not truncation: -21 | -20 -19 -11 | -10 -1"
        assert g.groups[(0,)].n_match == 12 and (2**31 // 10,) in g.groups


# ---- 6. overflow ----
def test_overflow_by_tuples_where_no_field_overflows():
    """8 x 8 values: 64 tuples, each dictionary holds 8. cap 64 fits, cap 63 does not; an exact query right behind the overflow"""
    n = 64 * 3
    i = np.arange(n)
    m = Model(wam.node_ids(n, 340))
    m.set(FB, i, (i % 8) * 5 - 9)
    m.set(FK, i, ((i // 8) % 8) * (BIG // 9) - BIG // 2)
    m.set(FM, i, i)
    with _engine(m, (FB, FK, FM)) as e:
        for cap, over in ((64, 0), (63, 1), (64, 0), (33, 1), (32, 1), (1, 1), (65, 0)):
            recs, res = mm.ask(e, m, FB, EVERY, [FB, FK], FM, cap)
            assert int(res["flags"]) == over and (over or len(recs) == 64)
            recs, res = mm.ask(e, m, FB, [[(FB, -9, 1)]], [FK, FB], FM, cap if cap > 24 else 24)       # 3 x 8 tuples: exact right behind it
            assert len(recs) == 24 and int(res["flags"]) == 0


@pytest.mark.parametrize("which", [0, 1, 2])
def test_overflow_of_one_dictionary(which):
    """cap 8: 64 slots per dictionary. Key `which` of three has 70 values (more than its dictionary has slots), the others one each: that dictionary finds no
    room. And 40 values: room in the dictionary, but more tuples than cap."""
    n = 70 * 4
    i = np.arange(n)
    fields = [F1, F2, FK]
    m = Model(wam.node_ids(n, 350 + which))
    m.set(FB, i, i % 70)
    for j, f in enumerate(fields):
        m.set(f, i, (i % 70) * 1000003 - 10**7 if j == which else np.full(n, j - 1))
    m.set(FM, i, 2 * i)
    with _engine(m, [FB, FM] + fields) as e:
        for hi, over in ((69, 1), (7, 0), (39, 1), (8, 1), (7, 0)):
            recs, res = mm.ask(e, m, FB, [[(FB, 0, hi)]], fields, FM, 8)
            assert int(res["flags"]) == over and int(res["total"]["n_match"]) == 4 * (hi + 1)
            assert over or len(recs) == hi + 1
        recs, _ = mm.ask(e, m, FB, EVERY, fields, FM, 70)
        assert len(recs) == 70


def test_five_queries_in_a_row_with_disjoint_values():
    """cap - 2 values per query, disjoint between the queries: dictionaries that are not emptied behind a query would find no room by the third"""
    cap, n = 32, 5 * 30 * 3
    i = np.arange(n)
    m = Model(wam.node_ids(n, 360))
    q = i // 90
    m.set(FB, i, q)
    m.set(FK, i, 10**6 * q + (i % 30) * 7919)
    m.set(F1, i, (i % 30) - 1000 * q)
    with _engine(m, (FB, FK, F1)) as e:
        for k in range(5):
            recs, res = mm.ask(e, m, FB, [[(FB, k, k)]], [FK, F1], FB, cap)
            assert len(recs) == cap - 2 and int(res["flags"]) == 0
        for k in range(5):
            recs, res = mm.ask(e, m, FB, [[(FB, k, k)]], [(FK, 0, 1), (F1, 5, 1), (FK, -1, 1)], None, cap)
            assert len(recs) == cap - 2


# ---- 7. the top bits of the packed word ----
@pytest.mark.parametrize("nk,cap", [(4, 1 << 14), (3, 1 << 20)])
def test_codes_in_the_top_slots_of_the_largest_tables(nk, cap):
    """the largest cap of a 4-key and of a 3-key call: values chosen, from the model's home(), so that every key's code is one of the two top slots of its
    dictionary — the top bits of every field of the packed word (60 and 63 bits) are used"""
    slots = gm.slots_for(cap)
    assert nk * mm.shift_for(cap) == (60 if nk == 4 else 63)
    v = np.arange(1, 1 << 24, dtype=np.int64)
    h = gm.mix_np(v) & np.uint64(slots - 1)
    top = [int(v[np.nonzero(h == np.uint64(slots - 1 - k))[0][0]]) for k in (0, 1)]
    assert [gm.home(t, slots) for t in top] == [slots - 1, slots - 2]
    fields = [F1, F2, F3, FK][:nk]
    n = 3 << nk
    i = np.arange(n)
    m = Model(wam.node_ids(n, 370 + nk))
    m.set(FB, i, i % 3)
    for j, f in enumerate(fields):
        m.set(f, i, np.array(top, np.int64)[(i >> j) & 1])
    m.set(FM, i, i * i - 9)
    with _engine(m, [FB, FM] + fields) as e:
        recs, res = mm.ask(e, m, FB, EVERY, fields, FM, cap)
        assert len(recs) == 1 << nk and (recs["agg"]["n_match"] == 3).all()
        recs, res = mm.ask(e, m, FB, [[(FB, 1, 2)]], fields, None, 7)
        assert int(res["flags"]) == bmx.GROUP_OVERFLOW
        recs, res = mm.ask(e, m, FB, [[(FB, 1, 2)]], fields, None, 64)
        assert len(recs) == 1 << nk


# ---- 8. device memory ----
def test_device_memory_back_to_back(seeded):
    """device mode into poisoned buffers: four queries enqueued back to back (deep, overflowing, empty selection, bucketed) with one synchronisation at the end;
    the answers equal host mode as sets of whole records"""
    m, tombs = seeded[False]
    qs = mm.seeded_queries()
    deep = max((q[0] for q in qs), key=lambda p: int(m.mask(FB, p).sum()))
    queries = [(deep, [FK, F1], FM, 4096), (deep, [FK, F1], FM, 4), ([[(FB, 5000, 6000)]], [FK, FB], FM, 16), (qs[2][0], [FB, (FM, 0, 1 << 36)], None, 4096)]
    dev = torch.device("cuda", 0)
    with bmx.Engine(16 * m.N) as e:
        _load_seeded(e, m, tombs)
        host = [mm.ask(e, m, FB, p, ks, me, cap) for p, ks, me, cap in queries]
        assert len(host[0][0]) >= 2 and int(host[1][1]["flags"]) == 1 and int(host[2][1]["total"]["n_match"]) == 0 and len(host[3][0]) >= 2
        outs = [torch.full((10 * (cap + 1),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev) for _, _, _, cap in queries]
        ress = [torch.full((14,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev) for _ in queries]
        for (p, ks, me, cap), o, r in zip(queries, outs, ress):
            e.where_group_multi_dev(FB, p, ks, o, r, measure=me, cap=cap)
        e.sync()
        for (p, ks, me, cap), o, r, h in zip(queries, outs, ress, host):
            res = r.cpu().numpy().view(mm.GROUP_RES_DTYPE)[0]
            recs = o.cpu().numpy().view(mm.MGROUP_DTYPE)
            bad = mm.check(recs, res, *mm.answer(m, FB, p, ks, me, cap), cap, host=False)
            assert bad is None, bad
            d = 0 if int(res["flags"]) else int(res["n_groups"])
            assert {x.tobytes() for x in recs[:d]} == {x.tobytes() for x in h[0]}, "the same set of whole records as in host mode"
            assert res.tobytes()[16:] == h[1].tobytes()[16:] and int(res["flags"]) == int(h[1]["flags"])


# ---- 9. the neighbours' scratch ----
def test_interleaved_with_where_group_and_where_join_group(seeded):
    """bmx_where_group and bmx_where_join_group keep their own tables: their answers before, between and behind calls of the new one are the same bytes"""
    m, tombs = seeded[False]
    qs = mm.seeded_queries()
    p = max((q[0] for q in qs), key=lambda p: int(m.mask(FB, p).sum()))
    with bmx.Engine(16 * m.N) as e:
        _load_seeded(e, m, tombs)

        def neighbours():
            a = gm.raw_group(e, FB, p, FK, FM, 512)
            j = e.where_join_group(FB, p, F1, FB, EVERY, F1, F2, measure=FM, cap=64, map_cap=64)
            return a[0].tobytes() + a[1].tobytes() + j.records.tobytes() + bytes([j.flags])

        first = neighbours()
        assert gm.check(*gm.raw_group(e, FB, p, FK, FM, 512), *gm.answer(m, FB, p, FK, FM, 512), 512) is None
        for keys, cap in (([FK, F1], 4096), ([FK, F1], 4), ([FB, (FM, 0, 1 << 36), F2], 4096)):
            mm.ask(e, m, FB, p, keys, FM, cap)
            assert neighbours() == first
            mm.ask(e, m, FB, p, keys, FM, cap)


# ---- 10. seeded programs ----
@pytest.mark.parametrize("wide", [False, True])
def test_seeded_programs(seeded, wide):
    """the 60 programs x key sets of mgroup_model.seeded_queries (test_mgroup_model.py asserts that they select tuples, absent rows and buckets), each with room
    for every tuple and every fourth also with cap = 4 directly in front of it: an overflowing query leaves the state clean for the next"""
    m, tombs = seeded[wide]
    with bmx.Engine(16 * m.N) as e:
        _load_seeded(e, m, tombs)
        assert e.index_size(FB) == m.N
        groups = overflows = 0
        for k, (p, keys, measure) in enumerate(mm.seeded_queries()):
            want = mm.answer(m, FB, p, keys, measure, 1 << 14)
            if k % 4 == 2:
                _, res = mm.ask(e, m, FB, p, keys, measure, cap=4)
                overflows += int(res["flags"])
            recs, res = mm.ask(e, m, FB, p, keys, measure, cap=1 << 14, want=want)
            assert int(res["total"]["n_match"]) == e.scan_where(FB, p, count_only=True), (k, p)
            assert int(res["flags"]) == 0
            groups += len(recs) >= 2
        assert groups >= 30 and overflows >= 5


# ---- 11. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(78)
    N0, EXTRA = 8192 + 5, 300
    m = Model(wam.node_ids(N0 + EXTRA, 9950))
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
            out += [mm.ask(e, m, FB, p, [FK, F1], FM, 512)[0], mm.ask(e, m, FB, p, [FB, (FK, -BIG, 1 << 50)], FK, 512)[0], mm.ask(e, m, FB, p, [F1, FB, FM], None, 512)[0]]
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
        # a merge that changes key values, base rows, and creates rows
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
        # tombstones on key, measure and base rows
        wam.tombstone(e, m, FK, np.nonzero(m.st[FK] == DATA)[0][::9], ts=200)
        wam.tombstone(e, m, FM, np.nonzero(m.st[FM] == DATA)[0][::7], ts=200)
        wam.tombstone(e, m, FB, np.concatenate([old[5::40], new[1::7]]), ts=200)
        third = ask(e)
        assert not same(third, second)
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
        fields = np.array([FB, F1, FK, FM, F2, F3, F["four"], F["five"]], np.uint32)      # 8 x N0 distinct (node, field) keys >= nb
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
        mm.ask(e, m, FB, progs[1], [FK, F1], FM, 512)
        assert e.deferred_counts()[0] == d0 + 1 and int(n_applied.item()) == nb
        ask(e)
        # a base value beyond int32: the index switches to its int64 column
        merge(e, FB, [7, N0 + 3], np.array([WIDE, -(2**35)]), 2000)
        ask(e)
        recs, _ = mm.ask(e, m, FB, [[(FB, 2**39, wam.I64MAX)], [(FB, wam.I64MIN, -(2**33))]], [(FB, 0, 1 << 30), FB], FB, 8)
        assert recs["key"][:, :2].tolist() == [[-(2**35) >> 30, -(2**35)], [WIDE >> 30, WIDE]]
