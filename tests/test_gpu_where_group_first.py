"""GPU: the first node per group (include/bmx_first.h bmx_where_group_first). Every answer is compared exactly with first_model.answer — a brute force through
Python dicts and ints over the rows the test itself loaded: every byte of every record and of res, every cell and clock, the sorted order in host mode, and the
fill pattern behind row D and, on overflow, in every buffer.

The shapes are small: the kernels' geometry (cache, walks, waves, workgroups, ragged units) is test_gpu_where_group_first_kernel_edges.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import first_model as fm
import group_model as gm
import where_agg_model as wam
from where_agg_model import DATA, Model

F = fm.names()
FB, FG, FO, FS, NOBODY, F1, F2, F3 = F["base"], F["group"], F["order"], F["select"], F["nobody"], F["one"], F["two"], F["three"]
EVERY = [[(NOBODY, 0, 0, True)]]
BIG, WIDE = fm.BIG, gm.WIDE
POISON = 0x5A5A5A5A5A5A5A5A


def _engine(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    return e


# ---- 1. the truth table of the two cells ----
@pytest.mark.parametrize("wide", [False, True])
def test_truth_table_of_group_and_order_cells(wide):
    """group cell x order cell in data / tombstone / absent, four nodes of each kind in two groups; a third group whose members all lack the order value"""
    n = 9 * 4 + 3
    j = np.arange(n)
    gs, os_ = j % 3, (j // 3) % 3                                   # 0 data, 1 tombstone, 2 absent
    gs[36:] = 0; os_[36:] = [1, 2, 2]
    m = Model(wam.node_ids(n, 91000 + wide))
    m.set(FB, j, j + (WIDE if wide else 0))
    m.set(FG, j[gs != 2], np.where(j >= 36, 99, 5 + (j // 18))[gs != 2])
    m.set(FO, j[os_ != 2], (100 - j)[os_ != 2])
    with _engine(m, (FB, FG, FO)) as e:
        wam.tombstone(e, m, FG, j[gs == 1]); wam.tombstone(e, m, FO, j[os_ == 1])
        for desc in (False, True):
            recs, vals, ts, res = fm.ask(e, m, FB, EVERY, FG, FO, (FG, FO, FB), desc, True, 8)
            assert recs["key"].tolist() == [5, 6, 99] and recs["n_match"].tolist() == [6, 6, 3] and recs["n"].tolist() == [2, 2, 0]
            assert int(res["absent"]) == 24 and int(res["total"]) == n and int(res["n_ordered"]) == 4
            assert int(recs[2]["id"]) == fm.NO_NODE and int(recs[2]["val"]) == fm.VAL_DELETED
            assert vals[:, 2].tolist() == [fm.VAL_DELETED] * 3 and ts[:, 2].tolist() == [-1] * 3, "a record without a node gets absent cells"
        # projecting cells in all three states from the winner
        wam.tombstone(e, m, F1, j[:1])                               # (a tombstone on a field the node never held)
        fm.ask(e, m, FB, EVERY, FG, FO, (F1, NOBODY, FO), False, True, 8)


# ---- 2. where the group and the order value come from ----
def test_group_and_order_from_column_program_and_unnamed_fields():
    n = 900
    rng = np.random.default_rng(5)
    m = Model(wam.node_ids(n, 92000))
    i = np.arange(n)
    m.set(FB, i, rng.integers(0, 12, n))
    for f, pr, top in ((F1, 0.8, 6), (F2, 0.7, 4), (FG, 0.8, 9), (FO, 0.7, 5)):
        idx = i[rng.random(n) < pr]
        m.set(f, idx, rng.integers(-2, top, len(idx)))
    prog = [[(F1, 0, 4), (FB, 1, 10)], [(F2, 3, 3)]]
    with _engine(m, (FB, F1, F2, FG, FO)) as e:
        wam.tombstone(e, m, FG, i[::13]); wam.tombstone(e, m, FO, i[::11]); wam.tombstone(e, m, F1, i[::17])
        for group in (FB, F1, FG):
            for order in (FB, F1, FO, F2, group):
                for desc in (False, True):
                    recs = fm.ask(e, m, FB, prog, group, order, (order, group), desc, False, 64)[0]
                    assert len(recs) >= 3
                    if order == group:
                        assert (recs["val"] == recs["key"]).all() and (recs["n"] == recs["n_match"]).all(), "every member ties: one representative per group"


def test_a_smaller_valued_node_that_the_program_rejects():
    m = Model(wam.node_ids(6, 93000))
    m.set(FB, np.arange(6), [1, 1, 1, 2, 2, 2])
    m.set(FG, np.arange(6), [7, 7, 7, 7, 7, 7])
    m.set(FO, np.arange(6), [50, 40, 60, 10, 70, 20])
    with _engine(m, (FB, FG, FO)) as e:
        recs = fm.ask(e, m, FB, [[(FB, 1, 1)]], FG, FO, (FO,), False, False, 8)[0]
        assert recs.tolist() == [(7, int(m.ids[1]), 40, 3, 3)]
        recs = fm.ask(e, m, FB, [[(FB, 1, 1)]], FG, FO, (FO,), True, False, 8)[0]
        assert recs.tolist() == [(7, int(m.ids[2]), 60, 3, 3)]
        recs = fm.ask(e, m, FB, [[(FO, 15, 65)]], FG, FO, (), False, False, 8)[0]
        assert recs.tolist() == [(7, int(m.ids[5]), 20, 4, 4)]


# ---- 3. ties, ids, values ----
@pytest.mark.parametrize("desc", [False, True])
def test_ties_on_the_extreme_are_decided_by_the_unsigned_id(desc):
    ids = np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 2, 12345], np.uint64)
    m = Model(ids)
    m.set(FB, np.arange(6), np.arange(6))
    m.set(FG, np.arange(6), np.full(6, -3))
    m.set(FO, np.arange(6), [4, 4, 4, 4, 4, -9 if desc else 9])     # the five tie on the extreme; the sixth is off it
    with _engine(m, (FB, FG, FO)) as e:
        for first in range(5):                                      # the tying nodes first .. 4 selected: the smallest id among them wins, ascending AND descending
            recs = fm.ask(e, m, FB, [[(FB, first, 5)]], FG, FO, (FB,), desc, True, 8)[0]
            assert recs.tolist() == [(-3, int(ids[first]), 4, 6 - first, 6 - first)]
        recs = fm.ask(e, m, FB, [[(FB, 3, 4)], [(FB, 0, 0)]], FG, FO, (), desc, False, 8)[0]
        assert int(recs[0]["id"]) == 0
        recs = fm.ask(e, m, FB, [[(FB, 3, 4)]], FG, FO, (), desc, False, 8)[0]
        assert int(recs[0]["id"]) == 2**63


@pytest.mark.parametrize("wide", [False, True])
def test_keys_and_order_values_at_the_ends_of_the_domain(wide):
    vals = np.array([0, 1, -1, BIG, -BIG], np.int64)
    n = 25
    i = np.arange(n)
    m = Model(wam.node_ids(n, 94000))
    m.set(FB, i, vals[i % 5] if wide else i)
    m.set(FG, i, vals[i % 5]); m.set(FO, i, vals[i // 5])
    with _engine(m, (FB, FG, FO)) as e:
        for desc in (False, True):
            recs = fm.ask(e, m, FB, EVERY, FG, FO, (FG, FO), desc, True, 8)[0]
            assert recs["key"].tolist() == [-BIG, -1, 0, 1, BIG] and (recs["val"] == (BIG if desc else -BIG)).all()
            recs = fm.ask(e, m, FB, EVERY, FO, FG, (), desc, False, 8)[0]
            assert (recs["val"] == (BIG if desc else -BIG)).all()
            if wide:
                recs = fm.ask(e, m, FB, EVERY, FB, FB, (FB,), desc, False, 8)[0]
                assert recs["key"].tolist() == [-BIG, -1, 0, 1, BIG] and (recs["n"] == 5).all()


# ---- 4. fit, overflow, fields ----
def test_cap_at_d_and_below_with_an_exact_query_right_behind():
    n = 500
    rng = np.random.default_rng(7)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 95000))
    m.set(FB, i, rng.integers(0, 12, n))
    m.set(FG, i, (i % 37) * 1000003 - 10**7)
    m.set(FO, i[i % 4 != 0], rng.integers(0, 6, n)[i % 4 != 0])
    with _engine(m, (FB, FG, FO)) as e:
        d = 37
        for cap in (d, d - 1, 1, d, 64, 2, 70000, d - 1, d):
            want = fm.ask(e, m, FB, EVERY, FG, FO, (FO, FB), cap % 2 == 0, True, cap)
            assert int(want[3]["flags"]) == (fm.OVERFLOW if cap < d else 0) and int(want[3]["total"]) == n and int(want[3]["n_ordered"]) == int((i % 4 != 0).sum())
        r = e.where_group_first(FB, [[(FG, -10**7, -10**7 + 2000006)]], FG, FO, fields=(FO,), cap=3)
        assert not r.overflow and r.n_groups == 3 and list(r.first) == [-10**7, 1000003 - 10**7, 2000006 - 10**7] and r.vals.shape == (1, 3) and r.ts is None
        assert e.where_group_first(FB, EVERY, FG, FO, cap=8).overflow


def test_zero_one_and_eight_fields_with_and_without_clocks():
    n = 300
    rng = np.random.default_rng(8)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 96000))
    m.set(FB, i, rng.integers(0, 12, n))
    m.set(FG, i[i % 7 != 0], (i % 5)[i % 7 != 0]); m.set(FO, i[i % 3 != 0], rng.integers(-4, 4, n)[i % 3 != 0]); m.set(F1, i[::2], i[::2] * 3)
    with _engine(m, (FB, FG, FO, F1)) as e:
        wam.tombstone(e, m, F1, i[::6])
        for fields in ((), (FO,), (FB, FG, FO, FO, F1, NOBODY, FB, F1)):
            for with_ts in (False, True):
                for desc in (False, True):
                    fm.ask(e, m, FB, [[(FB, 2, 11)]], FG, FO, fields, desc, with_ts, 8)
        r = e.where_group_first(FB, EVERY, FG, FO, fields=(FO, F1), with_ts=True, desc=True)
        assert r.vals.shape == (2, 5) == r.ts.shape and (r.vals[0] == r.records["val"]).all() and r.total == n


def test_device_mode_into_poisoned_buffers():
    n = 8192 + 300
    rng = np.random.default_rng(9)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 97000))
    m.set(FB, i, rng.integers(0, 2000, n))
    idx = i[rng.random(n) < 0.8]; m.set(FG, idx, rng.integers(-BIG, BIG, 1500)[rng.integers(0, 1500, len(idx))])
    idx = i[rng.random(n) < 0.6]; m.set(FO, idx, rng.integers(-3, 3, len(idx)))
    deep = [[(FB, 100, 1800)], [(FO, 0, 3, True), (FB, 0, 50)]]
    dev = torch.device("cuda", 0)
    queries = [(deep, FG, FO, (FO, FB), False, 2048), (deep, FG, FO, (FO,), True, 16), ([[(FB, 5000, 6000)]], FG, FO, (FO,), False, 16), (deep, FB, FG, (), True, 2048)]
    with _engine(m, (FB, FG, FO)) as e:
        wam.tombstone(e, m, FG, np.nonzero(m.st[FG] == DATA)[0][::10])
        bufs = []
        for p, g, o, fields, desc, cap in queries:
            nf = len(fields)
            bufs.append((torch.full((5 * (cap + 1),), POISON, dtype=torch.int64, device=dev), torch.full((nf * cap + cap + 1,), POISON, dtype=torch.int64, device=dev),
                         torch.full((nf * cap + cap + 1,), POISON, dtype=torch.int64, device=dev), torch.full((5,), POISON, dtype=torch.int64, device=dev)))
        for (p, g, o, fields, desc, cap), (out, val, ts, res) in zip(queries, bufs):              # enqueued back to back, one synchronisation at the end
            e.where_group_first_dev(FB, p, g, o, out, val, ts, res, fields=fields, desc=desc, cap=cap)
        e.sync()
        seen = []
        for (p, g, o, fields, desc, cap), (out, val, ts, res) in zip(queries, bufs):
            nf = len(fields)
            v, t = val.cpu().numpy(), ts.cpu().numpy()
            assert (v[nf * cap:] == POISON).all() and (t[nf * cap:] == POISON).all()
            gv = np.full((nf, cap + 1), POISON, np.int64); gt = gv.copy()
            for f in range(nf):
                gv[f, :cap] = v[f * cap:(f + 1) * cap]; gt[f, :cap] = t[f * cap:(f + 1) * cap]
            got = (out.cpu().numpy().view(fm.FIRST_DTYPE), gv, gt, res.cpu().numpy().view(fm.FIRST_RES_DTYPE)[0])
            want = fm.answer(m, FB, p, g, o, fields, desc, cap, True)
            bad = fm.check(got, want, cap, nf, True, host=False)
            assert bad is None, bad
            seen.append((int(want[3]["flags"]), len(want[0])))
        assert seen[0][1] > gm.CACHE and seen[1][0] == 1 and seen[2][1] == 0 and seen[3][1] > 100


def test_group_by_and_join_interleaved_on_the_same_context():
    n = 2000
    rng = np.random.default_rng(10)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 98000))
    m.set(FB, i, rng.integers(0, 12, n)); m.set(FG, i[i % 9 != 0], rng.integers(0, 40, n)[i % 9 != 0] * 77 - 1000); m.set(FO, i[i % 5 != 0], rng.integers(0, 8, n)[i % 5 != 0])
    m.set(F1, i, i % 40 * 77 - 1000); m.set(F2, i, (i % 40) % 5 - 2)
    p = [[(FB, 1, 9)]]
    with _engine(m, (FB, FG, FO, F1, F2)) as e:
        g0 = e.where_group(FB, p, FG, FO, cap=64).records.tobytes()
        j0 = e.where_join_group(FB, p, FG, FB, EVERY, F1, F2, measure=FO, cap=64, map_cap=4096)
        for cap in (64, 8, 64):
            fm.ask(e, m, FB, p, FG, FO, (FO,), cap == 8, True, cap)
            recs, res = gm.ask(e, m, FB, p, FG, FO, 64)
            assert recs.tobytes() == g0
            fm.ask(e, m, FB, p, FG, FO, (), False, False, cap)
            j1 = e.where_join_group(FB, p, FG, FB, EVERY, F1, F2, measure=FO, cap=64, map_cap=4096)
            assert j1.records.tobytes() == j0.records.tobytes() and len(j0.records) > 2
            assert gm.raw_group(e, FB, p, FG, FO, cap=4)[1]["flags"] == bmx.GROUP_OVERFLOW       # a group-by that overflows right in front
            fm.ask(e, m, FB, p, FG, FO, (FO,), True, False, 64)


# ---- 5. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(11)
    N0, EXTRA = 8192 + 5, 200
    m = Model(wam.node_ids(N0 + EXTRA, 99000))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 12, N0))
    pool = rng.integers(-BIG, BIG, 30)
    idx = old[rng.random(N0) < 0.8]; m.set(FG, idx, pool[rng.integers(0, 30, len(idx))])
    idx = old[rng.random(N0) < 0.7]; m.set(FO, idx, rng.integers(10, 1000, len(idx)))
    idx = old[rng.random(N0) < 0.9]; m.set(F1, idx, rng.integers(0, 6, len(idx)))
    progs = [[[(F1, 1, 3), (FB, 2, 9)]], [[(F1, 0, 1)], [(FO, 500, 1000), (FB, 0, 5)]], EVERY]
    dev = torch.device("cuda", 0)

    def ask(e):
        out = []
        for k, p in enumerate(progs):
            out += [fm.ask(e, m, FB, p, FG, FO, (FO, FB), bool(k % 2), False, 64), fm.ask(e, m, FB, p, FB, FO, (), not k % 2, False, 64), fm.ask(e, m, FB, p, F1, FB, (FG,), False, False, 8)]
        return out

    def same(a, b):
        return all(fm.same_answer(x, y) for x, y in zip(a, b))

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.asarray(vals, np.int64), want_flags=False)
        m.set(f, idx, vals)

    with _engine(m, (FB, FG, FO, F1), 8 * (N0 + EXTRA)) as e:
        first = ask(e)
        assert all(len(a[0]) >= 2 for a in first)
        # a merge that lowers another node below the winner of one group
        w = first[6]                                                # EVERY, ascending, grouped by FG
        key = int(w[0][3]["key"]); win = int(m.index_of(np.array([w[0][3]["id"]], np.uint64))[0])
        members = np.nonzero((m.st[FG] == DATA) & (m.val[FG] == key) & (m.st[FB] == DATA))[0]
        other = int(members[members != win][0])
        merge(e, FO, [other], [int(w[0][3]["val"]) - 1], 100)
        r = fm.ask(e, m, FB, EVERY, FG, FO, (FO,), False, False, 64)
        assert int(r[0][3]["id"]) == int(m.ids[other]) and int(r[0][3]["val"]) == int(w[0][3]["val"]) - 1
        # a tombstone on the winner's order field: the runner-up wins
        wam.tombstone(e, m, FO, [other], ts=200)
        r2 = fm.ask(e, m, FB, EVERY, FG, FO, (FO,), False, False, 64)
        assert int(r2[0][3]["id"]) == int(m.ids[win]) and int(r2[0][3]["n"]) == int(r[0][3]["n"]) - 1 and int(r2[0][3]["n_match"]) == int(r[0][3]["n_match"])
        # ... and one on its group field: it leaves the group
        wam.tombstone(e, m, FG, [win], ts=200)
        r3 = fm.ask(e, m, FB, EVERY, FG, FO, (FO,), False, False, 64)
        assert int(r3[0][3]["id"]) not in (int(m.ids[win]), int(m.ids[other])) and int(r3[0][3]["n_match"]) == int(r2[0][3]["n_match"]) - 1
        assert int(r3[3]["absent"]) == int(r2[3]["absent"]) + 1
        # new rows, then growth
        new = np.arange(N0, N0 + EXTRA)
        merge(e, FB, new, rng.integers(0, 12, EXTRA), 101); merge(e, FG, new[::2], pool[rng.integers(0, 30, len(new[::2]))], 101); merge(e, FO, new, rng.integers(0, 12, EXTRA), 101)
        second = ask(e)
        assert e.index_size(FB) == N0 + EXTRA and not same(first, second)
        e.reserve(32 * (N0 + EXTRA))
        assert same(ask(e), second)
        # a value-ordered view on the base field: the same answers, and the view's counters untouched
        e.index_set_ordered(FB, 1)
        assert set(e.scan_range(FB, 2, 9).tolist()) == set(m.ids[m.mask(FB, [[(FB, 2, 9)]])].tolist())
        assert e.index_ordered_info(FB)[1], "the view answers"
        s0 = e.index_ordered_stats(FB)
        assert same(ask(e), second)
        assert e.index_ordered_stats(FB) == s0 and e.index_ordered_info(FB)[1], "the calls leave the view as it was"
        e.index_set_ordered(FB, 0)
        # deferred compaction (switched on explicitly): a device batch large enough to defer, asked right behind it
        e.set_deferred(True)
        nb = 65_536
        fields = np.array([FB, F1, FG, FO, F2, F3, FS, F["extra"]], np.uint32)      # 8 x N0 distinct (node, field) keys >= nb
        keys = rng.permutation(len(fields) * N0)[:nb]
        kn, kf = keys % N0, fields[keys // N0]
        kv = np.where(kf == FB, rng.integers(0, 12, nb), np.where(kf == FG, pool[rng.integers(0, 30, nb)] - 1, rng.integers(0, 6, nb))).astype(np.int64)
        cols = (torch.from_numpy(m.ids[kn].view(np.int64)).to(dev), torch.from_numpy(kf.view(np.int32)).to(dev),
                torch.full((nb,), 300, dtype=torch.int64, device=dev), torch.from_numpy(kv).to(dev))
        applied = torch.zeros(nb, dtype=torch.int32, device=dev); n_applied = torch.zeros(1, dtype=torch.int64, device=dev)
        d0 = e.deferred_counts()[0]
        e.merge_batch_dev(nb, *cols, bmx.INSERT_REFERENCE, applied=applied, n_applied=n_applied)
        for f in fields:
            m.set(int(f), kn[kf == f], kv[kf == f])
        fm.ask(e, m, FB, progs[1], FG, FO, (FO,), True, False, 256)
        assert e.deferred_counts()[0] == d0 + 1 and int(n_applied.item()) == nb
        ask(e)
        # a base value beyond int32: the index switches to its int64 column
        merge(e, FB, [7, N0 + 3], np.array([WIDE, -(2**35)]), 2000)
        ask(e)
        recs = fm.ask(e, m, FB, [[(FB, 2**39, wam.I64MAX)], [(FB, wam.I64MIN, -(2**33))]], FB, FB, (FB,), False, False, 8)[0]
        assert recs["key"].tolist() == [-(2**35), WIDE]


# ---- 6. seeded programs ----
def test_seeded_programs():
    """the 60 programs of first_model.seeded_queries; each has a group with a tie on its extreme and a group without a contender (asserted here on the model, so
    the test cannot quietly stop covering them); every fourth also with cap = 2 directly in front: an overflowing query leaves the state clean for the next"""
    m, tombs = fm.seeded_model()
    fields = [FB, F1, F2, F3, FG, FO]
    with bmx.Engine(16 * m.N) as e:
        wam.load(e, m, fields)
        for f, idx in tombs.items():
            wam.tombstone(e, m, f, idx)
        assert e.index_size(FB) == m.N
        qs = fm.seeded_queries(m)
        assert len(qs) == 60
        overflows = 0
        for k, (p, group, order, desc) in enumerate(qs):
            assert fm.has_tie_and_empty(m, FB, p, group, order, desc), (k, p)
            if k % 4 == 2:
                overflows += int(fm.ask(e, m, FB, p, group, order, (order,), desc, True, 2)[3]["flags"])
            want = fm.ask(e, m, FB, p, group, order, (order, FB, group)[: 1 + k % 3], desc, bool(k % 2), 64)
            assert int(want[3]["total"]) == e.scan_where(FB, p, count_only=True) and int(want[3]["flags"]) == 0
        assert overflows >= 10
