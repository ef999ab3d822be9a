"""GPU: aggregates over boolean filters (include/bmx_where_agg.h bmx_where_aggregate). Every answer is compared exactly — all 48 bytes of every record — with
the numpy model of where_agg_model.py over the rows the test itself loaded, or with bmx_scan_aggregate where the two calls must agree.

The shapes are the smallest at which each piece can go wrong (csrc/where_agg_kernels.h, csrc/top_kernels.h top_sweep): E = 4 (int32 column) or 2 (int64) values
per lane and load; one round of a workgroup is 512 lanes x 4 loads = 2048 units: 8192 int32 rows or 4096 int64 rows; a second workgroup exists only above
32768 int32 rows or 16384 int64 rows; the groups live in LDS up to 1024 of them and in global memory from 1025 on. A base value >= 2^31 forces the int64 column."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import where_agg_model as wam
from oracle import streams
from where_agg_model import DATA, Model

FB, F1, F2, F3, F4, F5, FM = (streams.fnv1a32(s) for s in ("base", "one", "two", "three", "four", "five", "measure"))
MORE = [streams.fnv1a32("extra%d" % k) for k in range(3)]
NOBODY = streams.fnv1a32("nobody")
PROBED = [F1, F2, F3, F4, F5]
I64MIN, I64MAX = wam.I64MIN, wam.I64MAX
BIG = 2**53 - 1
WIDE = 2**40
EVERY = [[(NOBODY, 0, 0, True)]]            # a negated literal on a field nobody has: true for every candidate


def _engine(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    return e


def _check(e, m, base, clauses, measure=None, group=None, group_lo=0, ngroups=0):
    got = wam.raw_where_agg(e, base, clauses, measure, group, group_lo, ngroups)
    bad = wam.same_records(got, wam.agg(m, base, clauses, measure, group, group_lo, ngroups))
    assert bad is None, (clauses, measure, group, group_lo, ngroups, bad)
    return got


# ---- 1. truth table ----
def test_truth_table():
    """The 12 nodes of test_gpu_where.py::test_truth_table (F1 absent, tombstoned, below / at the lower end of / inside / at the upper end of / above 10..20;
    the base field itself absent in node 10 and tombstoned in node 11), three times over: with the measure field absent, tombstoned and holding data."""
    m = Model(wam.node_ids(36))
    for s in range(3):                                             # s: the state of the measure field, 0 absent, 1 tombstone, 2 data
        o = 12 * s
        m.set(FB, o + np.arange(10), np.arange(10) * 10)
        m.set(FB, [o + 11], [55])
        m.set(F1, o + np.array([1, 2, 3, 4, 5, 6, 7, 8, 10, 11]), [15, 9, 10, 15, 20, 21, -BIG, BIG, 15, 15])
        m.set(F2, o + np.array([0, 1, 2, 3, 10, 11]), [1, 1, 2, 2, 1, 1])
        if s:
            m.set(FM, o + np.arange(12), 100 * s + np.arange(12) - 5)
    with _engine(m, (FB, F1, F2, FM)) as e:
        for s in range(3):
            o = 12 * s
            wam.tombstone(e, m, F1, [o + 1]); wam.tombstone(e, m, FB, [o + 11]); wam.tombstone(e, m, F2, [o + 3])
        wam.tombstone(e, m, FM, 12 + np.arange(12))
        table = [                                                  # program -> the nodes of one copy that it selects (the sets of test_gpu_where.py)
            ([[(F1, 10, 20)]], [3, 4, 5]),
            ([[(F1, 10, 20, True)]], [0, 1, 2, 6, 7, 8, 9]),
            ([[(F1, 20, 10)]], []),
            ([[(F1, 20, 10, True)]], list(range(10))),
            ([[(FB, 50, 40)]], []),
            ([[(FB, 50, 40, True)]], list(range(10))),
            ([[(F1, I64MIN, I64MAX, True)]], [0, 1, 9]),
            ([[(F1, I64MIN, I64MAX)]], [2, 3, 4, 5, 6, 7, 8]),
            ([[(F1, I64MIN, 0, True)]], [0, 1, 2, 3, 4, 5, 6, 8, 9]),
            ([[(F1, I64MIN, I64MIN)]], []),
            ([[(F1, -BIG, -BIG)]], [7]),
            ([[(F1, BIG, I64MAX)]], [8]),
            ([[(FB, 20, 40)]], [2, 3, 4]),
            ([[(FB, 20, 40, True)]], [0, 1, 5, 6, 7, 8, 9]),
            ([[(FB, I64MIN, I64MAX)]], list(range(10))),
            ([[(FB, I64MIN, I64MAX, True)]], []),
            ([[(F1, 10, 20), (FB, 40, 90)]], [4, 5]),
            ([[(F1, 10, 20)], [(F2, 1, 1)]], [0, 1, 3, 4, 5]),
            ([[(F1, 10, 20), (F1, 15, 30)]], [4, 5]),
            ([[(F1, 10, 20), (F1, 10, 20, True)]], []),
            ([[(F1, 10, 20)], [(F1, 10, 20, True)]], list(range(10))),
            ([[(F2, 2, 2, True), (F1, 0, 100, True)], [(F2, 2, 2)]], [0, 1, 2, 7, 8, 9]),
            ([[(NOBODY, I64MIN, I64MAX)]], []),
            ([[(NOBODY, 0, 0, True)]], list(range(10))),
            ([[(FM, I64MIN, I64MAX, True)]], list(range(10)) * 2),                          # the measure field in the program: the absent and the tombstoned copy
            ([[(FM, 200, 204), (F1, 10, 20, True)]], None),
        ]
        for p, nodes in table:
            r = _check(e, m, FB, p, FM)[0]
            if nodes is not None and FM not in {t[0] for c in p for t in c}:
                vals = [200 + i - 5 for i in nodes]                                         # only the third copy holds the measure
                assert int(r["n_match"]) == 3 * len(nodes) and int(r["n"]) == len(nodes), p
                assert (int(r["sum_hi"]) << 64) + int(r["sum_lo"]) == sum(vals), p
                assert (int(r["min"]), int(r["max"])) == ((min(vals), max(vals)) if vals else (I64MAX, I64MIN)), p
            # the other measures: none, the base field, a program field, grouped by the measure's copy
            _check(e, m, FB, p); _check(e, m, FB, p, FB); _check(e, m, FB, p, F1); _check(e, m, FB, p, F1, FM, 190, 20)


# ---- 2. equality with bmx_scan_aggregate ----
@pytest.mark.parametrize("wide", [False, True])
def test_one_positive_clause_is_scan_aggregate(wide):
    n = 3000
    rng = np.random.default_rng(5 + wide)
    m = Model(wam.node_ids(n, 200))
    off = WIDE if wide else 0
    m.set(FB, np.arange(n), off + rng.integers(0, 1100, n))
    idx = np.nonzero(rng.random(n) < 0.9)[0]; m.set(F1, idx, rng.integers(0, 1100, len(idx)))
    idx = np.nonzero(rng.random(n) < 0.7)[0]; m.set(F3, idx, rng.integers(-3, 1100, len(idx)))
    with _engine(m, (FB, F1, F3)) as e:
        wam.tombstone(e, m, F1, np.nonzero(m.st[F1] == DATA)[0][::13]); wam.tombstone(e, m, F3, np.nonzero(m.st[F3] == DATA)[0][::11])
        assert e.index_size(FB) == n
        seen = 0
        for terms in ([(FB, off + 100, off + 1050), (F1, 50, 1000)], [(FB, off, off + 1099)], [(FB, off + 7, off + 7), (F1, I64MIN, I64MAX), (F3, 0, 2000)]):
            for ng in (0, 5, 1024, 1025):
                for group, lo in ((FB, off + 60), (F1, 60), (F3, -1)):
                    if group not in {t[0] for t in terms} | {F3}:
                        continue
                    for measure in (None, FB, F1, F3):
                        a = wam.raw_where_agg(e, FB, [terms], measure, group if ng else None, lo, ng)
                        b = wam.raw_scan_agg(e, terms, measure, group if ng else None, lo, ng)
                        assert wam.same_records(a, b) is None, (terms, ng, group, measure, wam.same_records(a, b))
                        assert wam.same_records(a, wam.agg(m, FB, [terms], measure, group if ng else None, lo, ng)) is None
                        seen += int(a["n_match"].sum()) > 0
        assert seen > 50


# ---- 3. seeded programs ----
N_RAND = 5000


def _random_model():
    rng = np.random.default_rng(4343)
    m = Model(wam.node_ids(N_RAND, 7100))
    m.set(FB, np.arange(N_RAND), rng.integers(0, 12, N_RAND))
    tombs = {}
    for f, pr in zip(PROBED + MORE, (0.9, 0.7, 0.5, 0.3, 0.6, 0.33, 0.33, 0.33)):
        idx = np.nonzero(rng.random(N_RAND) < pr)[0]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
        tombs[f] = idx[rng.random(len(idx)) < 0.1]
    tombs[FB] = np.arange(17, N_RAND, 97)
    return m, tombs


def test_seeded_programs():
    m, tombs = _random_model()
    progs = wam.random_programs(100, 20250301, FB, PROBED, MORE)
    assert max(sum(len(c) for c in p) for p in progs) == 32 and len({t[0] for c in progs[-1] for t in c} - {FB}) == 8 and max(len(p) for p in progs) == 8
    rng = np.random.default_rng(99)
    with bmx.Engine(16 * N_RAND) as e:
        wam.load(e, m, [FB] + PROBED + MORE)
        for f, idx in tombs.items():
            wam.tombstone(e, m, f, idx)
        assert all(set(np.unique(m.st[f])) == {0, 1, 2} for f in PROBED), "the probed fields in all three states"
        counts = []
        for k, p in enumerate(progs):
            measure = [None, FB, PROBED[k % 5], MORE[k % 3], NOBODY][int(rng.integers(0, 5))]
            one = _check(e, m, FB, p, measure)[0]
            assert int(one["n_match"]) == e.scan_where(FB, p, count_only=True), (k, p)
            group, lo, ng = [(FB, 2, 7), (PROBED[(k + 1) % 5], 0, 6), (PROBED[k % 5], 1, 3), (MORE[k % 3], -1, 1030)][k % 4]
            grouped = _check(e, m, FB, p, measure, group, lo, ng)
            assert int(grouped["n_match"].sum()) == int(one["n_match"]) and int(grouped["n"].sum()) == int(one["n"]), (k, p)
            counts.append(int(one["n_match"]))
        counts = np.array(counts)
        assert (counts == 0).any() and ((counts > 0) & (counts < N_RAND)).sum() >= 25


# ---- 4. the exact sum ----
def test_exact_sum():
    n = 4100
    m = Model(wam.node_ids(n, 900))
    m.set(FB, np.arange(n), np.full(n, BIG))                      # (beyond int32: the int64 column)
    m.set(FM, np.arange(n), np.full(n, -BIG))
    m.set(F1, np.arange(n), np.arange(n) % 3)
    with _engine(m, (FB, FM, F1)) as e:
        for measure, sign in ((FB, 1), (FM, -1)):
            for p in (EVERY, [[(F1, 0, 0)], [(F1, 0, 0, True)]]):
                r = _check(e, m, FB, p, measure)[0]
                assert (int(r["sum_hi"]) << 64) + int(r["sum_lo"]) == sign * n * BIG and int(r["n"]) == n
                assert e.where_aggregate(FB, p, measure).sum == sign * n * BIG
                g = _check(e, m, FB, p, measure, F1, 0, 2)
                assert [(int(x["sum_hi"]) << 64) + int(x["sum_lo"]) for x in g] == [sign * c * BIG for c in (1367, 1367, 1366)]
        # both signs in one sum: it cancels exactly
        m.set(FM, np.arange(0, n, 2), np.full(n // 2, BIG)); e.put_rows(*m.rows(FM, 50))
        r = _check(e, m, FB, EVERY, FM)[0]
        assert (int(r["sum_hi"]), int(r["sum_lo"]), int(r["min"]), int(r["max"])) == (0, 0, -BIG, BIG)


# ---- 5. edges of the column ----
@pytest.mark.parametrize("n,wide", [(1, False), (3, False), (4, False), (5, False), (8191, False), (8192, False), (8193, False), (32769, False),
                                    (1, True), (2, True), (3, True), (4095, True), (4096, True), (4097, True)])
def test_edges_of_the_column(n, wide):
    """A program that is true for every candidate: a lane that read beyond the column, or a skipped tail, changes the count and the sum. Then the only match in
    the first position of the column, and only in the last. 32769 int32 rows: two workgroups flush into one set of accumulators."""
    m = Model(wam.node_ids(n, 3000 + n))
    v = np.arange(n, dtype=np.int64) + 1 + (WIDE if wide else 0)
    m.set(FB, np.arange(n), v)
    m.set(F1, np.arange(n), np.arange(n) % 7)
    with _engine(m, (FB, F1)) as e:
        pos_ids = e.index_ids(FB)
        node = m.index_of(pos_ids)
        m.set(F2, [node[-1]], [2 if n > 1 else 1]); m.set(F2, [node[0]], [1])
        e.load_rows(*m.rows(F2, 5))
        last2 = 2 if n > 1 else 1
        assert np.array_equal(e.index_ids(FB), pos_ids)
        r = _check(e, m, FB, EVERY, FB)[0]
        assert int(r["n_match"]) == n == int(r["n"]) and (int(r["sum_hi"]) << 64) + int(r["sum_lo"]) == int(v.sum())
        g = _check(e, m, FB, EVERY, F1, F1, 0, 7)                  # LDS groups
        assert int(g["n_match"].sum()) == n and int(g[7]["n_match"]) == 0
        g = _check(e, m, FB, EVERY, FB, F1, 0, 1025)               # global groups
        assert int(g["n_match"].sum()) == n
        first, last = int(v[node[0]]), int(v[node[-1]])
        for p, want in (([[(FB, first, first)]], first), ([[(F2, 1, 1), (F1, 7, 9, True)]], first), ([[(FB, last, last)]], last),
                        ([[(F2, last2, last2)], [(F1, 9, 9)]], last), ([[(FB, last, last, True), (F1, 0, 6, True)], [(FB, last, last)]], last)):
            r = _check(e, m, FB, p, FB)[0]
            assert (int(r["n_match"]), int(r["min"]), int(r["max"])) == (1, want, want), (n, p)
            _check(e, m, FB, p, F1, FB, first, 3)


# ---- 6. state hygiene ----
def test_back_to_back_in_device_memory():
    """device mode, nothing synchronised in between: grouped, ungrouped, bmx_scan_aggregate, grouped with another ngroups, bmx_where_top in between — every
    answer as when the query runs alone"""
    n = 8192 + 500
    rng = np.random.default_rng(12)
    m = Model(wam.node_ids(n, 400))
    m.set(FB, np.arange(n), rng.integers(0, 2000, n))
    idx = np.nonzero(rng.random(n) < 0.8)[0]; m.set(F1, idx, rng.integers(0, 40, len(idx)))
    idx = np.nonzero(rng.random(n) < 0.6)[0]; m.set(F2, idx, rng.integers(-5, 5, len(idx)))
    p = [[(F1, 3, 20), (FB, 100, 1800)], [(F2, 0, 4, True), (FB, 0, 50)]]
    terms = [(FB, 100, 1800), (F1, 3, 20)]
    dev = torch.device("cuda", 0)
    with _engine(m, (FB, F1, F2)) as e:
        wam.tombstone(e, m, F1, np.nonzero(m.st[F1] == DATA)[0][::10])
        alone = [wam.raw_where_agg(e, FB, p, F2, F1, 0, 40), wam.raw_where_agg(e, FB, p, F2), wam.raw_scan_agg(e, terms, F2, F1, 0, 40),
                 wam.raw_where_agg(e, FB, p, FB, FB, 90, 1500), wam.raw_where_agg(e, FB, p, F1, F2, -5, 3)]
        top_alone = e.where_top(FB, p, 50)
        assert wam.same_records(alone[0], wam.agg(m, FB, p, F2, F1, 0, 40)) is None and wam.top_equals(top_alone, wam.top(m, FB, p, 50))
        assert int(alone[1][0]["n_match"]) > 100
        bufs = [torch.full((6 * (ng + 2),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev) for ng in (40, 0, 40, 1500, 3)]
        t_out = torch.full((2 * 50,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev); t_cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        e.where_aggregate_dev(FB, p, bufs[0], F2, F1, 0, 40)
        e.where_aggregate_dev(FB, p, bufs[1], F2)
        e.where_top_dev(FB, p, 50, t_out, t_cnt[0:1], t_cnt[1:2])
        e.scan_aggregate_dev(terms, bufs[2], F2, F1, 0, 40)
        e.where_aggregate_dev(FB, p, bufs[3], FB, FB, 90, 1500)
        e.where_aggregate_dev(FB, p, bufs[4], F1, F2, -5, 3)
        e.sync()
        for k, ng in enumerate((40, 0, 40, 1500, 3)):
            h = bufs[k].cpu().numpy().view(wam.AGG_DTYPE)
            nrec = ng + 1 if ng else 1
            assert wam.same_records(h[:nrec], alone[k]) is None, (k, wam.same_records(h[:nrec], alone[k]))
            assert (h[nrec:].view(np.uint8) == 0x5A).all(), "every record written, nothing behind them"
        c = t_cnt.cpu().numpy()
        recs = t_out.cpu().numpy().view(bmx.TOP_DTYPE)[:int(c[0])]
        assert int(c[0]) == len(top_alone[0]) and int(c[1]) == top_alone[1] and np.array_equal(recs, top_alone[0])


# ---- 7. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(67)
    N0, EXTRA = 8192 + 5, 300
    m = Model(wam.node_ids(N0 + EXTRA, 9100))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 12, N0))
    for f, pr in ((F1, 0.9), (F2, 0.5)):
        idx = old[rng.random(N0) < pr]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
    progs = [[[(F1, 1, 3), (FB, 2, 9), (F2, 2, 2, True)]], [[(F1, 0, 1)], [(F2, 4, 5), (FB, 0, 5)]], [[(FB, 3, 3, True), (F1, 0, 5, True)], [(FB, 0, 1), (F2, 0, 2)]]]

    def ask(e):
        out = []
        for p in progs:
            out += [_check(e, m, FB, p, F2), _check(e, m, FB, p, FB, F1, 0, 6), _check(e, m, FB, p, F1, FB, 0, 12)]
        return out

    def same(a, b):
        return all(wam.same_records(x, y) is None for x, y in zip(a, b))

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), vals, want_flags=False)
        m.set(f, idx, vals)

    with _engine(m, (FB, F1, F2), 8 * (N0 + EXTRA)) as e:
        first = ask(e)
        assert all(0 < int(a["n_match"].sum()) < N0 for a in first)
        # a merge that changes base rows and creates new ones: the index is maintained from the change log
        builds = e.index_refresh_counts()[0]
        idx = old[::3]; merge(e, FB, idx, rng.integers(0, 12, len(idx)), 100)
        new = np.arange(N0, N0 + EXTRA)
        merge(e, FB, new, rng.integers(0, 12, EXTRA), 101)
        merge(e, F1, new[::2], rng.integers(0, 6, len(new[::2])), 101)
        second = ask(e)
        assert e.index_refresh_counts()[0] == builds and e.index_size(FB) == N0 + EXTRA and not same(first, second)
        # growth
        e.reserve(32 * (N0 + EXTRA))
        assert same(ask(e), second)
        # tombstones on base rows and on a probed field
        wam.tombstone(e, m, FB, np.concatenate([old[5::40], new[1::7]]), ts=200)
        wam.tombstone(e, m, F1, np.nonzero(m.st[F1] == DATA)[0][::9], ts=200)
        off = ask(e)
        assert not same(off, second)
        # a value-ordered view on the base field, in its three states: off (above), current, carrying a pending patch
        e.index_set_ordered(FB, 1)
        assert set(e.scan_range(FB, 2, 9).tolist()) == set(m.ids[m.mask(FB, [[(FB, 2, 9)]])].tolist())
        assert e.index_ordered_info(FB)[1], "the view answers"
        s0 = e.index_ordered_stats(FB)
        assert same(ask(e), off)
        assert e.index_ordered_stats(FB) == s0 and e.index_ordered_info(FB)[1], "the calls leave the view as it was"
        pick = rng.choice(N0, N0 // 100, replace=False)
        merge(e, FB, pick, rng.integers(0, 12, len(pick)), 1000)
        patched = ask(e)                                            # (the first of them refreshes the index, which patches the view)
        s1 = e.index_ordered_stats(FB)
        assert s1["pending_keys"] > 0 and e.index_ordered_info(FB)[1], "the view carries a pending patch"
        assert same(ask(e), patched)
        assert e.index_ordered_stats(FB) == s1, "the pending patch survives the calls"
        assert set(e.scan_range(FB, 2, 9).tolist()) == set(m.ids[m.mask(FB, [[(FB, 2, 9)]])].tolist())
        e.index_set_ordered(FB, 0)
        assert same(ask(e), patched)
        # a base value beyond int32: the index switches to its int64 column
        merge(e, FB, [7, N0 + 3], np.array([WIDE, -(2**35)]), 2000)
        ask(e)
        r = _check(e, m, FB, [[(FB, 2**39, I64MAX)], [(FB, I64MIN, -(2**33))]], FB)[0]
        assert (int(r["n_match"]), int(r["min"]), int(r["max"])) == (2, -(2**35), WIDE)
