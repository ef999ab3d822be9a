"""GPU: field-to-field literals of a boolean filter (include/bmx_where.h BMX_LIT_MINUS): lo <= value(A) - value(B) <= hi. Every answer is compared exactly, ids in
index order, with the model of tests/where_diff_model.py over the rows the test itself loaded: the brute force with Python ints on the small hand-made tables,
its numpy form (held against the brute force in test_where_diff_model.py) on the seeded ones. The families that wrap the same program are checked
differentially: the call with a pair literal on (A, B) against the same call with a plain literal on a field D that the test loaded as A - B."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import where_agg_model as wam
import where_diff_model as wdm
from where_diff_model import DATA, F1, F2, F3, F4, FB, I64MAX, I64MIN, PROBED, VAL_MAX

BLOCK = 8192
FD = wdm.streams.fnv1a32("diff.derived")
FT = wdm.streams.fnv1a32("diff.target")
NOBODY = wdm.streams.fnv1a32("diff.nobody")
DMAX = 2 * VAL_MAX            # 2^54 - 2


def _want(e, m, truth):
    pos_ids = e.index_ids(FB)
    return pos_ids[truth[m.index_of(pos_ids)]]


def _check(e, m, clauses, brute=False):
    want = _want(e, m, wdm.brute(m, FB, clauses) if brute else m.mask(FB, clauses))
    got = e.scan_where(FB, clauses)
    assert np.array_equal(got, want), (clauses, len(got), len(want))
    assert e.scan_where(FB, clauses, count_only=True) == len(want), clauses
    return got


# ---- 1. the truth table ----
@pytest.mark.parametrize("wide", [False, True])
def test_truth_table(wide):
    """nodes 0..8: the 9 combinations of (absent, data, tombstone) for A = F1 and B = F2; nodes 9..15: data on both with the differences 0, +-1, +-(2^54 - 2),
    and 5, -5; node 16 has everything but the base field; node 17's base field is tombstoned. wide: the base values lie beyond int32 (the int64 column)."""
    m = wdm.DiffModel(wdm.node_ids(18, 77))
    off = (1 << 40) if wide else 0
    m.set(FB, np.arange(16), np.arange(16) + off); m.set(FB, [17], [3 + off])
    st = [(a, b) for a in range(3) for b in range(3)]                              # node k: (state of A, state of B)
    held_a = [k for k, (a, _) in enumerate(st) if a] + list(range(9, 18)); held_b = [k for k, (_, b) in enumerate(st) if b] + list(range(9, 18))
    m.set(F1, held_a, [7] * (len(held_a) - 9) + [4, 5, 4, VAL_MAX, -VAL_MAX, 9, 4, 4, 4])
    m.set(F2, held_b, [7] * (len(held_b) - 9) + [4, 4, 5, -VAL_MAX, VAL_MAX, 4, 9, 4, 4])
    m.set(F3, np.arange(0, 18, 2), np.arange(0, 18, 2) % 3)
    with bmx.Engine(4096) as e:
        wam.load(e, m, (FB, F1, F2, F3))
        wam.tombstone(e, m, F1, [k for k, (a, _) in enumerate(st) if a == 2]); wam.tombstone(e, m, F2, [k for k, (_, b) in enumerate(st) if b == 2])
        wam.tombstone(e, m, FB, [17])
        P, Q = (F1, F2), (F2, F1)

        def ask(clauses):
            got = _check(e, m, clauses, brute=True)
            return set(m.index_of(got).tolist())

        both = {4, 9, 10, 11, 12, 13, 14, 15}
        rest = set(range(16)) - both
        assert ask([[(P, I64MIN, I64MAX)]]) == both and ask([[(P, I64MIN, I64MAX, True)]]) == rest, "9 states, plain and NOT"
        assert ask([[(P, 0, 0)]]) == {4, 9} and ask([[(P, 0, 0, True)]]) == set(range(16)) - {4, 9}
        assert ask([[(P, 1, I64MAX)]]) == {10, 12, 14} and ask([[(P, I64MIN, -1)]]) == {11, 13, 15}
        assert ask([[(P, 1, 1)]]) == {10} and ask([[(P, -1, -1)]]) == {11} and ask([[(P, -1, 1)]]) == {4, 9, 10, 11}
        assert ask([[(P, DMAX, DMAX)]]) == {12} and ask([[(P, -DMAX, -DMAX)]]) == {13} and ask([[(P, DMAX + 1, I64MAX)]]) == set()
        assert ask([[(P, I64MIN, 5)]]) == both - {12} and ask([[(P, I64MIN, 4)]]) == both - {12, 14}
        assert ask([[(P, I64MIN, I64MIN)]]) == set() and ask([[(P, I64MAX, I64MAX)]]) == set()
        assert ask([[(P, I64MIN, I64MIN, True)]]) == set(range(16)), "a tombstone is no difference of INT64_MIN"
        assert ask([[(P, 3, 2)]]) == set() and ask([[(P, 3, 2, True)]]) == set(range(16)), "lo > hi"
        assert ask([[(P, I64MAX, I64MIN)]]) == set() and ask([[(P, I64MAX, I64MIN, True)]]) == set(range(16))
        # either side the base column; a side the program also uses alone; a field nobody has
        for t in (((FB, F2), I64MIN, 0), ((FB, F2), 1 + off, I64MAX, True), ((F1, FB), -off - 3, -off + 3), ((F1, FB), 0, 0, True), ((FB, F1), I64MIN, I64MAX),
                  ((FB, NOBODY), I64MIN, I64MAX, True), ((NOBODY, FB), 0, 0), ((NOBODY, F3), 0, 0, True)):
            ask([[t]])
        assert ask([[((FB, F2), off - 3, off + 3)]]) == {k for k in range(16) if m.st[F2][k] == DATA and abs(k - int(m.val[F2][k])) <= 3}
        ask([[(F1, 4, 5), (P, 0, 1)]]); ask([[(P, 0, 1), (F2, 4, 4, True)]]); ask([[(F2, 4, 9), (F1, 4, 9), (P, -5, 0)]])
        ask([[(FB, off, off + 12), ((FB, F1), I64MIN, I64MAX), (F1, 0, 9, True)], [(P, 5, 5)]])
        # two literals on one pair; (A, B) and (B, A) in one program; a pair literal in clause 2 only
        assert ask([[(P, -1, I64MAX), (P, I64MIN, 1)]]) == {4, 9, 10, 11} and ask([[(P, 0, I64MAX), (P, 0, 0, True)]]) == {10, 12, 14}
        assert ask([[(P, 1, I64MAX)], [(Q, 1, I64MAX)]]) == both - {4, 9} and ask([[(P, 0, I64MAX), (Q, 0, I64MAX)]]) == {4, 9}
        assert ask([[(P, 5, 5), (Q, -5, -5)], [(Q, 5, 5, True), (P, I64MIN, I64MAX)]]) == both - {15}
        assert ask([[(FB, off + 2, off + 3)], [(P, 1, 1)]]) == {2, 3, 10} and ask([[(F3, 0, 0)], [(P, 0, 0, True), (F3, 1, 2)]]) == set(ask([[(F3, 0, 0)]])) | {2, 8, 10, 14}


# ---- 2. seeded programs ----
N_SEEDED = BLOCK + 300


@pytest.fixture(scope="module")
def seeded():
    m, tombs = wdm.seeded_table(N_SEEDED)
    e = bmx.Engine(16 * N_SEEDED)
    wdm.load_table(e, m, tombs)
    yield e, m
    e.close()


def test_seeded_programs(seeded):
    e, m = seeded
    pos_ids = e.index_ids(FB)
    node = m.index_of(pos_ids)
    counts = []
    for k, p in enumerate(wdm.seeded_programs()):
        want = pos_ids[m.mask(FB, p)[node]]
        got = e.scan_where(FB, p)
        assert np.array_equal(got, want), (k, p, len(got), len(want))
        counts.append(len(want))
    assert sum(0 < c < len(pos_ids) for c in counts) >= 40


def test_device_mode_into_poisoned_buffers(seeded):
    e, m = seeded
    dev = torch.device("cuda", 0)
    FILL = 0x5A5A5A5A5A5A5A5A
    some = 0
    for p in [q for q in wdm.seeded_programs(40, 7) if any(wdm.is_pair(t) for c in q for t in c)][:8]:
        want = _want(e, m, m.mask(FB, p))
        M = len(want)
        for cap in sorted({1, M // 2, M, M + 5} - {0}):
            d_out = torch.full((cap + 4,), FILL, dtype=torch.int64, device=dev)
            d_cnt = torch.full((2,), FILL, dtype=torch.int64, device=dev)
            e.scan_where_dev(FB, p, d_out, cap, d_cnt[0:1])
            e.sync()
            h = d_out.cpu().numpy().view(np.uint64); c = d_cnt.cpu().numpy()
            assert int(c[0]) == M and int(c[1]) == FILL
            assert np.array_equal(h[:min(cap, M)], want[:cap]) and (h[min(cap, M):] == FILL).all(), (cap, M)
        d_cnt = torch.full((2,), FILL, dtype=torch.int64, device=dev)
        e.scan_where_dev(FB, p, None, 0, d_cnt[0:1])
        e.sync()
        assert d_cnt.cpu().numpy().tolist() == [M, FILL]
        some += M > 4
    assert some >= 3


# ---- 3. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(91)
    N0, EXTRA = BLOCK + 5, 200
    m = wdm.DiffModel(wdm.node_ids(N0 + EXTRA, 9100))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 8, N0))
    for f, pr in ((F1, 0.9), (F2, 0.7)):
        idx = old[rng.random(N0) < pr]
        m.set(f, idx, rng.integers(0, 8, len(idx)))
    P = (F1, F2)
    progs = [[[(P, 1, I64MAX)]], [[(P, 0, 0, True), (FB, 2, 6)]], [[((FB, F2), I64MIN, 0)], [((F1, FB), 2, 3), (F2, 0, 3, True)]], [[(P, -1, 1), ((F2, F1), 0, I64MAX)]]]

    def ask(e):
        return [_check(e, m, p) for p in progs]

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.asarray(vals, np.int64), want_flags=False)
        m.set(f, idx, vals)

    with bmx.Engine(8 * (N0 + EXTRA)) as e:
        wam.load(e, m, (FB, F1, F2))
        first = ask(e)
        assert all(0 < len(a) < N0 for a in first)
        # a merge that flips literals: B moves past A on nodes where a > b held, and the other way round
        gt = np.nonzero((m.st[F1] == DATA) & (m.st[F2] == DATA) & (m.val[F1] > m.val[F2]))[0][::2]
        le = np.nonzero((m.st[F1] == DATA) & (m.st[F2] == DATA) & (m.val[F1] <= m.val[F2]))[0][::3]
        merge(e, F2, gt, m.val[F1][gt] + 1, 100); merge(e, F2, le, m.val[F1][le] - 1, 100)
        flipped = ask(e)
        assert not np.isin(m.ids[gt], flipped[0]).any() and np.isin(m.ids[le], flipped[0]).all()
        # tombstones on either side flip the negated literal on; on the base field they take the node away
        wam.tombstone(e, m, F2, gt[::2], ts=200); wam.tombstone(e, m, F1, le[::2], ts=200); wam.tombstone(e, m, FB, old[7::50], ts=200)
        ask(e)
        # new nodes through the change log, then a larger table
        new = np.arange(N0, N0 + EXTRA)
        merge(e, FB, new, rng.integers(0, 8, EXTRA), 201); merge(e, F1, new[::2], rng.integers(0, 8, len(new[::2])), 201); merge(e, F2, new[::3], rng.integers(0, 8, len(new[::3])), 201)
        assert np.isin(m.ids[new], ask(e)[1]).any()
        e.reserve(32 * (N0 + EXTRA))
        before = ask(e)
        # a value-ordered view on the base field changes nothing
        e.index_set_ordered(FB, 1)
        assert all(np.array_equal(a, b) for a, b in zip(before, ask(e)))
        e.index_set_ordered(FB, 0)
        # a base value beyond int32: the int64 column
        merge(e, FB, [11, N0 + 3], np.array([2**40, -(2**35)]), 400)
        ask(e)
        _check(e, m, [[((FB, F1), 2**39, I64MAX)], [((F2, FB), 2**34, I64MAX)]])


# ---- 4. every family that wraps the program: the pair literal against a plain literal on D = A - B ----
N_FAM = 3000


def _bytes(x):
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, C.Structure):
        return bytes(x)
    if isinstance(x, (tuple, list)):
        return tuple(_bytes(y) for y in x)
    if isinstance(x, dict):
        return tuple((k, _bytes(v)) for k, v in x.items())
    if hasattr(x, "__slots__"):
        return tuple((k, _bytes(getattr(x, k))) for k in x.__slots__)
    return x


def _family_engine():
    """-> (engine, model): the seeded table (no value at +-VAL_MAX: D stays in the value domain) with its tombstones, and D = F1 - F2 where both hold data"""
    m, tombs = wdm.seeded_table(N_FAM, seed=31, far=0.0)
    e = bmx.Engine(16 * N_FAM)
    wdm.load_table(e, m, tombs)
    m.derived(FD, F1, F2)
    wam.load(e, m, [FD])
    return e, m


PAIR = (F1, F2)
PROG = [[(PAIR, 1, I64MAX), (F3, 0, 3)], [(PAIR, 0, 0, True), (FB, 0, 2)], [(F4, 5, 5), (PAIR, -2, -1)]]
INNER_PROG = [[(PAIR, 0, I64MAX)], [(F3, 5, 5)]]
TWIN, INNER_TWIN = wdm.plain_twin(PROG, PAIR, FD), wdm.plain_twin(INNER_PROG, PAIR, FD)

FAMILIES = {
    "where_aggregate": lambda e, p, q: (e.where_aggregate(FB, p, measure=F4), e.where_aggregate(FB, p, measure=F3, group=F4, group_lo=0, ngroups=6)),
    "where_top": lambda e, p, q: (e.where_top(FB, p, 50), e.where_top(FB, p, 50, desc=True)),
    "where_group": lambda e, p, q: e.where_group(FB, p, F3, measure=F4),
    "where_group_multi": lambda e, p, q: e.where_group_multi(FB, p, [F3, (F4, 0, 2)], measure=FB),
    "where_quantiles": lambda e, p, q: (e.where_quantiles(FB, p, F4, [(1, 2), (0, 1), (9, 10)]), e.where_quantiles(FB, p, FB, [(1, 4)])),
    "where_semijoin": lambda e, p, q: (e.where_semijoin(FB, p, F3, FB, q, F4), e.where_semijoin(FB, q, F3, FB, p, F4, anti=True)),
    "where_join_group": lambda e, p, q: e.where_join_group(FB, p, F3, FB, q, F4, F1, measure=F4),
    "where_join_rows": lambda e, p, q: e.where_join_rows(FB, p, F3, [F1, F2], FB, q, F4, [F3], cap=500, with_ts=True),
    "where_reach": lambda e, p, q: e.where_reach(FB, p, F3, F4, FB, q, F3, max_depth=4),
    "where_group_first": lambda e, p, q: e.where_group_first(FB, p, F3, F4, fields=[F1, F2]),
    "where_group_top": lambda e, p, q: e.where_group_top(FB, p, F3, F4, 3, fields=[F1]),
}


@pytest.fixture(scope="module")
def family_engine():
    e, m = _family_engine()
    yield e, m
    e.close()


def test_the_twin_programs_select_the_same_and_something(family_engine):
    e, m = family_engine
    a, b = _check(e, m, PROG), _check(e, m, TWIN)
    assert np.array_equal(a, b) and 100 < len(a) < e.index_size(FB) - 100
    assert np.array_equal(_check(e, m, INNER_PROG), _check(e, m, INNER_TWIN))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_differential(family_engine, family):
    e, _ = family_engine
    got, want = FAMILIES[family](e, PROG, INNER_PROG), FAMILIES[family](e, TWIN, INNER_TWIN)
    assert _bytes(got) == _bytes(want), family


def test_where_rows_paged_differential(family_engine):
    e, _ = family_engine

    def pages(p):
        start, out = 0, []
        while True:
            r = e.where_rows(FB, p, [F1, F2, FB], cap=97, with_ts=True, start=start)
            out.append(_bytes(r))
            if r.n_out < 97:
                return out
            start = r.next_pos

    got, want = pages(PROG), pages(TWIN)
    assert got == want and len(got) >= 3


def test_watch_differential_across_a_merge_that_changes_b():
    x, m = _family_engine()                                               # a table of its own: this test moves it
    with x:
        wp, wd = x.watch_create(FB, PROG), x.watch_create(FB, TWIN)
        a, b = x.watch_poll(wp), x.watch_poll(wd)
        assert _bytes(a) == _bytes(b) and a.n_match > 100
        idx = np.nonzero((m.st[F1] == DATA) & (m.st[F2] == DATA))[0][::4]
        m.set(F2, idx, (m.val[F2][idx] + 2) % 6)
        m.derived(FD, F1, F2)
        for f in (F2, FD):
            x.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 50, np.int64), m.val[f][idx], want_flags=False)
        a, b = x.watch_poll(wp), x.watch_poll(wd)
        assert _bytes(a) == _bytes(b) and a.n_entered > 0 and a.n_left > 0
        assert a.n_match == int(m.mask(FB, PROG).sum())


def test_where_update_differential():
    """SET on a third field, the same call on two engines that hold the same rows"""
    res = []
    for p in (PROG, TWIN):
        x, m = _family_engine()
        with x:
            r = x.where_update(FB, p, FT, bmx.UPD_SET, operand=42, ts=77, want_ids=True)
            after = x.where_rows(FB, [[(FB, I64MIN, I64MAX)]], [FT], with_ts=True)
            # two engines lay the same rows out in their own order, and the index order follows the table's: the records are compared id by id, and
            # everything of the result but the layout stamp of each engine
            order = np.argsort(after.ids)
            res.append((_bytes(r)[:8], _bytes(np.sort(r.ids)), _bytes(after.ids[order]), _bytes(after.vals[:, order]), _bytes(after.ts[:, order])))
            assert r.n_applied == r.n_match == int(m.mask(FB, PROG).sum()) > 100
    assert res[0] == res[1]
