"""GPU: clock literals of a boolean filter (include/bmx_where.h BMX_LIT_CLOCK / BMX_LIT_CLOCK_TOMB): the row of a field exists in a state the literal names and
lo <= its clock <= hi. Every answer is compared exactly, ids in index order, with the model of tests/where_clock_model.py over the rows the test itself stored:
the brute force with Python ints on the small hand-made tables, its numpy form (held against the brute force in test_where_clock_model.py) on the seeded ones.
The query forms that wrap the same program are checked differentially: the call with a clock literal on F against the same call with a plain literal on a shadow
field S that the test loaded with val = clock(F) on exactly the nodes where F holds data (or, for BMX_LIT_CLOCK_TOMB, where F is tombstoned)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import where_clock_model as wcm
from where_clock_model import CK, DATA, F1, F2, F3, F4, FB, I64MAX, I64MIN, PROBED, TOMB, TS_MAX

BLOCK = 8192
FS, FT, FU = (wcm.wdm.streams.fnv1a32(s) for s in ("clock.shadow", "clock.shadow.tombs", "clock.target"))
NOBODY = wcm.wdm.streams.fnv1a32("clock.nobody")
STATES = ("data", "deleted", "any")


def _want(e, m, truth):
    pos_ids = e.index_ids(FB)
    return pos_ids[truth[m.index_of(pos_ids)]]


def _check(e, m, clauses, brute=False):
    want = _want(e, m, wcm.brute(m, FB, clauses) if brute else m.mask(FB, clauses))
    got = e.scan_where(FB, clauses)
    assert np.array_equal(got, want), (clauses, len(got), len(want))
    assert e.scan_where(FB, clauses, count_only=True) == len(want), clauses
    return got


def _clocks_as_the_engine_reports_them(e, m, fields):
    for f in fields:
        ts, val, found = e.get_rows(m.ids, np.full(m.N, f, np.uint32))
        assert np.array_equal(found, m.st[f] != wcm.ABSENT) and np.array_equal(ts[found], m.ts[f][found]), f
        assert np.array_equal(val[found] == wcm.VAL_DELETED, m.st[f][found] == TOMB), f


# ---- 1. the truth table ----
LO, HI = 100, 200
TS5 = [LO - 1, LO, 150, HI, HI + 1]


@pytest.mark.parametrize("wide", [False, True])
def test_truth_table(wide):
    """node 5 * s + k: F1 in state s (0 absent, 1 data, 2 tombstoned) with the clock TS5[k] (an absent row has none); 3 state-bit combinations x plain / NOT;
    then the clock bounds 0, 1, 2^53 - 1, INT64_MIN, INT64_MAX and lo > hi. wide: the base values lie beyond int32 (the int64 column)."""
    n = 15
    m = wcm.ClockModel(wcm.node_ids(n + 2, 88))
    off = (1 << 40) if wide else 0
    m.set(FB, np.arange(n), np.arange(n) + off, ts=150)
    m.set(F1, np.arange(5, 15), np.full(10, 150), ts=np.array(TS5 * 2))       # value 150: a kernel that took the value for the clock would put every row inside
    m.tomb(F1, np.arange(10, 15), ts=np.array(TS5))
    m.set(F1, [15], [150], ts=150)                                             # node 15 has the field and no base field; node 16 has a tombstoned base field
    m.set(FB, [16], [3 + off], ts=150); m.tomb(FB, [16], ts=150); m.set(F1, [16], [150], ts=150)
    every = set(range(n))
    with bmx.Engine(4096) as e:
        wcm.put(e, m, (FB, F1))
        _clocks_as_the_engine_reports_them(e, m, (FB, F1))

        def ask(*clauses):
            return set(m.index_of(_check(e, m, list(clauses) if isinstance(clauses[0], list) else [list(clauses)], brute=True)).tolist())

        inside = {"data": {6, 7, 8}, "deleted": {11, 12, 13}, "any": {6, 7, 8, 11, 12, 13}}
        for st in STATES:
            assert ask((CK(F1, st), LO, HI)) == inside[st], st
            assert ask((CK(F1, st), LO, HI, True)) == every - inside[st], st
        held = {"data": set(range(5, 10)), "deleted": set(range(10, 15)), "any": set(range(5, 15))}
        for st in STATES:
            assert ask((CK(F1, st), I64MIN, I64MAX)) == held[st] and ask((CK(F1, st), I64MIN, I64MAX, True)) == every - held[st], st
            assert ask((CK(F1, st), I64MIN, I64MIN)) == set() and ask((CK(F1, st), I64MAX, I64MAX)) == set(), st
            assert ask((CK(F1, st), HI, LO)) == set() and ask((CK(F1, st), HI, LO, True)) == every, "lo > hi"
            assert ask((CK(F1, st), I64MAX, I64MIN)) == set() and ask((CK(F1, st), I64MAX, I64MIN, True)) == every
        assert ask((CK(F1, "any"), I64MIN, I64MIN, True)) == every, "a tombstone's value is no clock of INT64_MIN"
        assert ask((CK(F1), LO, LO)) == {6} and ask((CK(F1), HI, HI)) == {8} and ask((CK(F1, "deleted"), LO - 1, LO - 1)) == {10} and ask((CK(F1, "any"), HI + 1, I64MAX)) == {9, 14}
        # the clocks 0, 1 and 2^53 - 1
        for k, (node, ts) in enumerate(((5, 0), (6, 1), (7, TS_MAX), (10, 0), (11, 1), (12, TS_MAX))):
            wcm.write(e, m, F1, [node], [150] if node < 10 else None, ts=ts)
        _clocks_as_the_engine_reports_them(e, m, (F1,))
        assert ask((CK(F1), 0, 0)) == {5} and ask((CK(F1, "any"), 0, 0)) == {5, 10} and ask((CK(F1, "any"), I64MIN, 0)) == {5, 10} and ask((CK(F1, "any"), I64MIN, -1)) == set()
        assert ask((CK(F1, "any"), 1, 1)) == {6, 11} and ask((CK(F1, "deleted"), 0, 1)) == {10, 11} and ask((CK(F1), 0, 1, True)) == every - {5, 6}
        assert ask((CK(F1), TS_MAX, TS_MAX)) == {7} and ask((CK(F1, "any"), TS_MAX, I64MAX)) == {7, 12} and ask((CK(F1, "any"), TS_MAX + 1, I64MAX)) == set()
        assert ask((CK(F1, "deleted"), 2, TS_MAX - 1)) == {13, 14} and ask((CK(F1, "any"), 2, TS_MAX - 1, True)) == every - {8, 9, 13, 14}
        # the base field: its own row's clock; candidates hold data; a field nobody has
        assert ask((CK(FB), 150, 150)) == every and ask((CK(FB), off, off + 20)) == set() and ask((CK(FB, "any"), 150, 150, True)) == set()
        assert ask((CK(FB, "deleted"), I64MIN, I64MAX)) == set() and ask((CK(FB, "deleted"), I64MIN, I64MAX, True)) == every
        assert ask((CK(FB), 150, 150), (FB, off + 3, off + 4)) == {3, 4} and ask([(CK(FB), 0, 9)], [(FB, off + 3, off + 4, True), (CK(FB, "any"), 100, 200)]) == every - {3, 4}
        assert ask((CK(NOBODY, "any"), I64MIN, I64MAX)) == set() and ask((CK(NOBODY, "any"), I64MIN, I64MAX, True)) == every
        # a value literal and a clock literal of one field: in one clause, across clauses
        assert ask((F1, 150, 150), (CK(F1), 2, I64MAX)) == {8, 9} | {7} and ask((F1, 150, 150, True), (CK(F1, "deleted"), 0, 1)) == {10, 11}
        assert ask([(F1, 0, 9)], [(CK(F1, "any"), 0, 0)], [(CK(F1, "deleted"), TS_MAX, TS_MAX), (F1, I64MIN, I64MAX, True)]) == {5, 10, 12}
        for clauses in ([[(F1, 150, 150), (CK(F1), 2, I64MAX)]], [[(F1, 0, 9)], [(CK(F1, "any"), 0, 0)], [(CK(F1, "deleted"), TS_MAX, TS_MAX), (F1, I64MIN, I64MAX, True)]]):
            probes = []
            wcm.standin(m, FB, clauses, probes=probes)
            assert set(probes) == {(F1, "ts")} and len(probes) <= n, "one slot, one probe per candidate at most"
        # a field in a pair and in a clock literal
        m.set(F2, np.arange(0, n, 2), np.arange(0, n, 2) % 4, ts=3); wcm.put(e, m, (F2,))
        ask(((F1, F2), 147, 149), (CK(F1), 2, I64MAX)); ask([((F2, F1), I64MIN, I64MAX, True), (CK(F2), 3, 3)], [(CK(F1, "deleted"), 0, I64MAX), ((FB, F2), off, off + 9)])


def test_eight_slots_all_with_clock_literals():
    n = 300
    rng = np.random.default_rng(8)
    m = wcm.ClockModel(wcm.node_ids(n, 808))
    fields = [FB] + [wcm.wdm.streams.fnv1a32("clock.eight.%d" % k) for k in range(7)]
    m.set(FB, np.arange(n), rng.integers(0, 4, n), ts=rng.integers(0, 4, n))
    for f in fields[1:]:
        held = np.nonzero(rng.random(n) < 0.9)[0]
        m.set(f, held, rng.integers(0, 4, len(held)), ts=rng.integers(0, 4, len(held)))
        m.tomb(f, held[::5], ts=rng.integers(0, 4, len(held[::5])))
    with bmx.Engine(8192) as e:
        wcm.put(e, m, fields)
        prog = [[(CK(f, STATES[k % 3]), 1, 3, k == 1) for k, f in enumerate(fields[:4])] + [(fields[1], 0, 2, True)], [(CK(f, STATES[k % 3]), 0, 1, k == 2) for k, f in enumerate(fields[4:])],
                [(CK(f, "any"), I64MIN, I64MAX, True) for f in fields[1:3]]]
        W = wcm.prepare(FB, prog)
        assert len(W["slots"]) == 8 and all(W["slot_clock"])
        assert 10 < int(m.mask(FB, prog).sum()) < n - 10 and np.array_equal(m.mask(FB, prog), wcm.brute(m, FB, prog))
        _check(e, m, prog)


# ---- 2. seeded programs ----
N_SEEDED = BLOCK + 300


@pytest.fixture(scope="module")
def seeded():
    m = wcm.seeded_table(N_SEEDED)
    e = bmx.Engine(16 * N_SEEDED)
    wcm.put(e, m, [FB] + PROBED)
    yield e, m
    e.close()


def test_seeded_programs(seeded):
    e, m = seeded
    pos_ids = e.index_ids(FB)
    node = m.index_of(pos_ids)
    counts = []
    for k, p in enumerate(wcm.seeded_programs()):
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
    for p in [q for q in wcm.seeded_programs(40, 7) if any(wcm.is_clock(t) for c in q for t in c)][:8]:
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
    rng = np.random.default_rng(92)
    N0, EXTRA = BLOCK + 5, 200
    m = wcm.ClockModel(wcm.node_ids(N0 + EXTRA, 9200))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 8, N0), ts=rng.integers(1, 50, N0))
    for f, pr in ((F1, 0.9), (F2, 0.7)):
        idx = old[rng.random(N0) < pr]
        m.set(f, idx, rng.integers(0, 8, len(idx)), ts=rng.integers(1, 50, len(idx)))
    since = [[(CK(F1), 100, I64MAX)]]
    gone = [[(CK(F1, "deleted"), 100, I64MAX)]]
    progs = [since, gone, [[(CK(F1, "any"), 25, 120, True), (FB, 2, 6)]], [[(CK(FB), 30, I64MAX), (F2, 0, 3)], [(CK(F2, "any"), I64MIN, I64MAX, True), (CK(FB), 0, 10)]]]

    def ask(e):
        return [_check(e, m, p) for p in progs]

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        # (INSERT_DELTA: a row the merge creates takes the delta's clock; the default mode gives it the reference's clock of 2)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.asarray(vals, np.int64), insert_mode=bmx.INSERT_DELTA, want_flags=False)
        m.set(f, idx, vals, ts=ts)

    def delete(e, f, idx, ts):                                     # (a delete is a row decided elsewhere: a merge takes no tombstone as a delta)
        wcm.write(e, m, f, idx, None, ts=ts)

    with bmx.Engine(8 * (N0 + EXTRA)) as e:
        wcm.put(e, m, (FB, F1, F2))
        first = ask(e)
        assert len(first[0]) == 0 and len(first[1]) == 0 and all(0 < len(a) < N0 for a in first[2:])
        # a merge that raises the clock under an unchanged value flips the literal
        up = np.nonzero(m.st[F1] == DATA)[0][::3]
        merge(e, F1, up, m.val[F1][up], 100)
        _clocks_as_the_engine_reports_them(e, m, (F1,))
        assert np.array_equal(np.sort(ask(e)[0]), np.sort(m.ids[up][m.st[FB][up] == DATA]))
        # delete flips BMX_LIT_CLOCK off and BMX_LIT_CLOCK_TOMB on; a resurrection flips them back
        dead = up[::2]
        delete(e, F1, dead, 200)
        a = ask(e)
        assert not np.isin(m.ids[dead], a[0]).any() and np.array_equal(np.sort(a[1]), np.sort(m.ids[dead][m.st[FB][dead] == DATA]))
        back = dead[::2]
        merge(e, F1, back, np.full(len(back), 5), 300)
        a = ask(e)
        assert np.isin(m.ids[back][m.st[FB][back] == DATA], a[0]).all() and not np.isin(m.ids[back], a[1]).any() and len(a[1]) > 0
        _clocks_as_the_engine_reports_them(e, m, (F1,))
        # a tombstoned base field takes the node away; new nodes through the change log, then a larger table
        delete(e, FB, old[7::50], 400)
        new = np.arange(N0, N0 + EXTRA)
        merge(e, FB, new, rng.integers(0, 8, EXTRA), 401); merge(e, F1, new[::2], rng.integers(0, 8, len(new[::2])), 402)
        _clocks_as_the_engine_reports_them(e, m, (FB, F1))
        assert np.isin(m.ids[new[::2]], ask(e)[0]).all()
        e.reserve(32 * (N0 + EXTRA))
        before = ask(e)
        # a value-ordered view on the base field changes nothing
        e.index_set_ordered(FB, 1)
        assert all(np.array_equal(a, b) for a, b in zip(before, ask(e)))
        e.index_set_ordered(FB, 0)
        # a base value beyond int32: the int64 column
        merge(e, FB, [11, N0 + 3], np.array([2**40, -(2**35)]), 500)
        ask(e)
        assert np.isin(m.ids[[11, N0 + 3]], _check(e, m, [[(CK(FB), 500, 500)]])).all()


# ---- 4. every query form that wraps the program: the clock literal against a plain literal on a shadow field ----
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
    """-> (engine, model): the seeded table, FS = the clock of F1 where F1 holds data, FT = the clock of F1 where F1 is tombstoned"""
    m = wcm.seeded_table(N_FAM, seed=41)
    e = bmx.Engine(16 * N_FAM)
    wcm.put(e, m, [FB] + PROBED)
    m.shadow(FS, F1, DATA); m.shadow(FT, F1, TOMB)
    wcm.put(e, m, [FS, FT])
    return e, m


PROG = {DATA: [[(CK(F1), 4, I64MAX), (F3, 0, 3)], [(CK(F1), 2, 3, True), (FB, 0, 2)], [(F4, 5, 5), (CK(F1), 0, 1), (F1, 0, 4)]],
        TOMB: [[(CK(F1, "deleted"), 3, I64MAX)], [(CK(F1, "deleted"), I64MIN, I64MAX, True), (F3, 0, 1), (F1, 2, 5)]]}
INNER = {DATA: [[(CK(F1), 5, I64MAX)], [(F3, 5, 5)]], TOMB: [[(CK(F1, "deleted"), 0, 4, True), (F2, 0, 3)]]}
SHADOW = {DATA: FS, TOMB: FT}
TWIN = {s: wcm.plain_twin(PROG[s], F1, s, SHADOW[s]) for s in (DATA, TOMB)}
INNER_TWIN = {s: wcm.plain_twin(INNER[s], F1, s, SHADOW[s]) for s in (DATA, TOMB)}

FAMILIES = {
    "where_aggregate": lambda e, p, q: (e.where_aggregate(FB, p, measure=F4), e.where_aggregate(FB, p, measure=F3, group=F4, group_lo=0, ngroups=6)),
    "where_top": lambda e, p, q: (e.where_top(FB, p, 50), e.where_top(FB, p, 50, desc=True)),
    "where_group": lambda e, p, q: e.where_group(FB, p, F3, measure=F4),
    "where_group_multi": lambda e, p, q: e.where_group_multi(FB, p, [F3, (F4, 0, 2)], measure=FB),
    "where_quantiles": lambda e, p, q: (e.where_quantiles(FB, p, F4, [(1, 2), (0, 1), (9, 10)]), e.where_quantiles(FB, p, FB, [(1, 4)])),
    "where_semijoin": lambda e, p, q: (e.where_semijoin(FB, p, F3, FB, q, F4), e.where_semijoin(FB, q, F3, FB, p, F4, anti=True)),
    "where_join_group": lambda e, p, q: e.where_join_group(FB, p, F3, FB, q, F4, F1, measure=F4),
    "where_join_rows": lambda e, p, q: (e.where_join_rows(FB, p, F3, [F1, F2], FB, q, F4, [F3], cap=500, with_ts=True),
                                        e.where_join_rows(FB, p, F3, [F1], FB, q, F4, [F3], cap=500, with_ts=True, inner=True)),
    "where_reach": lambda e, p, q: e.where_reach(FB, p, F3, F4, FB, q, F3, max_depth=4),
    "where_group_first": lambda e, p, q: e.where_group_first(FB, p, F3, F4, fields=[F1, F2]),
    "where_group_top": lambda e, p, q: e.where_group_top(FB, p, F3, F4, 3, fields=[F1]),
}


@pytest.fixture(scope="module")
def family_engine():
    e, m = _family_engine()
    yield e, m
    e.close()


@pytest.mark.parametrize("state", [DATA, TOMB])
def test_the_twin_programs_select_the_same_and_something(family_engine, state):
    e, m = family_engine
    a, b = _check(e, m, PROG[state]), _check(e, m, TWIN[state])
    assert np.array_equal(a, b) and 100 < len(a) < e.index_size(FB) - 100
    assert np.array_equal(_check(e, m, INNER[state]), _check(e, m, INNER_TWIN[state]))


@pytest.mark.parametrize("state", [DATA, TOMB])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_differential(family_engine, family, state):
    e, _ = family_engine
    got, want = FAMILIES[family](e, PROG[state], INNER[state]), FAMILIES[family](e, TWIN[state], INNER_TWIN[state])
    assert _bytes(got) == _bytes(want), family


@pytest.mark.parametrize("state", [DATA, TOMB])
def test_where_rows_paged_differential(family_engine, state):
    e, m = family_engine

    def pages(p):
        start, out = 0, []
        while True:
            r = e.where_rows(FB, p, [F1, F2, FB], cap=97, with_ts=True, start=start)
            out.append(r)
            if r.n_out < 97:
                return out
            start = r.next_pos

    got, want = pages(PROG[state]), pages(TWIN[state])
    assert [_bytes(r) for r in got] == [_bytes(r) for r in want] and len(got) >= 3
    # the clocks the rows come with are the clocks the literal ranged over
    r = e.where_rows(FB, [[(CK(F1, "any"), 3, 6)]], [F1], with_ts=True)
    node = m.index_of(r.ids[:r.n_out])
    assert r.n_out > 100 and np.array_equal(r.ts[0][:r.n_out], m.ts[F1][node]) and ((r.ts[0][:r.n_out] >= 3) & (r.ts[0][:r.n_out] <= 6)).all()


@pytest.mark.parametrize("state", [DATA, TOMB])
def test_watch_differential_across_a_merge_that_moves_clocks(state):
    x, m = _family_engine()                                               # a table of its own: this test moves it
    with x:
        wp, wd = x.watch_create(FB, PROG[state]), x.watch_create(FB, TWIN[state])
        a, b = x.watch_poll(wp), x.watch_poll(wd)
        assert _bytes(a) == _bytes(b) and a.n_match > 100
        # a window nobody is in yet; a merge moves clocks into it under unchanged values (for the tombstones: rows deleted at a clock inside it)
        win = x.watch_create(FB, [[(CK(F1, "data" if state == DATA else "deleted"), 50, 59)]])
        assert x.watch_poll(win).n_match == 0
        idx = np.nonzero((m.st[F1] == DATA) & (m.st[FB] == DATA) & (m.ts[F1] < 55))[0][::4]          # (a row with a later clock would win against the merge)
        if state == DATA:
            x.merge_batch(m.ids[idx], np.full(len(idx), F1, np.uint32), np.full(len(idx), 55, np.int64), m.val[F1][idx], want_flags=False)
            m.set(F1, idx, m.val[F1][idx], ts=55)
        else:
            wcm.write(x, m, F1, idx, None, ts=55)
        for s, f in ((DATA, FS), (TOMB, FT)):
            old = m.st[f].copy()
            m.shadow(f, F1, s)
            left = np.nonzero((old == DATA) & (m.st[f] != DATA))[0]
            m.tomb(f, left, ts=56)                                        # a shadow row whose F1 left the state is deleted, as absent to a plain literal
            wcm.put(x, m, [f])
        r = x.watch_poll(win)
        assert r.n_entered == len(idx) and r.n_left == 0 and np.array_equal(np.sort(r.entered), np.sort(m.ids[idx])), "the nodes whose clock moved into the window entered"
        a, b = x.watch_poll(wp), x.watch_poll(wd)
        assert _bytes(a) == _bytes(b) and a.n_entered + a.n_left > 0
        assert a.n_match == int(m.mask(FB, PROG[state]).sum())


@pytest.mark.parametrize("state", [DATA, TOMB])
def test_where_update_differential(state):
    """SET on a third field, the same call on two engines that hold the same rows"""
    res = []
    for p in (PROG[state], TWIN[state]):
        x, m = _family_engine()
        with x:
            r = x.where_update(FB, p, FU, bmx.UPD_SET, operand=42, ts=77, want_ids=True)
            after = x.where_rows(FB, [[(FB, I64MIN, I64MAX)]], [FU], with_ts=True)
            order = np.argsort(after.ids)
            res.append((_bytes(r)[:8], _bytes(np.sort(r.ids)), _bytes(after.ids[order]), _bytes(after.vals[:, order]), _bytes(after.ts[:, order])))
            assert r.n_applied == r.n_match == int(m.mask(FB, PROG[state]).sum()) > 100
    assert res[0] == res[1]
