"""CPU: the numpy model of bmx_where_aggregate / bmx_where_top (where_agg_model.py) against plain Python loops that restate include/bmx_where_agg.h node by
node, on 200 nodes whose fields take every state (absent, data, tombstone) — the base field, the measure field and the group field included."""
import numpy as np

import where_agg_model as wam
from where_agg_model import ABSENT, DATA, TOMB

FB, F1, F2, F3, NOBODY = 11, 22, 33, 44, 55
N = 200
I64MIN, I64MAX = wam.I64MIN, wam.I64MAX
BIG = 2**53 - 1


def _table():
    rng = np.random.default_rng(7)
    m = wam.Model(np.arange(1, N + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    for f, top in ((FB, 12), (F1, 6), (F2, 6), (F3, 4)):
        st = rng.integers(0, 3, N)                                   # every state, a third each
        idx = np.nonzero(st != ABSENT)[0]
        m.set(f, idx, rng.integers(-2, top, len(idx)))
        m.tomb(f, np.nonzero(st == TOMB)[0])
    big = np.nonzero((m.st[F2] == DATA) & (m.st[FB] == DATA))[0][:6]                        # the ends of the value domain in a measure: the sum leaves 64 bits behind
    m.val[F2][big] = [BIG, BIG, -BIG, BIG, BIG, BIG]
    m._f(NOBODY)
    assert all(set(np.unique(m.st[f])) == {ABSENT, DATA, TOMB} for f in (FB, F1, F2, F3))
    return m


PROGRAMS = [
    [[(FB, 0, 5)]],
    [[(F1, 0, 2, True)]],                                            # negated only
    [[(NOBODY, 0, 0, True)]],                                        # true for every candidate
    [[(F1, 1, 3), (FB, 2, 9)], [(F3, 0, 1, True), (F2, I64MIN, I64MAX)]],
    [[(FB, 5, 4)]],                                                  # lo > hi: nothing
    [[(F1, I64MIN, I64MAX, True)], [(F2, BIG, BIG)]],
]


def _lit(m, i, t):
    f, lo, hi = t[0], t[1], t[2]
    pos = m.st[f][i] == DATA and lo <= int(m.val[f][i]) <= hi
    return (not pos) if len(t) > 3 and t[3] else pos


def _selected(m, base, clauses):
    return [i for i in range(m.N) if m.st[base][i] == DATA and any(all(_lit(m, i, t) for t in c) for c in clauses)]


def _rec(m, rows, measure):
    vals = None if measure is None else [int(m.val[measure][i]) for i in rows if m.st[measure][i] == DATA]
    n = len(rows) if vals is None else len(vals)
    s = sum(vals or [])
    return (len(rows), n, min(vals) if vals else I64MAX, max(vals) if vals else I64MIN, s)


def _as_tuple(r):
    return (int(r["n_match"]), int(r["n"]), int(r["min"]), int(r["max"]), (int(r["sum_hi"]) << 64) + int(r["sum_lo"]))


def test_aggregate_model_equals_loops():
    m = _table()
    seen_far_sum = False
    for p in PROGRAMS:
        rows = _selected(m, FB, p)
        for measure in (None, FB, F1, F2, NOBODY):
            assert _as_tuple(wam.agg(m, FB, p, measure)[0]) == _rec(m, rows, measure), (p, measure)
            for group, lo, ng in ((FB, 0, 5), (F3, -2, 3), (F3, -5, 20), (F1, 2, 1), (NOBODY, 0, 4)):
                got = wam.agg(m, FB, p, measure, group, lo, ng)
                assert len(got) == ng + 1
                inside = lambda i: m.st[group][i] == DATA and lo <= int(m.val[group][i]) < lo + ng
                for g in range(ng):
                    assert _as_tuple(got[g]) == _rec(m, [i for i in rows if inside(i) and int(m.val[group][i]) == lo + g], measure), (p, measure, group, g)
                assert _as_tuple(got[ng]) == _rec(m, [i for i in rows if not inside(i)], measure), (p, measure, group)
                assert int(got["n_match"].sum()) == len(rows)
            seen_far_sum |= measure == F2 and abs(_rec(m, rows, F2)[4]) > 2**54
    assert seen_far_sum
    assert len(_selected(m, FB, PROGRAMS[2])) == int((m.st[FB] == DATA).sum()) and not _selected(m, FB, PROGRAMS[4])


def test_the_sum_words_are_twos_complement():
    r = wam.record(3, np.array([-BIG, -BIG, 5], np.int64))
    assert int(r["sum_hi"]) == -1 and int(r["sum_lo"]) == (5 - 2 * BIG) % 2**64 and _as_tuple(r)[4] == 5 - 2 * BIG
    r = wam.record(4100, np.full(4100, BIG, np.int64))
    assert _as_tuple(r)[4] == 4100 * BIG and int(r["sum_hi"]) == (4100 * BIG) >> 64
    r = wam.record(2, None)
    assert _as_tuple(r) == (2, 2, I64MAX, I64MIN, 0)
    assert _as_tuple(wam.record(2, np.zeros(0, np.int64))) == (2, 0, I64MAX, I64MIN, 0)


def test_top_model_equals_loops():
    m = _table()
    for p in PROGRAMS:
        rows = _selected(m, FB, p)
        for desc in (False, True):
            order = sorted(rows, key=lambda i: (-int(m.val[FB][i]) if desc else int(m.val[FB][i]), int(m.ids[i])))
            full = [(int(m.ids[i]), int(m.val[FB][i])) for i in order]
            for k in (1, 7, 4096):
                ids, vals, ne = wam.top(m, FB, p, k, desc)
                assert list(zip(ids.tolist(), vals.tolist())) == full[:k] and ne == len(full)
            # cursors: an existing row (ties on its value are told apart by id), and one that names no row
            cursors = full[::5] + [(0, 3), (2**64 - 2, 3), (12345, -100), (12345, 100)]
            for cur in cursors:
                behind = [r for r in full if ((-r[1], r[0]) if desc else (r[1], r[0])) > ((-cur[1], cur[0]) if desc else (cur[1], cur[0]))]
                ids, vals, ne = wam.top(m, FB, p, 7, desc, cur)
                assert list(zip(ids.tolist(), vals.tolist())) == behind[:7] and ne == len(behind), (p, desc, cur)
