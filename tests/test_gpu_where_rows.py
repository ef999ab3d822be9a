"""GPU: row projection (include/bmx_rows.h bmx_where_rows). Every answer is compared exactly with the numpy model of rows_model.py over the rows the test itself
loaded: the ids, every cell of every column, the clocks, n_match, n_out, next_pos. Every buffer handed to the library held 0x5A bytes and is checked untouched
behind n_out in every column (rows_model.raw_rows).

The shapes are small; what they pin is the contract: the three states of a cell, the base field as a projected field with and without clocks, fields of the
program, repeats, 0 / 1 / 8 fields, the caps around n_match, pages, cursors, the int64 column, a living table (merge, growth, view) and the device mode. The
geometry of the two kernels is test_gpu_where_rows_kernel_edges.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import rows_model as rm
import where_agg_model as wam
from oracle import streams
from rows_model import DATA, Table

FB, F1, F2, FM = (streams.fnv1a32(s) for s in ("base", "one", "two", "measure"))
NOBODY = streams.fnv1a32("nobody")
MORE = [streams.fnv1a32("extra%d" % k) for k in range(4)]
I64MIN, I64MAX = wam.I64MIN, wam.I64MAX
BIG = 2**53 - 1
WIDE = 2**40
EVERY = [[(NOBODY, 0, 0, True)]]            # a negated literal on a field nobody has: true for every candidate


def _engine(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    return e


def _check(e, m, base, clauses, fields, with_ts=False, start=0, cap=None, order=None):
    order = e.index_ids(base) if order is None else order
    cap = len(order) if cap is None else cap
    got = rm.raw_rows(e, base, clauses, fields, with_ts, start, cap)
    bad = rm.same(got, rm.rows(m, order, base, clauses, fields, with_ts, start, cap))
    assert bad is None, (clauses, fields, with_ts, start, cap, bad)
    assert int(got[3]["next_shard"]) == 0 and int(got[3]["layout"]) != 0
    return got


# ---- 1. truth table x the three states of a projected field ----
def _truth_table():
    """The 12 nodes of test_gpu_where_agg.py::test_truth_table, three times over: with the projected field FM absent, tombstoned and holding data."""
    m = Table(wam.node_ids(36))
    for s in range(3):
        o = 12 * s
        m.set(FB, o + np.arange(10), np.arange(10) * 10, 5 + np.arange(10))
        m.set(FB, [o + 11], [55])
        m.set(F1, o + np.array([1, 2, 3, 4, 5, 6, 7, 8, 10, 11]), [15, 9, 10, 15, 20, 21, -BIG, BIG, 15, 15], 20 + np.arange(10))
        m.set(F2, o + np.array([0, 1, 2, 3, 10, 11]), [1, 1, 2, 2, 1, 1])
        if s:
            m.set(FM, o + np.arange(12), 100 * s + np.arange(12) - 5, 40 + np.arange(12))
    return m


TABLE = [
    [[(F1, 10, 20)]], [[(F1, 10, 20, True)]], [[(F1, 20, 10)]], [[(F1, 20, 10, True)]], [[(FB, 50, 40)]], [[(FB, 50, 40, True)]], [[(F1, I64MIN, I64MAX, True)]],
    [[(F1, I64MIN, I64MAX)]], [[(F1, I64MIN, 0, True)]], [[(F1, I64MIN, I64MIN)]], [[(F1, -BIG, -BIG)]], [[(F1, BIG, I64MAX)]], [[(FB, 20, 40)]], [[(FB, 20, 40, True)]],
    [[(FB, I64MIN, I64MAX)]], [[(FB, I64MIN, I64MAX, True)]], [[(F1, 10, 20), (FB, 40, 90)]], [[(F1, 10, 20)], [(F2, 1, 1)]], [[(F1, 10, 20), (F1, 15, 30)]],
    [[(F1, 10, 20), (F1, 10, 20, True)]], [[(F1, 10, 20)], [(F1, 10, 20, True)]], [[(F2, 2, 2, True), (F1, 0, 100, True)], [(F2, 2, 2)]], [[(NOBODY, I64MIN, I64MAX)]],
    [[(NOBODY, 0, 0, True)]], [[(FM, I64MIN, I64MAX, True)]], [[(FM, 200, 204), (F1, 10, 20, True)]],
]


def test_truth_table():
    m = _truth_table()
    with _engine(m, (FB, F1, F2, FM)) as e:
        for s in range(3):
            o = 12 * s
            rm.tombstone(e, m, F1, [o + 1]); rm.tombstone(e, m, FB, [o + 11]); rm.tombstone(e, m, F2, [o + 3])
        rm.tombstone(e, m, FM, 12 + np.arange(12), ts=77)
        order = e.index_ids(FB)
        assert len(order) == 33
        states = set()
        for p in TABLE:
            for with_ts in (False, True):
                ids, vals, ts, r = _check(e, m, FB, p, [FM, F1, F2], with_ts, order=order)
                assert np.array_equal(ids, e.scan_where(FB, p))
                if with_ts:
                    states |= {("data" if v != rm.VAL_DELETED else ("tomb" if t != rm.NO_CLOCK else "absent")) for v, t in zip(vals[0].tolist(), ts[0].tolist())}
                    assert set(ts[0][vals[0] == rm.VAL_DELETED].tolist()) <= {77, rm.NO_CLOCK}
        assert states == {"data", "tomb", "absent"}


# ---- 2. which fields ----
def test_the_fields():
    """the base field among the fields (with and without clocks), a field of the program, a repeated field, 0 / 1 / 8 fields"""
    m = _truth_table()
    with _engine(m, (FB, F1, F2, FM)) as e:
        rm.tombstone(e, m, F1, [1, 13]); rm.tombstone(e, m, FB, [11])
        order = e.index_ids(FB)
        progs = [EVERY, [[(F1, 10, 20)], [(F2, 1, 1)]], [[(FB, 20, 70)]]]
        for p in progs:
            for with_ts in (False, True):
                for fields in ([], [FB], [F1], [FB, F1, FB], [F1, F1], [NOBODY], [FB, F1, F2, FM, NOBODY, F1, FB, MORE[0]]):
                    ids, vals, ts, r = _check(e, m, FB, p, fields, with_ts, order=order)
                    for k, f in enumerate(fields):
                        if f == FB:
                            assert (vals[k] != rm.VAL_DELETED).all() and (ts is None or (ts[k] >= 5).all()), "a selected node holds the base field"
            got = rm.raw_rows(e, FB, p, [], False, 0, 5)
            assert np.array_equal(got[0], e.scan_where(FB, p, cap=5)) and int(got[3]["n_match"]) == e.scan_where(FB, p, count_only=True), "no fields: bmx_scan_where's answer"
        r = e.where_rows(FB, progs[1], [FB, F1], with_ts=True)
        w = rm.rows(m, order, FB, progs[1], [FB, F1], True)
        assert np.array_equal(r.ids, w[0]) and np.array_equal(r.vals, w[1]) and np.array_equal(r.ts, w[2]) and (r.n_match, r.next_pos) == (w[3], w[4]) and r.layout
        r = e.where_rows(FB, progs[1], [F2], cap=2)
        assert r.ts is None and r.vals.shape == (1, 2) and r.n_out == 2 and r.n_match == w[3]


# ---- 3. caps, pages, cursors; both widths ----
def _random_model(n, wide, seed=4343):
    rng = np.random.default_rng(seed)
    m = Table(wam.node_ids(n, 7100 + n))
    m.set(FB, np.arange(n), (WIDE if wide else 0) + rng.integers(0, 12, n), rng.integers(1, 50, n))
    tombs = {}
    for f, pr in ((F1, 0.8), (F2, 0.5), (FM, 0.6)):
        idx = np.nonzero(rng.random(n) < pr)[0]
        m.set(f, idx, rng.integers(-BIG, BIG, len(idx)) if f == FM else rng.integers(0, 6, len(idx)), rng.integers(1, 50, len(idx)))
        tombs[f] = idx[rng.random(len(idx)) < 0.15]
    tombs[FB] = np.arange(17, n, 97)
    return m, tombs


@pytest.mark.parametrize("wide", [False, True])
def test_caps_pages_and_cursors(wide):
    n = 2 * 8192 + 300
    off = WIDE if wide else 0
    m, tombs = _random_model(n, wide)
    with _engine(m, (FB, F1, F2, FM), 8 * n) as e:
        for f, idx in tombs.items():
            rm.tombstone(e, m, f, idx, ts=60)
        order = e.index_ids(FB)
        assert len(order) == n
        progs = [[[(FB, off + 3, off + 5), (F1, 2, 5)], [(F2, 0, 0), (F1, 0, 9, True)]], [[(FB, off + 6, off + 9), (F2, 1, 4)]]]
        fields = [F1, FM, FB]
        for p in progs:
            one = _check(e, m, FB, p, fields, True, order=order)
            nm = int(one[3]["n_match"])
            assert nm > 1100
            layout = int(one[3]["layout"])
            for cap in (0, 1, nm - 1, nm, nm + 1):
                got = _check(e, m, FB, p, fields, True, 0, cap, order=order)
                assert int(got[3]["n_out"]) == min(cap, nm) and int(got[3]["layout"]) == layout
            first = int(_check(e, m, FB, p, [], False, 0, 0, order=order)[3]["next_pos"])
            assert order[first] == one[0][0], "cap 0: the position of the first selected node"
            for cap in (1, 7, 1000):
                ids, vals, ts, start, pages = [], [], [], 0, 0
                if cap == 1:
                    start = int(rm.rows(m, order, FB, p, [], False, 0, nm - 40)[4])      # (cap 1: the last 40 nodes, not 4000 calls)
                while start < n:
                    g = _check(e, m, FB, p, fields, True, start, cap, order=order)
                    assert int(g[3]["layout"]) == layout
                    ids.append(g[0]); vals.append(g[1]); ts.append(g[2]); pages += 1
                    start = int(g[3]["next_pos"])
                k = 40 if cap == 1 else nm
                assert np.array_equal(np.concatenate(ids), one[0][nm - k:]) and np.array_equal(np.concatenate(vals, axis=1), one[1][:, nm - k:])
                assert np.array_equal(np.concatenate(ts, axis=1), one[2][:, nm - k:]) and pages == -(-k // cap)
            for start in (n - 1, n, n + 5, 1 << 40):
                g = _check(e, m, FB, p, fields, True, start, 4, order=order)
                if start >= n:
                    assert (int(g[3]["next_pos"]), int(g[3]["n_match"]), int(g[3]["n_out"])) == (n, 0, 0), "a cursor beyond the index selects nothing"


# ---- 4. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(77)
    N0, EXTRA = 8192 + 5, 300
    m = Table(wam.node_ids(N0 + EXTRA, 9900))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 12, N0))
    for f, pr in ((F1, 0.9), (FM, 0.8)):
        idx = old[rng.random(N0) < pr]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
    progs = [[[(F1, 1, 3), (FB, 2, 9)]], [[(F1, 0, 1)], [(FM, 4, 5), (FB, 0, 5)]], [[(FB, 3, 3, True), (F1, 0, 5, True)], [(FB, 0, 1)]]]
    fields = [FM, FB, F1]

    def ask(e):
        return [_check(e, m, FB, p, fields, True) for p in progs]

    def same(a, b):
        return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a, b))

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), vals, insert_mode=bmx.INSERT_DELTA, want_flags=False)
        m.set(f, idx, vals, ts)                                    # (BMX_INSERT_DELTA: a created row keeps the delta's own clock; ts is above every stored clock)

    with _engine(m, (FB, F1, FM), 8 * (N0 + EXTRA)) as e:
        first = ask(e)
        layout = int(first[0][3]["layout"])
        order0 = e.index_ids(FB)
        # a merge that changes projected values and base rows and creates rows: the index is refreshed from the log, the appended rows come last
        idx = old[::3]; merge(e, FM, idx, rng.integers(0, 6, len(idx)) + 10, 100)
        idx = old[1::5]; merge(e, FB, idx, rng.integers(0, 12, len(idx)), 100)
        new = np.arange(N0, N0 + EXTRA)
        merge(e, FB, new, rng.integers(0, 12, EXTRA), 101)
        merge(e, F1, new, rng.integers(0, 6, EXTRA), 101)
        second = ask(e)
        order1 = e.index_ids(FB)
        assert not same(first, second) and len(order1) == N0 + EXTRA and np.array_equal(order1[:N0], order0), "appended behind the old rows"
        assert all(int(x[3]["layout"]) == layout for x in second), "a refresh from the log keeps the layout"
        assert all(set(x[0].tolist()) & set(m.ids[new].tolist()) for x in second)
        # growth: the table moves, the index is built again — a new layout
        e.reserve(32 * (N0 + EXTRA))
        third = ask(e)
        assert all(int(x[3]["layout"]) != layout for x in third), "a cursor of the old layout is void"
        assert all(sorted(x[0].tolist()) == sorted(y[0].tolist()) for x, y in zip(second, third))
        # tombstones on projected and base rows
        rm.tombstone(e, m, FM, np.nonzero(m.st[FM] == DATA)[0][::7], ts=200)
        rm.tombstone(e, m, FB, np.concatenate([old[5::40], new[1::7]]), ts=200)
        fourth = ask(e)
        assert not same(third, fourth)
        # a value-ordered view on the base field: the same arrays, and the view's counters untouched
        e.index_set_ordered(FB, 1)
        assert set(e.scan_range(FB, 2, 9).tolist()) == set(m.ids[m.mask(FB, [[(FB, 2, 9)]])].tolist())
        assert e.index_ordered_info(FB)[1], "the view answers"
        s0 = e.index_ordered_stats(FB)
        assert same(ask(e), fourth)
        assert e.index_ordered_stats(FB) == s0 and e.index_ordered_info(FB)[1], "the calls leave the view as it was"


# ---- 5. seeded programs ----
@pytest.mark.parametrize("with_ts", [False, True])
def test_seeded_programs(with_ts):
    m, tombs = rm.seeded_table()
    F = rm.names()
    every = [F["base"], F["one"], F["two"], F["three"]] + F["more"]
    with bmx.Engine(16 * m.N * len(every)) as e:
        wam.load(e, m, every)
        rm.apply_tombs(m, tombs, e)
        order = e.index_ids(F["base"])
        counts = []
        for p, fields in rm.seeded_cases():
            got = _check(e, m, F["base"], p, fields, with_ts, order=order)
            counts.append(int(got[3]["n_match"]))
            if counts[-1] > 2:
                _check(e, m, F["base"], p, fields, with_ts, len(order) // 2, 3, order=order)
        assert sum(c > 0 for c in counts) >= 60


# ---- 6. device memory ----
def test_device_memory_back_to_back():
    """device mode: the answers equal host mode; three calls enqueued back to back (one cut off by its cap, one with cap 0, one selecting nothing) with one
    synchronisation at the end; nothing is written behind n_out"""
    n = 8192 + 700
    m, tombs = _random_model(n, False, seed=31)
    dev = torch.device("cuda", 0)
    deep = [[(FB, 2, 9), (F1, 0, 4)], [(F2, 0, 1), (FB, 0, 1)]]
    queries = [(deep, [F1, FM, FB], True, 0, n), (deep, [FM, F1], False, 100, 50), (deep, [F1], True, 0, 0), ([[(FB, 50, 60)]], [F1, F2], True, 0, 16), (deep, [], False, 8192, 700)]
    PAT = 0x5A5A5A5A5A5A5A5A
    with _engine(m, (FB, F1, F2, FM), 8 * n) as e:
        for f, idx in tombs.items():
            rm.tombstone(e, m, f, idx, ts=60)
        order = e.index_ids(FB)
        host = [rm.raw_rows(e, FB, p, f, t, s, c) for p, f, t, s, c in queries]
        bufs = [(torch.full((c + 1,), PAT, dtype=torch.int64, device=dev), torch.full((max(len(f), 1) * c + 1,), PAT, dtype=torch.int64, device=dev),
                 torch.full((max(len(f), 1) * c + 1,), PAT, dtype=torch.int64, device=dev), torch.full((5,), PAT, dtype=torch.int64, device=dev)) for p, f, t, s, c in queries]
        for (p, f, t, s, c), (di, dv, dt, dr) in zip(queries, bufs):
            e.where_rows_dev(FB, p, f, c, di, dv, dt if t else None, dr, start=s)
        e.sync()
        for (p, f, t, s, c), (di, dv, dt, dr), h in zip(queries, bufs, host):
            r = dr.cpu().numpy().view(rm.RES_DTYPE)[0]
            assert r.tobytes() == h[3].tobytes(), "the same record as in host mode"
            k = int(r["n_out"])
            ids = di.cpu().numpy().view(np.uint64); vals = dv.cpu().numpy(); ts = dt.cpu().numpy()
            assert np.array_equal(ids[:k], h[0]) and (ids[k:].view(np.int64) == PAT).all()
            for j in range(len(f)):
                assert np.array_equal(vals[j * c:j * c + k], h[1][j]) and (vals[j * c + k:(j + 1) * c] == PAT).all()
                if t:
                    assert np.array_equal(ts[j * c:j * c + k], h[2][j]) and (ts[j * c + k:(j + 1) * c] == PAT).all()
            assert vals[len(f) * c] == PAT and (t or (ts == PAT).all())
            assert rm.same((h[0], h[1], h[2], r), rm.rows(m, order, FB, p, f, t, s, c)) is None
