"""CPU: the numpy model of bmx_where_rows (rows_model.py) against plain Python loops that restate include/bmx_rows.h node by node and cell by cell, over the
100 seeded programs of the GPU test and a seeded table whose cells take every state. The table is checked not to be degenerate here: most programs select
something, and many deliver an absent and a tombstoned cell side by side."""
import numpy as np

import rows_model as rm
from rows_model import ABSENT, DATA, TOMB


def _lit(m, i, t):
    f, lo, hi = t[0], t[1], t[2]
    m._f(f)
    pos = m.st[f][i] == DATA and lo <= int(m.val[f][i]) <= hi
    return (not pos) if len(t) > 3 and t[3] else pos


def _loops(m, order, base, clauses, fields, with_ts, start, cap):
    """order: node numbers by index position"""
    sel = [p for p, i in enumerate(order) if p >= start and m.st[base][i] == DATA and any(all(_lit(m, i, t) for t in c) for c in clauses)]
    out = sel[:cap]
    ids = [int(m.ids[order[p]]) for p in out]
    vals, ts = [], []
    for f in fields:
        m._f(f)
        col_v, col_t = [], []
        for p in out:
            i = order[p]
            st = m.st[f][i]
            col_v.append(int(m.val[f][i]) if st == DATA else rm.VAL_DELETED)
            col_t.append(rm.NO_CLOCK if st == ABSENT else int(m.clk[f][i]))
        vals.append(col_v); ts.append(col_t)
    return ids, vals, (ts if with_ts else None), len(sel), (sel[cap] if len(sel) > cap else len(order))


def _table():
    m, tombs = rm.seeded_table()
    rm.apply_tombs(m, tombs)
    F = rm.names()
    assert all(set(np.unique(m.st[f])) == {ABSENT, DATA, TOMB} for f in (F["base"], F["one"], F["two"], F["three"]))
    order = np.random.default_rng(5).permutation(m.N)              # some index order: the model must follow it, not the node numbers
    return m, order


def test_model_equals_loops():
    m, order = _table()
    FB = rm.names()["base"]
    order_ids = m.ids[order]
    selecting = both = 0
    for k, (p, fields) in enumerate(rm.seeded_cases()):
        full = _loops(m, order, FB, p, fields, True, 0, m.N)
        n = full[3]
        selecting += n > 0
        flat_v = [v for col in full[1] for v in col]; flat_t = [t for col in full[2] for t in col]
        both += any(v == rm.VAL_DELETED and t == rm.NO_CLOCK for v, t in zip(flat_v, flat_t)) and any(v == rm.VAL_DELETED and t != rm.NO_CLOCK for v, t in zip(flat_v, flat_t))
        for with_ts in (False, True):
            for start, cap in ((0, None), (0, 0), (0, 1), (0, max(n - 1, 0)), (0, n), (0, n + 1), (m.N // 3, 7), (m.N - 1, 2), (m.N, 5), (m.N + 9, 5)):
                want = _loops(m, order, FB, p, fields, with_ts, start, m.N if cap is None else cap)
                ids, vals, ts, n_match, next_pos = rm.rows(m, order_ids, FB, p, fields, with_ts, start, cap)
                assert ids.tolist() == want[0] and vals.tolist() == want[1] and n_match == want[3] and next_pos == want[4], (k, with_ts, start, cap)
                assert (ts is None and want[2] is None) or ts.tolist() == want[2], (k, start, cap)
                assert vals.shape == (len(fields), len(ids))
    assert selecting >= 60, selecting
    assert both >= 30, both


def test_pages_concatenate():
    m, order = _table()
    FB = rm.names()["base"]
    order_ids = m.ids[order]
    for p, fields in rm.seeded_cases()[::7]:
        one = rm.rows(m, order_ids, FB, p, fields, True)
        for cap in (1, 7, 1000):
            ids, vals, ts, start, pages = [], [], [], 0, 0
            while True:
                a, v, t, n_match, nxt = rm.rows(m, order_ids, FB, p, fields, True, start, cap)
                assert n_match == one[3] - len(np.concatenate(ids)) if ids else n_match == one[3]
                ids.append(a); vals.append(v); ts.append(t); pages += 1
                if nxt == m.N:
                    break
                start = nxt
            assert np.array_equal(np.concatenate(ids), one[0]) and np.array_equal(np.concatenate(vals, axis=1), one[1]) and np.array_equal(np.concatenate(ts, axis=1), one[2])
            assert pages == max(-(-one[3] // cap), 1)


def test_an_empty_index_and_the_table_helper():
    m, _ = _table()
    F = rm.names()
    ids, vals, ts, n_match, next_pos = rm.rows(m, np.zeros(0, np.uint64), F["base"], [[(F["base"], 0, 5)]], [F["one"]], True, 0, 4)
    assert len(ids) == 0 and vals.shape == (1, 0) and ts.shape == (1, 0) and n_match == 0 and next_pos == 0
    rid, rf, rts, rval = m.rows(F["one"])
    i = m.index_of(rid)
    assert (m.st[F["one"]][i] == DATA).all() and np.array_equal(rts, m.clk[F["one"]][i]) and np.array_equal(rval, m.val[F["one"]][i]) and (rf == F["one"]).all()
    assert (m.clk[F["nobody"]] == rm.NO_CLOCK).all()
