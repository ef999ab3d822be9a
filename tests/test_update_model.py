"""CPU: the numpy model of the update by query (update_model.py) against plain Python loops over the seeded table of rows_model.py, and its last-writer-wins
rule against the oracle's merge (oracle.py, BMX_INSERT_DELTA) on a few hundred generated deltas: equal clocks with larger and smaller values, and tombstones met
with a clock below, at and above their own."""
import numpy as np

import rows_model as rm
import update_model as um
from oracle.oracle import INSERT_DELTA, Oracle
from update_model import ABSENT, ADD, COPY, DATA, DELETE, SET, TOMB, VAL_DELETED, VAL_MAX


def _table():
    m, tombs = rm.seeded_table()
    rm.apply_tombs(m, tombs)
    return m


def _lit(m, node, t):
    f, lo, hi = t[0], int(t[1]), int(t[2])
    m._f(f)
    pos = m.st[f][node] == DATA and lo <= int(m.val[f][node]) <= hi
    return (not pos) if len(t) > 3 and t[3] else pos


def _loops(m, order, base, clauses, target, op, operand, src, ts, force, start, cap):
    """update() once more, node by node"""
    cells = {f: [(int(m.st[f][i]), int(m.clk[f][i]), int(m.val[f][i])) for i in range(m.N)] for f in m.st}
    cells.setdefault(target, [(ABSENT, rm.NO_CLOCK, 0)] * m.N)
    cells[target] = list(cells[target])
    res = dict(n_match=0, n_nosrc=0, n_range=0, n_sent=0, n_applied=0, next_pos=len(order))
    applied = []
    m._f(base)
    for pos in range(start, len(order)):
        node = int(m.index_of(np.asarray([order[pos]], np.uint64))[0])
        if m.st[base][node] != DATA or not any(all(_lit(m, node, t) for t in c) for c in clauses):
            continue
        res["n_match"] += 1
        if op == SET:
            v = operand
        elif op == DELETE:
            v = VAL_DELETED
        else:
            m._f(src)
            if m.st[src][node] != DATA:
                res["n_nosrc"] += 1
                continue
            v = int(m.val[src][node]) + (operand if op == ADD else 0)
            if abs(v) > VAL_MAX:
                res["n_range"] += 1
                continue
        if res["n_sent"] == cap:
            if res["next_pos"] == len(order):
                res["next_pos"] = pos
            continue
        res["n_sent"] += 1
        st, cts, cval = (int(m.st[target][node]), int(m.clk[target][node]), int(m.val[target][node])) if target in m.st else (ABSENT, rm.NO_CLOCK, 0)
        win = force or st == ABSENT or (st == TOMB and ts >= cts) or (st == DATA and (ts > cts or (ts == cts and v > cval)))
        if win:
            res["n_applied"] += 1
            applied.append(int(m.ids[node]))
            cells[target][node] = (TOMB, ts, cval) if v == VAL_DELETED else (DATA, ts, v)
    res["n_rows"] = sum(1 for f in cells for c in cells[f] if c[0] != ABSENT)
    return cells, res, applied


def test_model_against_loops():
    m = _table()
    F = rm.names()
    rng = np.random.default_rng(5)
    order = m.ids[rng.permutation(m.N)]                               # some index order
    progs = [p for p, _ in rm.seeded_cases(24)]
    targets = [F["base"], F["one"], F["nobody"], F["two"], F["more"][0]]
    seen = set()
    for k, p in enumerate(progs):
        op = (SET, DELETE, COPY, ADD)[k % 4]
        force = op == DELETE or k % 3 == 0
        src = [F["base"], F["one"], F["two"], F["three"]][(k // 4) % 4]
        target = src if k % 5 == 0 and op in (COPY, ADD) else targets[k % len(targets)]
        operand = [0, 1, -1, VAL_MAX, -VAL_MAX, 7][k % 6]
        ts = [0, 3, 500, 999, 1500, 2500][(k // 2) % 6]
        start = [0, 0, 17, 150][k % 4]
        full = um.update(m, order, F["base"], p, target, op, operand, src, ts, force, start)
        for cap in (None, 0, 1, max(full[1]["n_sent"] - 1, 0), full[1]["n_sent"] + 1):
            before = um.state_rows(m)
            out, res, ids = um.update(m, order, F["base"], p, target, op, operand, src, ts, force, start, cap)
            assert np.array_equal(um.state_rows(m), before), "the model's input is a snapshot"
            cells, wres, wids = _loops(m, order, F["base"], p, target, op, operand, src, ts, force, start, full[1]["n_sent"] if cap is None else cap)
            assert res == wres, (k, cap, res, wres)
            assert ids.tolist() == wids
            for f in cells:
                out._f(f)
                assert [(int(out.st[f][i]), int(out.clk[f][i])) for i in range(m.N)] == [(c[0], c[1]) for c in cells[f]], (k, f)
                assert all(int(out.val[f][i]) == c[2] for i, c in enumerate(cells[f]) if c[0] == DATA), (k, f)
            seen |= {(op, "nosrc" if res["n_nosrc"] else "", "range" if res["n_range"] else "", "lost" if res["n_applied"] < res["n_sent"] else "")}
    assert any(s[1] for s in seen) and any(s[2] for s in seen) and any(s[3] for s in seen), seen


def test_pages_add_up():
    m = _table()
    F = rm.names()
    order = m.ids[::-1].copy()
    p = [[(F["base"], 1, 1)]]                                         # "set x = 2 where x == 1": the pages behind the first must not see the first page's writes
    one, r1, ids1 = um.update(m, order, F["base"], p, F["base"], SET, 2, None, 5000, False)
    cur, start, got, sent = m, 0, [], 0
    while start < len(order):
        cur, r, ids = um.update(cur, order, F["base"], p, F["base"], SET, 2, None, 5000, False, start, 4)
        got += ids.tolist(); sent += r["n_sent"]; start = r["next_pos"]
    assert r1["n_sent"] == sent > 8 and got == ids1.tolist() and np.array_equal(um.state_rows(cur), um.state_rows(one))


def test_last_writer_wins_is_the_oracles():
    rng = np.random.default_rng(99)
    n = 400
    ids = np.arange(1, n + 1, dtype=np.uint64) * 7919
    f = 77
    state = rng.integers(0, 3, n)                                     # ABSENT / DATA / TOMB
    cts = rng.integers(10, 20, n)
    cval = rng.integers(-5, 6, n)
    # deltas around the cells' own clocks and values: below, at, above; equal clocks with larger, equal and smaller values
    ts = cts + rng.integers(-1, 2, n)
    val = np.where(rng.random(n) < 0.5, cval + rng.integers(-1, 2, n), rng.integers(-VAL_MAX, VAL_MAX, n))
    o = Oracle()
    have = state != ABSENT
    o.load_rows(ids[have], np.full(int(have.sum()), f, np.uint32), cts[have], np.where(state[have] == TOMB, VAL_DELETED, cval[have]))
    _, winners = o.merge_batch(ids, np.full(n, f, np.uint32), ts, val, INSERT_DELTA)
    want = [um.wins(int(state[i]), int(cts[i]), int(cval[i]), int(ts[i]), int(val[i])) for i in range(n)]
    assert np.array_equal(np.nonzero(want)[0], winners)
    kinds = {(int(state[i]), int(np.sign(ts[i] - cts[i])), int(np.sign(val[i] - cval[i])) if state[i] == DATA and ts[i] == cts[i] else 0) for i in range(n)}
    assert {(TOMB, -1, 0), (TOMB, 0, 0), (TOMB, 1, 0), (DATA, 0, 1), (DATA, 0, -1), (DATA, 0, 0), (DATA, 1, 0), (DATA, -1, 0)} <= kinds and (state == ABSENT).any()
    for i in range(n):                                                # the state afterwards, cell by cell
        row = o.get_row(int(ids[i]), f)
        if want[i]:
            assert row == (int(ts[i]), int(val[i]))
        elif state[i] != ABSENT:
            assert row == (int(cts[i]), VAL_DELETED if state[i] == TOMB else int(cval[i]))
