"""A numpy model of the update by query (include/bmx_update.h), shared by test_update_model.py (CPU: the model against plain Python loops and against the oracle's
merge) and the GPU tests (helper, not a test). The table is rows_model.Table (a state and a clock per cell), imported, not edited.

update(m, order_ids, base, clauses, target, op, operand, src, ts, force, start, cap) -> (the new table, every word of bmx_upd_res as a dict, the ids of the nodes
whose row changed in index order), when the base field's index holds the nodes `order_ids` in that order (Engine.index_ids(base)). `m` itself is left as it was:
the selection and every source value come from it (the snapshot)."""
import numpy as np

from rows_model import ABSENT, DATA, TOMB, NO_CLOCK, VAL_DELETED, Table  # noqa: F401  (re-exported)

SET, DELETE, COPY, ADD = 0, 1, 2, 3
VAL_MAX = 2**53 - 1
TS_MAX = 2**53 - 1
FILL = 0x5A
RES_DTYPE = np.dtype([("n_match", "<u8"), ("n_nosrc", "<u8"), ("n_range", "<u8"), ("n_sent", "<u8"), ("n_applied", "<u8"), ("n_rows", "<u8"), ("next_pos", "<u8"),
                      ("layout", "<u8"), ("next_shard", "<u4"), ("reserved", "<u4")])
WORDS = ("n_match", "n_nosrc", "n_range", "n_sent", "n_applied", "n_rows", "next_pos")


def clone(m):
    """a Table of its own with the same cells"""
    c = Table(m.ids)
    for f in m.val:
        c._f(f)
        c.val[f] = m.val[f].copy(); c.st[f] = m.st[f].copy(); c.clk[f] = m.clk[f].copy()
    return c


def n_rows(m):
    """resident rows: every cell that is not absent (a tombstone keeps its slot)"""
    return int(sum(int((m.st[f] != ABSENT).sum()) for f in m.st))


def wins(state, cts, cval, ts, val):
    """the last-writer-wins rule of BMX_INSERT_DELTA for one delta (ts, val) against one cell: an absent row is created, the lexicographic maximum of (ts, val)
    wins against data, a tombstone of clock cts loses to ts >= cts"""
    if state == ABSENT:
        return True
    if state == TOMB:
        return ts >= cts
    return (ts, val) > (cts, cval)


def records(m, order_ids, base, clauses, target, op, operand=0, src=None, start=0):
    """-> (positions of the writable nodes, their node numbers, their values, n_match, n_nosrc, n_range): the selection from `start` on, without cap"""
    order_ids = np.asarray(order_ids, np.uint64)
    pos_nodes = m.index_of(order_ids) if len(order_ids) else np.zeros(0, np.int64)
    sel = m.mask(base, clauses)[pos_nodes] if len(order_ids) else np.zeros(0, bool)
    sel[:start] = False
    hit = np.nonzero(sel)[0]
    nodes = pos_nodes[hit]
    n_match = len(hit)
    if op == SET:
        vals = np.full(n_match, int(operand), np.int64); ok = np.ones(n_match, bool); nosrc = rng_out = 0
    elif op == DELETE:
        vals = np.full(n_match, VAL_DELETED, np.int64); ok = np.ones(n_match, bool); nosrc = rng_out = 0
    else:
        m._f(src)
        have = m.st[src][nodes] == DATA
        sv = np.where(have, m.val[src][nodes], 0).astype(np.int64)
        vals = sv + (int(operand) if op == ADD else 0)                   # |sv|, |operand| <= 2^53 - 1: no overflow in int64
        inside = (vals >= -VAL_MAX) & (vals <= VAL_MAX)
        ok = have & inside
        nosrc = int((~have).sum()); rng_out = int((have & ~inside).sum())
    return hit[ok], nodes[ok], vals[ok], n_match, nosrc, rng_out


def update(m, order_ids, base, clauses, target, op, operand=0, src=None, ts=0, force=False, start=0, cap=None):
    pos, nodes, vals, n_match, nosrc, rng_out = records(m, order_ids, base, clauses, target, op, operand, src, start)
    cap = len(pos) if cap is None else int(cap)
    next_pos = int(pos[cap]) if len(pos) > cap else len(order_ids)
    nodes, vals = nodes[:cap], vals[:cap]
    out = clone(m)
    out._f(target)
    m._f(target)
    applied = []
    for i, v in zip(nodes.tolist(), vals.tolist()):
        if force or wins(int(m.st[target][i]), int(m.clk[target][i]), int(m.val[target][i]), int(ts), v):
            applied.append(i)
            if v == VAL_DELETED:
                out.st[target][i] = TOMB
            else:
                out.st[target][i] = DATA; out.val[target][i] = v
            out.clk[target][i] = ts
    res = {"n_match": n_match, "n_nosrc": nosrc, "n_range": rng_out, "n_sent": len(nodes), "n_applied": len(applied), "n_rows": n_rows(out), "next_pos": next_pos}
    return out, res, m.ids[np.asarray(applied, np.int64)]


def state_rows(m):
    """every cell that holds data as sorted (id, field, ts, val) rows: what dump_rows delivers, in a fixed order"""
    parts = [np.stack([m.ids[i].astype(np.uint64).view(np.int64), np.full(len(i), f, np.int64), m.clk[f][i], m.val[f][i]], 1)
             for f in sorted(m.st) for i in [np.nonzero(m.st[f] == DATA)[0]] if len(i)]
    a = np.concatenate(parts) if parts else np.zeros((0, 4), np.int64)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def dump_sorted(x):
    """Engine / Comm dump_rows in state_rows' form"""
    i, f, t, v = x.dump_rows()
    a = np.stack([np.asarray(i, np.uint64).view(np.int64), np.asarray(f, np.int64), np.asarray(t, np.int64), np.asarray(v, np.int64)], 1) if len(i) else np.zeros((0, 4), np.int64)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


# ---- helpers of the GPU tests ----
def raw_update(x, base, clauses, target, op, operand=0, src=None, ts=0, force=False, start=0, cap=0, want_ids=True, room=None):
    """bmx_where_update (Engine) / bmx_comm_where_update (Comm; start = (shard, pos)) into buffers that held a pattern; checks that nothing was written at or
    behind n_applied -> (ids, res record)"""
    import ctypes as C
    import bmx
    room = max(cap, 1) if room is None else room
    ids = np.full(room * 8, FILL, np.uint8).view(np.uint64)
    res = np.full(72, FILL, np.uint8)
    head = (*bmx._where_args(base, clauses), *bmx._upd_args(target, op, operand, src, ts, force))
    tail = (int(cap), bmx._ptr(ids) if want_ids else None, C.c_void_p(res.ctypes.data))
    if isinstance(x, bmx.Engine):
        x._chk(x.L.bmx_where_update(x.h, *head, int(start), *tail, bmx.MEM_HOST))
    else:
        x._chk(x.L.bmx_comm_where_update(x.h, *head, int(start[0]), int(start[1]), *tail))
    r = res.view(RES_DTYPE)[0]
    n = int(r["n_applied"]) if want_ids else 0
    assert int(r["reserved"]) == 0 and int(r["n_applied"]) <= int(r["n_sent"]) <= cap
    assert int(r["n_sent"]) == min(cap, int(r["n_match"]) - int(r["n_nosrc"]) - int(r["n_range"]))
    assert (ids[n:] == np.full(8, FILL, np.uint8).view(np.uint64)[0]).all(), "ids at or behind n_applied"
    return ids[:n].copy(), r


def same(got, want, index_size=None):
    """got: raw_update's tuple; want: update()'s (table, res, ids) -> None or what differs first"""
    ids, r = got
    _, w, wids = want
    for k in WORDS:
        if int(r[k]) != w[k]:
            return (k, int(r[k]), w[k])
    if ids is not None and not np.array_equal(ids, wids):
        return ("ids", ids[:8], wids[:8])
    return None
