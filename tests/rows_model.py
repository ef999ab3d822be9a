"""A numpy model of the row projection (include/bmx_rows.h), shared by test_rows_model.py (CPU: the model against plain Python loops) and the GPU tests (helper,
not a test). The table is watch_model.Model's (a state per field and node: absent, data, tombstone; mask(base, clauses) is bmx_scan_where's truth) with a clock
per cell beside it (Table).

rows(m, order_ids, base, clauses, fields, with_ts, start, cap) -> (ids, vals, ts, n_match, next_pos): what bmx_where_rows delivers when the base field's index
holds the nodes `order_ids` in that order (Engine.index_ids(base)): the selected positions from `start` on, the first `cap` of them delivered, vals / ts of shape
(len(fields), n_out), ts None without with_ts."""
import numpy as np

from oracle import streams
from watch_model import ABSENT, DATA, TOMB, Model  # noqa: F401  (re-exported)

VAL_DELETED = -(1 << 63)
NO_CLOCK = -1
FILL = 0x5A
RES_DTYPE = np.dtype([("n_match", "<u8"), ("n_out", "<u8"), ("next_pos", "<u8"), ("layout", "<u8"), ("next_shard", "<u4"), ("reserved", "<u4")])


class Table(Model):
    """Model with clk[f][i], the clock of the cell (NO_CLOCK while it is absent); rows(f) hands out the cells' own clocks"""

    def __init__(self, ids):
        super().__init__(ids); self.clk = {}

    def _f(self, f):
        if f not in self.val:
            super()._f(f); self.clk[f] = np.full(self.N, NO_CLOCK, np.int64)

    def set(self, f, idx, vals, ts=5):
        super().set(f, idx, vals); self.clk[f][idx] = ts

    def tomb(self, f, idx, ts=9):
        super().tomb(f, idx); self.clk[f][idx] = ts

    def rows(self, f, ts=None):
        i = np.nonzero(self.st[f] == DATA)[0]
        return self.ids[i], np.full(len(i), f, np.uint32), self.clk[f][i].copy(), self.val[f][i]


def rows(m, order_ids, base, clauses, fields, with_ts=False, start=0, cap=None):
    order_ids = np.asarray(order_ids, np.uint64)
    pos_nodes = m.index_of(order_ids) if len(order_ids) else np.zeros(0, np.int64)
    sel = m.mask(base, clauses)[pos_nodes]
    sel[:start] = False
    hit = np.nonzero(sel)[0]
    n_match = len(hit)
    cap = n_match if cap is None else int(cap)
    nodes = pos_nodes[hit[:cap]]
    next_pos = int(hit[cap]) if n_match > cap else len(order_ids)
    vals = np.full((len(fields), len(nodes)), VAL_DELETED, np.int64)
    ts = np.full((len(fields), len(nodes)), NO_CLOCK, np.int64)
    for k, f in enumerate(fields):
        m._f(f)
        st = m.st[f][nodes]
        vals[k] = np.where(st == DATA, m.val[f][nodes], VAL_DELETED)
        ts[k] = np.where(st == ABSENT, NO_CLOCK, m.clk[f][nodes])
    return m.ids[nodes], vals, (ts if with_ts else None), n_match, next_pos


# ---- the seeded table and programs of test_rows_model.py and test_gpu_where_rows.py ----
def names():
    f = {k: streams.fnv1a32("rows." + k) for k in ("base", "one", "two", "three", "nobody")}
    f["more"] = [streams.fnv1a32("rows.more%d" % k) for k in range(5)]
    return f


SEED, N = 20250611, 300


def seeded_table(salt=0):
    """300 nodes; the base field holds data on most of them, the probed fields take every state a third each, every cell has a clock of its own"""
    F = names()
    rng = np.random.default_rng(SEED)
    m = Table(streams.splitmix64_np(np.arange(1 + 77000 + salt, N + 1 + 77000 + salt, dtype=np.uint64)))
    tombs = {}
    for f, top, p_abs, p_tomb in [(F["base"], 12, 0.12, 0.12), (F["one"], 6, 1 / 3, 1 / 3), (F["two"], 6, 1 / 3, 1 / 3), (F["three"], 6, 1 / 3, 1 / 3)] + [(x, 6, 0.5, 0.2) for x in F["more"]]:
        u = rng.random(N)
        st = np.where(u < p_abs, ABSENT, np.where(u < p_abs + p_tomb, TOMB, DATA))
        idx = np.nonzero(st != ABSENT)[0]
        m.set(f, idx, rng.integers(-2, top, len(idx)), rng.integers(1, 1000, len(idx)))
        tombs[f] = np.nonzero(st == TOMB)[0]                       # loaded as data first, tombstoned afterwards (apply_tombs)
    m._f(F["nobody"])
    return m, tombs


def apply_tombs(m, tombs, x=None):
    """the tombstones of seeded_table into the model and, with x (an Engine or a Comm), into the library: each with a clock above the cell's own"""
    for f, idx in tombs.items():
        ts = m.clk[f][idx] + 1000
        if x is not None and len(idx):
            x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), ts, np.full(len(idx), VAL_DELETED, np.int64))
        m.tomb(f, idx, ts)


def seeded_cases(count=100):
    """-> [(clauses, fields)]: where_agg_model's seeded programs, each with 0..8 projected fields (the base field, program fields, a field nobody holds and
    repeats among them)"""
    import where_agg_model as wam
    F = names()
    progs = wam.random_programs(count, SEED + 1, F["base"], [F["one"], F["two"], F["three"]], F["more"])
    pool = [F["one"], F["two"], F["base"], F["three"], F["more"][0], F["nobody"], F["one"], F["more"][3]]
    return [(p, [pool[(k + j) % len(pool)] for j in range(k % 9)]) for k, p in enumerate(progs)]


# ---- helpers of the GPU tests ----
def tombstone(x, m, f, idx, ts=9):
    """where_agg_model.tombstone with the clock going into the model too"""
    idx = np.asarray(idx)
    x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.full(len(idx), VAL_DELETED, np.int64))
    m.tomb(f, idx, ts)


def raw_rows(x, base, clauses, fields, with_ts=False, start=0, cap=0, rows_alloc=None):
    """bmx_where_rows (Engine) / bmx_comm_where_rows (Comm; start = (shard, pos)) into buffers that held a pattern; checks that nothing was written behind
    n_out in any column -> (ids, vals, ts, res record)"""
    import ctypes as C
    import bmx
    room = max(cap, 1) if rows_alloc is None else rows_alloc
    nf, farr, flags = bmx._rows_fields(fields, with_ts)
    ids = np.full(room * 8, FILL, np.uint8).view(np.uint64)
    vals = np.full(max(nf, 1) * room * 8, FILL, np.uint8).view(np.int64)
    ts = np.full(max(nf, 1) * room * 8, FILL, np.uint8).view(np.int64)
    res = np.full(40, FILL, np.uint8)
    tail = (int(cap), bmx._ptr(ids), bmx._ptr(vals), bmx._ptr(ts), C.c_void_p(res.ctypes.data))      # (a clock buffer also without BMX_ROWS_TS: it must stay as it is)
    if isinstance(x, bmx.Engine):
        x._chk(x.L.bmx_where_rows(x.h, *bmx._where_args(base, clauses), nf, farr, flags, int(start), *tail, bmx.MEM_HOST))
    else:
        x._chk(x.L.bmx_comm_where_rows(x.h, *bmx._where_args(base, clauses), nf, farr, flags, int(start[0]), int(start[1]), *tail))
    r = res.view(RES_DTYPE)[0]
    n = int(r["n_out"])
    assert n == min(int(r["n_match"]), cap) and int(r["reserved"]) == 0
    pat = np.full(8, FILL, np.uint8)
    assert (ids[n:] == pat.view(np.uint64)[0]).all(), "ids behind n_out"
    v2, t2 = vals[:nf * cap].reshape(nf, cap) if cap else vals[:0].reshape(nf, 0), ts[:nf * cap].reshape(nf, cap) if cap else ts[:0].reshape(nf, 0)
    assert (v2[:, n:] == pat.view(np.int64)[0]).all() and (vals[nf * cap:] == pat.view(np.int64)[0]).all(), "values behind n_out"
    assert (t2[:, n:] == pat.view(np.int64)[0]).all() and (ts[nf * cap:] == pat.view(np.int64)[0]).all(), "clocks behind n_out"
    if not with_ts:
        assert (ts == pat.view(np.int64)[0]).all(), "without BMX_ROWS_TS no clock is written"
    return ids[:n].copy(), v2[:, :n].copy(), (t2[:, :n].copy() if with_ts else None), r


def same(got, want, index_size=None):
    """got: raw_rows' tuple; want: rows()' tuple -> None or what differs first"""
    ids, vals, ts, r = got
    wids, wvals, wts, n_match, next_pos = want
    if int(r["n_match"]) != n_match:
        return ("n_match", int(r["n_match"]), n_match)
    if int(r["next_pos"]) != next_pos:
        return ("next_pos", int(r["next_pos"]), next_pos)
    if not np.array_equal(ids, wids):
        return ("ids", ids[:8], wids[:8])
    if vals.shape != wvals.shape or not np.array_equal(vals, wvals):
        return ("vals", vals.shape, wvals.shape, np.argwhere(vals != wvals)[:4] if vals.shape == wvals.shape else None)
    if (ts is None) != (wts is None) or (ts is not None and not np.array_equal(ts, wts)):
        return ("ts", None if ts is None else np.argwhere(ts != wts)[:4])
    return None
