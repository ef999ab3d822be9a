"""A numpy model of the aggregates and top-k over boolean filters (include/bmx_where_agg.h), shared by test_where_agg_model.py (CPU: the model against plain
Python loops) and the GPU tests (helper, not a test). The table and the selection are watch_model.Model's (a state per field and node: absent, data, tombstone;
mask(base, clauses) is bmx_scan_where's truth); the order is top_select_model.want's (lexsort by value, then id, the cursor applied).

agg(m, base, clauses, measure, group, group_lo, ngroups) : the records of bmx_where_aggregate, all 48 bytes of each (AGG_DTYPE): n_match, n, min, max and the
                                                           128-bit sum in its two words; ngroups + 1 records, or one with ngroups == 0.
top(m, base, clauses, k, desc, after)                    : (ids, vals, n_eligible) of bmx_where_top."""
import numpy as np

import top_select_model as tsm
from watch_model import ABSENT, DATA, TOMB, Model  # noqa: F401  (re-exported: the tests build their tables with these)

AGG_DTYPE = np.dtype([("n_match", "<u8"), ("n", "<u8"), ("min", "<i8"), ("max", "<i8"), ("sum_lo", "<u8"), ("sum_hi", "<i8")])
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
NO_FIELD = None


def _sum128(vals):
    """exact sum of int64 values (|v| <= 2^53 - 1, fewer than 2^31 of them) as a Python int: the two 32-bit halves summed apart never overflow int64"""
    v = np.asarray(vals, np.int64)
    return (int((v >> 32).sum()) << 32) + int((v & 0xFFFFFFFF).sum())


def record(n_match, measured):
    """one record: n_match selected nodes, `measured` the measure values of those that hold one (None: no measure field — n = n_match, nothing else)"""
    r = np.zeros((), AGG_DTYPE)
    r["n_match"] = n_match; r["min"] = I64MAX; r["max"] = I64MIN
    if measured is None:
        r["n"] = n_match
        return r
    r["n"] = len(measured)
    if len(measured):
        s = _sum128(measured) & ((1 << 128) - 1)                     # two's complement, 128 bits
        r["min"] = int(np.min(measured)); r["max"] = int(np.max(measured))
        r["sum_lo"] = s & ((1 << 64) - 1)
        hi = s >> 64
        r["sum_hi"] = hi - (1 << 64) if hi >= (1 << 63) else hi
    return r


def agg(m, base, clauses, measure=None, group=None, group_lo=0, ngroups=0):
    sel = m.mask(base, clauses)
    if measure is not None:
        m._f(measure)
    have_m = (m.st[measure] == DATA) if measure is not None else None

    def rec(rows):
        return record(int(rows.sum()), None if measure is None else m.val[measure][rows & have_m])

    if not ngroups:
        out = np.zeros(1, AGG_DTYPE); out[0] = rec(sel)
        return out
    m._f(group)
    gv = m.val[group]
    inside = sel & (m.st[group] == DATA) & (gv >= group_lo) & (gv < group_lo + ngroups)
    out = np.zeros(ngroups + 1, AGG_DTYPE)
    empty = record(0, None if measure is None else np.zeros(0, np.int64))
    out[:] = empty
    for g in np.unique(gv[inside] - group_lo):
        out[int(g)] = rec(inside & (gv == group_lo + int(g)))
    out[ngroups] = rec(sel & ~inside)
    return out


def top(m, base, clauses, k, desc=False, after=None):
    """after: (id, val) or None -> (ids, vals, n_eligible)"""
    sel = m.mask(base, clauses)
    return tsm.want(m.val[base][sel], m.ids[sel], k, desc, after)


# ---- helpers of the GPU tests (they load what the model holds and ask the library for raw records) ----
FILL = 0x5A
VAL_DELETED = -(1 << 63)


def node_ids(n, salt=0):
    from oracle import streams
    return streams.splitmix64_np(np.arange(1 + salt, n + 1 + salt, dtype=np.uint64))


def load(x, m, fields, ts=5):
    """x: an Engine or a Comm; the rows of `fields` that hold data"""
    for f in fields:
        if f in m.st and (m.st[f] == DATA).any():
            x.load_rows(*m.rows(f, ts))


def tombstone(x, m, f, idx, ts=9):
    idx = np.asarray(idx)
    x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.full(len(idx), VAL_DELETED, np.int64))
    m.tomb(f, idx)


def raw_where_agg(x, base, clauses, measure=None, group=None, group_lo=0, ngroups=0):
    """the records of bmx_where_aggregate (Engine) / bmx_comm_where_aggregate (Comm) as the library wrote them, into a buffer that held a pattern"""
    import bmx
    out = np.full(48 * (ngroups + 2), FILL, np.uint8).view(AGG_DTYPE)
    args = (*bmx._where_args(base, clauses), *bmx._where_agg_tail(measure, group, group_lo, ngroups), bmx._ptr(out))
    x._chk(x.L.bmx_where_aggregate(x.h, *args, bmx.MEM_HOST) if isinstance(x, bmx.Engine) else x.L.bmx_comm_where_aggregate(x.h, *args))
    nrec = ngroups + 1 if ngroups else 1
    assert (out[nrec:].view(np.uint8) == FILL).all(), "nothing is written behind the last record"
    return out[:nrec].copy()


def raw_scan_agg(e, terms, measure=None, group=None, group_lo=0, ngroups=0):
    import bmx
    out = np.full(48 * (ngroups + 1), FILL, np.uint8).view(AGG_DTYPE)
    e._chk(e.L.bmx_scan_aggregate(e.h, *bmx._agg_args(terms, measure, group, group_lo, ngroups), bmx._ptr(out), bmx.MEM_HOST))
    return out[:ngroups + 1 if ngroups else 1].copy()


def same_records(got, want):
    """all 48 bytes of every record; -> None or the first difference"""
    got, want = np.asarray(got), np.asarray(want)
    if len(got) != len(want):
        return ("length", len(got), len(want))
    bad = np.nonzero(got != want)[0]
    return None if not len(bad) else (int(bad[0]), got[bad[0]], want[bad[0]])


def top_equals(got, want):
    """got: (records, n_eligible) of where_top; want: (ids, vals, n_eligible) of top()"""
    recs, ne = got
    return ne == want[2] and np.array_equal(recs["id"], want[0]) and np.array_equal(recs["val"], want[1])


def random_lit(rng, fields, base, top_base=12, top=6):
    f = fields[int(rng.integers(0, len(fields)))]
    t = top_base if f == base else top
    kind = int(rng.integers(0, 10))
    if kind == 0:
        lo, hi = I64MIN, I64MAX                        # presence / absence
    elif kind == 1:
        lo = int(rng.integers(0, t)); hi = lo - 1 - int(rng.integers(0, 3))        # an empty range
    elif kind <= 4:
        lo = hi = int(rng.integers(-1, t + 1))         # an equality
    else:
        lo = int(rng.integers(-2, t)); hi = lo + int(rng.integers(0, t))
    return (f, lo, hi, bool(rng.random() < 0.35))


def random_programs(count, seed, base, probed, more):
    """count seeded programs over base + probed (1..8 clauses, at most 32 literals); the last one reaches every limit at once: 8 clauses, 32 literals, 8 probed
    fields (probed[:8 - len(more)] + more) and the base field"""
    rng = np.random.default_rng(seed)
    fields = [base] + list(probed)
    progs = []
    while len(progs) < count - 1:
        nc = int(rng.integers(1, 9))
        lens = [int(rng.integers(1, 9)) for _ in range(nc)]
        if rng.random() < 0.5:
            lens = [min(x, 3) for x in lens]           # half of them short clauses: long ANDs are mostly empty
        while sum(lens) > 32:
            lens[int(np.argmax(lens))] -= 1
        pool = [fields[i] for i in rng.choice(len(fields), int(rng.integers(1, len(fields) + 1)), replace=False)]
        progs.append([[random_lit(rng, pool, base) for _ in range(n)] for n in lens])
    eight = (list(probed) + list(more))[:8]
    assert len(eight) == 8
    progs.append([[(eight[(c + k) % 8], 0, 3 + (k % 3), (c + k) % 5 == 0) if k < 3 else (base, c, 11) for k in range(4)] for c in range(8)])
    return progs
