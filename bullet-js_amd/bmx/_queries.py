"""How each query's arguments go to the library, once: the builders (`_*_args`, `_*_tail`) make the C arguments that stand between the handle and the output
pointers, the same for the host form, the device form and the shard form of a call; _HostQueries adds what a host-memory call needs besides — buffers, the
"count first, then fetch" policy of a cap of None, the result object — for Engine and Comm alike."""
import ctypes as C

import numpy as np

from ._abi import (AGG_DTYPE, AGG_NO_FIELD, FIRST_DESC, FIRST_DTYPE, GROUP_DTYPE, GTOP_DESC, GTOP_GRP_DTYPE, GTOP_MAX_CAP, GTOP_MAX_PER, GTOP_MAX_ROWS, GTOP_ROW_DTYPE, JROWS_INNER,
                   LIT_CLOCK, LIT_CLOCK_TOMB, LIT_MINUS, LIT_NOT, LIT_SUBTRAHEND, QUANT_REC_DTYPE, REACH_OVERFLOW, ROWS_TS, SEMI_ANTI, SEMI_OVERFLOW, TOP_DESC,
                   TOP_DTYPE, UPD_FORCE, UPD_MAX_CAP, WATCH_OVERFLOW, Expr, FirstRes, GroupKey, GroupRes, GtopRes, JoinRowsRes, Lit, QuantQ, QuantRes, ReachRes, RowsRes,
                   SemiRes, Term, TopRec, UpdRes, WatchRes, _Handle, _np, _ptr, _ref)
from ._results import (FirstResult, GroupTopResult, JoinRowsResult, ReachResult, RowsResult, SemiResult, UpdateResult, WatchPoll,
                       agg_results)


def _field(f):
    """a measure or group field, None meaning "none"; a computed measure (bmx.Expr) goes by reference: the *_expr calls take it in the field's place"""
    return _ref(f) if isinstance(f, Expr) else AGG_NO_FIELD if f is None else int(f)


def _terms(terms):
    """a list of (field, lo, hi) -> (nterms, bmx_term array)"""
    return (len(terms), (Term * max(len(terms), 1))(*[Term(int(f), 0, int(lo), int(hi)) for f, lo, hi in terms]))


def _cursor(start, shard):
    """where a paged query begins: the index position, behind the shard's number in the shard form"""
    return (int(start),) if shard is None else (int(shard), int(start))


def _agg_args(terms, measure, group, group_lo, ngroups):
    return (*_terms(terms), *_where_agg_tail(measure, group, group_lo, ngroups))


def _where_agg_tail(measure, group, group_lo, ngroups):
    return (_field(measure), _field(group), int(group_lo), int(ngroups))


def _top_args(terms, k, desc, after):
    return (*_terms(terms), *_where_top_tail(k, desc, after))


def _where_top_tail(k, desc, after):
    """-> (flags, cursor, k) of bmx_scan_top; after: a record of an earlier answer, (id, val) or None"""
    cur = None
    if after is not None:
        cur = TopRec(int(after["id"]), int(after["val"])) if isinstance(after, (np.void, dict)) else TopRec(int(after[0]), int(after[1]))
    return (TOP_DESC if desc else 0, C.byref(cur) if cur is not None else None, int(k))


class Clock:
    """The field of a clock literal: (Clock(field, data=True, tombs=False), lo, hi[, negated]) is true iff the node's row of `field` exists in a state named
    here (data, tombstoned) and lo <= its clock <= hi; negated it is the exact complement (bmx_where.h BMX_LIT_CLOCK, BMX_LIT_CLOCK_TOMB)."""
    __slots__ = ("field", "flags")

    def __init__(self, field, data=True, tombs=False):
        if not (data or tombs):
            raise ValueError("bmx.Clock: a clock literal names data, tombstones or both")
        self.field, self.flags = int(field), (LIT_CLOCK if data else 0) | (LIT_CLOCK_TOMB if tombs else 0)


def _where_entries(t):
    """one literal of a clause -> its bmx_lit entries: one, or for ((a, b), lo, hi[, negated]) — lo <= a - b <= hi — the MINUS entry and its SUBTRAHEND entry;
    (Clock(f, ...), lo, hi[, negated]) ranges over the clock of f's row"""
    neg = LIT_NOT if len(t) > 3 and t[3] else 0
    if isinstance(t[0], Clock):
        return [Lit(t[0].field, t[0].flags | neg, int(t[1]), int(t[2]))]
    if isinstance(t[0], (tuple, list)):
        a, b = t[0]
        return [Lit(int(a), LIT_MINUS | neg, int(t[1]), int(t[2])), Lit(int(b), LIT_SUBTRAHEND, 0, 0)]
    return [Lit(int(t[0]), neg, int(t[1]), int(t[2]))]


def _where_args(base, clauses):
    """clauses: a list of lists of (field, lo, hi), (field, lo, hi, negated), comparing two fields of a node ((a, b), lo, hi[, negated]), or over a row's clock
    (Clock(field, ...), lo, hi[, negated])
    -> (base_field, nclauses, clause_len, lits)"""
    ents = [[e for t in c for e in _where_entries(t)] for c in clauses]
    flat = [e for c in ents for e in c]
    lens = (C.c_uint32 * max(len(clauses), 1))(*[len(c) for c in ents])
    lits = (Lit * max(len(flat), 1))(*flat)
    return (int(base), len(clauses), lens, lits)


def _group_tail(measure, group):
    return (_field(measure), _field(group))


def _mgroup_keys(keys):
    """keys: a list of field or (field, origin, width) -> (nkeys, bmx_group_key array)"""
    ks = [(k, 0, 1) if isinstance(k, (int, np.integer)) else k for k in keys]
    return (len(ks), (GroupKey * max(len(ks), 1))(*[GroupKey(int(f), 0, int(o), int(w)) for f, o, w in ks]))


def _fields(fields):
    """a list of fields to fetch -> (nfields, uint32 array)"""
    fields = [int(f) for f in fields]
    return (len(fields), (C.c_uint32 * max(len(fields), 1))(*fields))


def _rows_fields(fields, with_ts):
    """-> (nfields, fields, flags) of bmx_where_rows"""
    return (*_fields(fields), ROWS_TS if with_ts else 0)


def _rows_buffers(nfields, cap, with_ts):
    return np.zeros(max(cap, 1), np.uint64), np.zeros((nfields, max(cap, 1)), np.int64), np.zeros((nfields, max(cap, 1)), np.int64) if with_ts else None


def _first_tail(group, order, fields, desc, with_ts):
    """-> (group_field, order_field, nfields, fields, flags) of bmx_where_group_first"""
    nf, farr, flags = _rows_fields(fields, with_ts)
    return (int(group), int(order), nf, farr, flags | (FIRST_DESC if desc else 0))


def _first_buffers(nfields, cap, with_ts):
    return np.zeros(max(cap, 1), FIRST_DTYPE), np.zeros((nfields, max(cap, 1)), np.int64), np.zeros((nfields, max(cap, 1)), np.int64) if with_ts else None


def _gtop_tail(group, order, per, fields, desc, with_ts):
    """-> (group_field, order_field, per, nfields, fields, flags) of bmx_where_group_top"""
    nf, farr, flags = _rows_fields(fields, with_ts)
    return (int(group), int(order), int(per), nf, farr, flags | (GTOP_DESC if desc else 0))


def _gtop_buffers(nfields, cap, per, with_ts):
    rows = max(cap * per, 1)
    return (np.zeros(max(cap, 1), GTOP_GRP_DTYPE), np.zeros(rows, GTOP_ROW_DTYPE), np.zeros((nfields, rows), np.int64),
            np.zeros((nfields, rows), np.int64) if with_ts else None)


def _upd_args(target, op, operand, src, ts, force):
    """-> (target_field, op, src_field, operand, ts, flags) of bmx_where_update"""
    if ts is None:
        import time
        ts = int(time.time() * 1000)          # the reference's clock: milliseconds since the epoch
    return (int(target), int(op), 0 if src is None else int(src), int(operand), int(ts), UPD_FORCE if force else 0)


def _semi_values(values):
    v = _np(values, np.int64).ravel()
    return v, len(v)


def _join_pairs(keys, vals):
    k, v = _np(keys, np.int64).ravel(), _np(vals, np.int64).ravel()
    if len(k) != len(v):
        raise ValueError("keys and vals differ in length")
    return k, v, len(k)


def _jrows_pairs(keys, node_ids):
    k, v = _np(keys, np.int64).ravel(), _np(node_ids, np.uint64).ravel()
    if len(k) != len(v):
        raise ValueError("keys and node_ids differ in length")
    return k, v, len(k)


def _jrows_flags(with_ts, inner):
    return (ROWS_TS if with_ts else 0) | (JROWS_INNER if inner else 0)


def _quant_tail(measure, qs):
    """-> (measure_field, nq, qs) of bmx_where_quantiles; qs: a list of (num, den)"""
    arr = (QuantQ * max(len(qs), 1))(*[QuantQ(int(a), int(b)) for a, b in qs])
    return (_ref(measure) if isinstance(measure, Expr) else int(measure), len(qs), arr)


# ---- one builder per query: the arguments of bmx_<query> / bmx_comm_<query> from the program to the last input. `shard`: the cursor's shard, in the shard
# form; `measure`: a field, or the bmx.Expr of the *_expr call. Pointers (device or host arrays) go through _ptr; a host array must stay alive in its caller. ----
def _where_aggregate_args(base, clauses, measure, group, group_lo, ngroups):
    return (*_where_args(base, clauses), *_where_agg_tail(measure, group, group_lo, ngroups))


def _where_top_args(base, clauses, k, desc, after):
    return (*_where_args(base, clauses), *_where_top_tail(k, desc, after))


def _where_group_args(base, clauses, measure, group):
    return (*_where_args(base, clauses), *_group_tail(measure, group))


def _where_quantiles_args(base, clauses, measure, qs):
    return (*_where_args(base, clauses), *_quant_tail(measure, qs))


def _where_rows_args(base, clauses, fields, with_ts, start, shard=None):
    return (*_where_args(base, clauses), *_rows_fields(fields, with_ts), *_cursor(start, shard))


def _where_group_first_args(base, clauses, group, order, fields, desc, with_ts):
    return (*_where_args(base, clauses), *_first_tail(group, order, fields, desc, with_ts))


def _where_group_top_args(base, clauses, group, order, per, fields, desc, with_ts):
    return (*_where_args(base, clauses), *_gtop_tail(group, order, per, fields, desc, with_ts))


def _where_group_multi_args(base, clauses, keys, measure):
    return (*_where_args(base, clauses), _field(measure), *_mgroup_keys(keys))


def _where_update_args(base, clauses, target, op, operand, src, ts, force, start, shard=None):
    return (*_where_args(base, clauses), *_upd_args(target, op, operand, src, ts, force), *_cursor(start, shard))


def _where_semijoin_args(base, clauses, link, anti, inner_base, inner_clauses, key, set_cap):
    return (*_where_args(base, clauses), int(link), SEMI_ANTI if anti else 0, *_where_args(inner_base, inner_clauses), int(key), int(set_cap))


def _where_in_args(base, clauses, link, anti, values, nvalues):
    return (*_where_args(base, clauses), int(link), SEMI_ANTI if anti else 0, _ptr(values), int(nvalues))


def _where_reach_args(base, clauses, link, key, seed_base, seed_clauses, seed_field, max_depth, set_cap):
    return (*_where_args(base, clauses), int(link), int(key), 0, *_where_args(seed_base, seed_clauses), int(seed_field), int(max_depth), int(set_cap))


def _where_reach_from_args(base, clauses, link, key, values, nvalues, max_depth, set_cap):
    return (*_where_args(base, clauses), int(link), int(key), 0, _ptr(values), int(nvalues), int(max_depth), int(set_cap))


def _where_join_group_args(base, clauses, link, measure, inner_base, inner_clauses, key, attr, map_cap):
    return (*_where_args(base, clauses), int(link), _field(measure), *_where_args(inner_base, inner_clauses), int(key), int(attr), int(map_cap))


def _where_map_group_args(base, clauses, link, measure, keys, vals, npairs):
    return (*_where_args(base, clauses), int(link), _field(measure), _ptr(keys), _ptr(vals), int(npairs))


def _where_join_rows_args(base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, map_cap, with_ts, inner, start, shard=None):
    return (*_where_args(base, clauses), int(link), *_fields(fields), *_where_args(inner_base, inner_clauses), int(key),
            *_fields(in_fields), int(map_cap), _jrows_flags(with_ts, inner), *_cursor(start, shard))


def _where_map_rows_args(base, clauses, link, fields, keys, node_ids, npairs, in_fields, with_ts, inner, start, shard=None):
    return (*_where_args(base, clauses), int(link), *_fields(fields), _ptr(keys), _ptr(node_ids), int(npairs),
            *_fields(in_fields), _jrows_flags(with_ts, inner), *_cursor(start, shard))


class _HostQueries(_Handle):
    """The host-memory forms, for Engine and Comm alike: self._host(name, *args) calls bmx_<name> / bmx_comm_<name> on the handle and raises on an error. Where a
    cap of None reaches one of these, it counts first (a call with cap 0 and no buffers) and then fetches with room for exactly that; Engine sizes most of its
    buffers from the index instead and so never passes None there. xres: () or (ExprRes,), what a computed-measure form reports besides."""

    def _host_aggregate(self, name, args, ngroups, xres=()):
        out = np.zeros(int(ngroups) + 1, AGG_DTYPE)
        self._host(name, *args, _ptr(out), *map(_ref, xres))
        return agg_results(out, int(ngroups))

    def _host_top(self, name, args, k):
        out = np.zeros(max(int(k), 1), TOP_DTYPE)
        m, ne = C.c_uint64(), C.c_uint64()
        self._host(name, *args, _ptr(out), _ref(m), _ref(ne))
        return out[:m.value].copy(), ne.value

    def _host_scan_where(self, args, cap, count_only):
        m = C.c_uint64()
        if cap is None or count_only:
            self._host("scan_where", *args, None, 0, _ref(m))
            if count_only:
                return m.value
            cap = m.value
        out = np.zeros(max(cap, 1), np.uint64)
        self._host("scan_where", *args, _ptr(out), cap, _ref(m))
        return out[:min(m.value, cap)].copy()

    def _host_group(self, name, args, cap, xres=(), dtype=GROUP_DTYPE, res=GroupRes):
        """a query that answers with up to cap records and a summary -> (summary, records): the arguments of its result class"""
        out, res = np.zeros(max(int(cap), 1), dtype), res()
        self._host(name, *args, _ptr(out), int(cap), _ref(res), *map(_ref, xres))
        return res, out

    def _host_quantiles(self, name, args, nq, xres=()):
        """-> (records, QuantRes)"""
        out = np.zeros(max(nq, 1), QUANT_REC_DTYPE)
        res = QuantRes()
        self._host(name, *args, _ptr(out), _ref(res), *map(_ref, xres))
        return out[:nq].copy(), res

    def _host_rows(self, args, nf, with_ts, cap):
        res = RowsRes()
        if cap is None:
            self._host("where_rows", *args, 0, None, None, None, _ref(res))
            cap = int(res.n_match)
        ids, vals, ts = _rows_buffers(nf, int(cap), with_ts)
        self._host("where_rows", *args, int(cap), _ptr(ids), _ptr(vals), _ptr(ts), _ref(res))
        return RowsResult(res, ids, vals, ts)

    def _host_group_first(self, args, nf, with_ts, cap):
        out, vals, ts = _first_buffers(nf, cap, with_ts)
        res = FirstRes()
        self._host("where_group_first", *args, cap, _ptr(out), _ptr(vals), _ptr(ts), _ref(res))
        return FirstResult(res, out, vals, ts)

    def _host_group_top(self, args, nf, with_ts, cap, per):
        ok = 1 <= per <= GTOP_MAX_PER and 1 <= cap <= GTOP_MAX_CAP and cap * per <= GTOP_MAX_ROWS        # (otherwise the library refuses: no buffers needed)
        out, rows, vals, ts = _gtop_buffers(nf, cap if ok else 1, per if ok else 1, with_ts)
        res = GtopRes()
        self._host("where_group_top", *args, cap, _ptr(out), _ptr(rows), _ptr(vals), _ptr(ts), _ref(res))
        return GroupTopResult(res, out, rows, vals, ts)

    def _host_update(self, args, cap, want_ids):
        """cap None: exactly the writable nodes the count finds (at most UPD_MAX_CAP)"""
        res = UpdRes()
        if cap is None:
            self._host("where_update", *args, 0, None, _ref(res))
            cap = min(int(res.n_match - res.n_nosrc - res.n_range), UPD_MAX_CAP)
        ids = np.zeros(max(int(cap), 1), np.uint64) if want_ids else None
        self._host("where_update", *args, int(cap), _ptr(ids), _ref(res))
        return UpdateResult(res, ids)

    def _host_semi(self, name, args, cap, count_only):
        """where_semijoin / where_in; count_only, or an overflow of the set in the counting call: no ids"""
        res = SemiRes()
        if cap is None or count_only:
            self._host(name, *args, None, 0, _ref(res))
            if count_only or res.flags & SEMI_OVERFLOW:
                return SemiResult(res, None, 0)
            cap = int(res.n_match)
        ids = np.zeros(max(int(cap), 1), np.uint64)
        self._host(name, *args, _ptr(ids), int(cap), _ref(res))
        return SemiResult(res, ids, cap)

    def _host_reach(self, name, args, cap, count_only):
        """where_reach / where_reach_from; count_only, or an overflow of the set in the counting call: no ids"""
        res = ReachRes()
        if cap is None or count_only:
            self._host(name, *args, None, None, 0, _ref(res))
            if count_only or res.flags & REACH_OVERFLOW:
                return ReachResult(res, None, None, 0)
            cap = int(res.n_match)
        ids, depth = np.zeros(max(int(cap), 1), np.uint64), np.zeros(max(int(cap), 1), np.uint8)
        self._host(name, *args, _ptr(ids), _ptr(depth), int(cap), _ref(res))
        return ReachResult(res, ids, depth, cap)

    def _host_jrows(self, name, args, nf, nif, with_ts, cap):
        """where_join_rows / where_map_rows: args, cap, the six outputs, res -> JoinRowsResult"""
        res = JoinRowsRes()
        if cap is None:
            self._host(name, *args, 0, None, None, None, None, None, None, _ref(res))
            cap = int(res.n_match)
        cap = int(cap)
        ids, vals, ts = _rows_buffers(nf, cap, with_ts)
        in_ids, in_vals, in_ts = _rows_buffers(nif, cap, with_ts)
        self._host(name, *args, cap, _ptr(ids), _ptr(vals), _ptr(ts), _ptr(in_ids), _ptr(in_vals), _ptr(in_ts), _ref(res))
        return JoinRowsResult(res, ids, vals, ts, in_ids, in_vals, in_ts)

    def _host_watch_poll(self, w, cap_entered, cap_left):
        """a cap of None: the poll counts first (caps of 0: it commits only if nothing changed) and then fetches with room for exactly that"""
        res = WatchRes()
        if cap_entered is None or cap_left is None:
            self._host("watch_poll", int(w), None, 0, None, 0, _ref(res))
            if not res.flags & WATCH_OVERFLOW:
                return WatchPoll(res, np.zeros(0, np.uint64), np.zeros(0, np.uint64))
            cap_entered = int(res.n_entered) if cap_entered is None else cap_entered
            cap_left = int(res.n_left) if cap_left is None else cap_left
        ent, lft = np.zeros(max(int(cap_entered), 1), np.uint64), np.zeros(max(int(cap_left), 1), np.uint64)
        self._host("watch_poll", int(w), _ptr(ent), int(cap_entered), _ptr(lft), int(cap_left), _ref(res))
        return WatchPoll(res, ent[:int(cap_entered)], lft[:int(cap_left)])
