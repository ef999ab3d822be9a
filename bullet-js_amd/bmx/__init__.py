"""bmx — ctypes binding of libbmx.so (include/bmx.h), the MI355X CRDT-merge / index-scan engine.

This is the Python-side driver used by tests and bench.py. The product surface is the C ABI and the
N-API/JS host (bullet-js_amd/js); nothing here computes anything on the CPU: every call goes to the
HIP library and raises BmxError if it (or a GPU) is missing.
"""
import ctypes as C
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("BMX_LIB_PATH") or os.path.join(_PKG, "libbmx.so")   # the override exists for A/B measurements of two builds

OK = 0
ERR_INVALID, ERR_HIP, ERR_FULL, ERR_NOMEM, ERR_RANGE, ERR_INTERNAL, ERR_NO_DEVICE, ERR_NO_INDEX, ERR_OVERFLOW = -1, -2, -3, -4, -5, -6, -7, -8, -9
MEM_HOST, MEM_DEVICE = 0, 1
INSERT_REFERENCE, INSERT_DELTA = 0, 1
VAL_DELETED = -(1 << 63)   # BMX_VAL_DELETED: tombstone value of bmx_put_rows
MERGE_MARK_CREATED, APPLIED_CREATED, APPLIED_INDEX = 0x1000, 0x80000000, 0x00FFFFFF
MERGE_UNIQUE_KEYS = 0x100
MERGE_STRICT_FLAGS = 0x200
CTX_FIXED_CAPACITY = 2
FLAG_INCOMING, FLAG_CURRENT, FLAG_HISTORICAL = 1, 2, 4
MAX_BATCH = 1 << 24
AGG_NO_FIELD, AGG_MAX_GROUPS = 0xFFFFFFFF, 65536   # BMX_AGG_NO_FIELD ("no measure" / "no grouping"), BMX_AGG_MAX_GROUPS (bmx_scan_aggregate)
TOP_DESC, TOP_MAX_K = 1, 4096   # BMX_TOP_DESC, BMX_TOP_MAX_K (bmx_top.h bmx_scan_top)
LIT_NOT, WHERE_MAX_CLAUSES, WHERE_MAX_LITS, WHERE_MAX_FIELDS = 1, 8, 32, 8   # BMX_LIT_NOT and the limits of one program (bmx_where.h bmx_scan_where)
LIT_MINUS, LIT_SUBTRAHEND = 4, 8     # BMX_LIT_MINUS / BMX_LIT_SUBTRAHEND: the two entries of a field-to-field literal, lo <= a - b <= hi
LIT_CLOCK, LIT_CLOCK_TOMB = 16, 32   # BMX_LIT_CLOCK / BMX_LIT_CLOCK_TOMB: the literal ranges over the row's clock; a row that holds data / a tombstoned row qualifies
GROUP_OVERFLOW, GROUP_MAX_CAP = 1, 1 << 20   # BMX_GROUP_OVERFLOW (flags of bmx_group_res), BMX_GROUP_MAX_CAP (bmx_group.h bmx_where_group)
ROWS_MAX_FIELDS, ROWS_TS, ROWS_NO_CLOCK = 8, 1, -1   # BMX_ROWS_MAX_FIELDS, BMX_ROWS_TS (flags), BMX_ROWS_NO_CLOCK (the clock of an absent cell) (bmx_rows.h bmx_where_rows)
JOIN_MAP_OVERFLOW, JOIN_GROUP_OVERFLOW, JOIN_MAX_MAP = 1, 2, 1 << 20   # BMX_JOIN_MAP_OVERFLOW, BMX_JOIN_GROUP_OVERFLOW (flags of bmx_join_res), BMX_JOIN_MAX_MAP (bmx_join.h bmx_where_join_group)
SEMI_ANTI, SEMI_OVERFLOW, SEMI_MAX_SET = 1, 1, 1 << 20   # BMX_SEMI_ANTI (flags of the call), BMX_SEMI_OVERFLOW (flags of bmx_semi_res), BMX_SEMI_MAX_SET (bmx_semi.h bmx_where_semijoin)
QUANT_MAX, QUANT_MAX_DEN = 8, 1 << 20   # BMX_QUANT_MAX (quantiles per call), BMX_QUANT_MAX_DEN (the largest denominator) (bmx_quant.h bmx_where_quantiles)
WATCH_MAX, WATCH_RESET, WATCH_OVERFLOW = 16, 1, 2  # BMX_WATCH_MAX (live watches per context) and the flags of bmx_watch_res (bmx_watch.h bmx_watch_poll)
SYNC_TOMBSTONES, EXPORT_ONLY_TOMBSTONES = 1, 2   # BMX_SYNC_TOMBSTONES (bmx_digest), BMX_EXPORT_ONLY_TOMBSTONES (bmx_export_rows)

JROWS_INNER, JROWS_NO_NODE = 2, (1 << 64) - 1   # BMX_JROWS_INNER (flags, next to ROWS_TS), BMX_JROWS_NO_NODE (out_in_ids of a row without inner node) (bmx_join_rows.h bmx_where_join_rows)
EXPORTS = [
    "bmx_create", "bmx_create_ex", "bmx_destroy", "bmx_last_error", "bmx_abi_version", "bmx_selfcheck", "bmx_set_deferred_compaction", "bmx_set_side_stream", "bmx_set_wait_limit", "bmx_merge_fence", "bmx_get_deferred_counts", "bmx_get_info", "bmx_get_placement", "bmx_set_probe_waves", "bmx_sync", "bmx_set_stream", "bmx_get_stream", "bmx_seq_signal", "bmx_seq_wait",
    "bmx_load_rows", "bmx_put_rows", "bmx_merge_batch", "bmx_merge_submit", "bmx_merge_collect", "bmx_host_alloc", "bmx_host_free", "bmx_merge_records", "bmx_get_rows", "bmx_get_row", "bmx_dump_rows", "bmx_row_count", "bmx_reserve",
    "bmx_index_build", "bmx_index_drop", "bmx_index_size", "bmx_index_refresh_counts", "bmx_index_set_ordered", "bmx_index_ordered_info", "bmx_index_ordered_stats", "bmx_scan_range", "bmx_scan_equals", "bmx_scan_count", "bmx_scan_filter", "bmx_scan_range_pos", "bmx_index_ids",
    "bmx_owner_of", "bmx_partition_by_owner", "bmx_partition_by_owner_slabs", "bmx_partition_scatter", "bmx_merge_records_after", "bmx_ipc_alloc", "bmx_ipc_open", "bmx_ipc_close", "bmx_ipc_free", "bmx_seq_wait_all", "bmx_merge_tail_wait", "bmx_merge_notify", "bmx_timer_start", "bmx_timer_stop", "bmx_timer_mark", "bmx_timer_elapsed", "bmx_profile_enable", "bmx_profile_read", "bmx_profile_read_scan",
    "bmx_comm_create", "bmx_comm_destroy", "bmx_comm_last_error", "bmx_comm_nshards", "bmx_comm_shard", "bmx_comm_sync", "bmx_comm_load_rows", "bmx_comm_put_rows", "bmx_comm_merge",
    "bmx_comm_merge_dev", "bmx_comm_shard_result", "bmx_comm_row_count", "bmx_comm_get_rows", "bmx_comm_dump_rows", "bmx_comm_index_build", "bmx_comm_index_set_ordered",
    "bmx_comm_scan_range", "bmx_comm_scan_equals", "bmx_comm_scan_count", "bmx_comm_scan_filter",
    "bmx_vc_create", "bmx_vc_destroy", "bmx_vc_last_error", "bmx_vc_load_rows", "bmx_vc_merge_batch", "bmx_vc_get_rows", "bmx_vc_row_count", "bmx_vc_scan_range", "bmx_vc_merge_batch_dev", "bmx_vc_set_stream", "bmx_vc_sync",
    "bmx_vc_load_rows_ks", "bmx_vc_merge_batch_ks", "bmx_vc_get_rows_ks", "bmx_vc_merge_batch_ks_dev", "bmx_vc_keyset", "bmx_vc_keyset_dense",
    "bmx_key_bucket", "bmx_digest", "bmx_export_rows", "bmx_comm_digest", "bmx_comm_export_rows",
    "bmx_scan_aggregate", "bmx_comm_scan_aggregate",
]

# include/bmx_top.h: additions to the ABI that bmx.h does not declare
EXPORTS_TOP = ["bmx_scan_top", "bmx_comm_scan_top"]

# include/bmx_vc_sync.h: replica reconciliation of the vector-clock table, likewise
EXPORTS_VC_SYNC = ["bmx_vc_rec_digest", "bmx_vc_info", "bmx_vc_digest", "bmx_vc_frontier", "bmx_vc_export_rows", "bmx_vc_merge_records"]

# include/bmx_where.h: boolean filters, likewise
EXPORTS_WHERE = ["bmx_scan_where", "bmx_comm_scan_where"]

# include/bmx_watch.h: standing queries, likewise
EXPORTS_WATCH = ["bmx_watch_create", "bmx_watch_poll", "bmx_watch_destroy", "bmx_comm_watch_create", "bmx_comm_watch_poll", "bmx_comm_watch_destroy"]

# include/bmx_where_agg.h: aggregates and top-k over boolean filters, likewise
EXPORTS_WHERE_AGG = ["bmx_where_aggregate", "bmx_where_top", "bmx_comm_where_aggregate", "bmx_comm_where_top"]

# include/bmx_group.h: group-by over discovered values, likewise
EXPORTS_GROUP = ["bmx_where_group", "bmx_comm_where_group"]

# include/bmx_rows.h: row projection, likewise
EXPORTS_ROWS = ["bmx_where_rows", "bmx_comm_where_rows"]

# include/bmx_semi.h: semi-joins, likewise
EXPORTS_SEMI = ["bmx_where_semijoin", "bmx_where_in", "bmx_comm_where_semijoin", "bmx_comm_where_in"]
# include/bmx_join.h: lookup joins, likewise
EXPORTS_JOIN = ["bmx_where_join_group", "bmx_where_map_group", "bmx_comm_where_join_group", "bmx_comm_where_map_group"]
# include/bmx_quant.h: exact quantiles over boolean filters, likewise
# join projection (include/bmx_join_rows.h); a list of its own for the same reason
EXPORTS_JOIN_ROWS = ["bmx_where_join_rows", "bmx_where_map_rows", "bmx_comm_where_join_rows", "bmx_comm_where_map_rows"]
EXPORTS_QUANT = ["bmx_where_quantiles", "bmx_comm_where_quantiles"]
# the probe kernel's claim mode (include/bmx_claim.h), likewise
EXPORTS_CLAIM = ["bmx_selfcheck_claim", "bmx_get_claim_mode"]
# update and delete by query (include/bmx_update.h), likewise
EXPORTS_UPDATE = ["bmx_where_update", "bmx_comm_where_update"]
# group-by over several fields (include/bmx_group_multi.h), likewise
EXPORTS_GROUP_MULTI = ["bmx_where_group_multi", "bmx_comm_where_group_multi"]
# graph traversal (include/bmx_reach.h), likewise
EXPORTS_REACH = ["bmx_where_reach", "bmx_where_reach_from", "bmx_comm_where_reach", "bmx_comm_where_reach_from"]
REACH_OVERFLOW, REACH_MORE, REACH_MAX_SET, REACH_MAX_DEPTH = 1, 2, 1 << 20, 255   # BMX_REACH_OVERFLOW, BMX_REACH_MORE (flags of bmx_reach_res), BMX_REACH_MAX_SET, BMX_REACH_MAX_DEPTH (bmx_reach.h bmx_where_reach)
# the first node per group (include/bmx_first.h), likewise
EXPORTS_FIRST = ["bmx_where_group_first", "bmx_comm_where_group_first"]
FIRST_DESC, FIRST_OVERFLOW, FIRST_NO_NODE, FIRST_MAX_CAP = 2, 1, (1 << 64) - 1, 1 << 20   # BMX_FIRST_DESC (flags of the call, next to ROWS_TS), BMX_FIRST_OVERFLOW (flags of bmx_first_res), BMX_FIRST_NO_NODE, BMX_FIRST_MAX_CAP (bmx_first.h bmx_where_group_first)
# the first N nodes per group (include/bmx_group_top.h), likewise
EXPORTS_GROUP_TOP = ["bmx_where_group_top", "bmx_comm_where_group_top"]
GTOP_DESC, GTOP_OVERFLOW, GTOP_NO_NODE, GTOP_MAX_CAP, GTOP_MAX_PER, GTOP_MAX_ROWS = 2, 1, (1 << 64) - 1, 1 << 20, 16, 1 << 22   # BMX_GTOP_DESC (flags of the call, next to ROWS_TS), BMX_GTOP_OVERFLOW (flags of bmx_gtop_res), BMX_GTOP_NO_NODE, BMX_GTOP_MAX_CAP, BMX_GTOP_MAX_PER, BMX_GTOP_MAX_ROWS (bmx_group_top.h bmx_where_group_top)
# computed measures (include/bmx_expr.h), likewise
EXPORTS_EXPR = ["bmx_where_aggregate_expr", "bmx_where_group_expr", "bmx_where_quantiles_expr", "bmx_comm_where_aggregate_expr", "bmx_comm_where_group_expr",
                "bmx_comm_where_quantiles_expr"]
EXPR_ADD, EXPR_SUB, EXPR_MUL = 1, 2, 3   # BMX_EXPR_ADD, BMX_EXPR_SUB, BMX_EXPR_MUL (bmx_expr.h)
MGROUP_MAX_KEYS, MGROUP_MAX_CAP4 = 4, 1 << 14  # BMX_MGROUP_MAX_KEYS, BMX_MGROUP_MAX_CAP4 (bmx_group_multi.h bmx_where_group_multi)
UPD_SET, UPD_DELETE, UPD_COPY, UPD_ADD, UPD_FORCE, UPD_MAX_CAP = 0, 1, 2, 3, 1, 1 << 24   # the ops, BMX_UPD_FORCE (flags), BMX_UPD_MAX_CAP (bmx_update.h bmx_where_update)


class BmxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bmx error %d: %s" % (code, msg))
        self.code = code


class MergeStats(C.Structure):
    _fields_ = [("n_applied", C.c_uint64), ("n_conflicts", C.c_uint64), ("n_rows", C.c_uint64), ("reserved", C.c_uint64)]


class Term(C.Structure):
    _fields_ = [("field", C.c_uint32), ("reserved", C.c_uint32), ("lo", C.c_int64), ("hi", C.c_int64)]


class Agg(C.Structure):
    """bmx_agg: one record of bmx_scan_aggregate (48 bytes); the sum is a two's-complement 128-bit number in two words"""
    _fields_ = [("n_match", C.c_uint64), ("n", C.c_uint64), ("min", C.c_int64), ("max", C.c_int64), ("sum_lo", C.c_uint64), ("sum_hi", C.c_int64)]


AGG_DTYPE = np.dtype([("n_match", "<u8"), ("n", "<u8"), ("min", "<i8"), ("max", "<i8"), ("sum_lo", "<u8"), ("sum_hi", "<i8")])


class AggResult:
    """One group's aggregate: n_match nodes satisfy every term, n of them hold the measure; sum (a Python int, exact), min and max are over those n
    (min and max are None when nothing was measured: n == 0, or no measure field)."""
    __slots__ = ("n_match", "n", "min", "max", "sum")

    def __init__(self, rec):
        self.n_match = int(rec["n_match"]); self.n = int(rec["n"])
        self.sum = (int(rec["sum_hi"]) << 64) + int(rec["sum_lo"])
        measured = self.n and int(rec["min"]) <= int(rec["max"])      # (without a measure field n == n_match and min / max keep their empty values)
        self.min = int(rec["min"]) if measured else None
        self.max = int(rec["max"]) if measured else None

    def __eq__(self, o):
        return isinstance(o, AggResult) and all(getattr(self, k) == getattr(o, k) for k in self.__slots__)

    def __repr__(self):
        return "AggResult(n_match=%d, n=%d, min=%r, max=%r, sum=%d)" % (self.n_match, self.n, self.min, self.max, self.sum)


def agg_results(recs, ngroups):
    """records of one bmx_scan_aggregate call (AGG_DTYPE) -> one AggResult (ngroups == 0) or the list of ngroups + 1"""
    return AggResult(recs[0]) if not ngroups else [AggResult(r) for r in recs[:ngroups + 1]]


def _agg_args(terms, measure, group, group_lo, ngroups):
    arr = (Term * max(len(terms), 1))(*[Term(int(f), 0, int(lo), int(hi)) for f, lo, hi in terms])
    return (len(terms), arr, AGG_NO_FIELD if measure is None else int(measure), AGG_NO_FIELD if group is None else int(group), int(group_lo), int(ngroups))


class TopRec(C.Structure):
    """bmx_top_rec: one record of bmx_scan_top (16 bytes), also its cursor"""
    _fields_ = [("id", C.c_uint64), ("val", C.c_int64)]


TOP_DTYPE = np.dtype([("id", "<u8"), ("val", "<i8")])


def _top_args(terms, k, desc, after):
    arr = (Term * max(len(terms), 1))(*[Term(int(f), 0, int(lo), int(hi)) for f, lo, hi in terms])
    cur = None
    if after is not None:
        cur = TopRec(int(after["id"]), int(after["val"])) if isinstance(after, (np.void, dict)) else TopRec(int(after[0]), int(after[1]))
    return (len(terms), arr, TOP_DESC if desc else 0, C.byref(cur) if cur is not None else None, int(k))


def top_merge(lists, k, desc=False):
    """The merge bmx_comm_scan_top does with its shards' answers: `lists` are record arrays (TOP_DTYPE), each ordered by (val, id) — val descending with
    desc, id ascending either way; -> the first k records of their union in that order. Pure numpy: no library, no GPU."""
    parts = [np.asarray(x, TOP_DTYPE) for x in lists if len(x)]
    if not parts:
        return np.zeros(0, TOP_DTYPE)
    a = np.concatenate(parts)
    order = np.lexsort((a["id"], -a["val"] if desc else a["val"]))     # (|val| <= 2^53 - 1: the negation is exact)
    return a[order[:int(k)]]


class Lit(C.Structure):
    """bmx_lit: one literal of a bmx_scan_where program (24 bytes, the layout of bmx_term); flags: LIT_NOT, LIT_MINUS, LIT_SUBTRAHEND,
    LIT_CLOCK, LIT_CLOCK_TOMB"""
    _fields_ = [("field", C.c_uint32), ("flags", C.c_uint32), ("lo", C.c_int64), ("hi", C.c_int64)]


def _where_agg_tail(measure, group, group_lo, ngroups):
    return (AGG_NO_FIELD if measure is None else int(measure), AGG_NO_FIELD if group is None else int(group), int(group_lo), int(ngroups))


def _where_top_tail(k, desc, after):
    return _top_args([], k, desc, after)[2:]          # (flags, cursor, k)


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


GROUP_DTYPE = np.dtype([("key", "<i8"), ("agg", AGG_DTYPE)])      # bmx_group_rec: one record of bmx_where_group (56 bytes)


class GroupRes(C.Structure):
    """bmx_group_res: what one bmx_where_group found besides its records (112 bytes); flags: GROUP_OVERFLOW"""
    _fields_ = [("n_groups", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("absent", Agg), ("total", Agg)]


GROUP_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("flags", "<u4"), ("reserved", "<u4"), ("absent", AGG_DTYPE), ("total", AGG_DTYPE)])


class GroupResult:
    """One where_group answer: groups = {key: AggResult} in ascending key order (empty on overflow), records (GROUP_DTYPE, sorted by key), n_groups (the
    number of distinct keys, or on overflow a lower bound of it above cap), overflow, absent (selected nodes without a group value) and total (every
    selected node) as AggResult."""
    __slots__ = ("records", "groups", "n_groups", "overflow", "absent", "total")

    def __init__(self, res, recs):
        r = np.frombuffer(bytes(res), GROUP_RES_DTYPE)[0] if isinstance(res, GroupRes) else res
        self.n_groups = int(r["n_groups"]); self.overflow = bool(int(r["flags"]) & GROUP_OVERFLOW)
        self.absent, self.total = AggResult(r["absent"]), AggResult(r["total"])
        self.records = recs[:0 if self.overflow else self.n_groups].copy()
        self.groups = {int(x["key"]): AggResult(x["agg"]) for x in self.records}

    def __repr__(self):
        return "GroupResult(%d groups%s, absent=%r, total=%r)" % (self.n_groups, ", overflow" if self.overflow else "", self.absent, self.total)


def _group_fold(o, p):
    """o += p for one record of AGG_DTYPE (0-d views): counts and 128-bit sums add, minima and maxima fold"""
    o["n_match"] += p["n_match"]; o["n"] += p["n"]
    o["min"] = min(int(o["min"]), int(p["min"])); o["max"] = max(int(o["max"]), int(p["max"]))
    s = ((int(o["sum_hi"]) << 64) + int(o["sum_lo"]) + (int(p["sum_hi"]) << 64) + int(p["sum_lo"])) & ((1 << 128) - 1)
    o["sum_lo"] = s & ((1 << 64) - 1)
    hi = s >> 64
    o["sum_hi"] = hi - (1 << 64) if hi >= (1 << 63) else hi


def group_merge(lists):
    """The merge bmx_comm_where_group does with its shards' answers: `lists` are record arrays (GROUP_DTYPE), each with distinct keys; -> one array sorted
    ascending by key, the records of equal keys folded (counts and 128-bit sums add, minima and maxima fold). Pure numpy: no library, no GPU."""
    parts = [np.asarray(x, GROUP_DTYPE) for x in lists if len(x)]
    if not parts:
        return np.zeros(0, GROUP_DTYPE)
    a = np.concatenate(parts)
    a = a[np.argsort(a["key"], kind="stable")]
    first = np.ones(len(a), bool); first[1:] = a["key"][1:] != a["key"][:-1]
    out = a[first].copy()
    at = np.cumsum(first) - 1
    for i in np.nonzero(~first)[0]:
        _group_fold(out[at[i]]["agg"], a[i]["agg"])
    return out


def _group_tail(measure, group):
    return (AGG_NO_FIELD if measure is None else int(measure), AGG_NO_FIELD if group is None else int(group))


MGROUP_DTYPE = np.dtype([("key", "<i8", (4,)), ("agg", AGG_DTYPE)])      # bmx_mgroup_rec: one record of bmx_where_group_multi (80 bytes)


class GroupKey(C.Structure):
    """bmx_group_key: one key of bmx_where_group_multi (24 bytes): floor((value(field) - origin) / width)"""
    _fields_ = [("field", C.c_uint32), ("flags", C.c_uint32), ("origin", C.c_int64), ("width", C.c_int64)]


def _mgroup_keys(keys):
    """keys: a list of field or (field, origin, width) -> (nkeys, bmx_group_key array)"""
    ks = [(k, 0, 1) if isinstance(k, (int, np.integer)) else k for k in keys]
    return (len(ks), (GroupKey * max(len(ks), 1))(*[GroupKey(int(f), 0, int(o), int(w)) for f, o, w in ks]))


def mgroup_sort(recs):
    """records (MGROUP_DTYPE) in the order of a host-mode answer: lexicographic by (key[0], key[1], key[2], key[3]), each signed ascending"""
    recs = np.asarray(recs, MGROUP_DTYPE)
    k = recs["key"]
    return recs[np.lexsort((k[:, 3], k[:, 2], k[:, 1], k[:, 0]))]


class MultiGroupResult:
    """One where_group_multi answer: groups = {key tuple (nkeys ints): AggResult} in the records' sorted order (empty on overflow), records (MGROUP_DTYPE,
    sorted lexicographically by key), n_groups (the number of distinct tuples, or on overflow a lower bound of it above cap), overflow, absent (selected nodes
    that lack any of the keys) and total (every selected node) as AggResult."""
    __slots__ = ("records", "groups", "n_groups", "overflow", "absent", "total")

    def __init__(self, res, recs, nkeys):
        r = np.frombuffer(bytes(res), GROUP_RES_DTYPE)[0] if isinstance(res, GroupRes) else res
        self.n_groups = int(r["n_groups"]); self.overflow = bool(int(r["flags"]) & GROUP_OVERFLOW)
        self.absent, self.total = AggResult(r["absent"]), AggResult(r["total"])
        self.records = recs[:0 if self.overflow else self.n_groups].copy()
        self.groups = {tuple(int(v) for v in x["key"][:nkeys]): AggResult(x["agg"]) for x in self.records}

    def __repr__(self):
        return "MultiGroupResult(%d groups%s, absent=%r, total=%r)" % (self.n_groups, ", overflow" if self.overflow else "", self.absent, self.total)


def mgroup_merge(lists):
    """The merge bmx_comm_where_group_multi does with its shards' answers: `lists` are record arrays (MGROUP_DTYPE), each with distinct tuples; -> one array
    sorted lexicographically by key, the records of equal tuples folded (counts and 128-bit sums add, minima and maxima fold). Pure numpy: no library, no GPU."""
    parts = [np.asarray(x, MGROUP_DTYPE) for x in lists if len(x)]
    if not parts:
        return np.zeros(0, MGROUP_DTYPE)
    a = mgroup_sort(np.concatenate(parts))
    first = np.ones(len(a), bool); first[1:] = (a["key"][1:] != a["key"][:-1]).any(axis=1)
    out = a[first].copy()
    at = np.cumsum(first) - 1
    for i in np.nonzero(~first)[0]:
        _group_fold(out[at[i]]["agg"], a[i]["agg"])
    return out


class RowsRes(C.Structure):
    """bmx_rows_res: what one bmx_where_rows found besides its rows (40 bytes)"""
    _fields_ = [("n_match", C.c_uint64), ("n_out", C.c_uint64), ("next_pos", C.c_uint64), ("layout", C.c_uint64), ("next_shard", C.c_uint32), ("reserved", C.c_uint32)]


ROWS_RES_DTYPE = np.dtype([("n_match", "<u8"), ("n_out", "<u8"), ("next_pos", "<u8"), ("layout", "<u8"), ("next_shard", "<u4"), ("reserved", "<u4")])


class RowsResult:
    """One where_rows answer: ids (uint64, n_out of them, in index order of the base field), vals (int64, shape (nfields, n_out); VAL_DELETED in a cell
    without data), ts (the clocks, same shape; ROWS_NO_CLOCK in an absent cell; None without with_ts), n_match (the selected nodes at or behind the cursor),
    next_pos (and next_shard: the cursor of the next page) and layout (the cursor is good while this stays the same)."""
    __slots__ = ("ids", "vals", "ts", "n_match", "n_out", "next_pos", "next_shard", "layout")

    def __init__(self, res, ids, vals, ts):
        r = np.frombuffer(bytes(res), ROWS_RES_DTYPE)[0] if isinstance(res, RowsRes) else res
        self.n_match, self.n_out, self.next_pos, self.layout, self.next_shard = int(r["n_match"]), int(r["n_out"]), int(r["next_pos"]), int(r["layout"]), int(r["next_shard"])
        self.ids = ids[:self.n_out].copy()
        self.vals = vals[:, :self.n_out].copy()
        self.ts = None if ts is None else ts[:, :self.n_out].copy()

    def __repr__(self):
        return "RowsResult(%d of %d rows, %d fields, next_pos=%d)" % (self.n_out, self.n_match, self.vals.shape[0], self.next_pos)


def _rows_fields(fields, with_ts):
    """-> (nfields, fields, flags) of bmx_where_rows"""
    fields = [int(f) for f in fields]
    return (len(fields), (C.c_uint32 * max(len(fields), 1))(*fields), ROWS_TS if with_ts else 0)


def _rows_buffers(nfields, cap, with_ts):
    return np.zeros(max(cap, 1), np.uint64), np.zeros((nfields, max(cap, 1)), np.int64), np.zeros((nfields, max(cap, 1)), np.int64) if with_ts else None


class FirstRec(C.Structure):
    """bmx_first_rec: one record of bmx_where_group_first (40 bytes): the group value, its first node and that node's order value, the members, the contenders"""
    _fields_ = [("key", C.c_int64), ("id", C.c_uint64), ("val", C.c_int64), ("n_match", C.c_uint64), ("n", C.c_uint64)]


class FirstRes(C.Structure):
    """bmx_first_res: what one bmx_where_group_first found besides its records (40 bytes); flags: FIRST_OVERFLOW"""
    _fields_ = [("n_groups", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("total", C.c_uint64), ("absent", C.c_uint64), ("n_ordered", C.c_uint64)]


FIRST_DTYPE = np.dtype([("key", "<i8"), ("id", "<u8"), ("val", "<i8"), ("n_match", "<u8"), ("n", "<u8")])
FIRST_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("flags", "<u4"), ("reserved", "<u4"), ("total", "<u8"), ("absent", "<u8"), ("n_ordered", "<u8")])


class FirstResult:
    """One where_group_first answer: records (FIRST_DTYPE, sorted by key; none on overflow), vals (int64, shape (nfields, n_groups): the cells of each record's
    node; VAL_DELETED in a cell without data), ts (the clocks, same shape; ROWS_NO_CLOCK in an absent cell; None without with_ts), first = {key: id or None},
    n_groups (the number of distinct group values, or on overflow a lower bound of it above cap), overflow, total (every selected node), absent (those without
    a group value) and n_ordered (the contenders of all groups)."""
    __slots__ = ("records", "vals", "ts", "first", "n_groups", "overflow", "total", "absent", "n_ordered")

    def __init__(self, res, recs, vals, ts):
        r = np.frombuffer(bytes(res), FIRST_RES_DTYPE)[0] if isinstance(res, FirstRes) else res
        self.n_groups = int(r["n_groups"]); self.overflow = bool(int(r["flags"]) & FIRST_OVERFLOW)
        self.total, self.absent, self.n_ordered = int(r["total"]), int(r["absent"]), int(r["n_ordered"])
        m = 0 if self.overflow else self.n_groups
        self.records = recs[:m].copy()
        self.vals = vals[:, :m].copy()
        self.ts = None if ts is None else ts[:, :m].copy()
        self.first = {int(x["key"]): (int(x["id"]) if int(x["n"]) else None) for x in self.records}

    def __repr__(self):
        return "FirstResult(%d groups%s, total=%d, absent=%d, n_ordered=%d)" % (self.n_groups, ", overflow" if self.overflow else "", self.total, self.absent, self.n_ordered)


def _first_tail(group, order, fields, desc, with_ts):
    """-> (group_field, order_field, nfields, fields, flags) of bmx_where_group_first"""
    nf, farr, flags = _rows_fields(fields, with_ts)
    return (int(group), int(order), nf, farr, flags | (FIRST_DESC if desc else 0))


def _first_buffers(nfields, cap, with_ts):
    return np.zeros(max(cap, 1), FIRST_DTYPE), np.zeros((nfields, max(cap, 1)), np.int64), np.zeros((nfields, max(cap, 1)), np.int64) if with_ts else None


def first_merge(lists, desc=False):
    """The merge bmx_comm_where_group_first does with its shards' answers. `lists`: per shard (records, vals, ts) — records FIRST_DTYPE with distinct keys, vals
    and ts of shape (nfields, len(records)) (ts may be None) — -> (records sorted ascending by key, vals, ts): n_match and n of equal keys add; the better
    (val, id) under the order — val ascending, or descending with desc, then id ascending as an unsigned number — wins and brings ITS shard's cells; a
    record without a contender never beats one with. Pure Python and numpy: no library, no GPU."""
    best = {}
    for recs, vals, ts in lists:
        recs = np.asarray(recs, FIRST_DTYPE)
        for i in range(len(recs)):
            x = recs[i]
            cells = (None if vals is None else [int(v) for v in np.asarray(vals)[:, i]], None if ts is None else [int(v) for v in np.asarray(ts)[:, i]])
            cur = [int(x["key"]), int(x["id"]), int(x["val"]), int(x["n_match"]), int(x["n"]), cells]
            old = best.get(cur[0])
            if old is None:
                best[cur[0]] = cur
                continue
            nm, n = old[3] + cur[3], old[4] + cur[4]
            better = cur[4] and (not old[4] or ((cur[2] > old[2] if desc else cur[2] < old[2]) if cur[2] != old[2] else cur[1] < old[1]))
            win = cur if better else old
            win[3], win[4] = nm, n
            best[cur[0]] = win
    keys = sorted(best)
    out = np.zeros(len(keys), FIRST_DTYPE)
    nf = max([0] + [len(b[5][0]) for b in best.values() if b[5][0] is not None])
    have_ts = any(b[5][1] is not None for b in best.values())
    ovals = np.zeros((nf, len(keys)), np.int64)
    ots = np.zeros((nf, len(keys)), np.int64) if have_ts else None
    for i, k in enumerate(keys):
        b = best[k]
        out[i] = (b[0], b[1], b[2], b[3], b[4])
        if nf:
            ovals[:, i] = b[5][0]
            if have_ts:
                ots[:, i] = b[5][1]
    return out, ovals, ots


class GtopGrp(C.Structure):
    """bmx_gtop_grp: one group of bmx_where_group_top (32 bytes): the group value, the members, the contenders, the rows that carry a node"""
    _fields_ = [("key", C.c_int64), ("n_match", C.c_uint64), ("n", C.c_uint64), ("n_rows", C.c_uint64)]


class GtopRow(C.Structure):
    """bmx_gtop_row: one row of a group (16 bytes): the node and its order value; GTOP_NO_NODE and VAL_DELETED behind the group's last row"""
    _fields_ = [("id", C.c_uint64), ("val", C.c_int64)]


class GtopRes(C.Structure):
    """bmx_gtop_res: what one bmx_where_group_top found besides its groups (48 bytes); flags: GTOP_OVERFLOW"""
    _fields_ = [("n_groups", C.c_uint64), ("flags", C.c_uint32), ("per", C.c_uint32), ("total", C.c_uint64), ("absent", C.c_uint64), ("n_ordered", C.c_uint64),
                ("n_rows", C.c_uint64)]


GTOP_GRP_DTYPE = np.dtype([("key", "<i8"), ("n_match", "<u8"), ("n", "<u8"), ("n_rows", "<u8")])
GTOP_ROW_DTYPE = np.dtype([("id", "<u8"), ("val", "<i8")])
GTOP_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("flags", "<u4"), ("per", "<u4"), ("total", "<u8"), ("absent", "<u8"), ("n_ordered", "<u8"), ("n_rows", "<u8")])


class GroupTopResult:
    """One where_group_top answer: groups (GTOP_GRP_DTYPE, sorted by key; none on overflow), rows (GTOP_ROW_DTYPE, shape (n_groups, per): each group's first
    contenders in order, padded with (GTOP_NO_NODE, VAL_DELETED)), vals (int64, shape (nfields, n_groups, per): the cells of each row's node; VAL_DELETED in a
    cell without data), ts (the clocks, same shape; ROWS_NO_CLOCK in an absent cell; None without with_ts), top = {key: [ids in order]}, per, n_groups (the
    number of distinct group values, or on overflow a lower bound of it above cap), overflow, total (every selected node), absent (those without a group
    value), n_ordered (the contenders of all groups) and n_rows (the rows that carry a node)."""
    __slots__ = ("groups", "rows", "vals", "ts", "top", "per", "n_groups", "overflow", "total", "absent", "n_ordered", "n_rows")

    def __init__(self, res, groups, rows, vals, ts):
        r = np.frombuffer(bytes(res), GTOP_RES_DTYPE)[0] if isinstance(res, GtopRes) else res
        self.n_groups = int(r["n_groups"]); self.overflow = bool(int(r["flags"]) & GTOP_OVERFLOW); self.per = int(r["per"])
        self.total, self.absent, self.n_ordered, self.n_rows = int(r["total"]), int(r["absent"]), int(r["n_ordered"]), int(r["n_rows"])
        m, per = 0 if self.overflow else self.n_groups, self.per
        nf = vals.shape[0]
        self.groups = groups[:m].copy()
        self.rows = rows.reshape(-1)[:m * per].reshape(m, per).copy()
        self.vals = vals[:, :m * per].reshape(nf, m, per).copy()
        self.ts = None if ts is None else ts[:, :m * per].reshape(nf, m, per).copy()
        self.top = {int(g["key"]): [int(x) for x in self.rows[i]["id"][:int(g["n_rows"])]] for i, g in enumerate(self.groups)}

    def __repr__(self):
        return "GroupTopResult(%d groups%s, per=%d, n_rows=%d, total=%d, absent=%d, n_ordered=%d)" % (
            self.n_groups, ", overflow" if self.overflow else "", self.per, self.n_rows, self.total, self.absent, self.n_ordered)


def _gtop_tail(group, order, per, fields, desc, with_ts):
    """-> (group_field, order_field, per, nfields, fields, flags) of bmx_where_group_top"""
    nf, farr, flags = _rows_fields(fields, with_ts)
    return (int(group), int(order), int(per), nf, farr, flags | (GTOP_DESC if desc else 0))


def _gtop_buffers(nfields, cap, per, with_ts):
    rows = max(cap * per, 1)
    return (np.zeros(max(cap, 1), GTOP_GRP_DTYPE), np.zeros(rows, GTOP_ROW_DTYPE), np.zeros((nfields, rows), np.int64),
            np.zeros((nfields, rows), np.int64) if with_ts else None)


def gtop_merge(lists, per, desc=False):
    """The merge bmx_comm_where_group_top does with its shards' answers. `lists`: per shard (groups, rows, vals, ts) — groups GTOP_GRP_DTYPE with distinct keys,
    rows GTOP_ROW_DTYPE of shape (len(groups), per), vals and ts of shape (nfields, len(groups), per) (ts may be None) — -> (groups sorted ascending by key, rows,
    vals, ts): n_match and n of equal keys add; the rows of a key are the first `per` of the union of the shards' rows that carry a node, under the order — val
    ascending, or descending with desc, then id ascending as an unsigned number — and each row brings ITS shard's cells; n_rows is recomputed, and the rows
    behind it are (GTOP_NO_NODE, VAL_DELETED) with absent cells. Pure Python and numpy: no library, no GPU."""
    per = int(per)
    acc = {}                                        # key -> [n_match, n, [(sort key, id, val, cells, clocks)]]
    nf, have_ts = 0, False
    for groups, rows, vals, ts in lists:
        groups = np.asarray(groups, GTOP_GRP_DTYPE)
        rows = np.asarray(rows, GTOP_ROW_DTYPE).reshape(len(groups), per)
        vals = None if vals is None else np.asarray(vals)
        ts = None if ts is None else np.asarray(ts)
        if vals is not None:
            nf = max(nf, vals.shape[0])
        have_ts = have_ts or ts is not None
        for g in range(len(groups)):
            a = acc.setdefault(int(groups[g]["key"]), [0, 0, []])
            a[0] += int(groups[g]["n_match"]); a[1] += int(groups[g]["n"])
            for j in range(int(groups[g]["n_rows"])):
                i, v = int(rows[g, j]["id"]), int(rows[g, j]["val"])
                a[2].append(((-v if desc else v, i), i, v, None if vals is None else [int(x) for x in vals[:, g, j]], None if ts is None else [int(x) for x in ts[:, g, j]]))
    keys = sorted(acc)
    out = np.zeros(len(keys), GTOP_GRP_DTYPE)
    orows = np.zeros((len(keys), per), GTOP_ROW_DTYPE)
    orows["id"] = GTOP_NO_NODE; orows["val"] = VAL_DELETED
    ovals = np.full((nf, len(keys), per), VAL_DELETED, np.int64)
    ots = np.full((nf, len(keys), per), ROWS_NO_CLOCK, np.int64) if have_ts else None
    for g, k in enumerate(keys):
        nm, n, cand = acc[k]
        cand.sort(key=lambda c: c[0])
        cand = cand[:per]
        out[g] = (k, nm, n, min(per, n))
        assert len(cand) == min(per, n), "every shard delivered its first min(per, n) rows"
        for j, c in enumerate(cand):
            orows[g, j] = (c[1], c[2])
            if nf and c[3] is not None:
                ovals[:, g, j] = c[3]
            if have_ts and c[4] is not None:
                ots[:, g, j] = c[4]
    return out, orows, ovals, ots


class UpdRes(C.Structure):
    """bmx_upd_res: what one bmx_where_update found and wrote (72 bytes)"""
    _fields_ = [("n_match", C.c_uint64), ("n_nosrc", C.c_uint64), ("n_range", C.c_uint64), ("n_sent", C.c_uint64), ("n_applied", C.c_uint64), ("n_rows", C.c_uint64),
                ("next_pos", C.c_uint64), ("layout", C.c_uint64), ("next_shard", C.c_uint32), ("reserved", C.c_uint32)]


UPD_RES_DTYPE = np.dtype([("n_match", "<u8"), ("n_nosrc", "<u8"), ("n_range", "<u8"), ("n_sent", "<u8"), ("n_applied", "<u8"), ("n_rows", "<u8"), ("next_pos", "<u8"),
                          ("layout", "<u8"), ("next_shard", "<u4"), ("reserved", "<u4")])


class UpdateResult:
    """One where_update answer: n_match (the selected nodes at or behind the cursor), n_nosrc / n_range (of those: never written, for want of a source value or
    because the sum left the value range), n_sent (records handed to the merge), n_applied (rows that changed), n_rows (resident rows afterwards), next_pos (and
    next_shard: the cursor of the next page), layout (the cursor is good while the NEXT page reports the same) and ids (uint64, the n_applied nodes whose row
    changed, in index order; None unless asked for)."""
    __slots__ = ("n_match", "n_nosrc", "n_range", "n_sent", "n_applied", "n_rows", "next_pos", "next_shard", "layout", "ids")

    def __init__(self, res, ids=None):
        r = np.frombuffer(bytes(res), UPD_RES_DTYPE)[0] if isinstance(res, UpdRes) else res
        for k in ("n_match", "n_nosrc", "n_range", "n_sent", "n_applied", "n_rows", "next_pos", "next_shard", "layout"):
            setattr(self, k, int(r[k]))
        self.ids = None if ids is None else ids[:self.n_applied].copy()

    def __repr__(self):
        return "UpdateResult(%d matched, %d sent, %d applied, next_pos=%d)" % (self.n_match, self.n_sent, self.n_applied, self.next_pos)


def _upd_args(target, op, operand, src, ts, force):
    """-> (target_field, op, src_field, operand, ts, flags) of bmx_where_update"""
    if ts is None:
        import time
        ts = int(time.time() * 1000)          # the reference's clock: milliseconds since the epoch
    return (int(target), int(op), 0 if src is None else int(src), int(operand), int(ts), UPD_FORCE if force else 0)


class SemiRes(C.Structure):
    """bmx_semi_res: what one bmx_where_semijoin / bmx_where_in found besides its ids (32 bytes); flags: SEMI_OVERFLOW"""
    _fields_ = [("n_match", C.c_uint64), ("set_size", C.c_uint64), ("n_inner", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


SEMI_RES_DTYPE = np.dtype([("n_match", "<u8"), ("set_size", "<u8"), ("n_inner", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])


class SemiResult:
    """One where_semijoin / where_in answer: ids (uint64, min(n_match, cap) of them, in index order of the base field; none on overflow or with count_only),
    n_match (the selected nodes, however small cap was; 0 on overflow), set_size (distinct values in the set, or on overflow a lower bound of it above
    set_cap), n_inner (inner nodes selected / listed values inside the domain) and overflow."""
    __slots__ = ("ids", "n_match", "set_size", "n_inner", "overflow")

    def __init__(self, res, ids, cap):
        r = np.frombuffer(bytes(res), SEMI_RES_DTYPE)[0] if isinstance(res, SemiRes) else res
        self.n_match, self.set_size, self.n_inner = int(r["n_match"]), int(r["set_size"]), int(r["n_inner"])
        self.overflow = bool(int(r["flags"]) & SEMI_OVERFLOW)
        self.ids = np.zeros(0, np.uint64) if ids is None else ids[:min(self.n_match, int(cap))].copy()

    def __repr__(self):
        return "SemiResult(%d of %d ids, set of %d from %d%s)" % (len(self.ids), self.n_match, self.set_size, self.n_inner, ", overflow" if self.overflow else "")


def _semi_values(values):
    v = _np(values, np.int64).ravel()
    return v, len(v)


class ReachRes(C.Structure):
    """bmx_reach_res: what one bmx_where_reach / bmx_where_reach_from found besides its ids and depths (40 bytes); flags: REACH_OVERFLOW | REACH_MORE"""
    _fields_ = [("n_match", C.c_uint64), ("set_size", C.c_uint64), ("n_seed", C.c_uint64), ("n_edges", C.c_uint64), ("rounds", C.c_uint32), ("flags", C.c_uint32)]


REACH_RES_DTYPE = np.dtype([("n_match", "<u8"), ("set_size", "<u8"), ("n_seed", "<u8"), ("n_edges", "<u8"), ("rounds", "<u4"), ("flags", "<u4")])


class ReachResult:
    """One where_reach / where_reach_from answer: ids (uint64) and depth (uint8, 1..max_depth), min(n_match, cap) of each, in index order of the base field (none
    on overflow or with count_only); n_match (the nodes reached, however small cap was; 0 on overflow), set_size (distinct values at the end, seeds included,
    or on overflow a lower bound above set_cap), n_seed, n_edges, rounds (the largest depth in the answer), overflow, and more (some value has level max_depth:
    a frontier is left unexplored)."""
    __slots__ = ("ids", "depth", "n_match", "set_size", "n_seed", "n_edges", "rounds", "flags", "overflow", "more")

    def __init__(self, res, ids, depth, cap):
        r = np.frombuffer(bytes(res), REACH_RES_DTYPE)[0] if isinstance(res, ReachRes) else res
        self.n_match, self.set_size, self.n_seed, self.n_edges = int(r["n_match"]), int(r["set_size"]), int(r["n_seed"]), int(r["n_edges"])
        self.rounds, self.flags = int(r["rounds"]), int(r["flags"])
        self.overflow, self.more = bool(self.flags & REACH_OVERFLOW), bool(self.flags & REACH_MORE)
        k = min(self.n_match, int(cap))
        self.ids = np.zeros(0, np.uint64) if ids is None else ids[:k].copy()
        self.depth = np.zeros(0, np.uint8) if depth is None else depth[:k].copy()

    def __repr__(self):
        return "ReachResult(%d of %d nodes, %d rounds, set of %d from %d seeds over %d edges%s%s)" % (
            len(self.ids), self.n_match, self.rounds, self.set_size, self.n_seed, self.n_edges, ", overflow" if self.overflow else "", ", more" if self.more else "")


class JoinRes(C.Structure):
    """bmx_join_res: what one bmx_where_join_group / bmx_where_map_group found besides its records (184 bytes); flags: JOIN_MAP_OVERFLOW | JOIN_GROUP_OVERFLOW"""
    _fields_ = [("n_groups", C.c_uint64), ("map_size", C.c_uint64), ("n_inner", C.c_uint64), ("n_keyed", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("absent", Agg), ("unmatched", Agg), ("total", Agg)]


JOIN_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("map_size", "<u8"), ("n_inner", "<u8"), ("n_keyed", "<u8"), ("flags", "<u4"), ("reserved", "<u4"),
                           ("absent", AGG_DTYPE), ("unmatched", AGG_DTYPE), ("total", AGG_DTYPE)])


class JoinResult:
    """One where_join_group / where_map_group answer: groups = {attribute: AggResult} in ascending key order (empty on either overflow), records (GROUP_DTYPE,
    sorted by key), n_groups, map_size, n_inner, n_keyed, map_overflow, group_overflow, and absent (selected nodes whose key has no attribute), unmatched
    (selected nodes whose link is no key of the map) and total (every selected node) as AggResult."""
    __slots__ = ("records", "groups", "n_groups", "map_size", "n_inner", "n_keyed", "flags", "map_overflow", "group_overflow", "absent", "unmatched", "total")

    def __init__(self, res, recs):
        r = np.frombuffer(bytes(res), JOIN_RES_DTYPE)[0] if isinstance(res, JoinRes) else res
        self.n_groups, self.map_size, self.n_inner, self.n_keyed = int(r["n_groups"]), int(r["map_size"]), int(r["n_inner"]), int(r["n_keyed"])
        self.flags = int(r["flags"])
        self.map_overflow = bool(self.flags & JOIN_MAP_OVERFLOW); self.group_overflow = bool(self.flags & JOIN_GROUP_OVERFLOW)
        self.absent, self.unmatched, self.total = AggResult(r["absent"]), AggResult(r["unmatched"]), AggResult(r["total"])
        self.records = recs[:0 if self.flags else self.n_groups].copy()
        self.groups = {int(x["key"]): AggResult(x["agg"]) for x in self.records}

    def __repr__(self):
        return "JoinResult(%d groups, map of %d from %d/%d%s%s, absent=%r, unmatched=%r, total=%r)" % (
            self.n_groups, self.map_size, self.n_keyed, self.n_inner, ", map overflow" if self.map_overflow else "", ", group overflow" if self.group_overflow else "",
            self.absent, self.unmatched, self.total)


def _join_pairs(keys, vals):
    k, v = _np(keys, np.int64).ravel(), _np(vals, np.int64).ravel()
    if len(k) != len(v):
        raise ValueError("keys and vals differ in length")
    return k, v, len(k)


class JoinRowsRes(C.Structure):
    """bmx_jrows_res: what one bmx_where_join_rows / bmx_where_map_rows found besides its rows (72 bytes); flags: JOIN_MAP_OVERFLOW"""
    _fields_ = [("n_match", C.c_uint64), ("n_out", C.c_uint64), ("next_pos", C.c_uint64), ("layout", C.c_uint64), ("n_joined", C.c_uint64), ("map_size", C.c_uint64),
                ("n_inner", C.c_uint64), ("n_keyed", C.c_uint64), ("flags", C.c_uint32), ("next_shard", C.c_uint32)]


JROWS_RES_DTYPE = np.dtype([("n_match", "<u8"), ("n_out", "<u8"), ("next_pos", "<u8"), ("layout", "<u8"), ("n_joined", "<u8"), ("map_size", "<u8"), ("n_inner", "<u8"),
                            ("n_keyed", "<u8"), ("flags", "<u4"), ("next_shard", "<u4")])


class JoinRowsResult:
    """One where_join_rows / where_map_rows answer: ids, vals, ts of the outer nodes as RowsResult has them; in_ids (uint64, JROWS_NO_NODE in a row without
    inner node), in_vals, in_ts the same for the inner nodes (shape (n_in_fields, n_out)); n_match, n_out, next_pos, next_shard, layout as RowsResult; n_joined
    (delivered rows with an inner node), map_size, n_inner, n_keyed and map_overflow as JoinResult."""
    __slots__ = ("ids", "vals", "ts", "in_ids", "in_vals", "in_ts", "n_match", "n_out", "next_pos", "next_shard", "layout", "n_joined", "map_size", "n_inner", "n_keyed",
                 "flags", "map_overflow")

    def __init__(self, res, ids, vals, ts, in_ids, in_vals, in_ts):
        r = np.frombuffer(bytes(res), JROWS_RES_DTYPE)[0] if isinstance(res, JoinRowsRes) else res
        self.n_match, self.n_out, self.next_pos, self.layout, self.next_shard = int(r["n_match"]), int(r["n_out"]), int(r["next_pos"]), int(r["layout"]), int(r["next_shard"])
        self.n_joined, self.map_size, self.n_inner, self.n_keyed, self.flags = int(r["n_joined"]), int(r["map_size"]), int(r["n_inner"]), int(r["n_keyed"]), int(r["flags"])
        self.map_overflow = bool(self.flags & JOIN_MAP_OVERFLOW)
        n = self.n_out
        self.ids, self.vals, self.ts = ids[:n].copy(), vals[:, :n].copy(), None if ts is None else ts[:, :n].copy()
        self.in_ids, self.in_vals, self.in_ts = in_ids[:n].copy(), in_vals[:, :n].copy(), None if in_ts is None else in_ts[:, :n].copy()

    def __repr__(self):
        return "JoinRowsResult(%d of %d rows, %d joined, %d + %d fields, map of %d from %d/%d%s, next_pos=%d)" % (
            self.n_out, self.n_match, self.n_joined, self.vals.shape[0], self.in_vals.shape[0], self.map_size, self.n_keyed, self.n_inner,
            ", map overflow" if self.map_overflow else "", self.next_pos)


def _jrows_pairs(keys, node_ids):
    k, v = _np(keys, np.int64).ravel(), _np(node_ids, np.uint64).ravel()
    if len(k) != len(v):
        raise ValueError("keys and node_ids differ in length")
    return k, v, len(k)


def _jrows_flags(with_ts, inner):
    return (ROWS_TS if with_ts else 0) | (JROWS_INNER if inner else 0)


def _jrows_host(fn, h, chk, head, mid, nf, nif, with_ts, cap):
    """one host-memory call: fn(h, *head, *mid, cap, the six outputs, res) -> JoinRowsResult"""
    ids, vals, ts = _rows_buffers(nf, cap, with_ts)
    in_ids, in_vals, in_ts = _rows_buffers(nif, cap, with_ts)
    res = JoinRowsRes()
    chk(fn(h, *head, *mid, cap, _ptr(ids), _ptr(vals), _ptr(ts), _ptr(in_ids), _ptr(in_vals), _ptr(in_ts), C.cast(C.byref(res), C.c_void_p)))
    return JoinRowsResult(res, ids, vals, ts, in_ids, in_vals, in_ts)


class QuantQ(C.Structure):
    """bmx_quant_q: the quantile num / den (8 bytes)"""
    _fields_ = [("num", C.c_uint32), ("den", C.c_uint32)]


class QuantRec(C.Structure):
    """bmx_quant_rec: one record of bmx_where_quantiles (32 bytes): the sample's element of 0-based rank `rank`, how many elements are smaller, how many equal"""
    _fields_ = [("value", C.c_int64), ("rank", C.c_uint64), ("n_below", C.c_uint64), ("n_equal", C.c_uint64)]


class QuantRes(C.Structure):
    """bmx_quant_res: what one bmx_where_quantiles found besides its records (32 bytes): selected nodes, the sample's size, its minimum and maximum"""
    _fields_ = [("n_match", C.c_uint64), ("n", C.c_uint64), ("min", C.c_int64), ("max", C.c_int64)]


QUANT_REC_DTYPE = np.dtype([("value", "<i8"), ("rank", "<u8"), ("n_below", "<u8"), ("n_equal", "<u8")])
QUANT_RES_DTYPE = np.dtype([("n_match", "<u8"), ("n", "<u8"), ("min", "<i8"), ("max", "<i8")])


def quant_rank(num, den, n):
    """The rank rule of bmx_where_quantiles, in one place: the 0-based rank, in ascending order, of the quantile num / den of a sample of n >= 1 elements
    ("lower" nearest rank: numpy.sort(v)[quant_rank(num, den, len(v))]). 0/1 is the minimum, 1/1 the maximum, 1/2 the lower median."""
    num, den, n = int(num), int(den), int(n)
    if not (1 <= den <= QUANT_MAX_DEN and 0 <= num <= den and n >= 1):
        raise ValueError("quant_rank: 0 <= num <= den, 1 <= den <= %d and n >= 1" % QUANT_MAX_DEN)
    return (num * (n - 1)) // den


def _quant_tail(measure, qs):
    """-> (measure_field, nq, qs) of bmx_where_quantiles; qs: a list of (num, den)"""
    arr = (QuantQ * max(len(qs), 1))(*[QuantQ(int(a), int(b)) for a, b in qs])
    return (int(measure), len(qs), arr)


class Expr(C.Structure):
    """bmx_expr: a computed measure, value(a) op value(b) of the selected node (16 bytes). bmx.Expr(a, op, b) with op "+", "-" or "*"; a node whose a or b is
    absent or tombstoned is undefined, one whose exact result lies outside +-(2^53 - 1) is out of range, and neither is measured (bmx_expr.h)"""
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("op", C.c_uint32), ("reserved", C.c_uint32)]
    OPS = {"+": EXPR_ADD, "-": EXPR_SUB, "*": EXPR_MUL}

    def __init__(self, a, op, b):
        if op not in self.OPS:
            raise ValueError('bmx.Expr: op is "+", "-" or "*"')
        super().__init__(int(a), int(b), self.OPS[op], 0)


class ExprRes(C.Structure):
    """bmx_expr_res: the selected nodes a computed measure left unmeasured (16 bytes): n_undef (an operand absent or tombstoned), n_range (the exact result
    outside +-(2^53 - 1))"""
    _fields_ = [("n_undef", C.c_uint64), ("n_range", C.c_uint64)]

    def __repr__(self):
        return "ExprRes(n_undef=%d, n_range=%d)" % (self.n_undef, self.n_range)


EXPR_RES_DTYPE = np.dtype([("n_undef", "<u8"), ("n_range", "<u8")])


class WatchRes(C.Structure):
    """bmx_watch_res: what one bmx_watch_poll found (32 bytes); flags: WATCH_RESET, WATCH_OVERFLOW"""
    _fields_ = [("n_entered", C.c_uint64), ("n_left", C.c_uint64), ("n_match", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class WatchPoll:
    """One poll of a watch: entered / left (uint64 ids in index order, cut at the caps), the true counts n_entered / n_left, n_match = size of the answer now,
    reset (the lists are relative to the empty set: replace yours with `entered`), overflow (a list did not fit: nothing was committed, poll again with more room)."""
    __slots__ = ("entered", "left", "n_entered", "n_left", "n_match", "reset", "overflow")

    def __init__(self, res, entered, left):
        self.n_entered, self.n_left, self.n_match = int(res.n_entered), int(res.n_left), int(res.n_match)
        self.reset, self.overflow = bool(res.flags & WATCH_RESET), bool(res.flags & WATCH_OVERFLOW)
        self.entered, self.left = entered[:min(self.n_entered, len(entered))].copy(), left[:min(self.n_left, len(left))].copy()

    def __repr__(self):
        return "WatchPoll(+%d -%d, %d match%s%s)" % (self.n_entered, self.n_left, self.n_match, ", reset" if self.reset else "", ", overflow" if self.overflow else "")


class Info(C.Structure):
    _fields_ = [("capacity_rows", C.c_uint64), ("n_slots", C.c_uint64), ("table_bytes", C.c_uint64), ("n_rows", C.c_uint64),
                ("device", C.c_uint32), ("abi_version", C.c_uint32), ("n_indexes", C.c_uint32), ("epoch", C.c_uint32)]


DELTA_REC_DTYPE = np.dtype([("id", "<u8"), ("field", "<u4"), ("aux", "<u4"), ("ts", "<i8"), ("val", "<i8")])


class VcRec(C.Structure):
    """bmx_vc_rec: one row of a K-writer table as a delta (64 bytes, include/bmx_vc_sync.h)"""
    _fields_ = [("id", C.c_uint64), ("field", C.c_uint32), ("aux", C.c_uint32), ("val", C.c_int64), ("state", C.c_uint32), ("keyset", C.c_uint32), ("clock", C.c_uint32 * 8)]


VC_REC_DTYPE = np.dtype([("id", "<u8"), ("field", "<u4"), ("aux", "<u4"), ("val", "<i8"), ("state", "<u4"), ("keyset", "<u4"), ("clock", "<u4", (8,))])


class VcTableInfo(C.Structure):
    """bmx_vc_table_info (48 bytes)"""
    _fields_ = [("n_slots", C.c_uint64), ("n_rows", C.c_uint64), ("capacity_rows", C.c_uint64), ("table_bytes", C.c_uint64),
                ("k_writers", C.c_uint32), ("local_writer", C.c_uint32), ("device", C.c_uint32), ("reserved", C.c_uint32)]

# OR-ed into the flags of every Engine this process creates
DEFAULT_CTX_FLAGS = int(os.environ.get("BMX_CTX_FLAGS", "0"), 0)

_lib = None


def load_library():
    """dlopen libbmx.so and declare its signatures. No GPU is touched."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BmxError(ERR_NO_DEVICE, "libbmx.so not built (run __graft_entry__.build() or make -C bullet-js_amd): the engine has no CPU fallback")
    # Load order matters in a process that also uses PyTorch: its wheel bundles its own ROCm runtime (same sonames as /opt/rocm's). If
    # libbmx.so comes first it binds the system runtime and torch later brings a second one ("No HIP GPUs are available"); if torch comes
    # first, libbmx.so resolves libamdhip64.so.7 to the copy that is already loaded and both share streams and pointers.
    if "torch" not in sys.modules:
        try:
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, i64, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int64, C.c_int
    L.bmx_create.argtypes = [i32, u64, u32, C.POINTER(vp)]; L.bmx_create.restype = i32
    L.bmx_create_ex.argtypes = [i32, u64, u32, u32, C.POINTER(vp)]; L.bmx_create_ex.restype = i32
    L.bmx_destroy.argtypes = [vp]; L.bmx_destroy.restype = None
    L.bmx_last_error.argtypes = [vp]; L.bmx_last_error.restype = C.c_char_p
    L.bmx_abi_version.argtypes = []; L.bmx_abi_version.restype = i32
    L.bmx_selfcheck.argtypes = [i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]; L.bmx_selfcheck.restype = i32
    L.bmx_selfcheck_claim.argtypes = [i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]; L.bmx_selfcheck_claim.restype = i32
    L.bmx_get_claim_mode.argtypes = [vp]; L.bmx_get_claim_mode.restype = i32
    L.bmx_set_deferred_compaction.argtypes = [vp, i32]; L.bmx_set_deferred_compaction.restype = i32
    L.bmx_set_side_stream.argtypes = [vp, vp]; L.bmx_set_side_stream.restype = i32
    L.bmx_set_wait_limit.argtypes = [vp, C.c_double]; L.bmx_set_wait_limit.restype = i32
    L.bmx_merge_fence.argtypes = [vp]; L.bmx_merge_fence.restype = i32
    L.bmx_get_deferred_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]; L.bmx_get_deferred_counts.restype = i32
    L.bmx_get_info.argtypes = [vp, C.POINTER(Info)]; L.bmx_get_info.restype = i32
    L.bmx_set_probe_waves.argtypes = [vp, i32]; L.bmx_set_probe_waves.restype = i32
    L.bmx_get_placement.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(C.c_float)]; L.bmx_get_placement.restype = i32
    L.bmx_sync.argtypes = [vp]; L.bmx_sync.restype = i32
    L.bmx_set_stream.argtypes = [vp, vp]; L.bmx_set_stream.restype = i32
    L.bmx_get_stream.argtypes = [vp]; L.bmx_get_stream.restype = vp
    L.bmx_seq_signal.argtypes = [vp, vp, vp, u64]; L.bmx_seq_signal.restype = i32
    L.bmx_seq_wait.argtypes = [vp, vp, vp, u64]; L.bmx_seq_wait.restype = i32
    L.bmx_load_rows.argtypes = [vp, u64, vp, vp, vp, vp, i32]; L.bmx_load_rows.restype = i32
    L.bmx_put_rows.argtypes = [vp, u64, vp, vp, vp, vp, i32]; L.bmx_put_rows.restype = i32
    L.bmx_merge_batch.argtypes = [vp, u64, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]; L.bmx_merge_batch.restype = i32
    L.bmx_merge_records.argtypes = [vp, u64, vp, i32, vp, vp, vp, vp]; L.bmx_merge_records.restype = i32
    L.bmx_merge_submit.argtypes = [vp, u64, vp, vp, vp, vp, i32, i32, C.POINTER(u64)]; L.bmx_merge_submit.restype = i32
    L.bmx_merge_collect.argtypes = [vp, u64, vp, vp, vp, vp]; L.bmx_merge_collect.restype = i32
    L.bmx_get_rows.argtypes = [vp, u64, vp, vp, vp, vp, vp, i32]; L.bmx_get_rows.restype = i32
    L.bmx_get_row.argtypes = [vp, u64, u32, C.POINTER(i64), C.POINTER(i64)]; L.bmx_get_row.restype = i32
    L.bmx_dump_rows.argtypes = [vp, u64, vp, vp, vp, vp, vp, i32]; L.bmx_dump_rows.restype = i32
    L.bmx_row_count.argtypes = [vp, C.POINTER(u64)]; L.bmx_row_count.restype = i32
    L.bmx_reserve.argtypes = [vp, u64]; L.bmx_reserve.restype = i32
    L.bmx_index_build.argtypes = [vp, u32]; L.bmx_index_build.restype = i32
    L.bmx_index_drop.argtypes = [vp, u32]; L.bmx_index_drop.restype = i32
    L.bmx_index_size.argtypes = [vp, u32, C.POINTER(u64)]; L.bmx_index_size.restype = i32
    L.bmx_index_refresh_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]; L.bmx_index_refresh_counts.restype = i32
    L.bmx_index_set_ordered.argtypes = [vp, u32, u32]; L.bmx_index_set_ordered.restype = i32
    L.bmx_index_ordered_info.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(u64)]; L.bmx_index_ordered_info.restype = i32
    L.bmx_index_ordered_stats.argtypes = [vp, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(u64)]; L.bmx_index_ordered_stats.restype = i32
    L.bmx_scan_range.argtypes = [vp, u32, i64, i64, vp, u64, vp, i32]; L.bmx_scan_range.restype = i32
    L.bmx_scan_equals.argtypes = [vp, u32, i64, vp, u64, vp, i32]; L.bmx_scan_equals.restype = i32
    L.bmx_scan_count.argtypes = [vp, u32, i64, i64, vp, i32]; L.bmx_scan_count.restype = i32
    L.bmx_scan_filter.argtypes = [vp, u32, C.POINTER(Term), vp, u64, vp, i32]; L.bmx_scan_filter.restype = i32
    L.bmx_scan_range_pos.argtypes = [vp, u32, i64, i64, vp, u64, vp, i32]; L.bmx_scan_range_pos.restype = i32
    L.bmx_index_ids.argtypes = [vp, u32, u64, u64, vp, i32]; L.bmx_index_ids.restype = i32
    L.bmx_owner_of.argtypes = [u64, u32]; L.bmx_owner_of.restype = u32
    L.bmx_key_bucket.argtypes = [u64, u32, u32]; L.bmx_key_bucket.restype = u32
    L.bmx_digest.argtypes = [vp, u32, u32, vp, vp, i32]; L.bmx_digest.restype = i32
    L.bmx_export_rows.argtypes = [vp, i64, u32, vp, u32, vp, u64, vp, i32]; L.bmx_export_rows.restype = i32
    L.bmx_comm_digest.argtypes = [vp, u32, u32, vp, vp]; L.bmx_comm_digest.restype = i32
    L.bmx_comm_export_rows.argtypes = [vp, i64, u32, vp, u32, vp, u64, vp]; L.bmx_comm_export_rows.restype = i32
    L.bmx_scan_aggregate.argtypes = [vp, u32, C.POINTER(Term), u32, u32, i64, u32, vp, i32]; L.bmx_scan_aggregate.restype = i32
    L.bmx_comm_scan_aggregate.argtypes = [vp, u32, C.POINTER(Term), u32, u32, i64, u32, vp]; L.bmx_comm_scan_aggregate.restype = i32
    L.bmx_scan_top.argtypes = [vp, u32, C.POINTER(Term), u32, vp, u32, vp, vp, vp, i32]; L.bmx_scan_top.restype = i32
    L.bmx_comm_scan_top.argtypes = [vp, u32, C.POINTER(Term), u32, vp, u32, vp, vp, vp]; L.bmx_comm_scan_top.restype = i32
    L.bmx_scan_where.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), vp, u64, vp, i32]; L.bmx_scan_where.restype = i32
    L.bmx_comm_scan_where.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), vp, u64, vp]; L.bmx_comm_scan_where.restype = i32
    L.bmx_where_aggregate.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, u32, i64, u32, vp, i32]; L.bmx_where_aggregate.restype = i32
    L.bmx_where_top.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, vp, u32, vp, vp, vp, i32]; L.bmx_where_top.restype = i32
    L.bmx_comm_where_aggregate.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, u32, i64, u32, vp]; L.bmx_comm_where_aggregate.restype = i32
    L.bmx_comm_where_top.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, vp, u32, vp, vp, vp]; L.bmx_comm_where_top.restype = i32
    L.bmx_where_group.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, u32, vp, u64, vp, i32]; L.bmx_where_group.restype = i32
    L.bmx_comm_where_group.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, u32, vp, u64, vp]; L.bmx_comm_where_group.restype = i32
    L.bmx_where_quantiles.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, u32, vp, vp, vp, i32]; L.bmx_where_quantiles.restype = i32
    L.bmx_comm_where_quantiles.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, u32, vp, vp, vp]; L.bmx_comm_where_quantiles.restype = i32
    prog = [u32, u32, C.POINTER(u32), C.POINTER(Lit)]
    L.bmx_where_aggregate_expr.argtypes = [vp] + prog + [vp, u32, i64, u32, vp, vp, i32]; L.bmx_where_aggregate_expr.restype = i32
    L.bmx_where_group_expr.argtypes = [vp] + prog + [vp, u32, vp, u64, vp, vp, i32]; L.bmx_where_group_expr.restype = i32
    L.bmx_where_quantiles_expr.argtypes = [vp] + prog + [vp, u32, vp, vp, vp, vp, i32]; L.bmx_where_quantiles_expr.restype = i32
    L.bmx_comm_where_aggregate_expr.argtypes = [vp] + prog + [vp, u32, i64, u32, vp, vp]; L.bmx_comm_where_aggregate_expr.restype = i32
    L.bmx_comm_where_group_expr.argtypes = [vp] + prog + [vp, u32, vp, u64, vp, vp]; L.bmx_comm_where_group_expr.restype = i32
    L.bmx_comm_where_quantiles_expr.argtypes = [vp] + prog + [vp, u32, vp, vp, vp, vp]; L.bmx_comm_where_quantiles_expr.restype = i32
    L.bmx_where_semijoin.argtypes = [vp] + prog + [u32, u32] + prog + [u32, u64, vp, u64, vp, i32]; L.bmx_where_semijoin.restype = i32
    L.bmx_where_in.argtypes = [vp] + prog + [u32, u32, vp, u64, vp, u64, vp, i32]; L.bmx_where_in.restype = i32
    L.bmx_comm_where_semijoin.argtypes = [vp] + prog + [u32, u32] + prog + [u32, u64, vp, u64, vp]; L.bmx_comm_where_semijoin.restype = i32
    L.bmx_comm_where_in.argtypes = [vp] + prog + [u32, u32, vp, u64, vp, u64, vp]; L.bmx_comm_where_in.restype = i32
    reach_out = [u32, u64, vp, vp, u64, vp]                                  # max_depth, set_cap, out_ids, out_depth, cap, res
    L.bmx_where_reach.argtypes = [vp] + prog + [u32, u32, u32] + prog + [u32] + reach_out + [i32]; L.bmx_where_reach.restype = i32
    L.bmx_where_reach_from.argtypes = [vp] + prog + [u32, u32, u32, vp, u64] + reach_out + [i32]; L.bmx_where_reach_from.restype = i32
    L.bmx_comm_where_reach.argtypes = [vp] + prog + [u32, u32, u32] + prog + [u32] + reach_out; L.bmx_comm_where_reach.restype = i32
    L.bmx_comm_where_reach_from.argtypes = [vp] + prog + [u32, u32, u32, vp, u64] + reach_out; L.bmx_comm_where_reach_from.restype = i32
    L.bmx_where_join_group.argtypes = [vp] + prog + [u32, u32] + prog + [u32, u32, u64, vp, u64, vp, i32]; L.bmx_where_join_group.restype = i32
    L.bmx_where_map_group.argtypes = [vp] + prog + [u32, u32, vp, vp, u64, vp, u64, vp, i32]; L.bmx_where_map_group.restype = i32
    L.bmx_comm_where_join_group.argtypes = [vp] + prog + [u32, u32] + prog + [u32, u32, u64, vp, u64, vp]; L.bmx_comm_where_join_group.restype = i32
    L.bmx_comm_where_map_group.argtypes = [vp] + prog + [u32, u32, vp, vp, u64, vp, u64, vp]; L.bmx_comm_where_map_group.restype = i32
    jr_out = [vp, vp, vp, vp, vp, vp, vp]
    L.bmx_where_join_rows.argtypes = [vp] + prog + [u32, u32, C.POINTER(u32)] + prog + [u32, u32, C.POINTER(u32), u64, u32, u64, u64] + jr_out + [i32]; L.bmx_where_join_rows.restype = i32
    L.bmx_where_map_rows.argtypes = [vp] + prog + [u32, u32, C.POINTER(u32), vp, vp, u64, u32, C.POINTER(u32), u32, u64, u64] + jr_out + [i32]; L.bmx_where_map_rows.restype = i32
    L.bmx_comm_where_join_rows.argtypes = [vp] + prog + [u32, u32, C.POINTER(u32)] + prog + [u32, u32, C.POINTER(u32), u64, u32, u32, u64, u64] + jr_out; L.bmx_comm_where_join_rows.restype = i32
    L.bmx_comm_where_map_rows.argtypes = [vp] + prog + [u32, u32, C.POINTER(u32), vp, vp, u64, u32, C.POINTER(u32), u32, u32, u64, u64] + jr_out; L.bmx_comm_where_map_rows.restype = i32
    L.bmx_where_rows.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, C.POINTER(u32), u32, u64, u64, vp, vp, vp, vp, i32]; L.bmx_where_rows.restype = i32
    L.bmx_comm_where_rows.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), u32, C.POINTER(u32), u32, u32, u64, u64, vp, vp, vp, vp]; L.bmx_comm_where_rows.restype = i32
    first = [u32, u32, u32, C.POINTER(u32), u32, u64, vp, vp, vp, vp]       # group, order, nfields, fields, flags, cap, out, out_val, out_ts, res
    L.bmx_where_group_first.argtypes = [vp] + prog + first + [i32]; L.bmx_where_group_first.restype = i32
    L.bmx_comm_where_group_first.argtypes = [vp] + prog + first; L.bmx_comm_where_group_first.restype = i32
    gtop = [u32, u32, u32, u32, C.POINTER(u32), u32, u64, vp, vp, vp, vp, vp]  # group, order, per, nfields, fields, flags, cap, out, out_rows, out_val, out_ts, res
    L.bmx_where_group_top.argtypes = [vp] + prog + gtop + [i32]; L.bmx_where_group_top.restype = i32
    L.bmx_comm_where_group_top.argtypes = [vp] + prog + gtop; L.bmx_comm_where_group_top.restype = i32
    L.bmx_where_group_multi.argtypes = [vp] + prog + [u32, u32, C.POINTER(GroupKey), vp, u64, vp, i32]; L.bmx_where_group_multi.restype = i32
    L.bmx_comm_where_group_multi.argtypes = [vp] + prog + [u32, u32, C.POINTER(GroupKey), vp, u64, vp]; L.bmx_comm_where_group_multi.restype = i32
    upd = [u32, u32, u32, i64, i64, u32]
    L.bmx_where_update.argtypes = [vp] + prog + upd + [u64, u64, vp, vp, i32]; L.bmx_where_update.restype = i32
    L.bmx_comm_where_update.argtypes = [vp] + prog + upd + [u32, u64, u64, vp, vp]; L.bmx_comm_where_update.restype = i32
    L.bmx_watch_create.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), C.POINTER(u32)]; L.bmx_watch_create.restype = i32
    L.bmx_watch_poll.argtypes = [vp, u32, vp, u64, vp, u64, vp, i32]; L.bmx_watch_poll.restype = i32
    L.bmx_watch_destroy.argtypes = [vp, u32]; L.bmx_watch_destroy.restype = i32
    L.bmx_comm_watch_create.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(Lit), C.POINTER(u32)]; L.bmx_comm_watch_create.restype = i32
    L.bmx_comm_watch_poll.argtypes = [vp, u32, vp, u64, vp, u64, vp]; L.bmx_comm_watch_poll.restype = i32
    L.bmx_comm_watch_destroy.argtypes = [vp, u32]; L.bmx_comm_watch_destroy.restype = i32
    L.bmx_partition_by_owner.argtypes = [vp, u64, vp, vp, vp, vp, u32, vp, vp]; L.bmx_partition_by_owner.restype = i32
    L.bmx_partition_by_owner_slabs.argtypes = [vp, u64, vp, vp, vp, vp, u32, u64, vp, vp]; L.bmx_partition_by_owner_slabs.restype = i32
    L.bmx_partition_scatter.argtypes = [vp, u64, vp, vp, vp, vp, u32, u64, vp, vp, vp, u64, vp, u32, u64]; L.bmx_partition_scatter.restype = i32
    L.bmx_merge_records_after.argtypes = [vp, vp, u32, u64, u64, vp, i32, vp, vp, vp, vp]; L.bmx_merge_records_after.restype = i32
    L.bmx_ipc_alloc.argtypes = [vp, u64, u32, C.POINTER(vp), C.c_char_p]; L.bmx_ipc_alloc.restype = i32
    L.bmx_ipc_open.argtypes = [vp, C.c_char_p, i32, C.POINTER(vp)]; L.bmx_ipc_open.restype = i32
    L.bmx_ipc_close.argtypes = [vp, vp]; L.bmx_ipc_close.restype = i32
    L.bmx_ipc_free.argtypes = [vp, vp]; L.bmx_ipc_free.restype = i32
    L.bmx_host_alloc.argtypes = [C.c_uint64, C.POINTER(C.c_void_p)]; L.bmx_host_alloc.restype = i32
    L.bmx_host_free.argtypes = [vp]; L.bmx_host_free.restype = i32
    L.bmx_seq_wait_all.argtypes = [vp, vp, vp, u32, u64]; L.bmx_seq_wait_all.restype = i32
    L.bmx_merge_notify.argtypes = [vp, vp, u32]; L.bmx_merge_notify.restype = i32
    L.bmx_merge_tail_wait.argtypes = [vp, vp, u32, u64]; L.bmx_merge_tail_wait.restype = i32
    L.bmx_timer_start.argtypes = [vp]; L.bmx_timer_start.restype = i32
    L.bmx_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]; L.bmx_timer_stop.restype = i32
    L.bmx_timer_mark.argtypes = [vp]; L.bmx_timer_mark.restype = i32
    L.bmx_timer_elapsed.argtypes = [vp, C.POINTER(C.c_float)]; L.bmx_timer_elapsed.restype = i32
    L.bmx_profile_enable.argtypes = [vp, i32]; L.bmx_profile_enable.restype = i32
    L.bmx_profile_read.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(u32)]; L.bmx_profile_read.restype = i32
    L.bmx_profile_read_scan.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(u32)]; L.bmx_profile_read_scan.restype = i32
    L.bmx_comm_create.argtypes = [u32, C.POINTER(C.c_int), u64, u32, C.POINTER(vp)]; L.bmx_comm_create.restype = i32
    L.bmx_comm_destroy.argtypes = [vp]; L.bmx_comm_destroy.restype = None
    L.bmx_comm_last_error.argtypes = [vp]; L.bmx_comm_last_error.restype = C.c_char_p
    L.bmx_comm_nshards.argtypes = [vp]; L.bmx_comm_nshards.restype = u32
    L.bmx_comm_shard.argtypes = [vp, u32]; L.bmx_comm_shard.restype = vp
    L.bmx_comm_sync.argtypes = [vp]; L.bmx_comm_sync.restype = i32
    L.bmx_comm_load_rows.argtypes = [vp, u64, vp, vp, vp, vp]; L.bmx_comm_load_rows.restype = i32
    L.bmx_comm_put_rows.argtypes = [vp, u64, vp, vp, vp, vp]; L.bmx_comm_put_rows.restype = i32
    L.bmx_comm_merge.argtypes = [vp, u64, vp, vp, vp, vp, i32, vp, vp, vp]; L.bmx_comm_merge.restype = i32
    L.bmx_comm_merge_dev.argtypes = [vp, vp, vp, vp, vp, vp, i32, u64]; L.bmx_comm_merge_dev.restype = i32
    L.bmx_comm_shard_result.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]; L.bmx_comm_shard_result.restype = i32
    L.bmx_comm_row_count.argtypes = [vp, C.POINTER(u64)]; L.bmx_comm_row_count.restype = i32
    L.bmx_comm_get_rows.argtypes = [vp, u64, vp, vp, vp, vp, vp]; L.bmx_comm_get_rows.restype = i32
    L.bmx_comm_dump_rows.argtypes = [vp, u64, vp, vp, vp, vp, C.POINTER(u64)]; L.bmx_comm_dump_rows.restype = i32
    L.bmx_comm_index_build.argtypes = [vp, u32]; L.bmx_comm_index_build.restype = i32
    L.bmx_comm_index_set_ordered.argtypes = [vp, u32, u32]; L.bmx_comm_index_set_ordered.restype = i32
    L.bmx_comm_scan_range.argtypes = [vp, u32, i64, i64, vp, u64, C.POINTER(u64)]; L.bmx_comm_scan_range.restype = i32
    L.bmx_comm_scan_equals.argtypes = [vp, u32, i64, vp, u64, C.POINTER(u64)]; L.bmx_comm_scan_equals.restype = i32
    L.bmx_comm_scan_count.argtypes = [vp, u32, i64, i64, C.POINTER(u64)]; L.bmx_comm_scan_count.restype = i32
    L.bmx_comm_scan_filter.argtypes = [vp, u32, C.POINTER(Term), vp, u64, C.POINTER(u64)]; L.bmx_comm_scan_filter.restype = i32
    L.bmx_vc_create.argtypes = [i32, u64, u32, u32, C.POINTER(vp)]; L.bmx_vc_create.restype = i32
    L.bmx_vc_destroy.argtypes = [vp]; L.bmx_vc_destroy.restype = None
    L.bmx_vc_last_error.argtypes = [vp]; L.bmx_vc_last_error.restype = C.c_char_p
    L.bmx_vc_load_rows.argtypes = [vp, u64, vp, vp, vp, vp]; L.bmx_vc_load_rows.restype = i32
    L.bmx_vc_merge_batch.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]; L.bmx_vc_merge_batch.restype = i32
    L.bmx_vc_get_rows.argtypes = [vp, u64, vp, vp, vp, vp, vp]; L.bmx_vc_get_rows.restype = i32
    L.bmx_vc_row_count.argtypes = [vp, C.POINTER(u64)]; L.bmx_vc_row_count.restype = i32
    L.bmx_vc_scan_range.argtypes = [vp, u32, i64, i64, vp, u64, C.POINTER(u64)]; L.bmx_vc_scan_range.restype = i32
    L.bmx_vc_merge_batch_dev.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]; L.bmx_vc_merge_batch_dev.restype = i32
    L.bmx_vc_load_rows_ks.argtypes = [vp, u64, vp, vp, vp, vp, vp]; L.bmx_vc_load_rows_ks.restype = i32
    L.bmx_vc_merge_batch_ks.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]; L.bmx_vc_merge_batch_ks.restype = i32
    L.bmx_vc_get_rows_ks.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]; L.bmx_vc_get_rows_ks.restype = i32
    L.bmx_vc_merge_batch_ks_dev.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]; L.bmx_vc_merge_batch_ks_dev.restype = i32
    L.bmx_vc_keyset.argtypes = [vp, C.c_uint32]; L.bmx_vc_keyset.restype = C.c_uint32
    L.bmx_vc_keyset_dense.argtypes = [C.c_uint32]; L.bmx_vc_keyset_dense.restype = C.c_uint32
    L.bmx_vc_set_stream.argtypes = [vp, vp]; L.bmx_vc_set_stream.restype = i32
    L.bmx_vc_sync.argtypes = [vp]; L.bmx_vc_sync.restype = i32
    L.bmx_vc_rec_digest.argtypes = [vp]; L.bmx_vc_rec_digest.restype = u64
    L.bmx_vc_info.argtypes = [vp, C.POINTER(VcTableInfo)]; L.bmx_vc_info.restype = i32
    L.bmx_vc_digest.argtypes = [vp, u32, u32, vp, vp, i32]; L.bmx_vc_digest.restype = i32
    L.bmx_vc_frontier.argtypes = [vp, vp, i32]; L.bmx_vc_frontier.restype = i32
    L.bmx_vc_export_rows.argtypes = [vp, vp, u32, vp, u32, vp, u64, vp, i32]; L.bmx_vc_export_rows.restype = i32
    L.bmx_vc_merge_records.argtypes = [vp, u64, vp, vp, vp, vp, i32]; L.bmx_vc_merge_records.restype = i32
    _lib = L
    return L


def selfcheck(device=0):
    """bmx_selfcheck: (checked 16-byte loads, torn pairs seen, torn pairs of the split-store control). Raises if a pair tore."""
    L = load_library()
    r, t, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = L.bmx_selfcheck(int(device), C.byref(r), C.byref(t), C.byref(c))
    if rc:
        raise BmxError(rc, (L.bmx_last_error(None) or b"").decode())
    return r.value, t.value, c.value


def selfcheck_claim(device=0):
    """bmx_selfcheck_claim: (checked 16-byte loads, torn pairs seen beside team swaps, torn pairs of the three-instruction control). A torn pair is
    reported, not raised: contexts on such a device keep claim mode `store`."""
    L = load_library()
    r, t, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = L.bmx_selfcheck_claim(int(device), C.byref(r), C.byref(t), C.byref(c))
    if rc:
        raise BmxError(rc, (L.bmx_last_error(None) or b"").decode())
    return r.value, t.value, c.value


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _ptr(a):
    """numpy array -> void*, torch tensor -> data_ptr, int passes through, None -> NULL."""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(a.data_ptr())


class HostBuffer:
    """Page-locked host memory (bmx_host_alloc) seen as a numpy array: inputs and outputs of host-array calls placed here move at the
    link's rate. Freed by close() or when collected; arrays taken from it must not outlive it."""

    def __init__(self, nbytes):
        self.L = load_library()
        p = C.c_void_p()
        rc = self.L.bmx_host_alloc(int(nbytes), C.byref(p))
        if rc:
            raise BmxError(rc, (self.L.bmx_last_error(None) or b"").decode())
        self.ptr, self.nbytes = p.value, int(nbytes)
        self._raw = (C.c_uint8 * self.nbytes).from_address(self.ptr)

    def array(self, dtype, count, offset=0):
        dt = np.dtype(dtype)
        if offset % dt.itemsize or offset + count * dt.itemsize > self.nbytes:
            raise ValueError("HostBuffer.array: out of range or misaligned")
        return np.frombuffer(self._raw, dtype=dt, count=count, offset=offset)

    def close(self):
        if self.ptr:
            self._raw = None
            self.L.bmx_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_columns(n):
    """-> (HostBuffer, id u64[n], field u32[n], ts i64[n], val i64[n]) in page-locked memory, the layout merge_batch() takes."""
    hb = HostBuffer(max(n, 1) * 28)
    return hb, hb.array(np.uint64, n), hb.array(np.uint32, n, 24 * n), hb.array(np.int64, n, 8 * n), hb.array(np.int64, n, 16 * n)


class Engine:
    """One GPU-resident graph shard (a bmx_ctx). Host-array methods are synchronous; *_dev methods take
    device tensors/pointers and only enqueue work on the engine's stream."""

    def __init__(self, capacity_rows, device=0, flags=0, load_pct=0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.bmx_create_ex(int(device), int(capacity_rows), int(load_pct), int(flags) | DEFAULT_CTX_FLAGS, C.byref(h))
        if rc != OK:
            raise BmxError(rc, (self.L.bmx_last_error(None) or b"").decode())
        self.h = h
        self.device = device
        self._watch_base = {}        # watch id -> base field (watch_poll sizes its default lists from that field's index)

    def _chk(self, rc):
        if rc < 0:
            raise BmxError(rc, (self.L.bmx_last_error(self.h) or b"").decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.bmx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- host-array (synchronous) API ----
    def load_rows(self, id, field, ts, val):
        id, field, ts, val = _np(id, np.uint64), _np(field, np.uint32), _np(ts, np.int64), _np(val, np.int64)
        self._chk(self.L.bmx_load_rows(self.h, len(id), _ptr(id), _ptr(field), _ptr(ts), _ptr(val), MEM_HOST))

    def put_rows(self, id, field, ts, val):
        """rows decided elsewhere, stored as given (unique keys per call); val == VAL_DELETED leaves a tombstone"""
        id, field, ts, val = _np(id, np.uint64), _np(field, np.uint32), _np(ts, np.int64), _np(val, np.int64)
        self._chk(self.L.bmx_put_rows(self.h, len(id), _ptr(id), _ptr(field), _ptr(ts), _ptr(val), MEM_HOST))

    def merge_batch(self, id, field, ts, val, insert_mode=INSERT_REFERENCE, want_flags=True):
        """Returns (applied_idx u32[w] ascending, flags u8[n] or None, MergeStats)."""
        id, field, ts, val = _np(id, np.uint64), _np(field, np.uint32), _np(ts, np.int64), _np(val, np.int64)
        n = len(id)
        applied = np.zeros(max(n, 1), np.uint32)
        flags = np.zeros(max(n, 1), np.uint8) if want_flags else None
        na = C.c_uint64(0)
        st = MergeStats()
        self._chk(self.L.bmx_merge_batch(self.h, n, _ptr(id), _ptr(field), _ptr(ts), _ptr(val), int(insert_mode), MEM_HOST,
                                         _ptr(applied), C.cast(C.byref(na), C.c_void_p), _ptr(flags), C.cast(C.byref(st), C.c_void_p)))
        return applied[:na.value].copy(), (flags[:n] if want_flags else None), st

    def merge_submit(self, id, field, ts, val, insert_mode=INSERT_REFERENCE, want_flags=False):
        """Upload a host batch and enqueue its merge; -> ticket for merge_collect(). At most two batches in flight."""
        id, field, ts, val = _np(id, np.uint64), _np(field, np.uint32), _np(ts, np.int64), _np(val, np.int64)
        t = C.c_uint64()
        self._chk(self.L.bmx_merge_submit(self.h, len(id), _ptr(id), _ptr(field), _ptr(ts), _ptr(val), int(insert_mode), 1 if want_flags else 0, C.byref(t)))
        return (t.value, len(id), want_flags)

    def merge_collect(self, ticket):
        """-> (applied_idx u32[w], flags u8[n] or None, MergeStats) of a submitted batch (collect in submission order)."""
        t, n, want_flags = ticket
        applied = np.zeros(max(n, 1), np.uint32)
        flags = np.zeros(max(n, 1), np.uint8) if want_flags else None
        na = C.c_uint64(0)
        st = MergeStats()
        self._chk(self.L.bmx_merge_collect(self.h, int(t), _ptr(applied), C.cast(C.byref(na), C.c_void_p), _ptr(flags), C.cast(C.byref(st), C.c_void_p)))
        return applied[:na.value].copy(), (flags[:n] if want_flags else None), st

    def get_rows(self, id, field):
        id, field = _np(id, np.uint64), _np(field, np.uint32)
        n = len(id)
        ts = np.zeros(n, np.int64); val = np.zeros(n, np.int64); found = np.zeros(n, np.uint8)
        self._chk(self.L.bmx_get_rows(self.h, n, _ptr(id), _ptr(field), _ptr(ts), _ptr(val), _ptr(found), MEM_HOST))
        return ts, val, found.astype(bool)

    def get_row(self, id, field):
        ts, val = C.c_int64(), C.c_int64()
        rc = self._chk(self.L.bmx_get_row(self.h, int(id), int(field), C.byref(ts), C.byref(val)))
        return (ts.value, val.value) if rc == 1 else None

    def row_count(self):
        n = C.c_uint64()
        self._chk(self.L.bmx_row_count(self.h, C.byref(n)))
        return n.value

    def reserve(self, capacity_rows):
        self._chk(self.L.bmx_reserve(self.h, int(capacity_rows)))

    def dump_rows(self):
        n = self.row_count()
        id = np.zeros(n, np.uint64); field = np.zeros(n, np.uint32); ts = np.zeros(n, np.int64); val = np.zeros(n, np.int64)
        m = C.c_uint64()
        self._chk(self.L.bmx_dump_rows(self.h, n, _ptr(id), _ptr(field), _ptr(ts), _ptr(val), C.cast(C.byref(m), C.c_void_p), MEM_HOST))
        assert m.value <= n       # tombstones hold a slot (row_count) but are not dumped
        k = m.value
        return id[:k], field[:k], ts[:k], val[:k]

    # ---- replica reconciliation (include/bmx.h; bmx/replica.py drives it) ----
    def digest(self, log2_buckets=10, tombstones=False):
        """-> (sums u64[2^L], counts u64[2^L]): per-bucket sum of the row digests and number of rows; sums.sum() (mod 2^64) is the digest of
        dump_rows(). tombstones=True: tombstoned keys take part, hashed with val = VAL_DELETED."""
        B = 1 << int(log2_buckets)
        sums = np.zeros(B, np.uint64); counts = np.zeros(B, np.uint64)
        self._chk(self.L.bmx_digest(self.h, int(log2_buckets), SYNC_TOMBSTONES if tombstones else 0, _ptr(sums), _ptr(counts), MEM_HOST))
        return sums, counts

    def digest_dev(self, log2_buckets, sums, counts, tombstones=False):
        """same into device memory (u64[2^L] each); enqueue-only"""
        self._chk(self.L.bmx_digest(self.h, int(log2_buckets), SYNC_TOMBSTONES if tombstones else 0, _ptr(sums), _ptr(counts), MEM_DEVICE))

    def export_rows(self, since=0, log2_buckets=0, bucket_bits=None, only_tombstones=False, cap=None, out=None):
        """-> (records, n): the keys with clock >= since whose bucket's bit is set (bucket_bits: u64 words, None = every bucket) as DELTA_REC_DTYPE
        records in table order; n = number of matches, len(records) = min(n, cap). cap=None: everything (one counting call first).
        out: a DELTA_REC_DTYPE array to fill (e.g. in a HostBuffer) — its length is the cap and the result a view of it."""
        bits = _bucket_words(bucket_bits, log2_buckets)
        fl = EXPORT_ONLY_TOMBSTONES if only_tombstones else 0
        m = C.c_uint64()
        if out is not None:
            if out.dtype != DELTA_REC_DTYPE or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a contiguous DELTA_REC_DTYPE array")
            cap = len(out)
        elif cap is None:
            self._chk(self.L.bmx_export_rows(self.h, int(since), int(log2_buckets), _ptr(bits), fl, None, 0, C.cast(C.byref(m), C.c_void_p), MEM_HOST))
            cap = m.value
        recs = out if out is not None else np.zeros(int(cap), DELTA_REC_DTYPE)
        self._chk(self.L.bmx_export_rows(self.h, int(since), int(log2_buckets), _ptr(bits), fl, _ptr(recs) if cap else None, int(cap), C.cast(C.byref(m), C.c_void_p), MEM_HOST))
        return recs[:min(m.value, int(cap))], m.value

    def export_rows_dev(self, out, cap, n_out, since=0, log2_buckets=0, bucket_bits=None, only_tombstones=False):
        """same with device memory: out = room for cap 32-byte records (None: count only), n_out = one u64, bucket_bits = device u64 words or None; enqueue-only"""
        self._chk(self.L.bmx_export_rows(self.h, int(since), int(log2_buckets), _ptr(bucket_bits), EXPORT_ONLY_TOMBSTONES if only_tombstones else 0,
                                         _ptr(out), int(cap), _ptr(n_out), MEM_DEVICE))

    def index_build(self, field):
        self._chk(self.L.bmx_index_build(self.h, int(field)))

    def index_drop(self, field):
        self._chk(self.L.bmx_index_drop(self.h, int(field)))

    def index_size(self, field):
        n = C.c_uint64()
        self._chk(self.L.bmx_index_size(self.h, int(field), C.byref(n)))
        return n.value

    def index_refresh_counts(self):
        """-> (full index builds, incremental updates from the change log) since the engine was created"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.L.bmx_index_refresh_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def index_set_ordered(self, field, after_queries=1):
        """value-ordered view of the index (bmx_index_set_ordered): sorted again by the after_queries-th query since the field last changed; 0 = off"""
        self._chk(self.L.bmx_index_set_ordered(self.h, int(field), int(after_queries)))

    def index_ordered_info(self, field):
        """-> (after_queries, would the view answer the next query, sorts so far)"""
        a, v, n = C.c_uint32(), C.c_int32(), C.c_uint64()
        self._chk(self.L.bmx_index_ordered_info(self.h, int(field), C.byref(a), C.byref(v), C.byref(n)))
        return a.value, bool(v.value), n.value

    def index_ordered_stats(self, field):
        """{sorts, patches, keys_patched, last_sort_us, last_patch_us, rewrites (streaming merges into the view's main run), pending_keys} of the value-ordered view"""
        a, b, c, f, g = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        d, e = C.c_double(), C.c_double()
        self._chk(self.L.bmx_index_ordered_stats(self.h, int(field), C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e), C.byref(f), C.byref(g)))
        return {"sorts": a.value, "patches": b.value, "keys_patched": c.value, "last_sort_us": d.value, "last_patch_us": e.value, "rewrites": f.value, "pending_keys": g.value}

    def scan_range(self, field, lo, hi, cap=None, out=None):
        """ids of the rows whose value is in [lo, hi]. `out`: a caller's uint64 array the ids are written into (a view of it is returned, no copy) —
        one taken from a HostBuffer comes back at the link's rate."""
        if out is not None:
            cap = len(out) if cap is None else min(cap, len(out))
            m = C.c_uint64()
            self._chk(self.L.bmx_scan_range(self.h, int(field), int(lo), int(hi), _ptr(out), cap, C.cast(C.byref(m), C.c_void_p), MEM_HOST))
            return out[:min(m.value, cap)]
        cap = self.index_size(field) if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint64)
        m = C.c_uint64()
        self._chk(self.L.bmx_scan_range(self.h, int(field), int(lo), int(hi), _ptr(out), cap, C.cast(C.byref(m), C.c_void_p), MEM_HOST))
        return out[:min(m.value, cap)].copy()

    def scan_range_pos(self, field, lo, hi, cap=None):
        """positions (u32, ascending) of the matches in the index columns instead of their node ids"""
        cap = self.index_size(field) if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint32)
        m = C.c_uint64()
        self._chk(self.L.bmx_scan_range_pos(self.h, int(field), int(lo), int(hi), _ptr(out), cap, C.cast(C.byref(m), C.c_void_p), MEM_HOST))
        return out[:min(m.value, cap)].copy()

    def index_ids(self, field, first=0, count=None):
        count = self.index_size(field) - first if count is None else count
        out = np.zeros(max(count, 1), np.uint64)
        self._chk(self.L.bmx_index_ids(self.h, int(field), int(first), int(count), _ptr(out), MEM_HOST))
        return out[:count].copy()

    def scan_equals(self, field, value):
        return self.scan_range(field, value, value)

    def scan_count(self, field, lo, hi):
        m = C.c_uint64()
        self._chk(self.L.bmx_scan_count(self.h, int(field), int(lo), int(hi), C.cast(C.byref(m), C.c_void_p), MEM_HOST))
        return m.value

    def scan_filter(self, terms, cap=None):
        arr = (Term * len(terms))(*[Term(int(f), 0, int(lo), int(hi)) for f, lo, hi in terms])
        cap = self.index_size(terms[0][0]) if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint64)
        m = C.c_uint64()
        self._chk(self.L.bmx_scan_filter(self.h, len(terms), arr, _ptr(out), cap, C.cast(C.byref(m), C.c_void_p), MEM_HOST))
        return out[:min(m.value, cap)].copy()

    def scan_aggregate(self, terms, measure=None, group=None, group_lo=0, ngroups=0):
        """count / sum / min / max of field `measure` over the nodes that satisfy every (field, lo, hi) of `terms`, without fetching an id. ngroups == 0:
        one AggResult; otherwise the list of ngroups + 1: entry g for value(group) == group_lo + g, the last for the nodes outside the window."""
        out = np.zeros(int(ngroups) + 1, AGG_DTYPE)
        self._chk(self.L.bmx_scan_aggregate(self.h, *_agg_args(terms, measure, group, group_lo, ngroups), _ptr(out), MEM_HOST))
        return agg_results(out, int(ngroups))

    def scan_top(self, terms, k, desc=False, after=None):
        """The first k nodes, ordered by (value of terms[0]'s field, id) — value descending with desc — of the nodes that satisfy every (field, lo, hi) of
        `terms` and come strictly after the cursor `after` (a record of an earlier answer, or (id, val); None: from the beginning).
        -> (records: ndarray of TOP_DTYPE, n_eligible)"""
        out = np.zeros(max(int(k), 1), TOP_DTYPE)
        m, ne = C.c_uint64(), C.c_uint64()
        self._chk(self.L.bmx_scan_top(self.h, *_top_args(terms, k, desc, after), _ptr(out), C.cast(C.byref(m), C.c_void_p), C.cast(C.byref(ne), C.c_void_p), MEM_HOST))
        return out[:m.value].copy(), ne.value

    def scan_where(self, base, clauses, cap=None, count_only=False):
        """Boolean filter (bmx_where.h): the nodes holding data in field `base` for which some clause of `clauses` has all of its literals true; a literal is
        (field, lo, hi) or (field, lo, hi, negated), the negated one being true for an absent or tombstoned field too. -> ids in index order of `base`
        (at most cap of them). count_only (as Comm.scan_where has it): -> the number of matches, no id is fetched."""
        args = _where_args(base, clauses)
        m = C.c_uint64()
        if count_only:
            self._chk(self.L.bmx_scan_where(self.h, *args, None, 0, C.cast(C.byref(m), C.c_void_p), MEM_HOST))
            return m.value
        cap = self.index_size(base) if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint64)
        self._chk(self.L.bmx_scan_where(self.h, *args, _ptr(out), cap, C.cast(C.byref(m), C.c_void_p), MEM_HOST))
        return out[:min(m.value, cap)].copy()

    def where_aggregate(self, base, clauses, measure=None, group=None, group_lo=0, ngroups=0):
        """scan_aggregate over the selection of scan_where(base, clauses) (bmx_where_agg.h): count / sum / min / max of field `measure`, grouped by field `group`
        in the window group_lo .. group_lo + ngroups - 1, without fetching an id. -> what scan_aggregate returns"""
        out = np.zeros(int(ngroups) + 1, AGG_DTYPE)
        self._chk(self.L.bmx_where_aggregate(self.h, *_where_args(base, clauses), *_where_agg_tail(measure, group, group_lo, ngroups), _ptr(out), MEM_HOST))
        return agg_results(out, int(ngroups))

    def where_top(self, base, clauses, k, desc=False, after=None):
        """scan_top over the selection of scan_where(base, clauses): the first k nodes ordered by (value of `base`, id) — value descending with desc — that come
        strictly after the cursor `after`. -> (records: ndarray of TOP_DTYPE, n_eligible)"""
        out = np.zeros(max(int(k), 1), TOP_DTYPE)
        m, ne = C.c_uint64(), C.c_uint64()
        self._chk(self.L.bmx_where_top(self.h, *_where_args(base, clauses), *_where_top_tail(k, desc, after), _ptr(out), C.cast(C.byref(m), C.c_void_p),
                                       C.cast(C.byref(ne), C.c_void_p), MEM_HOST))
        return out[:m.value].copy(), ne.value

    def where_group(self, base, clauses, group, measure=None, cap=65536):
        """Group-by over discovered values (bmx_group.h): count / sum / min / max of field `measure` over the selection of scan_where(base, clauses), one
        record per distinct value of field `group` that occurs among the selected nodes; nobody has to know the values in advance. -> GroupResult (with
        overflow set and no records when there are more than cap distinct values: ask again with more room or a narrower program)"""
        out = np.zeros(max(int(cap), 1), GROUP_DTYPE)
        res = GroupRes()
        self._chk(self.L.bmx_where_group(self.h, *_where_args(base, clauses), *_group_tail(measure, group), _ptr(out), int(cap), C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return GroupResult(res, out)

    def where_quantiles(self, base, clauses, measure, qs):
        """Exact quantiles (bmx_quant.h): the order statistics of field `measure` over the selection of scan_where(base, clauses), selected on the device.
        qs: up to QUANT_MAX pairs (num, den), in any order, repeats allowed. -> (records: ndarray of QUANT_REC_DTYPE in the order of qs — value, rank
        (quant_rank(num, den, n)), n_below, n_equal — and a QuantRes: n_match, n, min, max)"""
        out = np.zeros(max(len(qs), 1), QUANT_REC_DTYPE)
        res = QuantRes()
        self._chk(self.L.bmx_where_quantiles(self.h, *_where_args(base, clauses), *_quant_tail(measure, qs), _ptr(out), C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return out[:len(qs)].copy(), res

    def where_aggregate_expr(self, base, clauses, expr, group=None, group_lo=0, ngroups=0):
        """where_aggregate with a computed measure (bmx_expr.h): expr = bmx.Expr(a, op, b), the measure of a selected node is value(a) op value(b).
        -> (what where_aggregate returns, ExprRes)"""
        out = np.zeros(int(ngroups) + 1, AGG_DTYPE)
        x = ExprRes()
        self._chk(self.L.bmx_where_aggregate_expr(self.h, *_where_args(base, clauses), C.cast(C.byref(expr), C.c_void_p), *_where_agg_tail(None, group, group_lo, ngroups)[1:],
                                                  _ptr(out), C.cast(C.byref(x), C.c_void_p), MEM_HOST))
        return agg_results(out, int(ngroups)), x

    def where_group_expr(self, base, clauses, group, expr, cap=65536):
        """where_group with a computed measure (bmx_expr.h). -> (GroupResult, ExprRes)"""
        out = np.zeros(max(int(cap), 1), GROUP_DTYPE)
        res, x = GroupRes(), ExprRes()
        self._chk(self.L.bmx_where_group_expr(self.h, *_where_args(base, clauses), C.cast(C.byref(expr), C.c_void_p), _group_tail(None, group)[1], _ptr(out), int(cap),
                                              C.cast(C.byref(res), C.c_void_p), C.cast(C.byref(x), C.c_void_p), MEM_HOST))
        return GroupResult(res, out), x

    def where_quantiles_expr(self, base, clauses, expr, qs):
        """where_quantiles with a computed measure (bmx_expr.h): the sample is value(a) op value(b) of the selected nodes where it is defined and in range.
        -> (records, QuantRes, ExprRes)"""
        out = np.zeros(max(len(qs), 1), QUANT_REC_DTYPE)
        res, x = QuantRes(), ExprRes()
        self._chk(self.L.bmx_where_quantiles_expr(self.h, *_where_args(base, clauses), C.cast(C.byref(expr), C.c_void_p), *_quant_tail(0, qs)[1:], _ptr(out),
                                                  C.cast(C.byref(res), C.c_void_p), C.cast(C.byref(x), C.c_void_p), MEM_HOST))
        return out[:len(qs)].copy(), res, x

    def where_rows(self, base, clauses, fields, cap=None, with_ts=False, start=0):
        """Row projection (bmx_rows.h): the selection of scan_where(base, clauses) from index position `start` on, and for each of the first cap selected nodes
        its id and the values (with_ts: and clocks) of `fields`, in one call. cap None: room for the whole index. -> RowsResult; its next_pos is the `start` of
        the next page."""
        cap = self.index_size(base) if cap is None else int(cap)
        nf, farr, flags = _rows_fields(fields, with_ts)
        ids, vals, ts = _rows_buffers(nf, cap, with_ts)
        res = RowsRes()
        self._chk(self.L.bmx_where_rows(self.h, *_where_args(base, clauses), nf, farr, flags, int(start), cap, _ptr(ids), _ptr(vals), _ptr(ts),
                                        C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return RowsResult(res, ids, vals, ts)

    def where_group_first(self, base, clauses, group, order, fields=(), desc=False, with_ts=False, cap=65536):
        """The first node per group (bmx_first.h): per distinct value of field `group` among the selection of scan_where(base, clauses), the node that comes
        first by the value of field `order` (descending with desc), then by id (always ascending, unsigned), with the values (with_ts: and clocks) of
        `fields` on that node. -> FirstResult (with overflow set and no records when there are more than cap distinct values)"""
        cap = int(cap)
        tail = _first_tail(group, order, fields, desc, with_ts)
        out, vals, ts = _first_buffers(tail[2], cap, with_ts)
        res = FirstRes()
        self._chk(self.L.bmx_where_group_first(self.h, *_where_args(base, clauses), *tail, cap, _ptr(out), _ptr(vals), _ptr(ts), C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return FirstResult(res, out, vals, ts)

    def where_group_top(self, base, clauses, group, order, per, fields=(), desc=False, with_ts=False, cap=65536):
        """The first `per` nodes per group (bmx_group_top.h): per distinct value of field `group` among the selection of scan_where(base, clauses), the `per`
        nodes that come first by the value of field `order` (descending with desc), then by id (always ascending, unsigned), in that order, with the values
        (with_ts: and clocks) of `fields` on each. -> GroupTopResult (with overflow set and no groups when there are more than cap distinct values)"""
        cap, per = int(cap), int(per)
        tail = _gtop_tail(group, order, per, fields, desc, with_ts)
        ok = 1 <= per <= GTOP_MAX_PER and 1 <= cap <= GTOP_MAX_CAP and cap * per <= GTOP_MAX_ROWS        # (otherwise the library refuses: no buffers needed)
        out, rows, vals, ts = _gtop_buffers(tail[3], cap if ok else 1, per if ok else 1, with_ts)
        res = GtopRes()
        self._chk(self.L.bmx_where_group_top(self.h, *_where_args(base, clauses), *tail, cap, _ptr(out), _ptr(rows), _ptr(vals), _ptr(ts), C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return GroupTopResult(res, out, rows, vals, ts)

    def where_group_multi(self, base, clauses, keys, measure=None, cap=65536):
        """Group-by over several fields (bmx_group_multi.h): count / sum / min / max of field `measure` over the selection of scan_where(base, clauses), one
        record per distinct key tuple that occurs among the selected nodes. keys: 1..4 of `field` (the value itself) or (field, origin, width) (the bucket
        (value - origin) // width). A node that lacks any key is counted in absent. -> MultiGroupResult (with overflow set and no groups if there are more
        than cap tuples; cap <= GROUP_MAX_CAP, <= MGROUP_MAX_CAP4 with four keys)."""
        out = np.zeros(max(int(cap), 1), MGROUP_DTYPE)
        res = GroupRes()
        nk, karr = _mgroup_keys(keys)
        self._chk(self.L.bmx_where_group_multi(self.h, *_where_args(base, clauses), AGG_NO_FIELD if measure is None else int(measure), nk, karr, _ptr(out), int(cap),
                                               C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return MultiGroupResult(res, out, nk)

    def where_update(self, base, clauses, target, op, operand=0, src=None, ts=None, force=False, cap=None, start=0, want_ids=False):
        """Update by query (bmx_update.h): on every node scan_where(base, clauses) selects from index position `start` on, field `target` gets the record
        (ts, val), val being `operand` (UPD_SET), a tombstone (UPD_DELETE; needs force), the node's value of `src` (UPD_COPY) or that value + operand (UPD_ADD).
        Default: through conflict resolution like merge_batch(INSERT_DELTA); force: stored as given like put_rows. cap None: min(index size, UPD_MAX_CAP);
        cap 0 counts only. ts None: the wall clock in milliseconds. want_ids: the ids of the nodes whose row changed. -> UpdateResult; its next_pos is the `start` of the next page."""
        cap = min(self.index_size(base), UPD_MAX_CAP) if cap is None else int(cap)
        ids = np.zeros(max(cap, 1), np.uint64) if want_ids else None
        res = UpdRes()
        self._chk(self.L.bmx_where_update(self.h, *_where_args(base, clauses), *_upd_args(target, op, operand, src, ts, force), int(start), cap, _ptr(ids),
                                          C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return UpdateResult(res, ids)

    def where_update_all(self, base, clauses, target, op, operand=0, src=None, ts=None, force=False, page=1 << 22):
        """where_update over the whole selection in pages of `page` records: counts first (cap 0), reserves room for row_count + n_match rows so that no page
        grows the table and lays the index out anew (which would make UPD_ADD onto its own source add twice when started over), then pages along the cursor
        and sums the results. -> UpdateResult (n_match, n_nosrc, n_range of the whole selection; ids None). Raises BmxError(ERR_INTERNAL) if the layout
        changes between two pages all the same, and says how many nodes were done."""
        first = self.where_update(base, clauses, target, op, operand, src, ts, force, cap=0)
        self.reserve(self.row_count() + first.n_match)
        tot = np.zeros(1, UPD_RES_DTYPE)[0]
        start, layout = 0, None
        while True:
            r = self.where_update(base, clauses, target, op, operand, src, ts, force, cap=int(page), start=start)
            if layout is not None and r.layout != layout:
                raise BmxError(ERR_INTERNAL, "where_update_all: the index was laid out anew between two pages; %d nodes were sent and %d rows changed before that"
                               % (int(tot["n_sent"]), int(tot["n_applied"])))
            if layout is None:
                tot["n_match"], tot["n_nosrc"], tot["n_range"] = r.n_match, r.n_nosrc, r.n_range
            layout = r.layout
            tot["n_sent"] += r.n_sent; tot["n_applied"] += r.n_applied
            tot["n_rows"], tot["next_pos"], tot["layout"] = r.n_rows, r.next_pos, r.layout
            if r.n_match - r.n_nosrc - r.n_range <= r.n_sent:
                return UpdateResult(tot)
            start = r.next_pos

    def where_semijoin(self, base, clauses, link, inner_base, inner_clauses, key, anti=False, cap=None, set_cap=65536, count_only=False):
        """Semi-join (bmx_semi.h): the selection of scan_where(base, clauses) whose field `link` holds a value that field `key` holds on some node of
        scan_where(inner_base, inner_clauses); anti: whose `link` holds no such value (or nothing). The set is built and tested on the device. cap None: room
        for the whole index of `base`; count_only: no id is fetched. -> SemiResult (with overflow set, n_match 0 and no ids when the inner side has more than
        set_cap distinct keys)"""
        cap = 0 if count_only else (self.index_size(base) if cap is None else int(cap))
        ids = None if count_only else np.zeros(max(cap, 1), np.uint64)
        res = SemiRes()
        self._chk(self.L.bmx_where_semijoin(self.h, *_where_args(base, clauses), int(link), SEMI_ANTI if anti else 0, *_where_args(inner_base, inner_clauses), int(key),
                                            int(set_cap), _ptr(ids), cap, C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return SemiResult(res, ids, cap)

    def where_in(self, base, clauses, link, values, anti=False, cap=None, count_only=False):
        """where_semijoin with the set given as a list of 1..SEMI_MAX_SET int64 values (duplicates allowed; a value outside +-(2^53 - 1) is skipped)"""
        cap = 0 if count_only else (self.index_size(base) if cap is None else int(cap))
        ids = None if count_only else np.zeros(max(cap, 1), np.uint64)
        v, n = _semi_values(values)
        res = SemiRes()
        self._chk(self.L.bmx_where_in(self.h, *_where_args(base, clauses), int(link), SEMI_ANTI if anti else 0, _ptr(v), n, _ptr(ids), cap,
                                      C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return SemiResult(res, ids, cap)

    def where_reach(self, base, clauses, link, key, seed_base, seed_clauses, seed_field, max_depth=REACH_MAX_DEPTH, set_cap=65536, cap=None, count_only=False):
        """Graph traversal (bmx_reach.h): the nodes of scan_where(base, clauses) reachable, over the edges link -> key of those nodes, from the values field
        `seed_field` holds on the nodes of scan_where(seed_base, seed_clauses), with their breadth-first depth; swapping link and key walks toward the
        ancestors. The closure runs on the device. cap None: room for the whole index of `base`; count_only: nothing is fetched. -> ReachResult (with overflow
        set, n_match 0 and no ids when seeds and contributed values are more than set_cap)"""
        cap = 0 if count_only else (self.index_size(base) if cap is None else int(cap))
        ids = None if count_only else np.zeros(max(cap, 1), np.uint64)
        depth = None if count_only else np.zeros(max(cap, 1), np.uint8)
        res = ReachRes()
        self._chk(self.L.bmx_where_reach(self.h, *_where_args(base, clauses), int(link), int(key), 0, *_where_args(seed_base, seed_clauses), int(seed_field),
                                         int(max_depth), int(set_cap), _ptr(ids), _ptr(depth), cap, C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return ReachResult(res, ids, depth, cap)

    def where_reach_from(self, base, clauses, link, key, values, max_depth=REACH_MAX_DEPTH, set_cap=65536, cap=None, count_only=False):
        """where_reach with the seeds given as a list of 1..REACH_MAX_SET int64 values (duplicates allowed; a value outside +-(2^53 - 1) is skipped)"""
        cap = 0 if count_only else (self.index_size(base) if cap is None else int(cap))
        ids = None if count_only else np.zeros(max(cap, 1), np.uint64)
        depth = None if count_only else np.zeros(max(cap, 1), np.uint8)
        v, n = _semi_values(values)
        res = ReachRes()
        self._chk(self.L.bmx_where_reach_from(self.h, *_where_args(base, clauses), int(link), int(key), 0, _ptr(v), n, int(max_depth), int(set_cap), _ptr(ids),
                                              _ptr(depth), cap, C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return ReachResult(res, ids, depth, cap)

    def where_join_group(self, base, clauses, link, inner_base, inner_clauses, key, attr, measure=None, cap=65536, map_cap=65536):
        """Lookup join (bmx_join.h): the selection of scan_where(base, clauses) grouped by the value field `attr` holds on the node of
        scan_where(inner_base, inner_clauses) whose field `key` equals the selected node's field `link` (the minimum of `attr` where several inner nodes share a
        key). The map is built and looked up on the device. -> JoinResult"""
        out = np.zeros(max(int(cap), 1), GROUP_DTYPE)
        res = JoinRes()
        self._chk(self.L.bmx_where_join_group(self.h, *_where_args(base, clauses), int(link), AGG_NO_FIELD if measure is None else int(measure),
                                              *_where_args(inner_base, inner_clauses), int(key), int(attr), int(map_cap), _ptr(out), int(cap),
                                              C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return JoinResult(res, out)

    def where_map_group(self, base, clauses, link, keys, vals, measure=None, cap=65536):
        """where_join_group with the map given as 1..JOIN_MAX_MAP (key, val) pairs (a key outside +-(2^53 - 1) is skipped, a val outside it means "no
        attribute", duplicate keys take the minimum of their vals)"""
        k, v, n = _join_pairs(keys, vals)
        out = np.zeros(max(int(cap), 1), GROUP_DTYPE)
        res = JoinRes()
        self._chk(self.L.bmx_where_map_group(self.h, *_where_args(base, clauses), int(link), AGG_NO_FIELD if measure is None else int(measure), _ptr(k), _ptr(v), n,
                                             _ptr(out), int(cap), C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return JoinResult(res, out)

    def where_join_rows(self, base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, cap=None, with_ts=False, inner=False, start=0, map_cap=65536):
        """Join projection (bmx_join_rows.h): the selection of scan_where(base, clauses) from index position `start` on, each row with the values (with_ts:
        and clocks) of `fields` and with the id and the `in_fields` of the node of scan_where(inner_base, inner_clauses) whose field `key` equals the row's
        field `link` (the smallest unsigned id where several share a key). A left join; inner=True drops the rows without inner node from the selection. cap
        None: room for the whole index of `base`. -> JoinRowsResult"""
        cap = self.index_size(base) if cap is None else int(cap)
        nf, farr, _ = _rows_fields(fields, with_ts)
        nif, ifarr, _ = _rows_fields(in_fields, with_ts)
        return _jrows_host(lambda *a: self.L.bmx_where_join_rows(*a, MEM_HOST), self.h, self._chk, (*_where_args(base, clauses), int(link), nf, farr),
                           (*_where_args(inner_base, inner_clauses), int(key), nif, ifarr, int(map_cap), _jrows_flags(with_ts, inner), int(start)), nf, nif, with_ts, cap)

    def where_map_rows(self, base, clauses, link, fields, keys, node_ids, in_fields, cap=None, with_ts=False, inner=False, start=0):
        """where_join_rows with the map given as 1..JOIN_MAX_MAP (key, node id) pairs (a key outside +-(2^53 - 1) or the id JROWS_NO_NODE is skipped,
        duplicate keys take the smallest id)"""
        cap = self.index_size(base) if cap is None else int(cap)
        nf, farr, _ = _rows_fields(fields, with_ts)
        nif, ifarr, _ = _rows_fields(in_fields, with_ts)
        k, v, n = _jrows_pairs(keys, node_ids)
        return _jrows_host(lambda *a: self.L.bmx_where_map_rows(*a, MEM_HOST), self.h, self._chk, (*_where_args(base, clauses), int(link), nf, farr),
                           (_ptr(k), _ptr(v), n, nif, ifarr, _jrows_flags(with_ts, inner), int(start)), nf, nif, with_ts, cap)

    def watch_create(self, base, clauses):
        """A standing query (bmx_watch.h): the program of scan_where(base, clauses), kept on the device together with its last committed answer. -> the watch id"""
        w = C.c_uint32()
        self._chk(self.L.bmx_watch_create(self.h, *_where_args(base, clauses), C.byref(w)))
        self._watch_base[w.value] = int(base)
        return w.value

    def watch_poll(self, w, cap_entered=None, cap_left=None):
        """What changed in the watch's answer since its last committed poll -> WatchPoll. A cap of None is room for the whole index (such a poll always commits)."""
        if cap_entered is None or cap_left is None:
            base = self._watch_base.get(int(w))
            n = self.index_size(base) if base is not None else 0       # (an unknown id: the library refuses it below)
            cap_entered = n if cap_entered is None else cap_entered
            cap_left = n if cap_left is None else cap_left
        ent, lft, res = np.zeros(max(int(cap_entered), 1), np.uint64), np.zeros(max(int(cap_left), 1), np.uint64), WatchRes()
        self._chk(self.L.bmx_watch_poll(self.h, int(w), _ptr(ent), int(cap_entered), _ptr(lft), int(cap_left), C.cast(C.byref(res), C.c_void_p), MEM_HOST))
        return WatchPoll(res, ent[:int(cap_entered)], lft[:int(cap_left)])

    def watch_destroy(self, w):
        self._chk(self.L.bmx_watch_destroy(self.h, int(w)))
        self._watch_base.pop(int(w), None)

    def info(self):
        i = Info()
        self._chk(self.L.bmx_get_info(self.h, C.byref(i)))
        return i

    # ---- device-pointer (asynchronous) API: arguments are torch CUDA tensors or raw device addresses ----
    def sync(self):
        self._chk(self.L.bmx_sync(self.h))

    def set_stream(self, stream_ptr):
        self._chk(self.L.bmx_set_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def set_deferred(self, on):
        """deferred compaction (bmx.h): the winner compaction of a device batch runs under the NEXT batch's probe kernel. On by default."""
        self._chk(self.L.bmx_set_deferred_compaction(self.h, 1 if on else 0))

    def set_side_stream(self, stream_ptr):
        """the stream the deferred compactions run on (0 / None: the context's own high-priority stream)"""
        self._chk(self.L.bmx_set_side_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def set_wait_limit(self, seconds):
        """device-side waits on this context's GPU give up after this long (default ~60 s): bmx_set_wait_limit"""
        self._chk(self.L.bmx_set_wait_limit(self.h, float(seconds)))

    def merge_fence(self):
        """enqueue-only: the engine's stream is ordered behind every compaction (for work the caller enqueues on that stream itself)"""
        self._chk(self.L.bmx_merge_fence(self.h))

    def set_probe_waves(self, waves_per_simd):
        """resident waves per SIMD the probe kernel may take (8, 6, 5, 4, 3): fewer leave room for kernels that run beside it (bmx_set_probe_waves)"""
        self._chk(self.L.bmx_set_probe_waves(self.h, int(waves_per_simd)))

    def claim_mode(self):
        """how the probe kernel claims a row: "team" (head, ts and val in one memory-side request) or "store" (exchange + store); BMX_CLAIM_MODE at create"""
        m = self.L.bmx_get_claim_mode(self.h)
        if m < 0:
            self._chk(m)
        return "team" if m == 1 else "store"

    def placement(self):
        """table placement tuning at create / growth: {candidates, probe_us_chosen, probe_us_slowest} (candidates 0: not tuned)"""
        n, a, b = C.c_uint32(), C.c_float(), C.c_float()
        self._chk(self.L.bmx_get_placement(self.h, C.byref(n), C.byref(a), C.byref(b)))
        return {"candidates": n.value, "probe_us_chosen": round(a.value, 2), "probe_us_slowest": round(b.value, 2)}

    def deferred_counts(self):
        """(merges whose compaction was deferred, of those: run on the side stream under the next probe kernel)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.L.bmx_get_deferred_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def seq_signal(self, stream_ptr, seq_dev, value):
        """enqueue on the stream (0 = the engine's): *seq_dev = value once everything before it on that stream is done."""
        self._chk(self.L.bmx_seq_signal(self.h, C.c_void_p(stream_ptr) if stream_ptr else None, _ptr(seq_dev), int(value)))

    def seq_wait(self, stream_ptr, seq_dev, at_least):
        """enqueue on the stream a device-side wait until *seq_dev >= at_least (the matching signal must already be enqueued)."""
        self._chk(self.L.bmx_seq_wait(self.h, C.c_void_p(stream_ptr) if stream_ptr else None, _ptr(seq_dev), int(at_least)))

    def load_rows_dev(self, n, id, field, ts, val):
        self._chk(self.L.bmx_load_rows(self.h, int(n), _ptr(id), _ptr(field), _ptr(ts), _ptr(val), MEM_DEVICE))

    def merge_batch_dev(self, n, id, field, ts, val, insert_mode=INSERT_REFERENCE, applied=None, n_applied=None, flags=None, stats=None):
        self._chk(self.L.bmx_merge_batch(self.h, int(n), _ptr(id), _ptr(field), _ptr(ts), _ptr(val), int(insert_mode), MEM_DEVICE,
                                         _ptr(applied), _ptr(n_applied), _ptr(flags), _ptr(stats)))

    def merge_records_dev(self, n, recs, insert_mode=INSERT_REFERENCE, applied=None, n_applied=None, flags=None, stats=None):
        self._chk(self.L.bmx_merge_records(self.h, int(n), _ptr(recs), int(insert_mode), _ptr(applied), _ptr(n_applied), _ptr(flags), _ptr(stats)))

    def partition_by_owner_dev(self, n, id, field, ts, val, nshards, recs_out, counts_out):
        self._chk(self.L.bmx_partition_by_owner(self.h, int(n), _ptr(id), _ptr(field), _ptr(ts), _ptr(val), int(nshards), _ptr(recs_out), _ptr(counts_out)))

    # ---- direct exchange between processes (bmx_ipc_* / bmx_partition_scatter): pointers are plain ints here ----
    def ipc_alloc(self, nbytes, uncached=True):
        """-> (device pointer, 64-byte handle another process opens with ipc_open). uncached: never served from this GPU's L2 (peers store into it)"""
        p = C.c_void_p()
        h = C.create_string_buffer(64)
        self._chk(self.L.bmx_ipc_alloc(self.h, int(nbytes), 1 if uncached else 0, C.byref(p), h))
        return int(p.value), h.raw

    def ipc_open(self, handle, peer_device=-1):
        p = C.c_void_p()
        self._chk(self.L.bmx_ipc_open(self.h, C.create_string_buffer(bytes(handle), 64), int(peer_device), C.byref(p)))
        return int(p.value)

    def ipc_close(self, ptr):
        self._chk(self.L.bmx_ipc_close(self.h, C.c_void_p(int(ptr))))

    def ipc_free(self, ptr):
        self._chk(self.L.bmx_ipc_free(self.h, C.c_void_p(int(ptr))))

    def partition_scatter_dev(self, n, id, field, ts, val, nshards, slab_records, dst_ptrs, counts_out, arrive_ptrs=None, arrive_value=0):
        """owner partition writing slab g straight to dst_ptrs[g] (this GPU's or a peer's memory); arrive_ptrs[g] := arrive_value when all is stored"""
        dst = (C.c_void_p * int(nshards))(*[C.c_void_p(int(x)) for x in dst_ptrs])
        arr = (C.c_void_p * int(nshards))(*[C.c_void_p(int(x)) if x else None for x in arrive_ptrs]) if arrive_ptrs is not None else None
        self._chk(self.L.bmx_partition_scatter(self.h, int(n), _ptr(id), _ptr(field), _ptr(ts), _ptr(val), int(nshards), int(slab_records), dst, _ptr(counts_out),
                                               arr, int(arrive_value), None, 0, 0))

    @staticmethod
    def ptr_array(ptrs):
        """a C array of device pointers, built once and reused (partition_scatter_raw): keeps the per-step host cost down"""
        return (C.c_void_p * max(len(ptrs), 1))(*[C.c_void_p(int(x)) if x else None for x in ptrs])

    def partition_scatter_raw(self, n, id, field, ts, val, nshards, slab_records, dst_arr, counts_out, arrive_arr, arrive_value, wait_ptr=0, n_wait=0, wait_at_least=0):
        """one host call per route: (optional) wait until n_wait words at wait_ptr are >= wait_at_least, partition + scatter, arrival words"""
        self._chk(self.L.bmx_partition_scatter(self.h, n, _ptr(id), _ptr(field), _ptr(ts), _ptr(val), nshards, slab_records, dst_arr, _ptr(counts_out),
                                               arrive_arr, arrive_value, wait_ptr if wait_ptr else None, n_wait, wait_at_least))

    def merge_records_after(self, wait_ptr, n_wait, wait_at_least, n, recs_ptr, insert_mode, applied, n_applied):
        """one host call per merge: wait for the arrival words, then merge the records"""
        self._chk(self.L.bmx_merge_records_after(self.h, wait_ptr, n_wait, wait_at_least, n, recs_ptr, insert_mode, _ptr(applied), _ptr(n_applied), None, None))

    def seq_wait_all(self, stream_ptr, words_ptr, nwords, at_least):
        self._chk(self.L.bmx_seq_wait_all(self.h, C.c_void_p(stream_ptr) if stream_ptr else None, _ptr(words_ptr), int(nwords), int(at_least)))

    def merge_tail_wait(self, words_ptr, nwords, at_least):
        """the NEXT merge's resolve kernel ends only once the words are >= at_least (bmx_merge_tail_wait); 0 words disarms"""
        self._chk(self.L.bmx_merge_tail_wait(self.h, C.c_void_p(int(words_ptr)) if words_ptr else None, int(nwords), int(at_least)))

    def merge_notify(self, word_ptrs):
        """every later merge stores the count of merges finished since into these words (peers' memory); [] switches it off"""
        n = len(word_ptrs)
        arr = (C.c_void_p * max(n, 1))(*[C.c_void_p(int(x)) if x else None for x in word_ptrs]) if n else None
        self._chk(self.L.bmx_merge_notify(self.h, arr, n))

    def partition_by_owner_slabs_dev(self, n, id, field, ts, val, nshards, slab_records, recs_out, counts_out):
        self._chk(self.L.bmx_partition_by_owner_slabs(self.h, int(n), _ptr(id), _ptr(field), _ptr(ts), _ptr(val), int(nshards), int(slab_records),
                                                      _ptr(recs_out), _ptr(counts_out)))

    def scan_range_dev(self, field, lo, hi, out_ids, cap, n_out):
        self._chk(self.L.bmx_scan_range(self.h, int(field), int(lo), int(hi), _ptr(out_ids), int(cap), _ptr(n_out), MEM_DEVICE))

    def scan_aggregate_dev(self, terms, out, measure=None, group=None, group_lo=0, ngroups=0):
        """scan_aggregate into device memory (`out`: room for ngroups + 1 records of 48 bytes, or 1 with ngroups == 0); enqueue-only — after sync(),
        agg_results(out.cpu().numpy().view(AGG_DTYPE), ngroups) reads it"""
        self._chk(self.L.bmx_scan_aggregate(self.h, *_agg_args(terms, measure, group, group_lo, ngroups), _ptr(out), MEM_DEVICE))

    def scan_top_dev(self, terms, k, out, n_out=None, n_eligible=None, desc=False, after=None):
        """scan_top into device memory (`out`: room for k records of 16 bytes; n_out, n_eligible: one uint64 each, or None); enqueue-only. The cursor is
        host data either way."""
        self._chk(self.L.bmx_scan_top(self.h, *_top_args(terms, k, desc, after), _ptr(out), _ptr(n_out), _ptr(n_eligible), MEM_DEVICE))

    def scan_where_dev(self, base, clauses, out, cap, n_out):
        """scan_where into device memory (`out`: room for cap ids, or None to count; n_out: one uint64); enqueue-only. The program is host data."""
        self._chk(self.L.bmx_scan_where(self.h, *_where_args(base, clauses), _ptr(out), int(cap), _ptr(n_out), MEM_DEVICE))

    def where_aggregate_dev(self, base, clauses, out, measure=None, group=None, group_lo=0, ngroups=0):
        """where_aggregate into device memory (`out` as for scan_aggregate_dev); enqueue-only. The program is host data."""
        self._chk(self.L.bmx_where_aggregate(self.h, *_where_args(base, clauses), *_where_agg_tail(measure, group, group_lo, ngroups), _ptr(out), MEM_DEVICE))

    def where_top_dev(self, base, clauses, k, out, n_out=None, n_eligible=None, desc=False, after=None):
        """where_top into device memory (`out`, n_out, n_eligible as for scan_top_dev); enqueue-only. The program and the cursor are host data."""
        self._chk(self.L.bmx_where_top(self.h, *_where_args(base, clauses), *_where_top_tail(k, desc, after), _ptr(out), _ptr(n_out), _ptr(n_eligible), MEM_DEVICE))

    def where_group_dev(self, base, clauses, group, out, res, measure=None, cap=65536):
        """where_group into device memory (`out`: room for cap records of 56 bytes; res: 112 bytes, a bmx_group_res); enqueue-only. The records come in no
        particular order; after sync(), GroupResult(res.cpu().numpy().view(GROUP_RES_DTYPE)[0], np.sort(out.cpu().numpy().view(GROUP_DTYPE)[:n], order="key"))
        reads them. The program is host data."""
        self._chk(self.L.bmx_where_group(self.h, *_where_args(base, clauses), *_group_tail(measure, group), _ptr(out), int(cap), _ptr(res), MEM_DEVICE))

    def where_quantiles_dev(self, base, clauses, measure, qs, out, res=None):
        """where_quantiles into device memory (`out`: room for len(qs) records of 32 bytes; res: 32 bytes, a bmx_quant_res, or None); enqueue-only. After
        sync(), out.cpu().numpy().view(QUANT_REC_DTYPE) and res.cpu().numpy().view(QUANT_RES_DTYPE)[0] read them. The program and qs are host data."""
        self._chk(self.L.bmx_where_quantiles(self.h, *_where_args(base, clauses), *_quant_tail(measure, qs), _ptr(out), _ptr(res), MEM_DEVICE))

    def where_aggregate_expr_dev(self, base, clauses, expr, out, xres=None, group=None, group_lo=0, ngroups=0):
        """where_aggregate_expr into device memory (`out` as for where_aggregate_dev; xres: 16 bytes, a bmx_expr_res, or None); enqueue-only. After sync(),
        xres.cpu().numpy().view(EXPR_RES_DTYPE)[0] reads the counters. The program and the expression are host data."""
        self._chk(self.L.bmx_where_aggregate_expr(self.h, *_where_args(base, clauses), C.cast(C.byref(expr), C.c_void_p), *_where_agg_tail(None, group, group_lo, ngroups)[1:],
                                                  _ptr(out), _ptr(xres), MEM_DEVICE))

    def where_group_expr_dev(self, base, clauses, group, expr, out, res, xres=None, cap=65536):
        """where_group_expr into device memory (`out`, res as for where_group_dev; xres as for where_aggregate_expr_dev); enqueue-only."""
        self._chk(self.L.bmx_where_group_expr(self.h, *_where_args(base, clauses), C.cast(C.byref(expr), C.c_void_p), _group_tail(None, group)[1], _ptr(out), int(cap),
                                              _ptr(res), _ptr(xres), MEM_DEVICE))

    def where_quantiles_expr_dev(self, base, clauses, expr, qs, out, res=None, xres=None):
        """where_quantiles_expr into device memory (`out`, res as for where_quantiles_dev; xres as for where_aggregate_expr_dev); enqueue-only."""
        self._chk(self.L.bmx_where_quantiles_expr(self.h, *_where_args(base, clauses), C.cast(C.byref(expr), C.c_void_p), *_quant_tail(0, qs)[1:], _ptr(out), _ptr(res),
                                                  _ptr(xres), MEM_DEVICE))

    def where_rows_dev(self, base, clauses, fields, cap, out_ids, out_val, out_ts, res, start=0):
        """where_rows into device memory (out_ids: room for cap ids; out_val: len(fields) columns of cap int64 each, field after field; out_ts: the same for
        the clocks, or None for none; res: 40 bytes, a bmx_rows_res); enqueue-only. After sync(), res.cpu().numpy().view(ROWS_RES_DTYPE)[0] reads the record.
        The program, the fields and the cursor are host data."""
        nf, farr, flags = _rows_fields(fields, out_ts is not None)
        self._chk(self.L.bmx_where_rows(self.h, *_where_args(base, clauses), nf, farr, flags, int(start), int(cap), _ptr(out_ids), _ptr(out_val), _ptr(out_ts), _ptr(res), MEM_DEVICE))

    def where_group_first_dev(self, base, clauses, group, order, out, out_val, out_ts, res, fields=(), desc=False, cap=65536):
        """where_group_first into device memory (`out`: room for cap records of 40 bytes; out_val: len(fields) columns of cap int64 each, field after field;
        out_ts: the same for the clocks, or None for none; res: 40 bytes, a bmx_first_res); enqueue-only. The records come in no particular order, but row r of
        every column belongs to out[r]; after sync(), res.cpu().numpy().view(FIRST_RES_DTYPE)[0] and out.cpu().numpy().view(FIRST_DTYPE)[:n] read them. The
        program and the fields are host data."""
        self._chk(self.L.bmx_where_group_first(self.h, *_where_args(base, clauses), *_first_tail(group, order, fields, desc, out_ts is not None), int(cap), _ptr(out),
                                               _ptr(out_val), _ptr(out_ts), _ptr(res), MEM_DEVICE))

    def where_group_top_dev(self, base, clauses, group, order, per, out, out_rows, out_val, out_ts, res, fields=(), desc=False, cap=65536):
        """where_group_top into device memory (`out`: room for cap groups of 32 bytes; out_rows: cap * per rows of 16 bytes; out_val: len(fields) columns of
        cap * per int64 each, field after field; out_ts: the same for the clocks, or None for none; res: 48 bytes, a bmx_gtop_res); enqueue-only. The groups
        come in no particular order, but block g of every array belongs to out[g]; after sync(), res.cpu().numpy().view(GTOP_RES_DTYPE)[0],
        out.cpu().numpy().view(GTOP_GRP_DTYPE)[:n] and out_rows.cpu().numpy().view(GTOP_ROW_DTYPE)[:n * per] read them. The program and the fields are host
        data."""
        self._chk(self.L.bmx_where_group_top(self.h, *_where_args(base, clauses), *_gtop_tail(group, order, per, fields, desc, out_ts is not None), int(cap), _ptr(out),
                                             _ptr(out_rows), _ptr(out_val), _ptr(out_ts), _ptr(res), MEM_DEVICE))

    def where_group_multi_dev(self, base, clauses, keys, out, res, measure=None, cap=65536):
        """where_group_multi into device memory (`out`: room for cap records of 80 bytes; res: 112 bytes, a bmx_group_res); enqueue-only. The keys are host
        data. The records come in no particular order; after sync(), MultiGroupResult(res.cpu().numpy().view(GROUP_RES_DTYPE)[0],
        mgroup_sort(out.cpu().numpy().view(MGROUP_DTYPE)[:n]), len(keys)) is what where_group_multi returns."""
        nk, karr = _mgroup_keys(keys)
        self._chk(self.L.bmx_where_group_multi(self.h, *_where_args(base, clauses), AGG_NO_FIELD if measure is None else int(measure), nk, karr, _ptr(out), int(cap),
                                               _ptr(res), MEM_DEVICE))

    def where_update_dev(self, base, clauses, target, op, cap, out_ids, res, operand=0, src=None, ts=None, force=False, start=0):
        """where_update with out_ids (room for cap ids, or None) and res (72 bytes, a bmx_upd_res) in device memory. NOT enqueue-only: the call waits once for
        the counts between its emit pass and the merge; out_ids and res are written by its last kernel and valid after sync() or in stream order, when
        res.cpu().numpy().view(UPD_RES_DTYPE)[0] reads the record. The program and the operands are host data."""
        self._chk(self.L.bmx_where_update(self.h, *_where_args(base, clauses), *_upd_args(target, op, operand, src, ts, force), int(start), int(cap), _ptr(out_ids),
                                          _ptr(res), MEM_DEVICE))

    def where_semijoin_dev(self, base, clauses, link, inner_base, inner_clauses, key, out_ids, cap, res, anti=False, set_cap=65536):
        """where_semijoin into device memory (out_ids: room for cap ids, or None with cap 0; res: 32 bytes, a bmx_semi_res); enqueue-only. After sync(),
        SemiResult(res.cpu().numpy().view(SEMI_RES_DTYPE)[0], out_ids.cpu().numpy(), cap) is what where_semijoin returns."""
        self._chk(self.L.bmx_where_semijoin(self.h, *_where_args(base, clauses), int(link), SEMI_ANTI if anti else 0, *_where_args(inner_base, inner_clauses), int(key),
                                            int(set_cap), _ptr(out_ids), int(cap), _ptr(res), MEM_DEVICE))

    def where_in_dev(self, base, clauses, link, values, nvalues, out_ids, cap, res, anti=False):
        """where_in into device memory; `values` is a device array of nvalues int64. Enqueue-only."""
        self._chk(self.L.bmx_where_in(self.h, *_where_args(base, clauses), int(link), SEMI_ANTI if anti else 0, _ptr(values), int(nvalues), _ptr(out_ids), int(cap),
                                      _ptr(res), MEM_DEVICE))

    def where_reach_dev(self, base, clauses, link, key, seed_base, seed_clauses, seed_field, out_ids, out_depth, cap, res, max_depth=REACH_MAX_DEPTH, set_cap=65536):
        """where_reach into device memory (out_ids: room for cap ids, out_depth: for cap bytes, or both None with cap 0; res: 40 bytes, a bmx_reach_res);
        enqueue-only, all max_depth rounds included. After sync(), ReachResult(res.cpu().numpy().view(REACH_RES_DTYPE)[0], out_ids.cpu().numpy(),
        out_depth.cpu().numpy(), cap) is what where_reach returns."""
        self._chk(self.L.bmx_where_reach(self.h, *_where_args(base, clauses), int(link), int(key), 0, *_where_args(seed_base, seed_clauses), int(seed_field),
                                         int(max_depth), int(set_cap), _ptr(out_ids), _ptr(out_depth), int(cap), _ptr(res), MEM_DEVICE))

    def where_reach_from_dev(self, base, clauses, link, key, values, nvalues, out_ids, out_depth, cap, res, max_depth=REACH_MAX_DEPTH, set_cap=65536):
        """where_reach_from into device memory; `values` is a device array of nvalues int64. Enqueue-only."""
        self._chk(self.L.bmx_where_reach_from(self.h, *_where_args(base, clauses), int(link), int(key), 0, _ptr(values), int(nvalues), int(max_depth), int(set_cap),
                                              _ptr(out_ids), _ptr(out_depth), int(cap), _ptr(res), MEM_DEVICE))

    def where_join_group_dev(self, base, clauses, link, inner_base, inner_clauses, key, attr, out, res, measure=None, cap=65536, map_cap=65536):
        """where_join_group into device memory (`out`: room for cap records of 56 bytes; res: 184 bytes, a bmx_join_res); enqueue-only. The records come in no
        particular order; after sync(), JoinResult(res.cpu().numpy().view(JOIN_RES_DTYPE)[0], np.sort(out.cpu().numpy().view(GROUP_DTYPE)[:n], order="key"))
        is what where_join_group returns."""
        self._chk(self.L.bmx_where_join_group(self.h, *_where_args(base, clauses), int(link), AGG_NO_FIELD if measure is None else int(measure),
                                              *_where_args(inner_base, inner_clauses), int(key), int(attr), int(map_cap), _ptr(out), int(cap), _ptr(res), MEM_DEVICE))

    def where_map_group_dev(self, base, clauses, link, keys, vals, npairs, out, res, measure=None, cap=65536):
        """where_map_group into device memory; `keys` and `vals` are device arrays of npairs int64. Enqueue-only."""
        self._chk(self.L.bmx_where_map_group(self.h, *_where_args(base, clauses), int(link), AGG_NO_FIELD if measure is None else int(measure), _ptr(keys), _ptr(vals),
                                             int(npairs), _ptr(out), int(cap), _ptr(res), MEM_DEVICE))

    def where_join_rows_dev(self, base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val,
                            out_in_ts, res, inner=False, start=0, map_cap=65536):
        """where_join_rows into device memory (out_ids / out_in_ids: room for cap ids; out_val / out_in_val: one column of cap int64 per field of that side;
        out_ts / out_in_ts: the same for the clocks, or both None for none; res: 72 bytes, a bmx_jrows_res); enqueue-only. After sync(),
        res.cpu().numpy().view(JROWS_RES_DTYPE)[0] reads the record."""
        nf, farr, _ = _rows_fields(fields, False)
        nif, ifarr, _ = _rows_fields(in_fields, False)
        flags = _jrows_flags(out_ts is not None or out_in_ts is not None, inner)
        self._chk(self.L.bmx_where_join_rows(self.h, *_where_args(base, clauses), int(link), nf, farr, *_where_args(inner_base, inner_clauses), int(key), nif, ifarr,
                                             int(map_cap), flags, int(start), int(cap), _ptr(out_ids), _ptr(out_val), _ptr(out_ts), _ptr(out_in_ids), _ptr(out_in_val),
                                             _ptr(out_in_ts), _ptr(res), MEM_DEVICE))

    def where_map_rows_dev(self, base, clauses, link, fields, keys, node_ids, npairs, in_fields, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val, out_in_ts, res,
                           inner=False, start=0):
        """where_map_rows into device memory; `keys` (int64) and `node_ids` (uint64 bit patterns) are device arrays of npairs words. Enqueue-only."""
        nf, farr, _ = _rows_fields(fields, False)
        nif, ifarr, _ = _rows_fields(in_fields, False)
        flags = _jrows_flags(out_ts is not None or out_in_ts is not None, inner)
        self._chk(self.L.bmx_where_map_rows(self.h, *_where_args(base, clauses), int(link), nf, farr, _ptr(keys), _ptr(node_ids), int(npairs), nif, ifarr, flags,
                                            int(start), int(cap), _ptr(out_ids), _ptr(out_val), _ptr(out_ts), _ptr(out_in_ids), _ptr(out_in_val), _ptr(out_in_ts),
                                            _ptr(res), MEM_DEVICE))

    def watch_poll_dev(self, w, entered, cap_entered, left, cap_left, res):
        """watch_poll into device memory (entered / left: room for cap ids each, or None with a cap of 0; res: 32 bytes, a bmx_watch_res); enqueue-only: the
        decision whether the poll commits is taken on the device."""
        self._chk(self.L.bmx_watch_poll(self.h, int(w), _ptr(entered), int(cap_entered), _ptr(left), int(cap_left), _ptr(res), MEM_DEVICE))

    def scan_range_pos_dev(self, field, lo, hi, out_pos, cap, n_out):
        self._chk(self.L.bmx_scan_range_pos(self.h, int(field), int(lo), int(hi), _ptr(out_pos), int(cap), _ptr(n_out), MEM_DEVICE))

    def index_ids_dev(self, field, first, count, out_ids):
        self._chk(self.L.bmx_index_ids(self.h, int(field), int(first), int(count), _ptr(out_ids), MEM_DEVICE))

    def profile_enable(self, on=True):
        self._chk(self.L.bmx_profile_enable(self.h, 1 if on else 0))

    def profile_read(self):
        """-> (dict stage -> average ms per merge call, number of calls)"""
        ms = (C.c_float * 3)()
        n = C.c_uint32()
        self._chk(self.L.bmx_profile_read(self.h, ms, C.byref(n)))
        return {"probe_apply": ms[0], "resolve_lists": ms[1], "compact": ms[2]}, n.value

    def profile_read_scan(self):
        """-> (dict stage -> average ms per scan call, number of calls)"""
        ms = (C.c_float * 2)()
        n = C.c_uint32()
        self._chk(self.L.bmx_profile_read_scan(self.h, ms, C.byref(n)))
        return {"scan_mask": ms[0], "emit": ms[1]}, n.value

    def timer_start(self):
        self._chk(self.L.bmx_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.L.bmx_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def timer_mark(self):
        """record the stop event now (enqueue only; the last batch's deferred compaction is launched in front of it)"""
        self._chk(self.L.bmx_timer_mark(self.h))

    def timer_elapsed(self):
        ms = C.c_float()
        self._chk(self.L.bmx_timer_elapsed(self.h, C.byref(ms)))
        return ms.value


class Comm:
    """N shards in one process (a bmx_comm): the graph split by node-id hash over N contexts. devices may repeat a GPU (logical shards)."""

    def __init__(self, devices, capacity_rows_per_shard, flags=0):
        self.L = load_library()
        self.N = len(devices)
        arr = (C.c_int * self.N)(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self.L.bmx_comm_create(self.N, arr, int(capacity_rows_per_shard), int(flags) | DEFAULT_CTX_FLAGS, C.byref(h))
        if rc != OK:
            raise BmxError(rc, (self.L.bmx_comm_last_error(None) or b"").decode())
        self.h = h

    def _chk(self, rc):
        if rc < 0:
            raise BmxError(rc, (self.L.bmx_comm_last_error(self.h) or b"").decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.bmx_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        self._chk(self.L.bmx_comm_sync(self.h))

    def load_rows(self, id, field, ts, val):
        id, field, ts, val = _np(id, np.uint64), _np(field, np.uint32), _np(ts, np.int64), _np(val, np.int64)
        self._chk(self.L.bmx_comm_load_rows(self.h, len(id), _ptr(id), _ptr(field), _ptr(ts), _ptr(val)))

    def put_rows(self, id, field, ts, val):
        id, field, ts, val = _np(id, np.uint64), _np(field, np.uint32), _np(ts, np.int64), _np(val, np.int64)
        self._chk(self.L.bmx_comm_put_rows(self.h, len(id), _ptr(id), _ptr(field), _ptr(ts), _ptr(val)))

    def merge(self, id, field, ts, val, insert_mode=INSERT_REFERENCE, applied_out=None):
        """host batch -> (applied_idx u32[w] ascending indices into the batch, MergeStats summed over the shards).
        applied_out: a uint32 array of at least n entries to receive the winners (e.g. page-locked: HostBuffer); the result is then a view of it."""
        id, field, ts, val = _np(id, np.uint64), _np(field, np.uint32), _np(ts, np.int64), _np(val, np.int64)
        n = len(id)
        if applied_out is not None and (applied_out.dtype != np.uint32 or len(applied_out) < n or not applied_out.flags["C_CONTIGUOUS"]):
            raise ValueError("applied_out must be a contiguous uint32 array of at least n entries")
        applied = applied_out if applied_out is not None else np.zeros(max(n, 1), np.uint32)
        na = C.c_uint64(0)
        st = MergeStats()
        self._chk(self.L.bmx_comm_merge(self.h, n, _ptr(id), _ptr(field), _ptr(ts), _ptr(val), int(insert_mode), _ptr(applied),
                                        C.cast(C.byref(na), C.c_void_p), C.cast(C.byref(st), C.c_void_p)))
        return (applied[:na.value] if applied_out is not None else applied[:na.value].copy()), st

    def merge_dev(self, batches, insert_mode=INSERT_REFERENCE, slab_records=0):
        """batches[i] = (n, id, field, ts, val): device tensors on shard i's GPU, the deltas shard i originates. Enqueue-only."""
        N = self.N
        assert len(batches) == N
        ns = (C.c_uint64 * N)(*[int(b[0]) for b in batches])
        cols = [(C.c_void_p * N)(*[(b[1 + k].data_ptr() if b[0] else 0) for b in batches]) for k in range(4)]
        self._chk(self.L.bmx_comm_merge_dev(self.h, ns, cols[0], cols[1], cols[2], cols[3], int(insert_mode), int(slab_records)))

    def shard_result(self, g):
        """-> (recs_ptr, applied_ptr, n_applied_ptr, stats_ptr, n_records): raw device addresses of shard g's last device step"""
        r, a, n, s = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        m = C.c_uint64()
        self._chk(self.L.bmx_comm_shard_result(self.h, int(g), C.byref(r), C.byref(a), C.byref(n), C.byref(s), C.byref(m)))
        return r.value, a.value, n.value, s.value, m.value

    def row_count(self):
        n = C.c_uint64()
        self._chk(self.L.bmx_comm_row_count(self.h, C.byref(n)))
        return n.value

    def get_rows(self, id, field):
        id, field = _np(id, np.uint64), _np(field, np.uint32)
        n = len(id)
        ts = np.zeros(n, np.int64); val = np.zeros(n, np.int64); found = np.zeros(n, np.uint8)
        self._chk(self.L.bmx_comm_get_rows(self.h, n, _ptr(id), _ptr(field), _ptr(ts), _ptr(val), _ptr(found)))
        return ts, val, found.astype(bool)

    def dump_rows(self):
        n = self.row_count()
        id = np.zeros(n, np.uint64); field = np.zeros(n, np.uint32); ts = np.zeros(n, np.int64); val = np.zeros(n, np.int64)
        m = C.c_uint64()
        self._chk(self.L.bmx_comm_dump_rows(self.h, n, _ptr(id), _ptr(field), _ptr(ts), _ptr(val), C.byref(m)))
        assert m.value <= n
        k = m.value
        return id[:k], field[:k], ts[:k], val[:k]

    def digest(self, log2_buckets=10, tombstones=False):
        """Engine.digest over all shards: the vectors one engine holding the same rows gives"""
        B = 1 << int(log2_buckets)
        sums = np.zeros(B, np.uint64); counts = np.zeros(B, np.uint64)
        self._chk(self.L.bmx_comm_digest(self.h, int(log2_buckets), SYNC_TOMBSTONES if tombstones else 0, _ptr(sums), _ptr(counts)))
        return sums, counts

    def export_rows(self, since=0, log2_buckets=0, bucket_bits=None, only_tombstones=False):
        """Engine.export_rows over all shards, shard after shard -> (records, n)"""
        bits = _bucket_words(bucket_bits, log2_buckets)
        fl = EXPORT_ONLY_TOMBSTONES if only_tombstones else 0
        m = C.c_uint64()
        self._chk(self.L.bmx_comm_export_rows(self.h, int(since), int(log2_buckets), _ptr(bits), fl, None, 0, C.byref(m)))
        recs = np.zeros(m.value, DELTA_REC_DTYPE)
        if m.value:
            self._chk(self.L.bmx_comm_export_rows(self.h, int(since), int(log2_buckets), _ptr(bits), fl, _ptr(recs), len(recs), C.byref(m)))
        return recs[:min(m.value, len(recs))], m.value

    def index_build(self, field):
        self._chk(self.L.bmx_comm_index_build(self.h, int(field)))

    def index_set_ordered(self, field, after_queries=1):
        self._chk(self.L.bmx_comm_index_set_ordered(self.h, int(field), int(after_queries)))

    def scan_count(self, field, lo, hi):
        m = C.c_uint64()
        self._chk(self.L.bmx_comm_scan_count(self.h, int(field), int(lo), int(hi), C.byref(m)))
        return m.value

    def scan_range(self, field, lo, hi):
        cap = self.scan_count(field, lo, hi)
        out = np.zeros(max(cap, 1), np.uint64)
        m = C.c_uint64()
        self._chk(self.L.bmx_comm_scan_range(self.h, int(field), int(lo), int(hi), _ptr(out), cap, C.byref(m)))
        return out[:min(m.value, cap)].copy()

    def scan_equals(self, field, value):
        return self.scan_range(field, value, value)

    def scan_aggregate(self, terms, measure=None, group=None, group_lo=0, ngroups=0):
        """Engine.scan_aggregate over all shards: the records one engine holding the same rows gives"""
        out = np.zeros(int(ngroups) + 1, AGG_DTYPE)
        self._chk(self.L.bmx_comm_scan_aggregate(self.h, *_agg_args(terms, measure, group, group_lo, ngroups), _ptr(out)))
        return agg_results(out, int(ngroups))

    def scan_top(self, terms, k, desc=False, after=None):
        """Engine.scan_top over all shards: every shard answers with its first k, the library merges them as top_merge does and adds up the n_eligible"""
        out = np.zeros(max(int(k), 1), TOP_DTYPE)
        m, ne = C.c_uint64(), C.c_uint64()
        self._chk(self.L.bmx_comm_scan_top(self.h, *_top_args(terms, k, desc, after), _ptr(out), C.cast(C.byref(m), C.c_void_p), C.cast(C.byref(ne), C.c_void_p)))
        return out[:m.value].copy(), ne.value

    def scan_filter(self, terms):
        arr = (Term * len(terms))(*[Term(int(f), 0, int(lo), int(hi)) for f, lo, hi in terms])
        m = C.c_uint64()
        self._chk(self.L.bmx_comm_scan_filter(self.h, len(terms), arr, None, 0, C.byref(m)))
        cap = m.value
        out = np.zeros(max(cap, 1), np.uint64)
        self._chk(self.L.bmx_comm_scan_filter(self.h, len(terms), arr, _ptr(out), cap, C.byref(m)))
        return out[:min(m.value, cap)].copy()

    def scan_where(self, base, clauses, count_only=False):
        """Engine.scan_where over all shards, shard after shard: the set one engine holding the same rows gives. It counts first and then fetches."""
        args = _where_args(base, clauses)
        m = C.c_uint64()
        self._chk(self.L.bmx_comm_scan_where(self.h, *args, None, 0, C.cast(C.byref(m), C.c_void_p)))
        if count_only:
            return m.value
        cap = m.value
        out = np.zeros(max(cap, 1), np.uint64)
        self._chk(self.L.bmx_comm_scan_where(self.h, *args, _ptr(out), cap, C.cast(C.byref(m), C.c_void_p)))
        return out[:min(m.value, cap)].copy()

    def where_aggregate(self, base, clauses, measure=None, group=None, group_lo=0, ngroups=0):
        """Engine.where_aggregate over all shards: the records one engine holding the same rows gives"""
        out = np.zeros(int(ngroups) + 1, AGG_DTYPE)
        self._chk(self.L.bmx_comm_where_aggregate(self.h, *_where_args(base, clauses), *_where_agg_tail(measure, group, group_lo, ngroups), _ptr(out)))
        return agg_results(out, int(ngroups))

    def where_top(self, base, clauses, k, desc=False, after=None):
        """Engine.where_top over all shards: every shard answers with its first k, the library merges them as top_merge does and adds up the n_eligible"""
        out = np.zeros(max(int(k), 1), TOP_DTYPE)
        m, ne = C.c_uint64(), C.c_uint64()
        self._chk(self.L.bmx_comm_where_top(self.h, *_where_args(base, clauses), *_where_top_tail(k, desc, after), _ptr(out), C.cast(C.byref(m), C.c_void_p),
                                            C.cast(C.byref(ne), C.c_void_p)))
        return out[:m.value].copy(), ne.value

    def where_group(self, base, clauses, group, measure=None, cap=65536):
        """Engine.where_group over all shards: every shard answers with its own groups, the library merges them by key as group_merge does"""
        out = np.zeros(max(int(cap), 1), GROUP_DTYPE)
        res = GroupRes()
        self._chk(self.L.bmx_comm_where_group(self.h, *_where_args(base, clauses), *_group_tail(measure, group), _ptr(out), int(cap), C.cast(C.byref(res), C.c_void_p)))
        return GroupResult(res, out)

    def where_quantiles(self, base, clauses, measure, qs):
        """Engine.where_quantiles over all shards: the quantiles of the shards do not combine, so the library steps one select over all of them (every shard
        sweeps, the histograms add on the host); the bytes one engine holding the same rows gives"""
        out = np.zeros(max(len(qs), 1), QUANT_REC_DTYPE)
        res = QuantRes()
        self._chk(self.L.bmx_comm_where_quantiles(self.h, *_where_args(base, clauses), *_quant_tail(measure, qs), _ptr(out), C.cast(C.byref(res), C.c_void_p)))
        return out[:len(qs)].copy(), res

    def where_aggregate_expr(self, base, clauses, expr, group=None, group_lo=0, ngroups=0):
        """Engine.where_aggregate_expr over all shards: the records one engine holding the same rows gives; the shards' n_undef and n_range add"""
        out = np.zeros(int(ngroups) + 1, AGG_DTYPE)
        x = ExprRes()
        self._chk(self.L.bmx_comm_where_aggregate_expr(self.h, *_where_args(base, clauses), C.cast(C.byref(expr), C.c_void_p),
                                                       *_where_agg_tail(None, group, group_lo, ngroups)[1:], _ptr(out), C.cast(C.byref(x), C.c_void_p)))
        return agg_results(out, int(ngroups)), x

    def where_group_expr(self, base, clauses, group, expr, cap=65536):
        """Engine.where_group_expr over all shards, merged by key as where_group's answers are"""
        out = np.zeros(max(int(cap), 1), GROUP_DTYPE)
        res, x = GroupRes(), ExprRes()
        self._chk(self.L.bmx_comm_where_group_expr(self.h, *_where_args(base, clauses), C.cast(C.byref(expr), C.c_void_p), _group_tail(None, group)[1], _ptr(out), int(cap),
                                                   C.cast(C.byref(res), C.c_void_p), C.cast(C.byref(x), C.c_void_p)))
        return GroupResult(res, out), x

    def where_quantiles_expr(self, base, clauses, expr, qs):
        """Engine.where_quantiles_expr over all shards: one select stepped over all of them, as where_quantiles"""
        out = np.zeros(max(len(qs), 1), QUANT_REC_DTYPE)
        res, x = QuantRes(), ExprRes()
        self._chk(self.L.bmx_comm_where_quantiles_expr(self.h, *_where_args(base, clauses), C.cast(C.byref(expr), C.c_void_p), *_quant_tail(0, qs)[1:], _ptr(out),
                                                       C.cast(C.byref(res), C.c_void_p), C.cast(C.byref(x), C.c_void_p)))
        return out[:len(qs)].copy(), res, x

    def where_rows(self, base, clauses, fields, cap=None, with_ts=False, start=(0, 0)):
        """Engine.where_rows over the shards, shard after shard from the cursor start = (shard, position) on: the rows one engine holding the same rows gives,
        in shard order. cap None: it counts first (cap 0) and then fetches with room for exactly that. -> RowsResult; (next_shard, next_pos) is the next start."""
        nf, farr, flags = _rows_fields(fields, with_ts)
        args = (*_where_args(base, clauses), nf, farr, flags, int(start[0]), int(start[1]))
        res = RowsRes()
        if cap is None:
            self._chk(self.L.bmx_comm_where_rows(self.h, *args, 0, None, None, None, C.cast(C.byref(res), C.c_void_p)))
            cap = int(res.n_match)
        ids, vals, ts = _rows_buffers(nf, int(cap), with_ts)
        self._chk(self.L.bmx_comm_where_rows(self.h, *args, int(cap), _ptr(ids), _ptr(vals), _ptr(ts), C.cast(C.byref(res), C.c_void_p)))
        return RowsResult(res, ids, vals, ts)

    def where_group_first(self, base, clauses, group, order, fields=(), desc=False, with_ts=False, cap=65536):
        """Engine.where_group_first over all shards: every shard answers with its own groups, the library merges them by key as first_merge does"""
        cap = int(cap)
        tail = _first_tail(group, order, fields, desc, with_ts)
        out, vals, ts = _first_buffers(tail[2], cap, with_ts)
        res = FirstRes()
        self._chk(self.L.bmx_comm_where_group_first(self.h, *_where_args(base, clauses), *tail, cap, _ptr(out), _ptr(vals), _ptr(ts), C.cast(C.byref(res), C.c_void_p)))
        return FirstResult(res, out, vals, ts)

    def where_group_top(self, base, clauses, group, order, per, fields=(), desc=False, with_ts=False, cap=65536):
        """Engine.where_group_top over all shards: every shard answers with its own groups, the library merges them by key as gtop_merge does"""
        cap, per = int(cap), int(per)
        tail = _gtop_tail(group, order, per, fields, desc, with_ts)
        ok = 1 <= per <= GTOP_MAX_PER and 1 <= cap <= GTOP_MAX_CAP and cap * per <= GTOP_MAX_ROWS        # (otherwise the library refuses: no buffers needed)
        out, rows, vals, ts = _gtop_buffers(tail[3], cap if ok else 1, per if ok else 1, with_ts)
        res = GtopRes()
        self._chk(self.L.bmx_comm_where_group_top(self.h, *_where_args(base, clauses), *tail, cap, _ptr(out), _ptr(rows), _ptr(vals), _ptr(ts), C.cast(C.byref(res), C.c_void_p)))
        return GroupTopResult(res, out, rows, vals, ts)

    def where_group_multi(self, base, clauses, keys, measure=None, cap=65536):
        """Engine.where_group_multi over all shards: every shard answers with its own tuples, the library merges them as mgroup_merge does"""
        out = np.zeros(max(int(cap), 1), MGROUP_DTYPE)
        res = GroupRes()
        nk, karr = _mgroup_keys(keys)
        self._chk(self.L.bmx_comm_where_group_multi(self.h, *_where_args(base, clauses), AGG_NO_FIELD if measure is None else int(measure), nk, karr, _ptr(out),
                                                    int(cap), C.cast(C.byref(res), C.c_void_p)))
        return MultiGroupResult(res, out, nk)

    def where_update(self, base, clauses, target, op, operand=0, src=None, ts=None, force=False, cap=None, start=(0, 0), want_ids=False):
        """Engine.where_update over the shards, shard after shard from the cursor start = (shard, position) on; every shard updates the nodes it owns. cap None:
        it counts first (cap 0) and then sends exactly the writable nodes (at most UPD_MAX_CAP). -> UpdateResult; (next_shard, next_pos) is the next start."""
        args = (*_where_args(base, clauses), *_upd_args(target, op, operand, src, ts, force), int(start[0]), int(start[1]))
        res = UpdRes()
        if cap is None:
            self._chk(self.L.bmx_comm_where_update(self.h, *args, 0, None, C.cast(C.byref(res), C.c_void_p)))
            cap = min(int(res.n_match - res.n_nosrc - res.n_range), UPD_MAX_CAP)
        ids = np.zeros(max(int(cap), 1), np.uint64) if want_ids else None
        self._chk(self.L.bmx_comm_where_update(self.h, *args, int(cap), _ptr(ids), C.cast(C.byref(res), C.c_void_p)))
        return UpdateResult(res, ids)

    def where_semijoin(self, base, clauses, link, inner_base, inner_clauses, key, anti=False, cap=None, set_cap=65536, count_only=False):
        """Engine.where_semijoin over all shards: every shard builds its own set, the library unites them and sends the union to every shard, so the answer
        is the set of ids one engine holding the same rows gives, in shard order. cap None: it counts first (cap 0) and then fetches with room for exactly that."""
        args = (*_where_args(base, clauses), int(link), SEMI_ANTI if anti else 0, *_where_args(inner_base, inner_clauses), int(key), int(set_cap))
        return self._semi(self.L.bmx_comm_where_semijoin, args, cap, count_only)

    def where_in(self, base, clauses, link, values, anti=False, cap=None, count_only=False):
        """Engine.where_in over all shards"""
        v, n = _semi_values(values)
        return self._semi(self.L.bmx_comm_where_in, (*_where_args(base, clauses), int(link), SEMI_ANTI if anti else 0, _ptr(v), n), cap, count_only)

    def _semi(self, fn, args, cap, count_only):
        res = SemiRes()
        if cap is None or count_only:
            self._chk(fn(self.h, *args, None, 0, C.cast(C.byref(res), C.c_void_p)))
            if count_only or res.flags & SEMI_OVERFLOW:
                return SemiResult(res, None, 0)
            cap = int(res.n_match)
        ids = np.zeros(max(int(cap), 1), np.uint64)
        self._chk(fn(self.h, *args, _ptr(ids), int(cap), C.cast(C.byref(res), C.c_void_p)))
        return SemiResult(res, ids, cap)

    def where_reach(self, base, clauses, link, key, seed_base, seed_clauses, seed_field, max_depth=REACH_MAX_DEPTH, set_cap=65536, cap=None, count_only=False):
        """Engine.where_reach over all shards: the library steps the rounds and unites every level's values across the shards, so ids and depths are what
        one engine holding the same rows gives, in shard order. cap None: it counts first (cap 0) and then fetches with room for exactly that."""
        args = (*_where_args(base, clauses), int(link), int(key), 0, *_where_args(seed_base, seed_clauses), int(seed_field), int(max_depth), int(set_cap))
        return self._reach(self.L.bmx_comm_where_reach, args, cap, count_only)

    def where_reach_from(self, base, clauses, link, key, values, max_depth=REACH_MAX_DEPTH, set_cap=65536, cap=None, count_only=False):
        """Engine.where_reach_from over all shards"""
        v, n = _semi_values(values)
        return self._reach(self.L.bmx_comm_where_reach_from, (*_where_args(base, clauses), int(link), int(key), 0, _ptr(v), n, int(max_depth), int(set_cap)), cap, count_only)

    def _reach(self, fn, args, cap, count_only):
        res = ReachRes()
        if cap is None or count_only:
            self._chk(fn(self.h, *args, None, None, 0, C.cast(C.byref(res), C.c_void_p)))
            if count_only or res.flags & REACH_OVERFLOW:
                return ReachResult(res, None, None, 0)
            cap = int(res.n_match)
        ids, depth = np.zeros(max(int(cap), 1), np.uint64), np.zeros(max(int(cap), 1), np.uint8)
        self._chk(fn(self.h, *args, _ptr(ids), _ptr(depth), int(cap), C.cast(C.byref(res), C.c_void_p)))
        return ReachResult(res, ids, depth, cap)

    def where_join_group(self, base, clauses, link, inner_base, inner_clauses, key, attr, measure=None, cap=65536, map_cap=65536):
        """Engine.where_join_group over all shards (every shard builds its own map, the library unites them by key with the minimum of the attributes and sends
        the union to every shard; the shards' records merge by key): the selection of scan_where(base, clauses) grouped by the value field `attr` holds on the node of
        scan_where(inner_base, inner_clauses) whose field `key` equals the selected node's field `link` (the minimum of `attr` where several inner nodes share a
        key). The map is built and looked up on the device. -> JoinResult"""
        out = np.zeros(max(int(cap), 1), GROUP_DTYPE)
        res = JoinRes()
        self._chk(self.L.bmx_comm_where_join_group(self.h, *_where_args(base, clauses), int(link), AGG_NO_FIELD if measure is None else int(measure),
                                              *_where_args(inner_base, inner_clauses), int(key), int(attr), int(map_cap), _ptr(out), int(cap),
                                              C.cast(C.byref(res), C.c_void_p)))
        return JoinResult(res, out)

    def where_map_group(self, base, clauses, link, keys, vals, measure=None, cap=65536):
        """Engine.where_map_group over all shards: where_join_group with the map given as 1..JOIN_MAX_MAP (key, val) pairs (a key outside +-(2^53 - 1) is skipped, a val outside it means "no
        attribute", duplicate keys take the minimum of their vals)"""
        k, v, n = _join_pairs(keys, vals)
        out = np.zeros(max(int(cap), 1), GROUP_DTYPE)
        res = JoinRes()
        self._chk(self.L.bmx_comm_where_map_group(self.h, *_where_args(base, clauses), int(link), AGG_NO_FIELD if measure is None else int(measure), _ptr(k), _ptr(v), n,
                                             _ptr(out), int(cap), C.cast(C.byref(res), C.c_void_p)))
        return JoinResult(res, out)

    def where_join_rows(self, base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, cap=None, with_ts=False, inner=False, start=(0, 0), map_cap=65536):
        """Engine.where_join_rows over the shards (every shard builds its own map, the library unites them by key with the smallest id and sends the union to
        every shard; the inner cells come from the shards that own the inner nodes): the rows one engine holding the same rows gives, shard after shard from
        the cursor start = (shard, position) on. cap None: it counts first (cap 0) and then fetches with room for exactly that. -> JoinRowsResult"""
        nf, farr, _ = _rows_fields(fields, with_ts)
        nif, ifarr, _ = _rows_fields(in_fields, with_ts)
        head = (*_where_args(base, clauses), int(link), nf, farr)
        mid = (*_where_args(inner_base, inner_clauses), int(key), nif, ifarr, int(map_cap), _jrows_flags(with_ts, inner), int(start[0]), int(start[1]))
        return self._jrows(self.L.bmx_comm_where_join_rows, head, mid, nf, nif, with_ts, cap)

    def where_map_rows(self, base, clauses, link, fields, keys, node_ids, in_fields, cap=None, with_ts=False, inner=False, start=(0, 0)):
        """Engine.where_map_rows over the shards: where_join_rows with the map given as 1..JOIN_MAX_MAP (key, node id) pairs"""
        nf, farr, _ = _rows_fields(fields, with_ts)
        nif, ifarr, _ = _rows_fields(in_fields, with_ts)
        k, v, n = _jrows_pairs(keys, node_ids)
        head = (*_where_args(base, clauses), int(link), nf, farr)
        mid = (_ptr(k), _ptr(v), n, nif, ifarr, _jrows_flags(with_ts, inner), int(start[0]), int(start[1]))
        return self._jrows(self.L.bmx_comm_where_map_rows, head, mid, nf, nif, with_ts, cap)

    def _jrows(self, fn, head, mid, nf, nif, with_ts, cap):
        if cap is None:
            res = JoinRowsRes()
            self._chk(fn(self.h, *head, *mid, 0, None, None, None, None, None, None, C.cast(C.byref(res), C.c_void_p)))
            cap = int(res.n_match)
        return _jrows_host(fn, self.h, self._chk, head, mid, nf, nif, with_ts, int(cap))

    def watch_create(self, base, clauses):
        """Engine.watch_create on every shard: one id, valid on all of them"""
        w = C.c_uint32()
        self._chk(self.L.bmx_comm_watch_create(self.h, *_where_args(base, clauses), C.byref(w)))
        return w.value

    def watch_poll(self, w, cap_entered=None, cap_left=None):
        """Engine.watch_poll over all shards: the lists are the shards' one after the other, the counts their sums, reset the OR of theirs; a poll that overflows
        commits on no shard. A cap of None: the poll counts first (caps of 0: it commits only if nothing changed) and then fetches with room for exactly that."""
        res = WatchRes()
        if cap_entered is None or cap_left is None:
            self._chk(self.L.bmx_comm_watch_poll(self.h, int(w), None, 0, None, 0, C.cast(C.byref(res), C.c_void_p)))
            if not res.flags & WATCH_OVERFLOW:
                return WatchPoll(res, np.zeros(0, np.uint64), np.zeros(0, np.uint64))
            cap_entered = int(res.n_entered) if cap_entered is None else cap_entered
            cap_left = int(res.n_left) if cap_left is None else cap_left
        ent, lft = np.zeros(max(int(cap_entered), 1), np.uint64), np.zeros(max(int(cap_left), 1), np.uint64)
        self._chk(self.L.bmx_comm_watch_poll(self.h, int(w), _ptr(ent), int(cap_entered), _ptr(lft), int(cap_left), C.cast(C.byref(res), C.c_void_p)))
        return WatchPoll(res, ent[:int(cap_entered)], lft[:int(cap_left)])

    def watch_destroy(self, w):
        self._chk(self.L.bmx_comm_watch_destroy(self.h, int(w)))


FLAG_CONCURRENT = 8
VC_ABSENT, VC_DENSE, VC_SPARSE = 0, 1, 2


class EngineVC:
    """N4 table (a bmx_vc): rows carry a K-writer vector clock instead of one timestamp. Host arrays only, synchronous.
    clocks are (n, K) uint32, component k = writer k's counter (0 = absent from the reference's clock object)."""

    def __init__(self, capacity_rows, k_writers, local_writer, device=0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.bmx_vc_create(int(device), int(capacity_rows), int(k_writers), int(local_writer), C.byref(h))
        if rc != OK:
            raise BmxError(rc, (self.L.bmx_vc_last_error(None) or b"").decode())
        self.h = h
        self.K = int(k_writers)
        self.device = int(device)

    def _chk(self, rc):
        if rc < 0:
            raise BmxError(rc, (self.L.bmx_vc_last_error(self.h) or b"").decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.bmx_vc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _cols(self, id, field, clocks, val):
        id = _np(id, np.uint64); field = _np(field, np.uint32); val = _np(val, np.int64)
        clocks = _np(clocks, np.uint32).reshape(len(id), self.K) if len(id) else np.zeros((0, self.K), np.uint32)
        if not (len(id) == len(field) == len(val)):
            raise ValueError("column lengths differ")
        return id, field, clocks, val

    def load_rows(self, id, field, clocks, val, keysets=None):
        """keysets (uint32[n], see keyset()): which writers each clock names and in which order; None = all K, in order."""
        id, field, clocks, val = self._cols(id, field, clocks, val)
        ks = None if keysets is None else _np(keysets, np.uint32)
        self._chk(self.L.bmx_vc_load_rows_ks(self.h, len(id), _ptr(id), _ptr(field), _ptr(clocks), _ptr(ks), _ptr(val)))

    def merge_batch(self, id, field, clocks, val, keysets=None):
        """-> (flags uint8[n], updated uint32[]): per-delta resolve() flags; for each touched row that changed, the index of the
        last delta that updated it, ascending."""
        id, field, clocks, val = self._cols(id, field, clocks, val)
        n = len(id)
        ks = None if keysets is None else _np(keysets, np.uint32)
        if ks is not None and len(ks) != n:
            raise ValueError("column lengths differ")
        flags = np.zeros(n, np.uint8); upd = np.zeros(max(n, 1), np.uint32); nu = C.c_uint64()
        self._chk(self.L.bmx_vc_merge_batch_ks(self.h, n, _ptr(id), _ptr(field), _ptr(clocks), _ptr(ks), _ptr(val), _ptr(upd), C.byref(nu), _ptr(flags)))
        return flags, upd[: nu.value].copy()

    def get_rows(self, id, field, with_keysets=False):
        """-> (clocks (n,K) uint32, val int64[n], state uint8[n]) with state VC_ABSENT / VC_DENSE / VC_SPARSE; with_keysets: + keysets uint32[n]."""
        id = _np(id, np.uint64); field = _np(field, np.uint32)
        n = len(id)
        clocks = np.zeros((n, self.K), np.uint32); val = np.zeros(n, np.int64); st = np.zeros(n, np.uint8)
        if with_keysets:
            ks = np.zeros(n, np.uint32)
            self._chk(self.L.bmx_vc_get_rows_ks(self.h, n, _ptr(id), _ptr(field), _ptr(clocks), _ptr(ks), _ptr(val), _ptr(st)))
            return clocks, val, st, ks
        self._chk(self.L.bmx_vc_get_rows(self.h, n, _ptr(id), _ptr(field), _ptr(clocks), _ptr(val), _ptr(st)))
        return clocks, val, st

    def row_count(self):
        n = C.c_uint64()
        self._chk(self.L.bmx_vc_row_count(self.h, C.byref(n)))
        return n.value

    def scan_range(self, field, lo, hi, count_only=False):
        """node ids of the rows of `field` with lo <= val <= hi (table order), or their number"""
        m = C.c_uint64()
        if count_only:
            self._chk(self.L.bmx_vc_scan_range(self.h, int(field), int(lo), int(hi), None, 0, C.byref(m)))
            return m.value
        cap = max(self.row_count(), 1)
        out = np.zeros(cap, np.uint64)
        self._chk(self.L.bmx_vc_scan_range(self.h, int(field), int(lo), int(hi), _ptr(out), cap, C.byref(m)))
        return out[:min(m.value, cap)].copy()

    # device-pointer form: torch tensors / raw pointers, enqueue-only
    def merge_batch_dev(self, n, id, field, clocks, val, updated=None, n_updated=None, flags=None, keysets=None):
        self._chk(self.L.bmx_vc_merge_batch_ks_dev(self.h, int(n), _ptr(id), _ptr(field), _ptr(clocks), _ptr(keysets), _ptr(val), _ptr(updated), _ptr(n_updated), _ptr(flags)))

    def set_stream(self, stream_ptr):
        self._chk(self.L.bmx_vc_set_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def sync(self):
        self._chk(self.L.bmx_vc_sync(self.h))

    # ---- replica reconciliation (include/bmx_vc_sync.h; bmx/replica.py pull_vc / reconcile_vc drive it) ----
    def info(self):
        out = VcTableInfo()
        self._chk(self.L.bmx_vc_info(self.h, C.byref(out)))
        return out

    def digest(self, log2_buckets=10):
        """-> (sums u64[2^L], counts u64[2^L]): per-bucket sum of the row digests (vc_rows_digest) and number of rows; counts.sum() == row_count()"""
        B = 1 << int(log2_buckets)
        sums = np.zeros(B, np.uint64); counts = np.zeros(B, np.uint64)
        self._chk(self.L.bmx_vc_digest(self.h, int(log2_buckets), 0, _ptr(sums), _ptr(counts), MEM_HOST))
        return sums, counts

    def digest_dev(self, log2_buckets, sums, counts):
        """same into device memory (u64[2^L] each); enqueue-only"""
        self._chk(self.L.bmx_vc_digest(self.h, int(log2_buckets), 0, _ptr(sums), _ptr(counts), MEM_DEVICE))

    def frontier(self):
        """-> u32[8]: the table's version vector, the component-wise maximum of its rows' clocks (zeros behind K and for an empty table)"""
        out = np.zeros(8, np.uint32)
        self._chk(self.L.bmx_vc_frontier(self.h, _ptr(out), MEM_HOST))
        return out

    def frontier_dev(self, out8):
        self._chk(self.L.bmx_vc_frontier(self.h, _ptr(out8), MEM_DEVICE))

    @staticmethod
    def _frontier_words(frontier):
        if frontier is None:
            return None
        f = np.zeros(8, np.uint32)
        v = _np(frontier, np.uint32)
        if len(v) > 8:
            raise ValueError("a frontier has at most 8 components")
        f[:len(v)] = v
        return f

    def export_rows(self, frontier=None, log2_buckets=0, bucket_bits=None, cap=None, out=None):
        """-> (records, n): the rows whose bucket's bit is set (bucket_bits: u64 words, None = every bucket) and, with a frontier (up to 8 u32), whose clock
        exceeds it in some component, as VC_REC_DTYPE records in slot order; n = number of matches, len(records) = min(n, cap). cap=None: everything (one
        counting call first). out: a VC_REC_DTYPE array to fill (e.g. in a HostBuffer) — its length is the cap and the result a view of it."""
        bits = _bucket_words(bucket_bits, log2_buckets)
        fr = self._frontier_words(frontier)
        m = C.c_uint64()
        if out is not None:
            if out.dtype != VC_REC_DTYPE or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a contiguous VC_REC_DTYPE array")
            cap = len(out)
        elif cap is None:
            self._chk(self.L.bmx_vc_export_rows(self.h, _ptr(fr), int(log2_buckets), _ptr(bits), 0, None, 0, C.cast(C.byref(m), C.c_void_p), MEM_HOST))
            cap = m.value
        recs = out if out is not None else np.zeros(int(cap), VC_REC_DTYPE)
        self._chk(self.L.bmx_vc_export_rows(self.h, _ptr(fr), int(log2_buckets), _ptr(bits), 0, _ptr(recs) if cap else None, int(cap), C.cast(C.byref(m), C.c_void_p), MEM_HOST))
        return recs[:min(m.value, int(cap))], m.value

    def export_rows_dev(self, out, cap, n_out, frontier=None, log2_buckets=0, bucket_bits=None):
        """same with device memory: out = room for cap 64-byte records (None: count only), n_out = one u64, bucket_bits = device u64 words or None; the frontier
        stays a host vector; enqueue-only"""
        self._chk(self.L.bmx_vc_export_rows(self.h, _ptr(self._frontier_words(frontier)), int(log2_buckets), _ptr(bucket_bits), 0, _ptr(out), int(cap), _ptr(n_out), MEM_DEVICE))

    def dump_rows(self):
        """every row as VC_REC_DTYPE records, in slot order"""
        return self.export_rows()[0]

    def merge_records(self, recs):
        """merge_batch over the records' columns (id, field, clock[:K], keyset, val) -> (flags uint8[n], updated uint32[])"""
        recs = np.ascontiguousarray(recs, VC_REC_DTYPE)
        n = len(recs)
        flags = np.zeros(n, np.uint8); upd = np.zeros(max(n, 1), np.uint32); nu = C.c_uint64()
        self._chk(self.L.bmx_vc_merge_records(self.h, n, _ptr(recs) if n else None, _ptr(upd), C.cast(C.byref(nu), C.c_void_p), _ptr(flags) if n else None, MEM_HOST))
        return flags, upd[: nu.value].copy()

    def merge_records_dev(self, n, recs, updated=None, n_updated=None, flags=None):
        """device-pointer form: recs = n 64-byte records in device memory; enqueue-only, errors are reported by sync()"""
        self._chk(self.L.bmx_vc_merge_records(self.h, int(n), _ptr(recs), _ptr(updated), _ptr(n_updated), _ptr(flags), MEM_DEVICE))


KEYSET_NONE = 0xFFFFFFFF


def keyset(writers):
    """Key-set word of a clock whose keys are the writers with these indices, in this order (include/bmx.h bmx_vc_keyset)."""
    ks = KEYSET_NONE
    for i, w in enumerate(writers):
        ks = (ks & ~(0xF << (4 * i))) | ((int(w) & 0xF) << (4 * i))
    return ks & 0xFFFFFFFF


def keyset_writers(ks):
    """inverse of keyset(): the writer indices a key-set word names, in order"""
    out = []
    for i in range(8):
        w = (int(ks) >> (4 * i)) & 0xF
        if w == 0xF:
            break
        out.append(w)
    return out


def vc_rows_digest(id, field, clocks8, keysets, state, val, summed=False):
    """The row digest of include/bmx_vc_sync.h, restated in numpy: eight chained splitmix64 over val, keyset | state << 32, the eight clock components in
    pairs, field, id. clocks8: (n, k) u32 with k <= 8 (padded with zeros). -> u64[n], or with summed=True their sum mod 2^64 as a Python int."""
    u = np.uint64
    id = np.asarray(id, u); n = len(id)
    c = np.zeros((n, 8), u)
    if n:
        cl = np.asarray(clocks8, np.uint32).reshape(n, -1)
        c[:, :cl.shape[1]] = cl
    with np.errstate(over="ignore"):
        def sm(x):
            z = x + u(0x9e3779b97f4a7c15)
            z = (z ^ (z >> u(30))) * u(0xbf58476d1ce4e5b9)
            z = (z ^ (z >> u(27))) * u(0x94d049bb133111eb)
            return z ^ (z >> u(31))
        h = sm(np.asarray(val, np.int64).astype(u))
        h = sm(h ^ (np.asarray(keysets, np.uint32).astype(u) | (np.asarray(state, np.uint32).astype(u) << u(32))))
        for i in range(4):
            h = sm(h ^ (c[:, 2 * i] | (c[:, 2 * i + 1] << u(32))))
        h = sm(h ^ np.asarray(field, np.uint32).astype(u))
        d = sm(h ^ id)
        return int(d.sum(dtype=u)) if summed else d


def owner_of(ids, nshards):
    L = load_library()
    return np.array([L.bmx_owner_of(int(i), int(nshards)) for i in np.asarray(ids, dtype=np.uint64)], dtype=np.uint32)


def _mix64(x):
    x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xff51afd7ed558ccd)
    x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(33))


def key_bucket(ids, fields, log2_buckets):
    """Bucket of every key (id, field) among 2^log2_buckets (0..16): the formula of include/bmx.h bmx_key_bucket, restated in numpy. u32 array."""
    L = int(log2_buckets)
    if not 0 <= L <= 16:
        raise ValueError("log2_buckets must be 0..16")
    ids = np.asarray(ids, np.uint64); fields = np.asarray(fields, np.uint32).astype(np.uint64)
    if L == 0:
        return np.zeros(np.broadcast(ids, fields).shape, np.uint32)
    with np.errstate(over="ignore"):
        h = _mix64(_mix64(ids ^ np.uint64(0xA0761D6478BD642F)) + fields * np.uint64(0xE7037ED1A0B428DB) + np.uint64(0x8EBC6AF09C88C6E3))
    return (h >> np.uint64(64 - L)).astype(np.uint32)


def _bucket_words(bucket_bits, log2_buckets):
    """None, or the bucket set as the contiguous u64 words bmx_export_rows reads (at least 2^L bits)"""
    if bucket_bits is None:
        return None
    bits = _np(bucket_bits, np.uint64)
    if len(bits) < max(1, (1 << int(log2_buckets)) // 64):
        raise ValueError("bucket_bits needs 2^log2_buckets bits (at least one u64 word)")
    return bits


def bucket_bits_of(buckets, log2_buckets):
    """bucket numbers -> the bit words export_rows takes"""
    w = np.zeros(max(1, (1 << int(log2_buckets)) // 64), np.uint64)
    for b in np.unique(np.asarray(buckets, np.int64)):
        w[int(b) >> 6] |= np.uint64(1 << (int(b) & 63))
    return w
