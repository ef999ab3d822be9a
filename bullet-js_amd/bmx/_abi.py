"""The C ABI as Python sees it: constants and export lists of include/*.h, the ctypes structures and numpy dtypes of its records, the signature of every
function (SIGNATURES, applied by load_library()), and the few helpers every module needs to hand memory to the library."""
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
REACH_OVERFLOW, REACH_MORE, REACH_MAX_SET, REACH_MAX_DEPTH = 1, 2, 1 << 20, 255   # BMX_REACH_OVERFLOW, BMX_REACH_MORE (flags of bmx_reach_res), BMX_REACH_MAX_SET, BMX_REACH_MAX_DEPTH (bmx_reach.h bmx_where_reach)
FIRST_DESC, FIRST_OVERFLOW, FIRST_NO_NODE, FIRST_MAX_CAP = 2, 1, (1 << 64) - 1, 1 << 20   # BMX_FIRST_DESC (flags of the call, next to ROWS_TS), BMX_FIRST_OVERFLOW (flags of bmx_first_res), BMX_FIRST_NO_NODE, BMX_FIRST_MAX_CAP (bmx_first.h bmx_where_group_first)
GTOP_DESC, GTOP_OVERFLOW, GTOP_NO_NODE, GTOP_MAX_CAP, GTOP_MAX_PER, GTOP_MAX_ROWS = 2, 1, (1 << 64) - 1, 1 << 20, 16, 1 << 22   # BMX_GTOP_DESC (flags of the call, next to ROWS_TS), BMX_GTOP_OVERFLOW (flags of bmx_gtop_res), BMX_GTOP_NO_NODE, BMX_GTOP_MAX_CAP, BMX_GTOP_MAX_PER, BMX_GTOP_MAX_ROWS (bmx_group_top.h bmx_where_group_top)
EXPR_ADD, EXPR_SUB, EXPR_MUL = 1, 2, 3   # BMX_EXPR_ADD, BMX_EXPR_SUB, BMX_EXPR_MUL (bmx_expr.h)
MGROUP_MAX_KEYS, MGROUP_MAX_CAP4 = 4, 1 << 14  # BMX_MGROUP_MAX_KEYS, BMX_MGROUP_MAX_CAP4 (bmx_group_multi.h bmx_where_group_multi)
UPD_SET, UPD_DELETE, UPD_COPY, UPD_ADD, UPD_FORCE, UPD_MAX_CAP = 0, 1, 2, 3, 1, 1 << 24   # the ops, BMX_UPD_FORCE (flags), BMX_UPD_MAX_CAP (bmx_update.h bmx_where_update)

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
# join projection (include/bmx_join_rows.h); a list of its own for the same reason
EXPORTS_JOIN_ROWS = ["bmx_where_join_rows", "bmx_where_map_rows", "bmx_comm_where_join_rows", "bmx_comm_where_map_rows"]
# include/bmx_quant.h: exact quantiles over boolean filters, likewise
EXPORTS_QUANT = ["bmx_where_quantiles", "bmx_comm_where_quantiles"]
# the probe kernel's claim mode (include/bmx_claim.h), likewise
EXPORTS_CLAIM = ["bmx_selfcheck_claim", "bmx_get_claim_mode"]
# update and delete by query (include/bmx_update.h), likewise
EXPORTS_UPDATE = ["bmx_where_update", "bmx_comm_where_update"]
# group-by over several fields (include/bmx_group_multi.h), likewise
EXPORTS_GROUP_MULTI = ["bmx_where_group_multi", "bmx_comm_where_group_multi"]
# graph traversal (include/bmx_reach.h), likewise
EXPORTS_REACH = ["bmx_where_reach", "bmx_where_reach_from", "bmx_comm_where_reach", "bmx_comm_where_reach_from"]
# the first node per group (include/bmx_first.h), likewise
EXPORTS_FIRST = ["bmx_where_group_first", "bmx_comm_where_group_first"]
# the first N nodes per group (include/bmx_group_top.h), likewise
EXPORTS_GROUP_TOP = ["bmx_where_group_top", "bmx_comm_where_group_top"]
# computed measures (include/bmx_expr.h), likewise
EXPORTS_EXPR = ["bmx_where_aggregate_expr", "bmx_where_group_expr", "bmx_where_quantiles_expr", "bmx_comm_where_aggregate_expr", "bmx_comm_where_group_expr",
                "bmx_comm_where_quantiles_expr"]
# every function the library must export: the lists above, in the order they came to the ABI
ALL_EXPORTS = (EXPORTS + EXPORTS_TOP + EXPORTS_VC_SYNC + EXPORTS_WHERE + EXPORTS_WATCH + EXPORTS_WHERE_AGG + EXPORTS_GROUP + EXPORTS_ROWS + EXPORTS_SEMI + EXPORTS_JOIN
               + EXPORTS_JOIN_ROWS + EXPORTS_QUANT + EXPORTS_CLAIM + EXPORTS_UPDATE + EXPORTS_GROUP_MULTI + EXPORTS_REACH + EXPORTS_FIRST + EXPORTS_GROUP_TOP + EXPORTS_EXPR)


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


class TopRec(C.Structure):
    """bmx_top_rec: one record of bmx_scan_top (16 bytes), also its cursor"""
    _fields_ = [("id", C.c_uint64), ("val", C.c_int64)]


TOP_DTYPE = np.dtype([("id", "<u8"), ("val", "<i8")])


class Lit(C.Structure):
    """bmx_lit: one literal of a bmx_scan_where program (24 bytes, the layout of bmx_term); flags: LIT_NOT, LIT_MINUS, LIT_SUBTRAHEND,
    LIT_CLOCK, LIT_CLOCK_TOMB"""
    _fields_ = [("field", C.c_uint32), ("flags", C.c_uint32), ("lo", C.c_int64), ("hi", C.c_int64)]


GROUP_DTYPE = np.dtype([("key", "<i8"), ("agg", AGG_DTYPE)])      # bmx_group_rec: one record of bmx_where_group (56 bytes)


class GroupRes(C.Structure):
    """bmx_group_res: what one bmx_where_group found besides its records (112 bytes); flags: GROUP_OVERFLOW"""
    _fields_ = [("n_groups", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("absent", Agg), ("total", Agg)]


GROUP_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("flags", "<u4"), ("reserved", "<u4"), ("absent", AGG_DTYPE), ("total", AGG_DTYPE)])


MGROUP_DTYPE = np.dtype([("key", "<i8", (4,)), ("agg", AGG_DTYPE)])      # bmx_mgroup_rec: one record of bmx_where_group_multi (80 bytes)


class GroupKey(C.Structure):
    """bmx_group_key: one key of bmx_where_group_multi (24 bytes): floor((value(field) - origin) / width)"""
    _fields_ = [("field", C.c_uint32), ("flags", C.c_uint32), ("origin", C.c_int64), ("width", C.c_int64)]


class RowsRes(C.Structure):
    """bmx_rows_res: what one bmx_where_rows found besides its rows (40 bytes)"""
    _fields_ = [("n_match", C.c_uint64), ("n_out", C.c_uint64), ("next_pos", C.c_uint64), ("layout", C.c_uint64), ("next_shard", C.c_uint32), ("reserved", C.c_uint32)]


ROWS_RES_DTYPE = np.dtype([("n_match", "<u8"), ("n_out", "<u8"), ("next_pos", "<u8"), ("layout", "<u8"), ("next_shard", "<u4"), ("reserved", "<u4")])


class FirstRec(C.Structure):
    """bmx_first_rec: one record of bmx_where_group_first (40 bytes): the group value, its first node and that node's order value, the members, the contenders"""
    _fields_ = [("key", C.c_int64), ("id", C.c_uint64), ("val", C.c_int64), ("n_match", C.c_uint64), ("n", C.c_uint64)]


class FirstRes(C.Structure):
    """bmx_first_res: what one bmx_where_group_first found besides its records (40 bytes); flags: FIRST_OVERFLOW"""
    _fields_ = [("n_groups", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("total", C.c_uint64), ("absent", C.c_uint64), ("n_ordered", C.c_uint64)]


FIRST_DTYPE = np.dtype([("key", "<i8"), ("id", "<u8"), ("val", "<i8"), ("n_match", "<u8"), ("n", "<u8")])
FIRST_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("flags", "<u4"), ("reserved", "<u4"), ("total", "<u8"), ("absent", "<u8"), ("n_ordered", "<u8")])


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


class UpdRes(C.Structure):
    """bmx_upd_res: what one bmx_where_update found and wrote (72 bytes)"""
    _fields_ = [("n_match", C.c_uint64), ("n_nosrc", C.c_uint64), ("n_range", C.c_uint64), ("n_sent", C.c_uint64), ("n_applied", C.c_uint64), ("n_rows", C.c_uint64),
                ("next_pos", C.c_uint64), ("layout", C.c_uint64), ("next_shard", C.c_uint32), ("reserved", C.c_uint32)]


UPD_RES_DTYPE = np.dtype([("n_match", "<u8"), ("n_nosrc", "<u8"), ("n_range", "<u8"), ("n_sent", "<u8"), ("n_applied", "<u8"), ("n_rows", "<u8"), ("next_pos", "<u8"),
                          ("layout", "<u8"), ("next_shard", "<u4"), ("reserved", "<u4")])


class SemiRes(C.Structure):
    """bmx_semi_res: what one bmx_where_semijoin / bmx_where_in found besides its ids (32 bytes); flags: SEMI_OVERFLOW"""
    _fields_ = [("n_match", C.c_uint64), ("set_size", C.c_uint64), ("n_inner", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


SEMI_RES_DTYPE = np.dtype([("n_match", "<u8"), ("set_size", "<u8"), ("n_inner", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])


class ReachRes(C.Structure):
    """bmx_reach_res: what one bmx_where_reach / bmx_where_reach_from found besides its ids and depths (40 bytes); flags: REACH_OVERFLOW | REACH_MORE"""
    _fields_ = [("n_match", C.c_uint64), ("set_size", C.c_uint64), ("n_seed", C.c_uint64), ("n_edges", C.c_uint64), ("rounds", C.c_uint32), ("flags", C.c_uint32)]


REACH_RES_DTYPE = np.dtype([("n_match", "<u8"), ("set_size", "<u8"), ("n_seed", "<u8"), ("n_edges", "<u8"), ("rounds", "<u4"), ("flags", "<u4")])


class JoinRes(C.Structure):
    """bmx_join_res: what one bmx_where_join_group / bmx_where_map_group found besides its records (184 bytes); flags: JOIN_MAP_OVERFLOW | JOIN_GROUP_OVERFLOW"""
    _fields_ = [("n_groups", C.c_uint64), ("map_size", C.c_uint64), ("n_inner", C.c_uint64), ("n_keyed", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("absent", Agg), ("unmatched", Agg), ("total", Agg)]


JOIN_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("map_size", "<u8"), ("n_inner", "<u8"), ("n_keyed", "<u8"), ("flags", "<u4"), ("reserved", "<u4"),
                           ("absent", AGG_DTYPE), ("unmatched", AGG_DTYPE), ("total", AGG_DTYPE)])


class JoinRowsRes(C.Structure):
    """bmx_jrows_res: what one bmx_where_join_rows / bmx_where_map_rows found besides its rows (72 bytes); flags: JOIN_MAP_OVERFLOW"""
    _fields_ = [("n_match", C.c_uint64), ("n_out", C.c_uint64), ("next_pos", C.c_uint64), ("layout", C.c_uint64), ("n_joined", C.c_uint64), ("map_size", C.c_uint64),
                ("n_inner", C.c_uint64), ("n_keyed", C.c_uint64), ("flags", C.c_uint32), ("next_shard", C.c_uint32)]


JROWS_RES_DTYPE = np.dtype([("n_match", "<u8"), ("n_out", "<u8"), ("next_pos", "<u8"), ("layout", "<u8"), ("n_joined", "<u8"), ("map_size", "<u8"), ("n_inner", "<u8"),
                            ("n_keyed", "<u8"), ("flags", "<u4"), ("next_shard", "<u4")])


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


def _signatures():
    """-> {name: (restype, argtypes)} of every exported function, as include/*.h declare them (tests/test_binding_signatures.py holds the two together).
    both(name, args) is the common case: bmx_<name>(ctx, *args, int mem) and its shard form bmx_comm_<name>(comm, *args); paged(name, head, tail) the paged
    queries, whose shard form takes the cursor's shard in front of the position: bmx_<name>(ctx, *head, *tail, int mem), bmx_comm_<name>(comm, *head,
    uint32_t shard, *tail). Everything else is listed in full."""
    P = C.POINTER
    vp, u64, u32, i64, i32, f32, f64, cstr = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_char_p
    S = {}

    def fn(names, args, res=i32):
        for name in names.split():
            S[name] = (res, args)

    def both(name, args):
        fn("bmx_" + name, [vp] + args + [i32])
        fn("bmx_comm_" + name, [vp] + args)

    def paged(name, head, tail):
        fn("bmx_" + name, [vp] + head + tail + [i32])
        fn("bmx_comm_" + name, [vp] + head + [u32] + tail)

    cols = [u64, vp, vp, vp, vp]                                             # n, id, field, ts (or clocks), val
    prog = [u32, u32, P(u32), P(Lit)]                                        # base_field, nclauses, clause_len, lits
    # contexts (bmx.h, bmx_claim.h)
    fn("bmx_create", [i32, u64, u32, P(vp)])
    fn("bmx_create_ex bmx_vc_create", [i32, u64, u32, u32, P(vp)])
    fn("bmx_comm_create", [u32, P(i32), u64, u32, P(vp)])
    fn("bmx_destroy bmx_comm_destroy bmx_vc_destroy", [vp], None)
    fn("bmx_last_error bmx_comm_last_error bmx_vc_last_error", [vp], cstr)
    fn("bmx_abi_version", [])
    fn("bmx_selfcheck bmx_selfcheck_claim", [i32, P(u64), P(u64), P(u64)])
    fn("bmx_get_claim_mode bmx_merge_fence bmx_sync bmx_comm_sync bmx_vc_sync bmx_timer_start bmx_timer_mark", [vp])
    fn("bmx_set_deferred_compaction bmx_set_probe_waves bmx_profile_enable", [vp, i32])
    fn("bmx_set_side_stream bmx_set_stream bmx_vc_set_stream bmx_ipc_close bmx_ipc_free", [vp, vp])
    fn("bmx_get_stream", [vp], vp)
    fn("bmx_set_wait_limit", [vp, f64])
    fn("bmx_get_deferred_counts bmx_index_refresh_counts", [vp, P(u64), P(u64)])
    fn("bmx_get_info", [vp, P(Info)])
    fn("bmx_get_placement", [vp, P(u32), P(f32), P(f32)])
    fn("bmx_seq_signal bmx_seq_wait", [vp, vp, vp, u64])
    fn("bmx_seq_wait_all", [vp, vp, vp, u32, u64])
    fn("bmx_timer_stop bmx_timer_elapsed", [vp, P(f32)])
    fn("bmx_profile_read bmx_profile_read_scan", [vp, P(f32), P(u32)])
    fn("bmx_host_alloc", [u64, P(vp)])
    fn("bmx_host_free", [vp])
    fn("bmx_ipc_alloc", [vp, u64, u32, P(vp), cstr])
    fn("bmx_ipc_open", [vp, cstr, i32, P(vp)])
    fn("bmx_comm_nshards", [vp], u32)
    fn("bmx_comm_shard", [vp, u32], vp)
    fn("bmx_comm_shard_result", [vp, u32, P(vp), P(vp), P(vp), P(vp), P(u64)])
    # rows and merges
    both("load_rows", cols)
    both("put_rows", cols)
    both("get_rows", [u64, vp, vp, vp, vp, vp])
    fn("bmx_get_row", [vp, u64, u32, P(i64), P(i64)])
    fn("bmx_dump_rows", [vp, u64, vp, vp, vp, vp, vp, i32])
    fn("bmx_comm_dump_rows", [vp, u64, vp, vp, vp, vp, P(u64)])
    fn("bmx_row_count bmx_comm_row_count bmx_vc_row_count", [vp, P(u64)])
    fn("bmx_reserve", [vp, u64])
    fn("bmx_merge_batch", [vp] + cols + [i32, i32, vp, vp, vp, vp])
    fn("bmx_merge_submit", [vp] + cols + [i32, i32, P(u64)])
    fn("bmx_merge_collect", [vp, u64, vp, vp, vp, vp])
    fn("bmx_merge_records", [vp, u64, vp, i32, vp, vp, vp, vp])
    fn("bmx_merge_records_after", [vp, vp, u32, u64, u64, vp, i32, vp, vp, vp, vp])
    fn("bmx_merge_notify", [vp, vp, u32])
    fn("bmx_merge_tail_wait", [vp, vp, u32, u64])
    fn("bmx_comm_merge", [vp] + cols + [i32, vp, vp, vp])
    fn("bmx_comm_merge_dev", [vp, vp, vp, vp, vp, vp, i32, u64])
    fn("bmx_owner_of", [u64, u32], u32)
    fn("bmx_partition_by_owner", [vp] + cols + [u32, vp, vp])
    fn("bmx_partition_by_owner_slabs", [vp] + cols + [u32, u64, vp, vp])
    fn("bmx_partition_scatter", [vp] + cols + [u32, u64, vp, vp, vp, u64, vp, u32, u64])
    # the vector-clock table (bmx.h, bmx_vc_sync.h)
    fn("bmx_vc_load_rows", [vp] + cols)
    fn("bmx_vc_load_rows_ks bmx_vc_get_rows", [vp, u64, vp, vp, vp, vp, vp])
    fn("bmx_vc_get_rows_ks", [vp, u64, vp, vp, vp, vp, vp, vp])
    fn("bmx_vc_merge_batch bmx_vc_merge_batch_dev", [vp, u64, vp, vp, vp, vp, vp, vp, vp])
    fn("bmx_vc_merge_batch_ks bmx_vc_merge_batch_ks_dev", [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp])
    fn("bmx_vc_keyset", [vp, u32], u32)
    fn("bmx_vc_keyset_dense", [u32], u32)
    fn("bmx_vc_rec_digest", [vp], u64)
    fn("bmx_vc_info", [vp, P(VcTableInfo)])
    fn("bmx_vc_digest", [vp, u32, u32, vp, vp, i32])
    fn("bmx_vc_frontier", [vp, vp, i32])
    fn("bmx_vc_export_rows", [vp, vp, u32, vp, u32, vp, u64, vp, i32])
    fn("bmx_vc_merge_records", [vp, u64, vp, vp, vp, vp, i32])
    # replica reconciliation
    fn("bmx_key_bucket", [u64, u32, u32], u32)
    both("digest", [u32, u32, vp, vp])
    both("export_rows", [i64, u32, vp, u32, vp, u64, vp])
    # indexes and scans: the shard forms report their count through a uint64_t*, so they are listed
    fn("bmx_index_build bmx_index_drop bmx_comm_index_build bmx_watch_destroy bmx_comm_watch_destroy", [vp, u32])
    fn("bmx_index_size", [vp, u32, P(u64)])
    fn("bmx_index_set_ordered bmx_comm_index_set_ordered", [vp, u32, u32])
    fn("bmx_index_ordered_info", [vp, u32, P(u32), P(i32), P(u64)])
    fn("bmx_index_ordered_stats", [vp, u32, P(u64), P(u64), P(u64), P(f64), P(f64), P(u64), P(u64)])
    fn("bmx_index_ids", [vp, u32, u64, u64, vp, i32])
    fn("bmx_scan_range bmx_scan_range_pos", [vp, u32, i64, i64, vp, u64, vp, i32])
    fn("bmx_scan_equals", [vp, u32, i64, vp, u64, vp, i32])
    fn("bmx_scan_count", [vp, u32, i64, i64, vp, i32])
    fn("bmx_scan_filter", [vp, u32, P(Term), vp, u64, vp, i32])
    fn("bmx_comm_scan_range bmx_vc_scan_range", [vp, u32, i64, i64, vp, u64, P(u64)])
    fn("bmx_comm_scan_equals", [vp, u32, i64, vp, u64, P(u64)])
    fn("bmx_comm_scan_count", [vp, u32, i64, i64, P(u64)])
    fn("bmx_comm_scan_filter", [vp, u32, P(Term), vp, u64, P(u64)])
    both("scan_aggregate", [u32, P(Term), u32, u32, i64, u32, vp])
    both("scan_top", [u32, P(Term), u32, vp, u32, vp, vp, vp])
    # queries over a program (bmx_where.h and the headers that build on it)
    both("scan_where", prog + [vp, u64, vp])
    both("where_aggregate", prog + [u32, u32, i64, u32, vp])
    both("where_top", prog + [u32, vp, u32, vp, vp, vp])
    both("where_group", prog + [u32, u32, vp, u64, vp])
    both("where_quantiles", prog + [u32, u32, vp, vp, vp])
    both("where_aggregate_expr", prog + [vp, u32, i64, u32, vp, vp])
    both("where_group_expr", prog + [vp, u32, vp, u64, vp, vp])
    both("where_quantiles_expr", prog + [vp, u32, vp, vp, vp, vp])
    both("where_semijoin", prog + [u32, u32] + prog + [u32, u64, vp, u64, vp])
    both("where_in", prog + [u32, u32, vp, u64, vp, u64, vp])
    reach_out = [u32, u64, vp, vp, u64, vp]                                  # max_depth, set_cap, out_ids, out_depth, cap, res
    both("where_reach", prog + [u32, u32, u32] + prog + [u32] + reach_out)
    both("where_reach_from", prog + [u32, u32, u32, vp, u64] + reach_out)
    both("where_join_group", prog + [u32, u32] + prog + [u32, u32, u64, vp, u64, vp])
    both("where_map_group", prog + [u32, u32, vp, vp, u64, vp, u64, vp])
    jr_out = [vp, vp, vp, vp, vp, vp, vp]
    paged("where_join_rows", prog + [u32, u32, P(u32)] + prog + [u32, u32, P(u32), u64, u32], [u64, u64] + jr_out)
    paged("where_map_rows", prog + [u32, u32, P(u32), vp, vp, u64, u32, P(u32), u32], [u64, u64] + jr_out)
    paged("where_rows", prog + [u32, P(u32), u32], [u64, u64, vp, vp, vp, vp])
    first = [u32, u32, u32, P(u32), u32, u64, vp, vp, vp, vp]               # group, order, nfields, fields, flags, cap, out, out_val, out_ts, res
    both("where_group_first", prog + first)
    gtop = [u32, u32, u32, u32, P(u32), u32, u64, vp, vp, vp, vp, vp]       # group, order, per, nfields, fields, flags, cap, out, out_rows, out_val, out_ts, res
    both("where_group_top", prog + gtop)
    both("where_group_multi", prog + [u32, u32, P(GroupKey), vp, u64, vp])
    upd = [u32, u32, u32, i64, i64, u32]
    paged("where_update", prog + upd, [u64, u64, vp, vp])
    fn("bmx_watch_create bmx_comm_watch_create", [vp] + prog + [P(u32)])
    both("watch_poll", [u32, vp, u64, vp, u64, vp])
    return S


SIGNATURES = _signatures()


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
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, restype
    _lib = L
    return L


def _selfcheck(fn, device):
    """one of the library's two self-checks -> its three counters; the library itself decides which outcome is an error"""
    L = load_library()
    r, t, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = getattr(L, fn)(int(device), C.byref(r), C.byref(t), C.byref(c))
    if rc:
        raise BmxError(rc, (L.bmx_last_error(None) or b"").decode())
    return r.value, t.value, c.value


def selfcheck(device=0):
    """bmx_selfcheck: (checked 16-byte loads, torn pairs seen, torn pairs of the split-store control). Raises if a pair tore."""
    return _selfcheck("bmx_selfcheck", device)


def selfcheck_claim(device=0):
    """bmx_selfcheck_claim: (checked 16-byte loads, torn pairs seen beside team swaps, torn pairs of the three-instruction control). A torn pair is
    reported, not raised: contexts on such a device keep claim mode `store`."""
    return _selfcheck("bmx_selfcheck_claim", device)


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


def _ref(x):
    """a ctypes object of the caller's -> void* to it (the object must outlive the call)"""
    return C.cast(C.byref(x), C.c_void_p)


class _Handle:
    """What Engine, Comm and EngineVC share: self.L (the library) and self.h (the handle) with one lifetime. A subclass names its own destroy function and
    its own error channel — bmx_last_error, bmx_comm_last_error and bmx_vc_last_error are three separate ones."""
    _destroy = _last_error = None

    def _create(self, fn, *args):
        """self.L, and self.h = the handle the library's create function `fn` returns through its last parameter"""
        self.L = load_library()
        h = C.c_void_p()
        rc = getattr(self.L, fn)(*args, C.byref(h))
        if rc != OK:
            raise BmxError(rc, (getattr(self.L, self._last_error)(None) or b"").decode())
        self.h = h

    def _chk(self, rc):
        if rc < 0:
            raise BmxError(rc, (getattr(self.L, self._last_error)(self.h) or b"").decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._destroy)(self.h)
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
    from . import HostBuffer          # (through the package, where a test may have put a stand-in)
    hb = HostBuffer(max(n, 1) * 28)
    return hb, hb.array(np.uint64, n), hb.array(np.uint32, n, 24 * n), hb.array(np.int64, n, 8 * n), hb.array(np.int64, n, 16 * n)
