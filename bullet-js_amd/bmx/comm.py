"""Comm: one bmx_comm, the shard forms of the host-array calls."""
import ctypes as C

import numpy as np

from . import _queries as Q
from ._abi import (DEFAULT_CTX_FLAGS, DELTA_REC_DTYPE, EXPORT_ONLY_TOMBSTONES, INSERT_REFERENCE, MGROUP_DTYPE, REACH_MAX_DEPTH, SYNC_TOMBSTONES, ExprRes, JoinRes, MergeStats, Term, _np,
                   _ptr, _ref)
from ._results import GroupResult, JoinResult, MultiGroupResult
from .engine import _bucket_words


class Comm(Q._HostQueries):
    """N shards in one process (a bmx_comm): the graph split by node-id hash over N contexts. devices may repeat a GPU (logical shards)."""
    _destroy, _last_error = "bmx_comm_destroy", "bmx_comm_last_error"

    def __init__(self, devices, capacity_rows_per_shard, flags=0):
        self.N = len(devices)
        arr = (C.c_int * self.N)(*[int(d) for d in devices])
        self._create("bmx_comm_create", self.N, arr, int(capacity_rows_per_shard), int(flags) | DEFAULT_CTX_FLAGS)

    def _host(self, name, *args):
        """bmx_comm_<name>(comm, *args): the shard form of a query; it has no device-pointer form"""
        return self._chk(getattr(self.L, "bmx_comm_" + name)(self.h, *args))

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
                                        _ref(na), _ref(st)))
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

    def scan_filter(self, terms):
        arr = (Term * len(terms))(*[Term(int(f), 0, int(lo), int(hi)) for f, lo, hi in terms])
        m = C.c_uint64()
        self._chk(self.L.bmx_comm_scan_filter(self.h, len(terms), arr, None, 0, C.byref(m)))
        cap = m.value
        out = np.zeros(max(cap, 1), np.uint64)
        self._chk(self.L.bmx_comm_scan_filter(self.h, len(terms), arr, _ptr(out), cap, C.byref(m)))
        return out[:min(m.value, cap)].copy()

    def scan_aggregate(self, terms, measure=None, group=None, group_lo=0, ngroups=0):
        """Engine.scan_aggregate over all shards: the records one engine holding the same rows gives"""
        return self._host_aggregate("scan_aggregate", Q._agg_args(terms, measure, group, group_lo, ngroups), ngroups)

    def scan_top(self, terms, k, desc=False, after=None):
        """Engine.scan_top over all shards: every shard answers with its first k, the library merges them as top_merge does and adds up the n_eligible"""
        return self._host_top("scan_top", Q._top_args(terms, k, desc, after), k)

    def scan_where(self, base, clauses, count_only=False):
        """Engine.scan_where over all shards, shard after shard: the set one engine holding the same rows gives. It counts first and then fetches."""
        return self._host_scan_where(Q._where_args(base, clauses), None, count_only)

    def where_aggregate(self, base, clauses, measure=None, group=None, group_lo=0, ngroups=0):
        """Engine.where_aggregate over all shards: the records one engine holding the same rows gives"""
        return self._host_aggregate("where_aggregate", Q._where_aggregate_args(base, clauses, measure, group, group_lo, ngroups), ngroups)

    def where_top(self, base, clauses, k, desc=False, after=None):
        """Engine.where_top over all shards: every shard answers with its first k, the library merges them as top_merge does and adds up the n_eligible"""
        return self._host_top("where_top", Q._where_top_args(base, clauses, k, desc, after), k)

    def where_group(self, base, clauses, group, measure=None, cap=65536):
        """Engine.where_group over all shards: every shard answers with its own groups, the library merges them by key as group_merge does"""
        return GroupResult(*self._host_group("where_group", Q._where_group_args(base, clauses, measure, group), cap))

    def where_quantiles(self, base, clauses, measure, qs):
        """Engine.where_quantiles over all shards: the quantiles of the shards do not combine, so the library steps one select over all of them (every shard
        sweeps, the histograms add on the host); the bytes one engine holding the same rows gives"""
        return self._host_quantiles("where_quantiles", Q._where_quantiles_args(base, clauses, measure, qs), len(qs))

    def where_aggregate_expr(self, base, clauses, expr, group=None, group_lo=0, ngroups=0):
        """Engine.where_aggregate_expr over all shards: the records one engine holding the same rows gives; the shards' n_undef and n_range add"""
        x = ExprRes()
        return self._host_aggregate("where_aggregate_expr", Q._where_aggregate_args(base, clauses, expr, group, group_lo, ngroups), ngroups, (x,)), x

    def where_group_expr(self, base, clauses, group, expr, cap=65536):
        """Engine.where_group_expr over all shards, merged by key as where_group's answers are"""
        x = ExprRes()
        return GroupResult(*self._host_group("where_group_expr", Q._where_group_args(base, clauses, expr, group), cap, (x,))), x

    def where_quantiles_expr(self, base, clauses, expr, qs):
        """Engine.where_quantiles_expr over all shards: one select stepped over all of them, as where_quantiles"""
        x = ExprRes()
        return (*self._host_quantiles("where_quantiles_expr", Q._where_quantiles_args(base, clauses, expr, qs), len(qs), (x,)), x)

    def where_rows(self, base, clauses, fields, cap=None, with_ts=False, start=(0, 0)):
        """Engine.where_rows over the shards, shard after shard from the cursor start = (shard, position) on: the rows one engine holding the same rows gives,
        in shard order. cap None: it counts first (cap 0) and then fetches with room for exactly that. -> RowsResult; (next_shard, next_pos) is the next start."""
        return self._host_rows(Q._where_rows_args(base, clauses, fields, with_ts, start[1], start[0]), len(fields), with_ts, cap)

    def where_group_first(self, base, clauses, group, order, fields=(), desc=False, with_ts=False, cap=65536):
        """Engine.where_group_first over all shards: every shard answers with its own groups, the library merges them by key as first_merge does"""
        return self._host_group_first(Q._where_group_first_args(base, clauses, group, order, fields, desc, with_ts), len(fields), with_ts, int(cap))

    def where_group_top(self, base, clauses, group, order, per, fields=(), desc=False, with_ts=False, cap=65536):
        """Engine.where_group_top over all shards: every shard answers with its own groups, the library merges them by key as gtop_merge does"""
        return self._host_group_top(Q._where_group_top_args(base, clauses, group, order, per, fields, desc, with_ts), len(fields), with_ts, int(cap), int(per))

    def where_group_multi(self, base, clauses, keys, measure=None, cap=65536):
        """Engine.where_group_multi over all shards: every shard answers with its own tuples, the library merges them as mgroup_merge does"""
        return MultiGroupResult(*self._host_group("where_group_multi", Q._where_group_multi_args(base, clauses, keys, measure), cap, dtype=MGROUP_DTYPE), len(keys))

    def where_update(self, base, clauses, target, op, operand=0, src=None, ts=None, force=False, cap=None, start=(0, 0), want_ids=False):
        """Engine.where_update over the shards, shard after shard from the cursor start = (shard, position) on; every shard updates the nodes it owns. cap None:
        it counts first (cap 0) and then sends exactly the writable nodes (at most UPD_MAX_CAP). -> UpdateResult; (next_shard, next_pos) is the next start."""
        return self._host_update(Q._where_update_args(base, clauses, target, op, operand, src, ts, force, start[1], start[0]), cap, want_ids)

    def where_semijoin(self, base, clauses, link, inner_base, inner_clauses, key, anti=False, cap=None, set_cap=65536, count_only=False):
        """Engine.where_semijoin over all shards: every shard builds its own set, the library unites them and sends the union to every shard, so the answer
        is the set of ids one engine holding the same rows gives, in shard order. cap None: it counts first (cap 0) and then fetches with room for exactly that."""
        return self._host_semi("where_semijoin", Q._where_semijoin_args(base, clauses, link, anti, inner_base, inner_clauses, key, set_cap), cap, count_only)

    def where_in(self, base, clauses, link, values, anti=False, cap=None, count_only=False):
        """Engine.where_in over all shards"""
        v, n = Q._semi_values(values)
        return self._host_semi("where_in", Q._where_in_args(base, clauses, link, anti, v, n), cap, count_only)

    def where_reach(self, base, clauses, link, key, seed_base, seed_clauses, seed_field, max_depth=REACH_MAX_DEPTH, set_cap=65536, cap=None, count_only=False):
        """Engine.where_reach over all shards: the library steps the rounds and unites every level's values across the shards, so ids and depths are what
        one engine holding the same rows gives, in shard order. cap None: it counts first (cap 0) and then fetches with room for exactly that."""
        return self._host_reach("where_reach", Q._where_reach_args(base, clauses, link, key, seed_base, seed_clauses, seed_field, max_depth, set_cap), cap, count_only)

    def where_reach_from(self, base, clauses, link, key, values, max_depth=REACH_MAX_DEPTH, set_cap=65536, cap=None, count_only=False):
        """Engine.where_reach_from over all shards"""
        v, n = Q._semi_values(values)
        return self._host_reach("where_reach_from", Q._where_reach_from_args(base, clauses, link, key, v, n, max_depth, set_cap), cap, count_only)

    def where_join_group(self, base, clauses, link, inner_base, inner_clauses, key, attr, measure=None, cap=65536, map_cap=65536):
        """Engine.where_join_group over all shards (every shard builds its own map, the library unites them by key with the minimum of the attributes and sends
        the union to every shard; the shards' records merge by key): the selection of scan_where(base, clauses) grouped by the value field `attr` holds on the node of
        scan_where(inner_base, inner_clauses) whose field `key` equals the selected node's field `link` (the minimum of `attr` where several inner nodes share a
        key). The map is built and looked up on the device. -> JoinResult"""
        return JoinResult(*self._host_group("where_join_group", Q._where_join_group_args(base, clauses, link, measure, inner_base, inner_clauses, key, attr, map_cap), cap, res=JoinRes))

    def where_map_group(self, base, clauses, link, keys, vals, measure=None, cap=65536):
        """Engine.where_map_group over all shards: where_join_group with the map given as 1..JOIN_MAX_MAP (key, val) pairs (a key outside +-(2^53 - 1) is skipped, a val outside it means "no
        attribute", duplicate keys take the minimum of their vals)"""
        k, v, n = Q._join_pairs(keys, vals)
        return JoinResult(*self._host_group("where_map_group", Q._where_map_group_args(base, clauses, link, measure, k, v, n), cap, res=JoinRes))

    def where_join_rows(self, base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, cap=None, with_ts=False, inner=False, start=(0, 0), map_cap=65536):
        """Engine.where_join_rows over the shards (every shard builds its own map, the library unites them by key with the smallest id and sends the union to
        every shard; the inner cells come from the shards that own the inner nodes): the rows one engine holding the same rows gives, shard after shard from
        the cursor start = (shard, position) on. cap None: it counts first (cap 0) and then fetches with room for exactly that. -> JoinRowsResult"""
        args = Q._where_join_rows_args(base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, map_cap, with_ts, inner, start[1], start[0])
        return self._host_jrows("where_join_rows", args, len(fields), len(in_fields), with_ts, cap)

    def where_map_rows(self, base, clauses, link, fields, keys, node_ids, in_fields, cap=None, with_ts=False, inner=False, start=(0, 0)):
        """Engine.where_map_rows over the shards: where_join_rows with the map given as 1..JOIN_MAX_MAP (key, node id) pairs"""
        k, v, n = Q._jrows_pairs(keys, node_ids)
        args = Q._where_map_rows_args(base, clauses, link, fields, k, v, n, in_fields, with_ts, inner, start[1], start[0])
        return self._host_jrows("where_map_rows", args, len(fields), len(in_fields), with_ts, cap)

    def watch_create(self, base, clauses):
        """Engine.watch_create on every shard: one id, valid on all of them"""
        w = C.c_uint32()
        self._chk(self.L.bmx_comm_watch_create(self.h, *Q._where_args(base, clauses), C.byref(w)))
        return w.value

    def watch_poll(self, w, cap_entered=None, cap_left=None):
        """Engine.watch_poll over all shards: the lists are the shards' one after the other, the counts their sums, reset the OR of theirs; a poll that overflows
        commits on no shard. A cap of None: the poll counts first (caps of 0: it commits only if nothing changed) and then fetches with room for exactly that."""
        return self._host_watch_poll(w, cap_entered, cap_left)

    def watch_destroy(self, w):
        self._chk(self.L.bmx_comm_watch_destroy(self.h, int(w)))
