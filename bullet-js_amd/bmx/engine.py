"""Engine: one bmx_ctx, with the host-array and the device-pointer form of every call; and the owner and bucket formulas of include/bmx.h in numpy."""
import ctypes as C

import numpy as np

from ._abi import (DEFAULT_CTX_FLAGS, DELTA_REC_DTYPE, ERR_INTERNAL, EXPORT_ONLY_TOMBSTONES, INSERT_REFERENCE, MEM_DEVICE, MEM_HOST, MGROUP_DTYPE, REACH_MAX_DEPTH, SYNC_TOMBSTONES,
                   UPD_MAX_CAP, UPD_RES_DTYPE, BmxError, ExprRes, Info, JoinRes, MergeStats, Term, _np, _ptr, _ref, load_library)
from . import _queries as Q
from ._results import GroupResult, JoinResult, MultiGroupResult, UpdateResult


class Engine(Q._HostQueries):
    """One GPU-resident graph shard (a bmx_ctx). Host-array methods are synchronous; *_dev methods take
    device tensors/pointers and only enqueue work on the engine's stream."""
    _destroy, _last_error = "bmx_destroy", "bmx_last_error"

    def __init__(self, capacity_rows, device=0, flags=0, load_pct=0):
        self._create("bmx_create_ex", int(device), int(capacity_rows), int(load_pct), int(flags) | DEFAULT_CTX_FLAGS)
        self.device = device
        self._watch_base = {}        # watch id -> base field (watch_poll sizes its default lists from that field's index)

    def _host(self, name, *args):
        """bmx_<name>(ctx, *args, BMX_MEM_HOST): the synchronous form of a query"""
        return self._chk(getattr(self.L, "bmx_" + name)(self.h, *args, MEM_HOST))

    def _dev(self, name, *args):
        """bmx_<name>(ctx, *args, BMX_MEM_DEVICE): the outputs are device memory"""
        return self._chk(getattr(self.L, "bmx_" + name)(self.h, *args, MEM_DEVICE))

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
                                         _ptr(applied), _ref(na), _ptr(flags), _ref(st)))
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
        self._chk(self.L.bmx_merge_collect(self.h, int(t), _ptr(applied), _ref(na), _ptr(flags), _ref(st)))
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
        self._chk(self.L.bmx_dump_rows(self.h, n, _ptr(id), _ptr(field), _ptr(ts), _ptr(val), _ref(m), MEM_HOST))
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
            self._chk(self.L.bmx_export_rows(self.h, int(since), int(log2_buckets), _ptr(bits), fl, None, 0, _ref(m), MEM_HOST))
            cap = m.value
        recs = out if out is not None else np.zeros(int(cap), DELTA_REC_DTYPE)
        self._chk(self.L.bmx_export_rows(self.h, int(since), int(log2_buckets), _ptr(bits), fl, _ptr(recs) if cap else None, int(cap), _ref(m), MEM_HOST))
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
            return self._scan_ids("scan_range", (int(field), int(lo), int(hi)), len(out) if cap is None else min(cap, len(out)), out)
        cap = self.index_size(field) if cap is None else cap
        return self._scan_ids("scan_range", (int(field), int(lo), int(hi)), cap, np.zeros(max(cap, 1), np.uint64)).copy()

    def _scan_ids(self, name, args, cap, out):
        """a scan that writes up to cap entries into `out` and counts its matches -> the written part of out"""
        m = C.c_uint64()
        self._host(name, *args, _ptr(out), cap, _ref(m))
        return out[:min(m.value, cap)]

    def scan_range_pos(self, field, lo, hi, cap=None):
        """positions (u32, ascending) of the matches in the index columns instead of their node ids"""
        cap = self.index_size(field) if cap is None else cap
        return self._scan_ids("scan_range_pos", (int(field), int(lo), int(hi)), cap, np.zeros(max(cap, 1), np.uint32)).copy()

    def index_ids(self, field, first=0, count=None):
        count = self.index_size(field) - first if count is None else count
        out = np.zeros(max(count, 1), np.uint64)
        self._chk(self.L.bmx_index_ids(self.h, int(field), int(first), int(count), _ptr(out), MEM_HOST))
        return out[:count].copy()

    def scan_equals(self, field, value):
        return self.scan_range(field, value, value)

    def scan_count(self, field, lo, hi):
        m = C.c_uint64()
        self._chk(self.L.bmx_scan_count(self.h, int(field), int(lo), int(hi), _ref(m), MEM_HOST))
        return m.value

    def scan_filter(self, terms, cap=None):
        arr = (Term * len(terms))(*[Term(int(f), 0, int(lo), int(hi)) for f, lo, hi in terms])
        cap = self.index_size(terms[0][0]) if cap is None else cap
        return self._scan_ids("scan_filter", (len(terms), arr), cap, np.zeros(max(cap, 1), np.uint64)).copy()

    def scan_aggregate(self, terms, measure=None, group=None, group_lo=0, ngroups=0):
        """count / sum / min / max of field `measure` over the nodes that satisfy every (field, lo, hi) of `terms`, without fetching an id. ngroups == 0:
        one AggResult; otherwise the list of ngroups + 1: entry g for value(group) == group_lo + g, the last for the nodes outside the window."""
        return self._host_aggregate("scan_aggregate", Q._agg_args(terms, measure, group, group_lo, ngroups), ngroups)

    def scan_top(self, terms, k, desc=False, after=None):
        """The first k nodes, ordered by (value of terms[0]'s field, id) — value descending with desc — of the nodes that satisfy every (field, lo, hi) of
        `terms` and come strictly after the cursor `after` (a record of an earlier answer, or (id, val); None: from the beginning).
        -> (records: ndarray of TOP_DTYPE, n_eligible)"""
        return self._host_top("scan_top", Q._top_args(terms, k, desc, after), k)

    def scan_where(self, base, clauses, cap=None, count_only=False):
        """Boolean filter (bmx_where.h): the nodes holding data in field `base` for which some clause of `clauses` has all of its literals true; a literal is
        (field, lo, hi) or (field, lo, hi, negated), the negated one being true for an absent or tombstoned field too. -> ids in index order of `base`
        (at most cap of them). count_only (as Comm.scan_where has it): -> the number of matches, no id is fetched."""
        if cap is None and not count_only:
            cap = self.index_size(base)
        return self._host_scan_where(Q._where_args(base, clauses), cap, count_only)

    def where_aggregate(self, base, clauses, measure=None, group=None, group_lo=0, ngroups=0):
        """scan_aggregate over the selection of scan_where(base, clauses) (bmx_where_agg.h): count / sum / min / max of field `measure`, grouped by field `group`
        in the window group_lo .. group_lo + ngroups - 1, without fetching an id. -> what scan_aggregate returns"""
        return self._host_aggregate("where_aggregate", Q._where_aggregate_args(base, clauses, measure, group, group_lo, ngroups), ngroups)

    def where_top(self, base, clauses, k, desc=False, after=None):
        """scan_top over the selection of scan_where(base, clauses): the first k nodes ordered by (value of `base`, id) — value descending with desc — that come
        strictly after the cursor `after`. -> (records: ndarray of TOP_DTYPE, n_eligible)"""
        return self._host_top("where_top", Q._where_top_args(base, clauses, k, desc, after), k)

    def where_group(self, base, clauses, group, measure=None, cap=65536):
        """Group-by over discovered values (bmx_group.h): count / sum / min / max of field `measure` over the selection of scan_where(base, clauses), one
        record per distinct value of field `group` that occurs among the selected nodes; nobody has to know the values in advance. -> GroupResult (with
        overflow set and no records when there are more than cap distinct values: ask again with more room or a narrower program)"""
        return GroupResult(*self._host_group("where_group", Q._where_group_args(base, clauses, measure, group), cap))

    def where_quantiles(self, base, clauses, measure, qs):
        """Exact quantiles (bmx_quant.h): the order statistics of field `measure` over the selection of scan_where(base, clauses), selected on the device.
        qs: up to QUANT_MAX pairs (num, den), in any order, repeats allowed. -> (records: ndarray of QUANT_REC_DTYPE in the order of qs — value, rank
        (quant_rank(num, den, n)), n_below, n_equal — and a QuantRes: n_match, n, min, max)"""
        return self._host_quantiles("where_quantiles", Q._where_quantiles_args(base, clauses, measure, qs), len(qs))

    def where_aggregate_expr(self, base, clauses, expr, group=None, group_lo=0, ngroups=0):
        """where_aggregate with a computed measure (bmx_expr.h): expr = bmx.Expr(a, op, b), the measure of a selected node is value(a) op value(b).
        -> (what where_aggregate returns, ExprRes)"""
        x = ExprRes()
        return self._host_aggregate("where_aggregate_expr", Q._where_aggregate_args(base, clauses, expr, group, group_lo, ngroups), ngroups, (x,)), x

    def where_group_expr(self, base, clauses, group, expr, cap=65536):
        """where_group with a computed measure (bmx_expr.h). -> (GroupResult, ExprRes)"""
        x = ExprRes()
        return GroupResult(*self._host_group("where_group_expr", Q._where_group_args(base, clauses, expr, group), cap, (x,))), x

    def where_quantiles_expr(self, base, clauses, expr, qs):
        """where_quantiles with a computed measure (bmx_expr.h): the sample is value(a) op value(b) of the selected nodes where it is defined and in range.
        -> (records, QuantRes, ExprRes)"""
        x = ExprRes()
        return (*self._host_quantiles("where_quantiles_expr", Q._where_quantiles_args(base, clauses, expr, qs), len(qs), (x,)), x)

    def where_rows(self, base, clauses, fields, cap=None, with_ts=False, start=0):
        """Row projection (bmx_rows.h): the selection of scan_where(base, clauses) from index position `start` on, and for each of the first cap selected nodes
        its id and the values (with_ts: and clocks) of `fields`, in one call. cap None: room for the whole index. -> RowsResult; its next_pos is the `start` of
        the next page."""
        cap = self.index_size(base) if cap is None else int(cap)
        return self._host_rows(Q._where_rows_args(base, clauses, fields, with_ts, start), len(fields), with_ts, cap)

    def where_group_first(self, base, clauses, group, order, fields=(), desc=False, with_ts=False, cap=65536):
        """The first node per group (bmx_first.h): per distinct value of field `group` among the selection of scan_where(base, clauses), the node that comes
        first by the value of field `order` (descending with desc), then by id (always ascending, unsigned), with the values (with_ts: and clocks) of
        `fields` on that node. -> FirstResult (with overflow set and no records when there are more than cap distinct values)"""
        return self._host_group_first(Q._where_group_first_args(base, clauses, group, order, fields, desc, with_ts), len(fields), with_ts, int(cap))

    def where_group_top(self, base, clauses, group, order, per, fields=(), desc=False, with_ts=False, cap=65536):
        """The first `per` nodes per group (bmx_group_top.h): per distinct value of field `group` among the selection of scan_where(base, clauses), the `per`
        nodes that come first by the value of field `order` (descending with desc), then by id (always ascending, unsigned), in that order, with the values
        (with_ts: and clocks) of `fields` on each. -> GroupTopResult (with overflow set and no groups when there are more than cap distinct values)"""
        return self._host_group_top(Q._where_group_top_args(base, clauses, group, order, per, fields, desc, with_ts), len(fields), with_ts, int(cap), int(per))

    def where_group_multi(self, base, clauses, keys, measure=None, cap=65536):
        """Group-by over several fields (bmx_group_multi.h): count / sum / min / max of field `measure` over the selection of scan_where(base, clauses), one
        record per distinct key tuple that occurs among the selected nodes. keys: 1..4 of `field` (the value itself) or (field, origin, width) (the bucket
        (value - origin) // width). A node that lacks any key is counted in absent. -> MultiGroupResult (with overflow set and no groups if there are more
        than cap tuples; cap <= GROUP_MAX_CAP, <= MGROUP_MAX_CAP4 with four keys)."""
        return MultiGroupResult(*self._host_group("where_group_multi", Q._where_group_multi_args(base, clauses, keys, measure), cap, dtype=MGROUP_DTYPE), len(keys))

    def where_update(self, base, clauses, target, op, operand=0, src=None, ts=None, force=False, cap=None, start=0, want_ids=False):
        """Update by query (bmx_update.h): on every node scan_where(base, clauses) selects from index position `start` on, field `target` gets the record
        (ts, val), val being `operand` (UPD_SET), a tombstone (UPD_DELETE; needs force), the node's value of `src` (UPD_COPY) or that value + operand (UPD_ADD).
        Default: through conflict resolution like merge_batch(INSERT_DELTA); force: stored as given like put_rows. cap None: min(index size, UPD_MAX_CAP);
        cap 0 counts only. ts None: the wall clock in milliseconds. want_ids: the ids of the nodes whose row changed. -> UpdateResult; its next_pos is the `start` of the next page."""
        cap = min(self.index_size(base), UPD_MAX_CAP) if cap is None else int(cap)
        return self._host_update(Q._where_update_args(base, clauses, target, op, operand, src, ts, force, start), cap, want_ids)

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
        cap = None if count_only else (self.index_size(base) if cap is None else int(cap))
        return self._host_semi("where_semijoin", Q._where_semijoin_args(base, clauses, link, anti, inner_base, inner_clauses, key, set_cap), cap, count_only)

    def where_in(self, base, clauses, link, values, anti=False, cap=None, count_only=False):
        """where_semijoin with the set given as a list of 1..SEMI_MAX_SET int64 values (duplicates allowed; a value outside +-(2^53 - 1) is skipped)"""
        cap = None if count_only else (self.index_size(base) if cap is None else int(cap))
        v, n = Q._semi_values(values)
        return self._host_semi("where_in", Q._where_in_args(base, clauses, link, anti, v, n), cap, count_only)

    def where_reach(self, base, clauses, link, key, seed_base, seed_clauses, seed_field, max_depth=REACH_MAX_DEPTH, set_cap=65536, cap=None, count_only=False):
        """Graph traversal (bmx_reach.h): the nodes of scan_where(base, clauses) reachable, over the edges link -> key of those nodes, from the values field
        `seed_field` holds on the nodes of scan_where(seed_base, seed_clauses), with their breadth-first depth; swapping link and key walks toward the
        ancestors. The closure runs on the device. cap None: room for the whole index of `base`; count_only: nothing is fetched. -> ReachResult (with overflow
        set, n_match 0 and no ids when seeds and contributed values are more than set_cap)"""
        cap = None if count_only else (self.index_size(base) if cap is None else int(cap))
        return self._host_reach("where_reach", Q._where_reach_args(base, clauses, link, key, seed_base, seed_clauses, seed_field, max_depth, set_cap), cap, count_only)

    def where_reach_from(self, base, clauses, link, key, values, max_depth=REACH_MAX_DEPTH, set_cap=65536, cap=None, count_only=False):
        """where_reach with the seeds given as a list of 1..REACH_MAX_SET int64 values (duplicates allowed; a value outside +-(2^53 - 1) is skipped)"""
        cap = None if count_only else (self.index_size(base) if cap is None else int(cap))
        v, n = Q._semi_values(values)
        return self._host_reach("where_reach_from", Q._where_reach_from_args(base, clauses, link, key, v, n, max_depth, set_cap), cap, count_only)

    def where_join_group(self, base, clauses, link, inner_base, inner_clauses, key, attr, measure=None, cap=65536, map_cap=65536):
        """Lookup join (bmx_join.h): the selection of scan_where(base, clauses) grouped by the value field `attr` holds on the node of
        scan_where(inner_base, inner_clauses) whose field `key` equals the selected node's field `link` (the minimum of `attr` where several inner nodes share a
        key). The map is built and looked up on the device. -> JoinResult"""
        return JoinResult(*self._host_group("where_join_group", Q._where_join_group_args(base, clauses, link, measure, inner_base, inner_clauses, key, attr, map_cap), cap, res=JoinRes))

    def where_map_group(self, base, clauses, link, keys, vals, measure=None, cap=65536):
        """where_join_group with the map given as 1..JOIN_MAX_MAP (key, val) pairs (a key outside +-(2^53 - 1) is skipped, a val outside it means "no
        attribute", duplicate keys take the minimum of their vals)"""
        k, v, n = Q._join_pairs(keys, vals)
        return JoinResult(*self._host_group("where_map_group", Q._where_map_group_args(base, clauses, link, measure, k, v, n), cap, res=JoinRes))

    def where_join_rows(self, base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, cap=None, with_ts=False, inner=False, start=0, map_cap=65536):
        """Join projection (bmx_join_rows.h): the selection of scan_where(base, clauses) from index position `start` on, each row with the values (with_ts:
        and clocks) of `fields` and with the id and the `in_fields` of the node of scan_where(inner_base, inner_clauses) whose field `key` equals the row's
        field `link` (the smallest unsigned id where several share a key). A left join; inner=True drops the rows without inner node from the selection. cap
        None: room for the whole index of `base`. -> JoinRowsResult"""
        cap = self.index_size(base) if cap is None else int(cap)
        args = Q._where_join_rows_args(base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, map_cap, with_ts, inner, start)
        return self._host_jrows("where_join_rows", args, len(fields), len(in_fields), with_ts, cap)

    def where_map_rows(self, base, clauses, link, fields, keys, node_ids, in_fields, cap=None, with_ts=False, inner=False, start=0):
        """where_join_rows with the map given as 1..JOIN_MAX_MAP (key, node id) pairs (a key outside +-(2^53 - 1) or the id JROWS_NO_NODE is skipped,
        duplicate keys take the smallest id)"""
        cap = self.index_size(base) if cap is None else int(cap)
        k, v, n = Q._jrows_pairs(keys, node_ids)
        args = Q._where_map_rows_args(base, clauses, link, fields, k, v, n, in_fields, with_ts, inner, start)
        return self._host_jrows("where_map_rows", args, len(fields), len(in_fields), with_ts, cap)

    def watch_create(self, base, clauses):
        """A standing query (bmx_watch.h): the program of scan_where(base, clauses), kept on the device together with its last committed answer. -> the watch id"""
        w = C.c_uint32()
        self._chk(self.L.bmx_watch_create(self.h, *Q._where_args(base, clauses), C.byref(w)))
        self._watch_base[w.value] = int(base)
        return w.value

    def watch_poll(self, w, cap_entered=None, cap_left=None):
        """What changed in the watch's answer since its last committed poll -> WatchPoll. A cap of None is room for the whole index (such a poll always commits)."""
        if cap_entered is None or cap_left is None:
            base = self._watch_base.get(int(w))
            n = self.index_size(base) if base is not None else 0       # (an unknown id: the library refuses it below)
            cap_entered = n if cap_entered is None else cap_entered
            cap_left = n if cap_left is None else cap_left
        return self._host_watch_poll(w, cap_entered, cap_left)

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
        self._dev("scan_aggregate", *Q._agg_args(terms, measure, group, group_lo, ngroups), _ptr(out))

    def scan_top_dev(self, terms, k, out, n_out=None, n_eligible=None, desc=False, after=None):
        """scan_top into device memory (`out`: room for k records of 16 bytes; n_out, n_eligible: one uint64 each, or None); enqueue-only. The cursor is
        host data either way."""
        self._dev("scan_top", *Q._top_args(terms, k, desc, after), _ptr(out), _ptr(n_out), _ptr(n_eligible))

    def scan_where_dev(self, base, clauses, out, cap, n_out):
        """scan_where into device memory (`out`: room for cap ids, or None to count; n_out: one uint64); enqueue-only. The program is host data."""
        self._dev("scan_where", *Q._where_args(base, clauses), _ptr(out), int(cap), _ptr(n_out))

    def where_aggregate_dev(self, base, clauses, out, measure=None, group=None, group_lo=0, ngroups=0):
        """where_aggregate into device memory (`out` as for scan_aggregate_dev); enqueue-only. The program is host data."""
        self._dev("where_aggregate", *Q._where_aggregate_args(base, clauses, measure, group, group_lo, ngroups), _ptr(out))

    def where_top_dev(self, base, clauses, k, out, n_out=None, n_eligible=None, desc=False, after=None):
        """where_top into device memory (`out`, n_out, n_eligible as for scan_top_dev); enqueue-only. The program and the cursor are host data."""
        self._dev("where_top", *Q._where_top_args(base, clauses, k, desc, after), _ptr(out), _ptr(n_out), _ptr(n_eligible))

    def where_group_dev(self, base, clauses, group, out, res, measure=None, cap=65536):
        """where_group into device memory (`out`: room for cap records of 56 bytes; res: 112 bytes, a bmx_group_res); enqueue-only. The records come in no
        particular order; after sync(), GroupResult(res.cpu().numpy().view(GROUP_RES_DTYPE)[0], np.sort(out.cpu().numpy().view(GROUP_DTYPE)[:n], order="key"))
        reads them. The program is host data."""
        self._dev("where_group", *Q._where_group_args(base, clauses, measure, group), _ptr(out), int(cap), _ptr(res))

    def where_quantiles_dev(self, base, clauses, measure, qs, out, res=None):
        """where_quantiles into device memory (`out`: room for len(qs) records of 32 bytes; res: 32 bytes, a bmx_quant_res, or None); enqueue-only. After
        sync(), out.cpu().numpy().view(QUANT_REC_DTYPE) and res.cpu().numpy().view(QUANT_RES_DTYPE)[0] read them. The program and qs are host data."""
        self._dev("where_quantiles", *Q._where_quantiles_args(base, clauses, measure, qs), _ptr(out), _ptr(res))

    def where_aggregate_expr_dev(self, base, clauses, expr, out, xres=None, group=None, group_lo=0, ngroups=0):
        """where_aggregate_expr into device memory (`out` as for where_aggregate_dev; xres: 16 bytes, a bmx_expr_res, or None); enqueue-only. After sync(),
        xres.cpu().numpy().view(EXPR_RES_DTYPE)[0] reads the counters. The program and the expression are host data."""
        self._dev("where_aggregate_expr", *Q._where_aggregate_args(base, clauses, expr, group, group_lo, ngroups), _ptr(out), _ptr(xres))

    def where_group_expr_dev(self, base, clauses, group, expr, out, res, xres=None, cap=65536):
        """where_group_expr into device memory (`out`, res as for where_group_dev; xres as for where_aggregate_expr_dev); enqueue-only."""
        self._dev("where_group_expr", *Q._where_group_args(base, clauses, expr, group), _ptr(out), int(cap), _ptr(res), _ptr(xres))

    def where_quantiles_expr_dev(self, base, clauses, expr, qs, out, res=None, xres=None):
        """where_quantiles_expr into device memory (`out`, res as for where_quantiles_dev; xres as for where_aggregate_expr_dev); enqueue-only."""
        self._dev("where_quantiles_expr", *Q._where_quantiles_args(base, clauses, expr, qs), _ptr(out), _ptr(res), _ptr(xres))

    def where_rows_dev(self, base, clauses, fields, cap, out_ids, out_val, out_ts, res, start=0):
        """where_rows into device memory (out_ids: room for cap ids; out_val: len(fields) columns of cap int64 each, field after field; out_ts: the same for
        the clocks, or None for none; res: 40 bytes, a bmx_rows_res); enqueue-only. After sync(), res.cpu().numpy().view(ROWS_RES_DTYPE)[0] reads the record.
        The program, the fields and the cursor are host data."""
        self._dev("where_rows", *Q._where_rows_args(base, clauses, fields, out_ts is not None, start), int(cap), _ptr(out_ids), _ptr(out_val), _ptr(out_ts), _ptr(res))

    def where_group_first_dev(self, base, clauses, group, order, out, out_val, out_ts, res, fields=(), desc=False, cap=65536):
        """where_group_first into device memory (`out`: room for cap records of 40 bytes; out_val: len(fields) columns of cap int64 each, field after field;
        out_ts: the same for the clocks, or None for none; res: 40 bytes, a bmx_first_res); enqueue-only. The records come in no particular order, but row r of
        every column belongs to out[r]; after sync(), res.cpu().numpy().view(FIRST_RES_DTYPE)[0] and out.cpu().numpy().view(FIRST_DTYPE)[:n] read them. The
        program and the fields are host data."""
        self._dev("where_group_first", *Q._where_group_first_args(base, clauses, group, order, fields, desc, out_ts is not None), int(cap), _ptr(out), _ptr(out_val),
                  _ptr(out_ts), _ptr(res))

    def where_group_top_dev(self, base, clauses, group, order, per, out, out_rows, out_val, out_ts, res, fields=(), desc=False, cap=65536):
        """where_group_top into device memory (`out`: room for cap groups of 32 bytes; out_rows: cap * per rows of 16 bytes; out_val: len(fields) columns of
        cap * per int64 each, field after field; out_ts: the same for the clocks, or None for none; res: 48 bytes, a bmx_gtop_res); enqueue-only. The groups
        come in no particular order, but block g of every array belongs to out[g]; after sync(), res.cpu().numpy().view(GTOP_RES_DTYPE)[0],
        out.cpu().numpy().view(GTOP_GRP_DTYPE)[:n] and out_rows.cpu().numpy().view(GTOP_ROW_DTYPE)[:n * per] read them. The program and the fields are host
        data."""
        self._dev("where_group_top", *Q._where_group_top_args(base, clauses, group, order, per, fields, desc, out_ts is not None), int(cap), _ptr(out), _ptr(out_rows),
                  _ptr(out_val), _ptr(out_ts), _ptr(res))

    def where_group_multi_dev(self, base, clauses, keys, out, res, measure=None, cap=65536):
        """where_group_multi into device memory (`out`: room for cap records of 80 bytes; res: 112 bytes, a bmx_group_res); enqueue-only. The keys are host
        data. The records come in no particular order; after sync(), MultiGroupResult(res.cpu().numpy().view(GROUP_RES_DTYPE)[0],
        mgroup_sort(out.cpu().numpy().view(MGROUP_DTYPE)[:n]), len(keys)) is what where_group_multi returns."""
        self._dev("where_group_multi", *Q._where_group_multi_args(base, clauses, keys, measure), _ptr(out), int(cap), _ptr(res))

    def where_update_dev(self, base, clauses, target, op, cap, out_ids, res, operand=0, src=None, ts=None, force=False, start=0):
        """where_update with out_ids (room for cap ids, or None) and res (72 bytes, a bmx_upd_res) in device memory. NOT enqueue-only: the call waits once for
        the counts between its emit pass and the merge; out_ids and res are written by its last kernel and valid after sync() or in stream order, when
        res.cpu().numpy().view(UPD_RES_DTYPE)[0] reads the record. The program and the operands are host data."""
        self._dev("where_update", *Q._where_update_args(base, clauses, target, op, operand, src, ts, force, start), int(cap), _ptr(out_ids), _ptr(res))

    def where_semijoin_dev(self, base, clauses, link, inner_base, inner_clauses, key, out_ids, cap, res, anti=False, set_cap=65536):
        """where_semijoin into device memory (out_ids: room for cap ids, or None with cap 0; res: 32 bytes, a bmx_semi_res); enqueue-only. After sync(),
        SemiResult(res.cpu().numpy().view(SEMI_RES_DTYPE)[0], out_ids.cpu().numpy(), cap) is what where_semijoin returns."""
        self._dev("where_semijoin", *Q._where_semijoin_args(base, clauses, link, anti, inner_base, inner_clauses, key, set_cap), _ptr(out_ids), int(cap), _ptr(res))

    def where_in_dev(self, base, clauses, link, values, nvalues, out_ids, cap, res, anti=False):
        """where_in into device memory; `values` is a device array of nvalues int64. Enqueue-only."""
        self._dev("where_in", *Q._where_in_args(base, clauses, link, anti, values, nvalues), _ptr(out_ids), int(cap), _ptr(res))

    def where_reach_dev(self, base, clauses, link, key, seed_base, seed_clauses, seed_field, out_ids, out_depth, cap, res, max_depth=REACH_MAX_DEPTH, set_cap=65536):
        """where_reach into device memory (out_ids: room for cap ids, out_depth: for cap bytes, or both None with cap 0; res: 40 bytes, a bmx_reach_res);
        enqueue-only, all max_depth rounds included. After sync(), ReachResult(res.cpu().numpy().view(REACH_RES_DTYPE)[0], out_ids.cpu().numpy(),
        out_depth.cpu().numpy(), cap) is what where_reach returns."""
        self._dev("where_reach", *Q._where_reach_args(base, clauses, link, key, seed_base, seed_clauses, seed_field, max_depth, set_cap), _ptr(out_ids), _ptr(out_depth),
                  int(cap), _ptr(res))

    def where_reach_from_dev(self, base, clauses, link, key, values, nvalues, out_ids, out_depth, cap, res, max_depth=REACH_MAX_DEPTH, set_cap=65536):
        """where_reach_from into device memory; `values` is a device array of nvalues int64. Enqueue-only."""
        self._dev("where_reach_from", *Q._where_reach_from_args(base, clauses, link, key, values, nvalues, max_depth, set_cap), _ptr(out_ids), _ptr(out_depth), int(cap),
                  _ptr(res))

    def where_join_group_dev(self, base, clauses, link, inner_base, inner_clauses, key, attr, out, res, measure=None, cap=65536, map_cap=65536):
        """where_join_group into device memory (`out`: room for cap records of 56 bytes; res: 184 bytes, a bmx_join_res); enqueue-only. The records come in no
        particular order; after sync(), JoinResult(res.cpu().numpy().view(JOIN_RES_DTYPE)[0], np.sort(out.cpu().numpy().view(GROUP_DTYPE)[:n], order="key"))
        is what where_join_group returns."""
        self._dev("where_join_group", *Q._where_join_group_args(base, clauses, link, measure, inner_base, inner_clauses, key, attr, map_cap), _ptr(out), int(cap), _ptr(res))

    def where_map_group_dev(self, base, clauses, link, keys, vals, npairs, out, res, measure=None, cap=65536):
        """where_map_group into device memory; `keys` and `vals` are device arrays of npairs int64. Enqueue-only."""
        self._dev("where_map_group", *Q._where_map_group_args(base, clauses, link, measure, keys, vals, npairs), _ptr(out), int(cap), _ptr(res))

    def where_join_rows_dev(self, base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val,
                            out_in_ts, res, inner=False, start=0, map_cap=65536):
        """where_join_rows into device memory (out_ids / out_in_ids: room for cap ids; out_val / out_in_val: one column of cap int64 per field of that side;
        out_ts / out_in_ts: the same for the clocks, or both None for none; res: 72 bytes, a bmx_jrows_res); enqueue-only. After sync(),
        res.cpu().numpy().view(JROWS_RES_DTYPE)[0] reads the record."""
        with_ts = out_ts is not None or out_in_ts is not None
        self._dev("where_join_rows", *Q._where_join_rows_args(base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, map_cap, with_ts, inner, start), int(cap),
                  _ptr(out_ids), _ptr(out_val), _ptr(out_ts), _ptr(out_in_ids), _ptr(out_in_val), _ptr(out_in_ts), _ptr(res))

    def where_map_rows_dev(self, base, clauses, link, fields, keys, node_ids, npairs, in_fields, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val, out_in_ts, res,
                           inner=False, start=0):
        """where_map_rows into device memory; `keys` (int64) and `node_ids` (uint64 bit patterns) are device arrays of npairs words. Enqueue-only."""
        with_ts = out_ts is not None or out_in_ts is not None
        self._dev("where_map_rows", *Q._where_map_rows_args(base, clauses, link, fields, keys, node_ids, npairs, in_fields, with_ts, inner, start), int(cap), _ptr(out_ids),
                  _ptr(out_val), _ptr(out_ts), _ptr(out_in_ids), _ptr(out_in_val), _ptr(out_in_ts), _ptr(res))

    def watch_poll_dev(self, w, entered, cap_entered, left, cap_left, res):
        """watch_poll into device memory (entered / left: room for cap ids each, or None with a cap of 0; res: 32 bytes, a bmx_watch_res); enqueue-only: the
        decision whether the poll commits is taken on the device."""
        self._dev("watch_poll", int(w), _ptr(entered), int(cap_entered), _ptr(left), int(cap_left), _ptr(res))

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
