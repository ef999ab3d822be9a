"""What the queries return, as Python objects over the library's records, and the host-side merges the shard forms do with their shards' answers, restated
in numpy for the tests. Nothing here calls the library."""
import numpy as np

from ._abi import (FIRST_DTYPE, FIRST_OVERFLOW, FIRST_RES_DTYPE, GROUP_DTYPE, GROUP_OVERFLOW, GROUP_RES_DTYPE, GTOP_GRP_DTYPE, GTOP_NO_NODE, GTOP_OVERFLOW,
                   GTOP_RES_DTYPE, GTOP_ROW_DTYPE, JOIN_GROUP_OVERFLOW, JOIN_MAP_OVERFLOW, JOIN_RES_DTYPE, JROWS_RES_DTYPE, MGROUP_DTYPE, QUANT_MAX_DEN, REACH_MORE,
                   REACH_OVERFLOW, REACH_RES_DTYPE, ROWS_NO_CLOCK, ROWS_RES_DTYPE, SEMI_OVERFLOW, SEMI_RES_DTYPE, TOP_DTYPE, UPD_RES_DTYPE, VAL_DELETED, WATCH_OVERFLOW,
                   WATCH_RESET, FirstRes, GroupRes, GtopRes, JoinRes, JoinRowsRes, ReachRes, RowsRes, SemiRes, UpdRes)


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


def top_merge(lists, k, desc=False):
    """The merge bmx_comm_scan_top does with its shards' answers: `lists` are record arrays (TOP_DTYPE), each ordered by (val, id) — val descending with
    desc, id ascending either way; -> the first k records of their union in that order. Pure numpy: no library, no GPU."""
    parts = [np.asarray(x, TOP_DTYPE) for x in lists if len(x)]
    if not parts:
        return np.zeros(0, TOP_DTYPE)
    a = np.concatenate(parts)
    order = np.lexsort((a["id"], -a["val"] if desc else a["val"]))     # (|val| <= 2^53 - 1: the negation is exact)
    return a[order[:int(k)]]


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


def quant_rank(num, den, n):
    """The rank rule of bmx_where_quantiles, in one place: the 0-based rank, in ascending order, of the quantile num / den of a sample of n >= 1 elements
    ("lower" nearest rank: numpy.sort(v)[quant_rank(num, den, len(v))]). 0/1 is the minimum, 1/1 the maximum, 1/2 the lower median."""
    num, den, n = int(num), int(den), int(n)
    if not (1 <= den <= QUANT_MAX_DEN and 0 <= num <= den and n >= 1):
        raise ValueError("quant_rank: 0 <= num <= den, 1 <= den <= %d and n >= 1" % QUANT_MAX_DEN)
    return (num * (n - 1)) // den


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
