"""A model of the group-by over several fields (include/bmx_group_multi.h, csrc/mgroup_kernels.h), shared by test_mgroup_model.py (CPU) and the GPU tests
(helper, not a test). The table and the selection are where_agg_model's (a state per field and node: absent, data, tombstone); the kernel's geometry (mix, home,
cache_set, slots_for, place, grid) is group_model's, which the new kernels reuse as they stand.

Two halves:

answer(m, base, clauses, keys, measure, cap) : the brute-force answer — the tuples through Python dicts, the sums as Python ints, // for the buckets -> (records
    sorted lexicographically, result record), or on overflow (no records, flags, absent, total). keys: a list of field or (field, origin, width).

Device(...) : a sequential stand-in of the design. Rows in position order; a row that lacks any key goes to absent; every other row looks each value up in
    that key's dictionary (group_model's walk: the code is the slot), packs the codes into one word and goes through group_model.Device's cache / bypass / flush /
    table under that word. It tags every dictionary access ('dict', j, 'home' / 'walk' / 'wrap' / 'noroom') and (('dict', j, 'len'), n), and every tuple-table
    access and row as group_model.Device does ('home', 'walk', 'wrap', 'noroom', ('len', n), 'hit', 'bypass'), and the workgroup's insert-only LDS cache
    value -> code in front of the dictionaries (('dcache', 'hit' / 'claim' / 'taken': the entry holds another value)). The dictionaries live in a Scratch that
    outlasts the query, as the context's do: finish() empties them.

What does not depend on the order in which lanes arrive, and is therefore what the GPU tests assert from the model: the answer; the set of values of a
dictionary; for values that all share one home slot the multiset of walk lengths. Which value gets which code depends on who comes first — unless every value of
a dictionary has a home of its own, which is how the layouts that need known packed words are built."""
import numpy as np

import group_model as gm
import where_agg_model as wam
from where_agg_model import DATA, Model  # noqa: F401

AGG_DTYPE = wam.AGG_DTYPE
MGROUP_DTYPE = np.dtype([("key", "<i8", (4,)), ("agg", AGG_DTYPE)])
GROUP_RES_DTYPE = gm.GROUP_RES_DTYPE
OVERFLOW, MAX_CAP, MAX_CAP4, MAX_KEYS = 1, 1 << 20, 1 << 14, 4
BIG, WIDE, FILL = gm.BIG, gm.WIDE, gm.FILL
I64MIN, I64MAX = wam.I64MIN, wam.I64MAX


def norm(keys):
    return [(int(k), 0, 1) if isinstance(k, (int, np.integer)) else (int(k[0]), int(k[1]), int(k[2])) for k in keys]


def bucket(v, origin, width):
    return (int(v) - origin) // width


def shift_for(cap):
    return gm.slots_for(cap).bit_length() - 1


def record(n_match, measured):
    """one bmx_agg record from Python ints: n_match rows, `measured` the list of measure values among them (None: no measure field)"""
    r = np.zeros((), AGG_DTYPE)
    r["n_match"] = n_match; r["min"] = I64MAX; r["max"] = I64MIN
    if measured is None:
        r["n"] = n_match
        return r
    r["n"] = len(measured)
    if measured:
        s = sum(int(v) for v in measured) & ((1 << 128) - 1)
        r["min"] = min(measured); r["max"] = max(measured)
        r["sum_lo"] = s & ((1 << 64) - 1)
        hi = s >> 64
        r["sum_hi"] = hi - (1 << 64) if hi >= (1 << 63) else hi
    return r


def sort_records(recs):
    recs = np.asarray(recs, MGROUP_DTYPE)
    k = recs["key"]
    return recs[np.lexsort((k[:, 3], k[:, 2], k[:, 1], k[:, 0]))]


# ---- the brute-force answer ----
def rows_of(m, base, clauses, keys, measure, nodes=None):
    """-> (sel, kvals, mval) by node (or by position with nodes = the node numbers of the positions): kvals[p] a tuple of raw values with None where the node
    lacks the field; mval[p] an int or None"""
    keys = norm(keys)
    sel = m.mask(base, clauses)
    for f, _, _ in keys:
        m._f(f)
    if measure is not None:
        m._f(measure)
    nodes = np.arange(m.N) if nodes is None else np.asarray(nodes)
    cols = [(m.val[f][nodes], m.st[f][nodes] == DATA) for f, _, _ in keys]
    kv = [tuple(int(v[p]) if h[p] else None for v, h in cols) for p in range(len(nodes))]
    if measure is None:
        mv = [None] * len(nodes)
    else:
        v, h = m.val[measure][nodes], m.st[measure][nodes] == DATA
        mv = [int(v[p]) if h[p] else None for p in range(len(nodes))]
    return sel[nodes], kv, mv


def answer(m, base, clauses, keys, measure=None, cap=65536):
    keys = norm(keys)
    sel, kv, mv = rows_of(m, base, clauses, keys, measure)
    groups, absent, total = {}, [], []
    for p in np.nonzero(sel)[0]:
        total.append(p)
        if any(v is None for v in kv[p]):
            absent.append(p)
            continue
        groups.setdefault(tuple(bucket(v, o, w) for v, (_, o, w) in zip(kv[p], keys)), []).append(p)

    def rec(rows):
        return record(len(rows), None if measure is None else [mv[p] for p in rows if mv[p] is not None])

    res = np.zeros((), GROUP_RES_DTYPE)
    res["absent"] = rec(absent); res["total"] = rec(total); res["n_groups"] = len(groups)
    if len(groups) > cap:
        res["flags"] = OVERFLOW
        return np.zeros(0, MGROUP_DTYPE), res
    out = np.zeros(len(groups), MGROUP_DTYPE)
    for i, t in enumerate(sorted(groups)):
        out[i]["key"][:len(t)] = t; out[i]["agg"] = rec(groups[t])
    return out, res


def sum_of(r):
    return (int(r["sum_hi"]) << 64) + int(r["sum_lo"])


def invariant(recs, res):
    t, a = res["total"], res["absent"]
    return (int(recs["agg"]["n_match"].sum()) + int(a["n_match"]) == int(t["n_match"]) and int(recs["agg"]["n"].sum()) + int(a["n"]) == int(t["n"])
            and sum(sum_of(x["agg"]) for x in recs) + sum_of(a) == sum_of(t))


def check(got_recs, got_res, want_recs, want_res, cap, host=True):
    """every comparison the tests make -> None or what differs. got_recs: the caller's whole buffer (cap + 1 records or more), pattern-filled before the call."""
    got_recs = np.asarray(got_recs, MGROUP_DTYPE)
    for k in ("absent", "total"):
        if np.asarray(got_res[k]).tobytes() != np.asarray(want_res[k]).tobytes():
            return (k, got_res[k], want_res[k])
    if int(got_res["reserved"]) != 0:
        return ("reserved", int(got_res["reserved"]))
    if int(want_res["flags"]) & OVERFLOW:
        if int(got_res["flags"]) != OVERFLOW or not (cap < int(got_res["n_groups"]) <= int(want_res["n_groups"])):
            return ("overflow", int(got_res["flags"]), int(got_res["n_groups"]))
        return None if (got_recs.view(np.uint8) == FILL).all() else ("out written on overflow",)
    if int(got_res["flags"]) != 0 or int(got_res["n_groups"]) != len(want_recs):
        return ("n_groups / flags", int(got_res["flags"]), int(got_res["n_groups"]), len(want_recs))
    d = len(want_recs)
    if not (got_recs[d:].view(np.uint8) == FILL).all():
        return ("written at or beyond out[D]",)
    g = got_recs[:d]
    if host and g.tobytes() != sort_records(g).tobytes():
        return ("host records not sorted lexicographically",)
    g = sort_records(g)
    if g.tobytes() != np.asarray(want_recs, MGROUP_DTYPE).tobytes():
        bad = [i for i in range(d) if g[i].tobytes() != want_recs[i].tobytes()]
        return ("record", bad[0], g[bad[0]], want_recs[bad[0]])
    if not invariant(g, got_res):
        return ("invariant",)
    return None


# ---- the sequential stand-in ----
class Scratch:
    """what outlasts a query: the dictionaries (slot -> value, per key). A correct query leaves them empty."""

    def __init__(self):
        self.dicts = [{} for _ in range(MAX_KEYS)]

    def empty(self):
        return not any(self.dicts)


DEFECTS = ("overlap", "trunc", "absent_in_group", "sort_key0", "write_on_overflow", "write_behind", "stale_dict")


class Device:
    """One query over a column laid out by position. defect: None or one of DEFECTS — 'overlap' (the code fields of the packed word overlap by one bit),
    'trunc' (the bucket truncates toward zero), 'absent_in_group' (a missing key counts as 0), 'sort_key0' (the host answer sorted by key[0] only),
    'write_on_overflow' / 'write_behind' (a record written on overflow / at out[D]), 'stale_dict' (the dictionaries are not emptied behind the query)."""

    def __init__(self, n, E, cap, keys, measured, scratch=None, cus=256, defect=None):
        self.n, self.E, self.cap, self.keys, self.measured, self.cus, self.defect = n, E, cap, norm(keys), measured, cus, defect
        self.slots = gm.slots_for(cap)
        self.shift = shift_for(cap) - (1 if defect == "overlap" else 0)
        self.scratch = scratch or Scratch()
        self.dclaims = [0] * MAX_KEYS                                 # (this query's claims: the counters start at zero whatever the dictionaries hold)
        self.T = gm.Device(n, E, cap, measured, cus)                 # the tuple table, the cache geometry and their tags
        self.tags = self.T.tags
        self.overflow = False
        self.absent, self.total = gm._Acc(), gm._Acc()

    def _bucket(self, v, o, w):
        if self.defect == "trunc":
            d = v - o
            return abs(d) // w * (1 if d >= 0 else -1)
        return bucket(v, o, w)

    def _code(self, j, v):
        """the workgroup's insert-only LDS cache value -> code first (it only spares the lookup: the code is the dictionary's), then the dictionary"""
        e = (j, gm.cache_set(v))
        if self.dcache.get(e, (None,))[0] == v:
            self.tags.add(("dcache", "hit"))
            return self.dcache[e][1]
        c = self._lookup(j, v)
        if c is not None:
            self.tags.add(("dcache", "taken") if e in self.dcache else ("dcache", "claim"))
            self.dcache.setdefault(e, (v, c))
        return c

    def _lookup(self, j, v):
        d, slots = self.scratch.dicts[j], self.slots
        h = gm.home(v, slots)
        for p in range(slots):
            s = (h + p) & (slots - 1)
            if s not in d:
                d[s] = v; self.dclaims[j] += 1
            if d[s] == v:
                self.tags.add(("dict", j, "home" if p == 0 else ("wrap" if h + p >= slots else "walk")))
                if p:
                    self.tags.add((("dict", j, "len"), p))
                return s
            if (p & 63) == 63 and self.dclaims[j] > self.cap:
                break
        self.overflow = True; self.tags.add(("dict", j, "noroom"))
        return None

    def run(self, sel, kvals, mval):
        pos = np.arange(self.n)
        wg = gm.place(pos, self.n, self.E, self.cus)[0]
        T = self.T
        for g in range(gm.grid(self.n, self.E, self.cus)):
            cache, self.dcache = {}, {}
            for p in pos[wg == g]:
                if not sel[p]:
                    continue
                self.total.add(1, mval[p])
                kv = kvals[p]
                if any(v is None for v in kv):
                    self.absent.add(1, mval[p])
                    if self.defect != "absent_in_group":
                        continue
                    kv = tuple(o if v is None else v for v, (_, o, _) in zip(kv, self.keys))      # (bucket 0)
                word = 0
                for j, (v, (_, o, w)) in enumerate(zip(kv, self.keys)):
                    c = self._code(j, self._bucket(v, o, w))
                    if c is None:
                        word = None
                        break
                    word |= c << (j * self.shift)
                if word is None:
                    continue
                ways = cache.setdefault(gm.cache_set(word), {})
                if word in ways or len(ways) < gm.WAYS:
                    ways.setdefault(word, gm._Acc()).add(1, mval[p]); T.tags.add("hit")
                    continue
                T.tags.add("bypass")
                s = T._slot(word)
                if s is not None:
                    T.acc[s].add(1, mval[p])
            for ways in cache.values():
                for word, a in ways.items():
                    s = T._slot(word)
                    if s is not None:
                        T.acc[s].merge(a)
        return self.finish()

    def finish(self, room=None):
        T = self.T
        res = np.zeros((), GROUP_RES_DTYPE)
        res["absent"] = self.absent.record(self.measured); res["total"] = self.total.record(self.measured)
        out = np.full(80 * ((self.cap if room is None else room) + 1), FILL, np.uint8).view(MGROUP_DTYPE)
        over = T.claims > self.cap or T.overflow or self.overflow
        res["n_groups"] = max([T.claims] + self.dclaims) if over else T.claims
        mask = self.slots - 1
        recs = np.zeros(len(T.table), MGROUP_DTYPE)
        for i, (s, word) in enumerate(sorted(T.table.items())):
            for j in range(len(self.keys)):
                recs[i]["key"][j] = self.scratch.dicts[j].get((word >> (j * self.shift)) & mask, 0)
            recs[i]["agg"] = T.acc[s].record(self.measured)
        recs = recs[np.argsort(recs["key"][:, 0], kind="stable")] if self.defect == "sort_key0" else sort_records(recs)
        if over:
            res["flags"] = OVERFLOW
            if self.defect == "write_on_overflow" and len(recs):
                out[0] = recs[0]
        else:
            out[:len(recs)] = recs
            if self.defect == "write_behind":
                out[len(recs)]["key"][0] = 0
        if self.defect != "stale_dict":
            for d in self.scratch.dicts:
                d.clear()
        return out, res


# ---- helpers of the GPU tests ----
def raw_mgroup(x, base, clauses, keys, measure=None, cap=64, room=None):
    """bmx_where_group_multi (Engine) / bmx_comm_where_group_multi (Comm), host memory, into pattern-filled buffers -> (the whole buffer, result record)"""
    import bmx
    out = np.full(80 * ((cap if room is None else room) + 1), FILL, np.uint8).view(MGROUP_DTYPE)
    res = np.full(112, FILL, np.uint8).view(GROUP_RES_DTYPE)
    nk, karr = bmx._mgroup_keys(keys)
    args = (*bmx._where_args(base, clauses), bmx.AGG_NO_FIELD if measure is None else int(measure), nk, karr, bmx._ptr(out), int(cap), bmx._ptr(res))
    x._chk(x.L.bmx_where_group_multi(x.h, *args, bmx.MEM_HOST) if isinstance(x, bmx.Engine) else x.L.bmx_comm_where_group_multi(x.h, *args))
    return out, res[0]


def ask(x, m, base, clauses, keys, measure=None, cap=64, want=None):
    """one query checked against the brute-force answer -> (records, result record)"""
    out, res = raw_mgroup(x, base, clauses, keys, measure, cap)
    want = answer(m, base, clauses, keys, measure, cap) if want is None else want
    bad = check(out, res, *want, cap)
    assert bad is None, (clauses, keys, measure, cap, bad)
    return out[:0 if int(res["flags"]) else int(res["n_groups"])].copy(), res


# ---- the seeded suite (the CPU test asserts what it relies on; the GPU test runs it) ----
def seeded_queries():
    """-> [(clauses, keys, measure field or None)]: group_model's 60 programs over group_model.seeded_model, crossed with six key sets (one key; two raw keys;
    a raw key and a bucket; three keys with a bucket; four keys with a bucket; one field at two widths) and measure = none / base / probed"""
    F = gm._names()
    sets = [
        [F["base"]],
        [F["key"], F["one"]],
        [F["base"], (F["measure"], 0, 1 << 36)],
        [(F["key"], -BIG, 1 << 50), F["two"], F["base"]],
        [F["one"], F["two"], F["base"], (F["measure"], -7, 1 << 38)],
        [(F["key"], 0, 1), (F["key"], 0, 1 << 51)],
    ]
    out = []
    for k, (p, _, measure) in enumerate(gm.seeded_queries()):
        out.append((p, sets[k % 6], measure))
    return out


def buckets_in(keys):
    return sum(1 for _, o, w in norm(keys) if (o, w) != (0, 1))


# ---- the edge suite: columns laid out by position (both the CPU stand-in and the GPU run them) ----
def values_by_home(slots, start=1):
    """-> a list of `slots` values, the h-th with home slot h: a dictionary of any of them holds each at its home, so its code is h whoever comes first"""
    out, k = [None] * slots, start
    left = slots
    while left:
        h = gm.home(k, slots)
        if out[h] is None:
            out[h] = k; left -= 1
        k += 1
    return out


def pairs_with_home(slot, slots, count):
    """-> `count` pairs of codes (c0, c1) whose packed word c0 | c1 << log2 slots has its home in `slot` of a table of `slots`"""
    sh = slots.bit_length() - 1
    out = []
    for c1 in range(slots):
        for c0 in range(slots):
            if gm.home(c0 | (c1 << sh), slots) == slot:
                out.append((c0, c1))
                if len(out) == count:
                    return out
    raise AssertionError("not enough pairs")


def edge_layouts(wide):
    """-> [dict(name, n, cap, nkeys, keys (int64, n x nkeys, by position), present (bool, n x nkeys), sel (bool by position), tags (what Device must reach))].
    Key j of the layouts is a probed field of its own; the GPU test also puts key 0 into the base column where base is set."""
    E = 2 if wide else 4
    rnd = gm.THREADS * gm.U * E
    start = WIDE if wide else 1
    L = []

    def add(name, n, cap, cols, tags, sel=None, present=None, base=False):
        keys = np.stack([np.asarray(c, np.int64) for c in cols], axis=1)
        L.append(dict(name=name, n=n, cap=cap, nkeys=keys.shape[1], keys=keys, present=np.ones(keys.shape, bool) if present is None else present,
                      sel=np.ones(n, bool) if sel is None else sel, tags=set(tags), base=base))

    pos = np.arange(300)
    ks = gm.keys_with_home(17, 64, 3, start)
    add("dict0_same_home", 300, 8, [np.array(ks)[pos % 3], pos % 2], {("dict", 0, "home"), ("dict", 0, "walk"), (("dict", 0, "len"), 2), ("dict", 1, "home")}, base=True)
    ks = gm.keys_with_home(63, 64, 2, start)
    add("dict1_wrap", 300, 8, [pos % 3 + start, np.array(ks)[pos % 2]], {("dict", 1, "home"), ("dict", 1, "wrap"), (("dict", 1, "len"), 1)}, base=True)
    ks = gm.keys_with_set(9, 3, start)
    add("values_share_an_lds_entry", 300, 8, [np.array(ks)[pos % 3], np.array(ks)[(pos // 3) % 2]], {("dcache", "hit"), ("dcache", "claim"), ("dcache", "taken")}, base=True)
    ks = gm.keys_with_home(40, 64, 65, start)
    pos = np.arange(700)
    add("dict_fills_the_table", 700, 8, [np.full(700, start + 5), np.array(ks[:64])[pos % 64]], {("dict", 1, "wrap"), (("dict", 1, "len"), 63)})
    add("dict_no_room", 700, 8, [np.array(ks)[pos % 65], np.full(700, 7)], {("dict", 0, "noroom")})
    add("dict2_of_3_no_room", 700, 8, [np.full(700, start), np.full(700, 9), np.array(ks)[pos % 65]], {("dict", 2, "noroom"), ("dict", 0, "home")})
    vals = values_by_home(64, start)
    pos = np.arange(300)
    for k in (2, 3, 5):
        pr = pairs_with_home(21, 64, k)
        add("words_same_home_%d" % k, 300, 8, [np.array([vals[a] for a, _ in pr])[pos % k], np.array([vals[b] for _, b in pr])[pos % k]], {"home", "walk", ("len", k - 1)})
    pr = pairs_with_home(63, 64, 2)
    add("words_wrap", 300, 8, [np.array([vals[a] for a, _ in pr])[pos % 2], np.array([vals[b] for _, b in pr])[pos % 2]], {"home", "wrap", ("len", 1)})
    # more words than one cache set holds: pairs of codes whose packed words share a set of the LDS cache
    sh, same_set = 6, []
    for w in range(64 * 64):
        if gm.cache_set(w) == gm.cache_set(5 | (9 << sh)):
            same_set.append((w & 63, w >> sh))
    same_set = same_set[:6]
    assert len(same_set) == 6
    add("set_overflows", 300, 8, [np.array([vals[a] for a, _ in same_set])[pos % 6], np.array([vals[b] for _, b in same_set])[pos % 6]], {"hit", "bypass"})
    n = 64 * E * 3
    lane = gm.place(np.arange(n), n, E)[2]
    add("wave_on_one_tuple", n, 8, [np.full(n, start + 6), np.full(n, -3), np.full(n, start)], {"hit", "home"}, base=True)
    add("lanes_on_64_tuples_one_key0", n, 64, [np.full(n, start + 2), lane * 3 - 90], {"hit"}, base=True)
    add("lane_0_alone", n, 8, [start + (np.arange(n) % 2), np.arange(n) % 3], {"hit"}, sel=lane == 0)
    add("lane_63_alone", n, 8, [start + (np.arange(n) % 2), np.arange(n) % 3], {"hit"}, sel=lane == 63)
    for n in (1, E - 1, E, E + 1, 64 * E - 1, 64 * E, 64 * E + 1, rnd - 1, rnd, rnd + 1, 4 * rnd + 1):
        # (4 rounds + 1 row: two workgroups; the same tuples in both, so the flushes add into one slot and both look the values up)
        a = np.arange(n)
        present = np.stack([a % 11 != 3, a % 13 != 5], axis=1)
        add("size_%d" % n, n, 8, [start + (a % 3) * 1000003, (a % 2) * -77], {"hit", "home"} if n > 13 else set(), present=present)
    return L
