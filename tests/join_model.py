"""A numpy model of the lookup joins (include/bmx_join.h, csrc/join_kernels.h), shared by test_join_model.py (CPU) and the GPU tests (helper, not a test). The
table and the selection are watch_model.Model's (a state per field and node: absent, data, tombstone); mask(base, clauses) is bmx_scan_where's truth.

Two halves:

answer(...) : the brute-force answer. inner_map(): the inner selection -> the distinct keys that are present, each with the minimum of the attributes present on
    its nodes (NO_ATTR when none is), n_inner and n_keyed; list_map(): the same from pairs. answer(): every selected outer node goes to `unmatched` (no link
    data, or a link that is no key), `absent` (a key without attribute) or the record of its attribute; both overflow rules. check() is every comparison the
    GPU tests make against pattern-filled buffers.

Device : a sequential stand-in of k_join_build / k_join_insert / k_join_group_sweep / k_join_finish on group_model's home() (same hash, linear probing with
    wrap, INT64_MIN = empty, INT64_MAX = no attribute). The sweep's hash aggregation is group_model.Device's (the LDS cache and its bypass). It tags its paths:
    'present' the key was there, 'claim' claimed at its home slot, ('walk', n) claimed or found n steps on, 'wrap' a walk passed the last slot, 'giveup' a
    walk ended without a slot, 'lowered' the minimum went down, 'min_skipped' the load showed a value at or below the node's, 'skipped' a listed pair outside
    the domain, 'grouped' / 'absent' / 'unmatched' the destinations of an outer row, 'bypass' a row that went past the LDS cache. Built with defect=... it is
    wrong in one way each, which test_join_model.py shows that check() notices.

The seeded suite: semi_model's seeded "orders" and "users" with an attribute on the users and a measure on the orders, and seeded_pairs(), 60 program pairs."""
import numpy as np

import group_model as gm
import semi_model as sm
import where_agg_model as wam
from oracle import streams
from watch_model import ABSENT, DATA, TOMB, Model  # noqa: F401

AGG_DTYPE, GROUP_DTYPE = wam.AGG_DTYPE, gm.GROUP_DTYPE
JOIN_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("map_size", "<u8"), ("n_inner", "<u8"), ("n_keyed", "<u8"), ("flags", "<u4"), ("reserved", "<u4"),
                           ("absent", AGG_DTYPE), ("unmatched", AGG_DTYPE), ("total", AGG_DTYPE)])
MAP_OVERFLOW, GROUP_OVERFLOW, MAX_MAP = 1, 2, 1 << 20
VAL_MAX = (1 << 53) - 1
EMPTY, NO_ATTR = -(1 << 63), (1 << 63) - 1
INT64_MIN, INT64_MAX = EMPTY, NO_ATTR
FILL = gm.FILL
WIDE = 1 << 40

FB, FL, FI, FK, F1, F2, NOBODY, EVERY = sm.FB, sm.FL, sm.FI, sm.FK, sm.F1, sm.F2, sm.NOBODY, sm.EVERY
FA, FM = streams.fnv1a32("join.attr"), streams.fnv1a32("join.measure")
ALL_FIELDS = [FB, FL, FI, FK, F1, F2, FA, FM]
slots_for, home, keys_with_home, keys_with_set = gm.slots_for, gm.home, gm.keys_with_home, gm.keys_with_set
uid = sm.uid


# ---- the brute-force answer ----
def unite(keys, vals):
    """pairs (vals: NO_ATTR = none) -> (distinct keys ascending, the minimum of each key's vals)"""
    keys, vals = np.asarray(keys, np.int64), np.asarray(vals, np.int64)
    K = np.unique(keys)
    V = np.full(len(K), NO_ATTR, np.int64)
    np.minimum.at(V, np.searchsorted(K, keys), vals)
    return K, V


def inner_pairs(m, inner_base, inner_clauses, key, attr):
    """-> (keys, vals (NO_ATTR = none) of the selected inner nodes that hold a key, node order; n_inner)"""
    sel = m.mask(inner_base, inner_clauses)
    m._f(key); m._f(attr)
    have = sel & (m.st[key] == DATA)
    vals = np.where(m.st[attr] == DATA, m.val[attr], NO_ATTR)
    return m.val[key][have], vals[have], int(sel.sum())


def inner_map(m, inner_base, inner_clauses, key, attr):
    """-> (K, V, n_inner, n_keyed)"""
    k, v, n_inner = inner_pairs(m, inner_base, inner_clauses, key, attr)
    return unite(k, v) + (n_inner, len(k))


def list_map(keys, vals):
    k, v = np.asarray(keys, np.int64).ravel(), np.asarray(vals, np.int64).ravel()
    ok = (k >= -VAL_MAX) & (k <= VAL_MAX)
    v = np.where((v >= -VAL_MAX) & (v <= VAL_MAX), v, NO_ATTR)
    return unite(k[ok], v[ok]) + (int(ok.sum()), int(ok.sum()))


def destinations(m, base, clauses, link, K, V):
    """-> (sel, unmatched, absent, grouped masks over the model's nodes; the attribute of every node (valid where grouped))"""
    sel = m.mask(base, clauses)
    m._f(link)
    at = np.searchsorted(K, m.val[link]) if len(K) else np.zeros(m.N, np.int64)
    at = np.minimum(at, max(len(K) - 1, 0))
    inside = (m.st[link] == DATA) & (K[at] == m.val[link] if len(K) else np.zeros(m.N, bool))
    attr = V[at] if len(K) else np.zeros(m.N, np.int64)
    return sel, sel & ~inside, sel & inside & (attr == NO_ATTR), sel & inside & (attr != NO_ATTR), attr


def answer(m, base, clauses, link, measure, M, cap=65536, map_cap=65536):
    """M = (K, V, n_inner, n_keyed) -> (records sorted by key, result record). On an overflow n_groups / map_size are the TRUE numbers: the device reports some
    number above the cap and at most that."""
    K, V, n_inner, n_keyed = M
    res = np.zeros((), JOIN_RES_DTYPE)
    res["map_size"] = len(K); res["n_inner"] = n_inner; res["n_keyed"] = n_keyed
    if measure is not None:
        m._f(measure)
    have_m = (m.st[measure] == DATA) if measure is not None else None

    def rec(rows):
        return wam.record(int(rows.sum()), None if measure is None else m.val[measure][rows & have_m])

    if len(K) > map_cap:
        res["flags"] = MAP_OVERFLOW
        res["absent"] = res["unmatched"] = res["total"] = wam.record(0, None)
        return np.zeros(0, GROUP_DTYPE), res
    sel, un, ab, gr, attr = destinations(m, base, clauses, link, K, V)
    res["absent"] = rec(ab); res["unmatched"] = rec(un); res["total"] = rec(sel)
    keys = np.unique(attr[gr])
    res["n_groups"] = len(keys)
    if len(keys) > cap:
        res["flags"] = GROUP_OVERFLOW
        return np.zeros(0, GROUP_DTYPE), res
    out = np.zeros(len(keys), GROUP_DTYPE)
    for i, k in enumerate(keys):
        out[i]["key"] = k; out[i]["agg"] = rec(gr & (attr == k))
    return out, res


sum_of = gm.sum_of


def invariant(recs, res):
    """sum of the records + absent + unmatched == total, for n_match, n and the sum"""
    t, a, u = res["total"], res["absent"], res["unmatched"]
    return (int(recs["agg"]["n_match"].sum()) + int(a["n_match"]) + int(u["n_match"]) == int(t["n_match"])
            and int(recs["agg"]["n"].sum()) + int(a["n"]) + int(u["n"]) == int(t["n"])
            and (sum(sum_of(x["agg"]) for x in recs) + sum_of(a) + sum_of(u) - sum_of(t)) % (1 << 128) == 0)


def check(got_recs, got_res, want_recs, want_res, cap, map_cap, host=True):
    """every comparison the GPU tests make -> None or what differs. got_recs: the caller's whole buffer of cap + 1 records, pattern-filled before the call."""
    got_recs = np.asarray(got_recs, GROUP_DTYPE)
    for k in ("absent", "unmatched", "total"):
        if np.asarray(got_res[k]).tobytes() != np.asarray(want_res[k]).tobytes():
            return (k, got_res[k], want_res[k])
    for k in ("n_inner", "n_keyed"):
        if int(got_res[k]) != int(want_res[k]):
            return (k, int(got_res[k]), int(want_res[k]))
    if int(got_res["reserved"]) != 0:
        return ("reserved", int(got_res["reserved"]))
    wf = int(want_res["flags"])
    if wf & MAP_OVERFLOW:
        if int(got_res["flags"]) != MAP_OVERFLOW or int(got_res["n_groups"]) != 0 or not (map_cap < int(got_res["map_size"]) <= int(want_res["map_size"])):
            return ("map overflow", int(got_res["flags"]), int(got_res["n_groups"]), int(got_res["map_size"]), int(want_res["map_size"]))
        return None if (got_recs.view(np.uint8) == FILL).all() else ("out written on a map overflow",)
    if int(got_res["map_size"]) != int(want_res["map_size"]):
        return ("map_size", int(got_res["map_size"]), int(want_res["map_size"]))
    if wf & GROUP_OVERFLOW:
        if int(got_res["flags"]) != GROUP_OVERFLOW or not (cap < int(got_res["n_groups"]) <= int(want_res["n_groups"])):
            return ("group overflow", int(got_res["flags"]), int(got_res["n_groups"]), int(want_res["n_groups"]))
        return None if (got_recs.view(np.uint8) == FILL).all() else ("out written on a group overflow",)
    if int(got_res["flags"]) != 0 or int(got_res["n_groups"]) != len(want_recs):
        return ("n_groups / flags", int(got_res["flags"]), int(got_res["n_groups"]), len(want_recs))
    d = len(want_recs)
    if not (got_recs[d:].view(np.uint8) == FILL).all():
        return ("written at or beyond out[D]",)
    g = got_recs[:d]
    if host and not np.array_equal(g["key"], np.sort(g["key"])):
        return ("host records not sorted by key",)
    g = g[np.argsort(g["key"], kind="stable")]
    if g.tobytes() != np.asarray(want_recs, GROUP_DTYPE).tobytes():
        bad = [i for i in range(d) if g[i].tobytes() != want_recs[i].tobytes()]
        return ("record", bad[0], g[bad[0]], want_recs[bad[0]])
    if not invariant(g, got_res):
        return ("invariant",)
    return None


# ---- queries as dictionaries: kind 'join' (two programs) or 'map' (a list of pairs) ----
def Q(base, clauses, link, inner_base, inner_clauses, key, attr, measure=None, cap=64, map_cap=64):
    return dict(kind="join", base=base, clauses=clauses, link=link, inner_base=inner_base, inner_clauses=inner_clauses, key=key, attr=attr, measure=measure, cap=cap,
                map_cap=map_cap)


def QMAP(base, clauses, link, keys, vals, measure=None, cap=64):
    return dict(kind="map", base=base, clauses=clauses, link=link, keys=[int(k) for k in keys], vals=[int(v) for v in vals], measure=measure, cap=cap)


def map_of(m, q):
    return list_map(q["keys"], q["vals"]) if q["kind"] == "map" else inner_map(m, q["inner_base"], q["inner_clauses"], q["key"], q["attr"])


def map_cap_of(q):
    return len(q["keys"]) if q["kind"] == "map" else q["map_cap"]


def want_of(m, q):
    return answer(m, q["base"], q["clauses"], q["link"], q["measure"], map_of(m, q), q["cap"], map_cap_of(q))


def variants(m, q):
    """the query with room for everything, then with cap = D and D - 1, map_cap = K and K - 1, and both one too small"""
    big = dict(q, cap=1 << 12) if q["kind"] == "map" else dict(q, cap=1 << 12, map_cap=1 << 12)
    recs, res = want_of(m, big)
    D, K = max(len(recs), 1), max(int(res["map_size"]), 1)
    out = [q, dict(q, cap=D), dict(q, cap=max(D - 1, 1))]
    if q["kind"] == "join":
        out += [dict(q, map_cap=K), dict(q, map_cap=max(K - 1, 1)), dict(q, cap=max(D - 1, 1), map_cap=max(K - 1, 1))]
    return out


def as_list(m, q):
    """the list form of a program query: the pairs of its inner selection, duplicates included; None when there is none"""
    k, v, _ = inner_pairs(m, q["inner_base"], q["inner_clauses"], q["key"], q["attr"])
    return QMAP(q["base"], q["clauses"], q["link"], k, v, q["measure"], q["cap"]) if len(k) else None


# ---- helpers of the GPU tests: raw calls into pattern-filled buffers ----
def buffers(cap):
    return np.full(56 * (cap + 1), FILL, np.uint8).view(GROUP_DTYPE), np.full(184, FILL, np.uint8).view(JOIN_RES_DTYPE)


def raw_of(x, q):
    """x: an Engine or a Comm, host memory -> (the whole buffer of cap + 1 records, the result record)"""
    import bmx
    out, res = buffers(q["cap"])
    nof = bmx.AGG_NO_FIELD
    head = (*bmx._where_args(q["base"], q["clauses"]), int(q["link"]), nof if q["measure"] is None else int(q["measure"]))
    tail = (bmx._ptr(out), int(q["cap"]), bmx._ptr(res))
    one = isinstance(x, bmx.Engine)
    if q["kind"] == "map":
        k, v = np.array(q["keys"], np.int64), np.array(q["vals"], np.int64)
        args = (*head, bmx._ptr(k), bmx._ptr(v), len(k), *tail)
        x._chk(x.L.bmx_where_map_group(x.h, *args, bmx.MEM_HOST) if one else x.L.bmx_comm_where_map_group(x.h, *args))
    else:
        args = (*head, *bmx._where_args(q["inner_base"], q["inner_clauses"]), int(q["key"]), int(q["attr"]), int(q["map_cap"]), *tail)
        x._chk(x.L.bmx_where_join_group(x.h, *args, bmx.MEM_HOST) if one else x.L.bmx_comm_where_join_group(x.h, *args))
    return out, res[0]


def ask(x, m, q, host=True):
    """one query checked against the brute-force answer -> (want records, want result record)"""
    out, res = raw_of(x, q)
    want = want_of(m, q)
    bad = check(out, res, *want, q["cap"], map_cap_of(q), host)
    assert bad is None, (bad, q, want[1])
    return want


# ---- the sequential stand-in ----
DEFECTS = ("max_not_min", "drop_no_attr", "unmatched_as_absent", "tomb_key", "write_on_map_overflow", "write_on_group_overflow", "write_behind_cap", "lost_wrap")


class Device:
    """build / insert_list, then sweep + finish — as the kernels do it, one row after the other in position order"""

    def __init__(self, map_cap, defect=None):
        assert defect is None or defect in DEFECTS
        self.cap, self.slots, self.defect = map_cap, slots_for(map_cap), defect
        self.keys, self.vals = [EMPTY] * self.slots, [NO_ATTR] * self.slots
        self.claims = self.n_inner = self.n_keyed = self.overflow = 0
        self.tags = set()

    def _walk(self, key, claim):
        """-> the slot of key (claimed if `claim` and not there), or None"""
        h = home(key, self.slots)
        for p in range(self.slots):
            s = h + p
            if s >= self.slots:
                if self.defect == "lost_wrap":
                    break                                             # the walk falls off the table's end
                s -= self.slots
                self.tags.add("wrap")
            k = self.keys[s]
            if k == EMPTY and claim:
                self.keys[s] = k = key; self.claims += 1
                self.tags.add("claim" if p == 0 else ("walk", p))
            elif k == key and claim:
                self.tags.add("present")
                if p:
                    self.tags.add(("walk", p))
            if k == key:
                return s
            if k == EMPTY:
                return None
            if claim and p & 63 == 63 and self.claims > self.cap:
                break
        return None

    def insert(self, key, val):
        key, val = int(key), int(val)
        if val == NO_ATTR and self.defect == "drop_no_attr":
            return
        s = self._walk(key, True)
        if s is None:
            self.overflow = 1; self.tags.add("giveup"); return
        if val == NO_ATTR:
            return
        if self.defect == "max_not_min":
            self.vals[s] = val if self.vals[s] == NO_ATTR else max(self.vals[s], val); return
        if self.vals[s] > val:
            self.vals[s] = val; self.tags.add("lowered")
        else:
            self.tags.add("min_skipped")

    def build(self, m, pn, inner_base, inner_clauses, key, attr):
        """pn: the inner base index's positions as node numbers"""
        sel = m.mask(inner_base, inner_clauses)
        m._f(key); m._f(attr)
        for i in pn:
            if not sel[i]:
                continue
            self.n_inner += 1
            if m.st[key][i] == DATA or (self.defect == "tomb_key" and m.st[key][i] == TOMB):
                self.n_keyed += 1
                self.insert(m.val[key][i], m.val[attr][i] if m.st[attr][i] == DATA else NO_ATTR)   # (the defect inserts the value the row held before its tombstone)

    def insert_list(self, keys, vals):
        for k, v in zip(np.asarray(keys, np.int64).tolist(), np.asarray(vals, np.int64).tolist()):
            if k < -VAL_MAX or k > VAL_MAX:
                self.tags.add("skipped"); continue
            self.n_inner += 1; self.n_keyed += 1
            self.insert(k, v if -VAL_MAX <= v <= VAL_MAX else NO_ATTR)

    def fits(self):
        return not self.overflow and self.claims <= self.cap

    def sweep(self, m, pn, base, clauses, link, measure, cap):
        """the group sweep and the finish -> (the caller's buffer of cap + 1 records, the result record)"""
        res = np.zeros((), JOIN_RES_DTYPE)
        res["map_size"] = self.claims; res["n_inner"] = self.n_inner; res["n_keyed"] = self.n_keyed
        mfits = self.fits()
        g = gm.Device(len(pn), 4, cap, measure is not None)
        un = gm._Acc()
        if mfits or self.defect == "write_on_map_overflow":
            sel = m.mask(base, clauses)[pn]
            m._f(link)
            if measure is not None:
                m._f(measure)
            gkey, mval, gsel = [], [], []
            for p, i in enumerate(pn):
                mv = int(m.val[measure][i]) if measure is not None and m.st[measure][i] == DATA else None
                mval.append(mv)
                s = self._walk(int(m.val[link][i]), False) if sel[p] and m.st[link][i] == DATA else None
                if sel[p] and s is None and self.defect != "unmatched_as_absent":
                    un.add(1, mv); self.tags.add("unmatched")
                    gsel.append(False); gkey.append(None); continue
                if sel[p]:
                    self.tags.add("absent" if s is None or self.vals[s] == NO_ATTR else "grouped")
                gsel.append(bool(sel[p])); gkey.append(None if s is None or self.vals[s] == NO_ATTR else self.vals[s])
            out, gres = g.run(np.array(gsel, bool), gkey, mval)
            self.tags |= {t for t in g.tags if t == "bypass"}
        else:
            out, gres = g.finish()
        total = gm._Acc(); total.merge(g.total); total.merge(un)
        res["absent"] = gres["absent"]; res["unmatched"] = un.record(measure is not None); res["total"] = total.record(measure is not None)
        gfits = not (int(gres["flags"]) & gm.OVERFLOW)
        res["n_groups"] = int(gres["n_groups"]) if mfits else 0
        res["flags"] = (0 if mfits else MAP_OVERFLOW) | (0 if gfits else GROUP_OVERFLOW)
        if not mfits and self.defect != "write_on_map_overflow":
            res["absent"] = res["unmatched"] = res["total"] = wam.record(0, None)
        if not gfits and self.defect == "write_on_group_overflow":
            out[0]["key"] = 0
        if mfits and gfits and self.defect == "write_behind_cap":
            out[int(gres["n_groups"])]["key"] = 0
        self.keys, self.vals = [EMPTY] * self.slots, [NO_ATTR] * self.slots
        self.claims = self.n_inner = self.n_keyed = self.overflow = 0
        return out, res


def device_of(m, q, defect=None, pn=None, inner_pn=None):
    """the stand-in's answer into pattern-filled buffers -> (out, res, the device: its tags)"""
    pn = np.arange(m.N) if pn is None else pn
    d = Device(map_cap_of(q), defect)
    if q["kind"] == "map":
        d.insert_list(q["keys"], q["vals"])
    else:
        d.build(m, np.arange(m.N) if inner_pn is None else inner_pn, q["inner_base"], q["inner_clauses"], q["key"], q["attr"])
    out, res = d.sweep(m, pn, q["base"], q["clauses"], q["link"], q["measure"], q["cap"])
    return out, res, d


# ---- the seeded suite ----
def seeded_model():
    """semi_model's orders and users, an attribute (200 values) on 70 % of the users and a measure on 90 % of the orders -> (model, tombstones)"""
    m, tombs = sm.seeded_model()
    rng = np.random.default_rng(sm.SEED + 7)
    users, everyone = np.arange(sm.N_USERS), np.arange(m.N)
    ua = users[rng.random(sm.N_USERS) < 0.7]
    m.set(FA, ua, rng.integers(0, 200, len(ua)) * 37 - 3000)
    om = everyone[rng.random(m.N) < 0.9]
    m.set(FM, om, rng.integers(-10**6, 10**6, len(om)))
    tombs = dict(tombs)
    tombs[FA] = rng.choice(np.nonzero(m.st[FA] == DATA)[0], 150, replace=False)
    tombs[FM] = rng.choice(np.nonzero(m.st[FM] == DATA)[0], 300, replace=False)
    return m, tombs


def seeded_pairs(count=60):
    """-> [query]; the outer base is FB, the inner base FI"""
    rng = np.random.default_rng(sm.SEED + 8)
    out = []
    for k, (outer, link, inner, key, _) in enumerate(sm.seeded_pairs(count)):
        if link == FL:
            lo = int(rng.integers(0, 120))
            inner = [[(FI, lo, lo + int(rng.integers(40, 80)))]] + inner[1:]
        attr = FK if k % 7 == 3 else (FI if k % 7 == 5 else FA)
        measure = (FM, None, FB)[k % 3]
        out.append(Q(FB, outer, link, FI, inner, key, attr, measure, cap=1024, map_cap=1024))
    return out


# ---- the edge layouts: small tables on which every rule of the header can go wrong; run by the stand-in (CPU) and by the library (GPU) ----
def truth_table(outer_wide=False, inner_wide=False):
    """{outer selected or not} x {link in M with attribute, in M without, not in M, tombstone, absent} x {measure data, tombstone, absent}, several nodes each; the
    first 16 nodes are the inner side: keys 100, 101 with attributes (four nodes each, all different: the minimum counts), 102 whose nodes have no attribute
    row, 103 whose nodes' attribute rows are tombstones"""
    n = 120
    ow, iw = (WIDE if outer_wide else 0), (WIDE if inner_wide else 0)
    m = Model(wam.node_ids(n, 71000 + 2 * outer_wide + inner_wide))
    i = np.arange(n)
    m.set(FB, i, ow + i % 2)
    lk, mk, sub = (i // 2) % 5, (i // 10) % 3, (i // 30) % 2
    m.set(FL, i[lk == 0], 100 + sub[lk == 0]); m.set(FL, i[lk == 1], 102 + sub[lk == 1]); m.set(FL, i[lk == 2], 500 + i[lk == 2]); m.set(FL, i[lk == 3], 100)
    m.set(FM, i[mk != 2], i[mk != 2] * 3 - 50)
    m.set(F1, i, i % 5)
    m.set(FI, i[:16], iw + 1 + i[:16] % 3); m.set(FK, i[:16], 100 + i[:16] % 4)
    a = i[:16][i[:16] % 4 != 2]
    m.set(FA, a, 1000 + 50 * (a % 4) - a // 4)                          # key 100: 1000, 999, 998, 997; key 101: 1050 .. 1047
    m.set(FI, i[16:24], iw + 9); m.set(FK, i[16:20], 104); m.set(FA, i[16:24], 7)   # inner nodes the programs below do not select; 20..23 have no key at all
    m.set(FI, i[24:26], iw + 2); m.set(FK, i[24:26], 105); m.set(FA, i[24:26], 8); m.set(FL, i[lk == 2][:4], 105)   # a selected inner node whose key row is a tombstone: 105 is no key
    tombs = {FL: i[lk == 3], FM: i[mk == 1], FA: i[:16][i[:16] % 4 == 3], FK: i[24:26]}
    sel = [[(FB, ow + 1, ow + 1)]]
    inner = [[(FI, iw + 1, iw + 3)]]
    qs = [Q(FB, sel, FL, FI, inner, FK, FA, FM)]                                                    # link, key, attribute and measure: unnamed fields
    qs += [Q(FB, sel, FL, FI, inner, FK, FA, None), Q(FB, sel, FL, FI, inner, FK, FA, FB)]           # no measure; the measure from the column
    qs += [Q(FB, [[(FB, ow + 1, ow + 1), (FM, -50, 400, True)], [(FL, 100, 103)]], FL, FI, [[(FI, iw + 1, iw + 3), (FK, 100, 103)], [(FA, 0, 5)]], FK, FA, FM)]   # fields the programs probe
    qs += [Q(FB, sel, FL, FI, inner, FK, FK, FM)]                                                    # attr_field == key_field
    qs += [Q(FB, EVERY, FL, FI, [[(FI, iw + 9, iw + 9)]], FK, FA, FM)]                               # key 104 alone; inner nodes without a key count in n_inner
    qs += [Q(FB, sel, FL, FI, [[(FI, iw + 50, iw + 60)]], FK, FA, FM)]                               # an empty inner selection
    qs += [Q(FB, sel, FL, FI, inner, NOBODY, FA, FM)]                                                # every key absent
    qs += [Q(FB, sel, FL, FI, inner, FK, NOBODY, FM)]                                                # every attribute absent
    qs += [Q(FB, sel, NOBODY, FI, inner, FK, FA, FM)]                                                # every link absent
    qs += [Q(FB, [[(FB, ow + 7, ow + 8)]], FL, FI, inner, FK, FA, FM)]                               # nothing selected
    return m, tombs, qs


def base_links():
    """link = the outer base field, key and attribute = the inner base field, and both programs over ONE base field"""
    n = 300
    m = Model(wam.node_ids(n, 72000))
    i = np.arange(n)
    m.set(FB, i, i % 50); m.set(FI, i[:120], (i[:120] * 7) % 90); m.set(F1, i, i % 6); m.set(FK, i[::3], i[::3] % 11); m.set(FA, i[::2], i[::2] % 13 - 6); m.set(FM, i, 1000 - i)
    tombs = {FB: i[5::40], FI: i[3:120:25]}
    qs = [Q(FB, EVERY, FB, FI, [[(FI, 10, 60)]], FI, FI, FB)]                                        # everything from the columns
    qs += [Q(FB, EVERY, FB, FI, [[(FI, 10, 60)]], FI, FA, FM)]                                       # key from the column, attribute probed
    qs += [Q(FB, EVERY, FB, FI, [[(FI, 10, 60)]], FK, FI, FM)]                                       # key probed, attribute from the column
    qs += [Q(FB, [[(F1, 0, 2)]], FB, FB, [[(FB, 0, 9)], [(F1, 5, 5)]], FB, FA, FM)]                  # one base field on both sides
    qs += [Q(FB, [[(FB, 0, 30)]], FB, FB, [[(FB, 20, 49)]], FK, FB, None)]                           # the same index, key probed, attribute the column
    qs += [Q(FB, [[(FB, 0, 30)]], FK, FI, [[(FI, 0, 40)]], FI, FA, FB)]                              # link probed
    return m, tombs, qs


def key_values():
    vals = np.array([0, 1, -1, VAL_MAX, -VAL_MAX, 1 << 31, -(1 << 31), (1 << 32) + 5, 7], np.int64)
    n = 6 * len(vals)
    m = Model(wam.node_ids(n, 73000))
    i = np.arange(n)
    m.set(FB, i, i); m.set(FL, i, vals[i % len(vals)]); m.set(FM, i, vals[(i * 5) % len(vals)])
    m.set(FI, i[:len(vals)], i[:len(vals)]); m.set(FK, i[:len(vals)], vals); m.set(FA, i[:len(vals)], vals[::-1])
    qs = []
    for lo, hi in ((0, 8), (0, 4), (3, 4), (0, 0), (5, 8)):
        qs += [Q(FB, EVERY, FL, FI, [[(FI, lo, hi)]], FK, FA, FM), Q(FB, EVERY, FL, FI, [[(FI, lo, hi)]], FK, FK, None)]
    qs += [QMAP(FB, EVERY, FL, [VAL_MAX, -VAL_MAX, 0, 1], [-VAL_MAX, VAL_MAX, 0, -1], FM)]
    qs += [QMAP(FB, EVERY, FL, [7, 7, 7, 1, 7, 1, 0, 0], [5, 3, 9, INT64_MAX, 3, 2, INT64_MAX, VAL_MAX + 1], FM)]   # duplicates: the minimum of the in-domain vals; key 0: none
    qs += [QMAP(FB, EVERY, FL, [VAL_MAX + 1, -VAL_MAX - 1, INT64_MIN, INT64_MAX, -1, 1], [1, 2, 3, 4, INT64_MIN, -VAL_MAX - 1], FM)]   # keys outside: skipped; vals outside: no attribute
    qs += [QMAP(FB, EVERY, FL, [INT64_MIN], [INT64_MAX], FM)]                                        # an empty map from a list
    qs += [QMAP(FB, EVERY, FL, [1 << 31], [-5], None)]                                               # npairs = 1
    qs += [QMAP(FB, [[(FB, 10, 30)]], FB, [11, 12, 29, 31, -4], [3, 3, INT64_MAX, 3, 3], FB)]        # the link is the base column
    return m, {}, qs


def table_edges():
    """map_cap <= 32, 64 slots: 32 keys that share one home; a cluster that wraps from slot 63 to 0; links to absent keys that walk the whole cluster to its
    empty word; 70 keys into 64 slots (the table fills up: walks give up)"""
    same = keys_with_home(5, 64, 33)                                  # 32 in the map, one more with the same home that is not
    wrap = keys_with_home(62, 64, 7, start=10**6)                     # 6 in the map: slots 62, 63, 0, 1, 2, 3
    many = [int(uid(j)) for j in range(70)]
    n = 200
    m = Model(wam.node_ids(n, 74000))
    i = np.arange(n)
    m.set(FB, i, i); m.set(FI, i, i); m.set(FM, i, i * i)
    kv = np.array(same[:32] + wrap[:6] + many + same[:32] + wrap[:6] + [0] * (n - 146), np.int64)   # nodes 108..145 hold the cluster keys a second time
    m.set(FK, i[:146], kv[:146])
    m.set(FA, i[:146], np.where(i[:146] < 108, 1000 + i[:146] % 9, 900 - i[:146] % 5))              # ... with lower attributes (the minimum is lowered)
    lv = np.array(same + wrap + many[:40] + [12345] * (n - 80), np.int64)   # links: every key of the two clusters, the two absent ones, 40 of the many
    m.set(FL, i, lv)
    qs = [Q(FB, EVERY, FL, FI, [[(FI, 0, 31)]], FK, FA, FM, map_cap=32)]                             # one home
    qs += [Q(FB, EVERY, FL, FI, [[(FI, 32, 37)]], FK, FA, FM, map_cap=6)]                            # the wrapping cluster
    qs += [Q(FB, EVERY, FL, FI, [[(FI, 0, 37)], [(FI, 108, 145)]], FK, FA, FM, map_cap=38)]          # both (128 slots), every key twice
    qs += [Q(FB, EVERY, FL, FI, [[(FI, 0, 31)], [(FI, 108, 139)]], FK, FA, FM, map_cap=32)]          # one home, every key twice: present + lowered
    qs += [Q(FB, EVERY, FL, FI, [[(FI, 38, 107)]], FK, FA, FM, map_cap=32)]                          # 70 keys into 64 slots
    qs += [Q(FB, EVERY, FL, FI, [[(FI, 38, 107)]], FK, FA, FM, map_cap=70)]
    qs += [QMAP(FB, EVERY, FL, same[:32] + same[:32], list(range(64, 0, -1)), FM)]
    return m, {}, qs


def cache_bypass():
    """six attributes in one LDS set (four ways): the fifth and sixth bypass the cache; and 64 keys that all map to one attribute"""
    attrs = keys_with_set(9, 6, start=1000)
    n = 256
    m = Model(wam.node_ids(n, 75000))
    i = np.arange(n)
    m.set(FB, i, i % 3); m.set(FM, i, i - 100)
    m.set(FI, i[:70], i[:70]); m.set(FK, i[:70], 5000 + i[:70]); m.set(FA, i[:6], attrs); m.set(FA, i[6:70], 4242)
    m.set(FL, i, np.where(i % 4 == 0, 5000 + (i // 4) % 6, 5006 + i % 64))
    qs = [Q(FB, EVERY, FL, FI, EVERY, FK, FA, FM, map_cap=128), Q(FB, [[(FB, 1, 2)]], FL, FI, [[(FI, 0, 5)]], FK, FA, None)]
    return m, {}, qs


def edge_layouts():
    yield ("truth table",) + truth_table()
    yield ("truth table, int64 outer column",) + truth_table(outer_wide=True)
    yield ("truth table, int64 inner column",) + truth_table(inner_wide=True)
    yield ("truth table, int64 on both sides",) + truth_table(True, True)
    yield ("base links",) + base_links()
    yield ("key values",) + key_values()
    yield ("table edges",) + table_edges()
    yield ("cache bypass",) + cache_bypass()


def apply_tombs(m, tombs):
    for f, idx in tombs.items():
        m.tomb(f, idx)
