"""A numpy model of the join projection (include/bmx_join_rows.h, csrc/join_rows_kernels.h), shared by test_join_rows_model.py (CPU) and the GPU tests (helper,
not a test). The table is rows_model.Table's (a state per field and node: absent, data, tombstone, with a clock per cell); mask(base, clauses) is
bmx_scan_where's truth.

answer(...) : the brute force. inner_map(): the inner selection -> the distinct keys that are present, each with the SMALLEST UNSIGNED id among its nodes,
    n_inner and n_keyed; list_map(): the same from (key, node id) pairs. answer(): the outer selection in index order, left or inner, behind the cursor, cut
    at cap; every cell of both sides; the whole result record. check() is every comparison the GPU tests make.

raw(x, q) : one call of the library (an Engine or a Comm, host memory) into buffers that held 0x5A bytes; checks that nothing was written behind n_out in any
    of the six columns nor behind row cap.

MapDevice : a sequential stand-in of the map (join_insert / join_find with the id carried as id ^ 2^63) on group_model's home(): same hash, linear probing with
    wrap. Built with signed=True it compares the ids as signed numbers, which check() notices."""
import numpy as np

import group_model as gm
import rows_model as rm
from oracle import streams
from rows_model import ABSENT, DATA, TOMB, Table  # noqa: F401

JROWS_RES_DTYPE = np.dtype([("n_match", "<u8"), ("n_out", "<u8"), ("next_pos", "<u8"), ("layout", "<u8"), ("n_joined", "<u8"), ("map_size", "<u8"), ("n_inner", "<u8"),
                            ("n_keyed", "<u8"), ("flags", "<u4"), ("next_shard", "<u4")])
MAP_OVERFLOW, MAX_MAP = 1, 1 << 20
TS, INNER = 1, 2
NO_NODE = (1 << 64) - 1
VAL_MAX = (1 << 53) - 1
VAL_DELETED, NO_CLOCK, FILL = rm.VAL_DELETED, rm.NO_CLOCK, rm.FILL
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
WIDE = 1 << 40
slots_for, home, keys_with_home = gm.slots_for, gm.home, gm.keys_with_home

FB, FL, FI, FK, F1, F2, FX, FY, NOBODY = (streams.fnv1a32("jrows." + s) for s in ("base", "link", "inner", "key", "one", "two", "x", "y", "nobody"))
ALL_FIELDS = [FB, FL, FI, FK, F1, F2, FX, FY]
EVERY = [[(NOBODY, 0, 0, True)]]


# ---- the brute-force answer ----
def unite(keys, ids):
    """pairs -> (distinct keys ascending, the smallest unsigned id of each)"""
    keys, ids = np.asarray(keys, np.int64), np.asarray(ids, np.uint64)
    K = np.unique(keys)
    I = np.full(len(K), NO_NODE, np.uint64)
    np.minimum.at(I, np.searchsorted(K, keys), ids)
    return K, I


def inner_pairs(m, inner_base, inner_clauses, key):
    """-> (keys, ids of the selected inner nodes that hold a key, node order; n_inner)"""
    sel = m.mask(inner_base, inner_clauses)
    m._f(key)
    have = sel & (m.st[key] == DATA)
    return m.val[key][have], m.ids[have], int(sel.sum())


def inner_map(m, inner_base, inner_clauses, key):
    """-> (K, I, n_inner, n_keyed)"""
    k, i, n_inner = inner_pairs(m, inner_base, inner_clauses, key)
    return unite(k, i) + (n_inner, len(k))


def list_map(keys, ids):
    k, i = np.asarray(keys, np.int64).ravel(), np.asarray(ids, np.uint64).ravel()
    ok = (k >= -VAL_MAX) & (k <= VAL_MAX) & (i != np.uint64(NO_NODE))
    return unite(k[ok], i[ok]) + (int(ok.sum()), int(ok.sum()))


def inner_of(m, link, K, I):
    """-> the inner id of every node of the model (NO_NODE: none)"""
    m._f(link)
    if not len(K):
        return np.full(m.N, NO_NODE, np.uint64)
    at = np.minimum(np.searchsorted(K, m.val[link]), len(K) - 1)
    inside = (m.st[link] == DATA) & (K[at] == m.val[link])
    return np.where(inside, I[at], np.uint64(NO_NODE)).astype(np.uint64)


def cells(m, fields, nodes, have):
    """the three-state cells of `fields` on the model's nodes `nodes` (have = False: no node, every cell absent) -> (vals, ts)"""
    vals = np.full((len(fields), len(nodes)), VAL_DELETED, np.int64)
    ts = np.full((len(fields), len(nodes)), NO_CLOCK, np.int64)
    for k, f in enumerate(fields):
        m._f(f)
        st = np.where(have, m.st[f][nodes], ABSENT)
        vals[k] = np.where(st == DATA, m.val[f][nodes], VAL_DELETED)
        ts[k] = np.where(st == ABSENT, NO_CLOCK, m.clk[f][nodes])
    return vals, ts


def answer(m, order_ids, q, M=None):
    """-> dict(ids, vals, ts, in_ids, in_vals, in_ts, res). order_ids: the outer base field's index (Engine.index_ids). On an overflow res['map_size'] is the
    TRUE number: the device reports some number above map_cap and at most that. res['layout'] is left 0."""
    K, I, n_inner, n_keyed = map_of(m, q) if M is None else M
    order_ids = np.asarray(order_ids, np.uint64)
    res = np.zeros((), JROWS_RES_DTYPE)
    res["map_size"] = len(K); res["n_inner"] = n_inner; res["n_keyed"] = n_keyed
    nf, nif = len(q["fields"]), len(q["in_fields"])
    if len(K) > map_cap_of(q):
        res["flags"] = MAP_OVERFLOW; res["next_pos"] = len(order_ids)
        z = np.zeros((0,), np.uint64)
        return dict(ids=z, vals=np.zeros((nf, 0), np.int64), ts=np.zeros((nf, 0), np.int64), in_ids=z, in_vals=np.zeros((nif, 0), np.int64), in_ts=np.zeros((nif, 0), np.int64), res=res)
    pos_nodes = m.index_of(order_ids) if len(order_ids) else np.zeros(0, np.int64)
    iid = inner_of(m, q["link"], K, I)
    sel = m.mask(q["base"], q["clauses"])[pos_nodes]
    if q["inner"]:
        sel &= iid[pos_nodes] != np.uint64(NO_NODE)
    sel[:q["start"]] = False
    hit = np.nonzero(sel)[0]
    cap = q["cap"]
    nodes = pos_nodes[hit[:cap]]
    res["n_match"] = len(hit); res["n_out"] = len(nodes); res["next_pos"] = int(hit[cap]) if len(hit) > cap else len(order_ids)
    vals, ts = cells(m, q["fields"], nodes, np.ones(len(nodes), bool))
    in_ids = iid[nodes]
    res["n_joined"] = int((in_ids != np.uint64(NO_NODE)).sum())
    # an inner id of a list need not be a node of the table: every cell of it is absent
    k = np.minimum(np.searchsorted(m.sorted_ids, in_ids), m.N - 1)
    known = m.sorted_ids[k] == in_ids
    in_vals, in_ts = cells(m, q["in_fields"], m.order[k], known)
    return dict(ids=m.ids[nodes], vals=vals, ts=ts, in_ids=in_ids, in_vals=in_vals, in_ts=in_ts, res=res)


def check(got, want, q):
    """got: raw()'s dictionary; want: answer()'s -> None or what differs first. Every word of the record is compared (layout: nonzero, next_shard: the
    caller's business)."""
    g, w = got["res"], want["res"]
    for k in ("n_inner", "n_keyed", "flags", "n_match", "n_out", "next_pos", "n_joined"):
        if int(g[k]) != int(w[k]):
            return (k, int(g[k]), int(w[k]))
    if int(w["flags"]) & MAP_OVERFLOW:
        if not (map_cap_of(q) < int(g["map_size"]) <= int(w["map_size"])):
            return ("map_size on overflow", int(g["map_size"]), int(w["map_size"]))
    elif int(g["map_size"]) != int(w["map_size"]):
        return ("map_size", int(g["map_size"]), int(w["map_size"]))
    if int(g["layout"]) == 0:
        return ("layout",)
    for k in ("ids", "in_ids", "vals", "in_vals"):
        if got[k].shape != want[k].shape or not np.array_equal(got[k], want[k]):
            return (k, got[k].shape, want[k].shape, np.argwhere(got[k] != want[k])[:4] if got[k].shape == want[k].shape else None)
    if q["with_ts"]:
        for k in ("ts", "in_ts"):
            if got[k].shape != want[k].shape or not np.array_equal(got[k], want[k]):
                return (k, got[k].shape, want[k].shape)
    if q["inner"] and int(g["n_joined"]) != int(g["n_out"]):
        return ("an inner join delivers joined rows only",)
    return None


# ---- queries as dictionaries: kind 'join' (two programs) or 'map' (a list of pairs) ----
def Q(base, clauses, link, fields, inner_base, inner_clauses, key, in_fields, with_ts=True, inner=False, start=0, cap=1 << 12, map_cap=1 << 12):
    return dict(kind="join", base=base, clauses=clauses, link=link, fields=list(fields), inner_base=inner_base, inner_clauses=inner_clauses, key=key,
                in_fields=list(in_fields), with_ts=with_ts, inner=inner, start=start, cap=cap, map_cap=map_cap)


def QMAP(base, clauses, link, fields, keys, ids, in_fields, with_ts=True, inner=False, start=0, cap=1 << 12):
    return dict(kind="map", base=base, clauses=clauses, link=link, fields=list(fields), keys=[int(k) for k in keys], ids=[int(i) for i in ids],
                in_fields=list(in_fields), with_ts=with_ts, inner=inner, start=start, cap=cap)


def map_of(m, q):
    return list_map(q["keys"], np.array(q["ids"], np.uint64)) if q["kind"] == "map" else inner_map(m, q["inner_base"], q["inner_clauses"], q["key"])


def map_cap_of(q):
    return len(q["keys"]) if q["kind"] == "map" else q["map_cap"]


def as_list(m, q):
    """the list form of a program query: the pairs of its inner selection, duplicates included, and two pairs that are skipped; None when there is none"""
    k, i, _ = inner_pairs(m, q["inner_base"], q["inner_clauses"], q["key"])
    if not len(k):
        return None
    keys = k.tolist() + [VAL_MAX + 1, int(k[0])]
    ids = i.tolist() + [int(i[0]), NO_NODE]
    return QMAP(q["base"], q["clauses"], q["link"], q["fields"], keys, ids, q["in_fields"], q["with_ts"], q["inner"], q["start"], q["cap"])


# ---- one call of the library into pattern-filled buffers ----
PAT_U, PAT_I = np.full(8, FILL, np.uint8).view(np.uint64)[0], np.full(8, FILL, np.uint8).view(np.int64)[0]


def call_args(q):
    """-> (head, mid) of the C call: everything in front of start_shard / start_pos (keeps its arrays alive in the tuple)"""
    import bmx
    nf, farr, _ = bmx._rows_fields(q["fields"], False)
    nif, ifarr, _ = bmx._rows_fields(q["in_fields"], False)
    flags = (TS if q["with_ts"] else 0) | (INNER if q["inner"] else 0)
    head = (*bmx._where_args(q["base"], q["clauses"]), int(q["link"]), nf, farr)
    if q["kind"] == "map":
        k, i = np.array(q["keys"], np.int64), np.array(q["ids"], np.uint64)
        return head, (bmx._ptr(k), bmx._ptr(i), len(k), nif, ifarr, flags), (k, i)
    return head, (*bmx._where_args(q["inner_base"], q["inner_clauses"]), int(q["key"]), nif, ifarr, int(q["map_cap"]), flags), None


def raw(x, q, start_shard=0):
    """-> dict(ids, vals, ts, in_ids, in_vals, in_ts, res); asserts that the library wrote nothing behind n_out in any column, nothing behind row cap, and no
    clock without BMX_ROWS_TS"""
    import ctypes as C
    import bmx
    cap, nf, nif = int(q["cap"]), len(q["fields"]), len(q["in_fields"])
    room = max(cap, 1)
    ids, in_ids = np.full(room + 1, PAT_U, np.uint64), np.full(room + 1, PAT_U, np.uint64)
    vals, ts = np.full(max(nf, 1) * room + 1, PAT_I, np.int64), np.full(max(nf, 1) * room + 1, PAT_I, np.int64)
    in_vals, in_ts = np.full(max(nif, 1) * room + 1, PAT_I, np.int64), np.full(max(nif, 1) * room + 1, PAT_I, np.int64)
    res = np.full(72, FILL, np.uint8)
    head, mid, keep = call_args(q)
    tail = (int(cap), bmx._ptr(ids), bmx._ptr(vals), bmx._ptr(ts), bmx._ptr(in_ids), bmx._ptr(in_vals), bmx._ptr(in_ts), C.c_void_p(res.ctypes.data))
    one = isinstance(x, bmx.Engine)
    name = ("bmx_where_" if one else "bmx_comm_where_") + ("map_rows" if q["kind"] == "map" else "join_rows")
    cursor = (int(q["start"]),) if one else (int(start_shard), int(q["start"]))
    x._chk(getattr(x.L, name)(x.h, *head, *mid, *cursor, *tail, *((bmx.MEM_HOST,) if one else ())))
    del keep
    r = res.view(JROWS_RES_DTYPE)[0]
    n = int(r["n_out"])
    assert n == min(int(r["n_match"]), cap), (n, int(r["n_match"]), cap)
    assert (ids[n:] == PAT_U).all() and (in_ids[n:] == PAT_U).all(), "ids behind n_out"
    out = dict(ids=ids[:n].copy(), in_ids=in_ids[:n].copy(), res=r)
    for name, buf, k in (("vals", vals, nf), ("ts", ts, nf), ("in_vals", in_vals, nif), ("in_ts", in_ts, nif)):
        b2 = buf[:k * cap].reshape(k, cap) if cap else buf[:0].reshape(k, 0)
        assert (b2[:, n:] == PAT_I).all() and (buf[k * cap:] == PAT_I).all(), name + " behind n_out"
        if name.endswith("ts") and not q["with_ts"]:
            assert (buf == PAT_I).all(), "without BMX_ROWS_TS no clock is written"
        out[name] = b2[:, :n].copy()
    return out


def ask(x, m, q, order=None):
    """one query of an Engine checked against the brute force -> (got, want)"""
    order = x.index_ids(q["base"]) if order is None else order
    got, want = raw(x, q), answer(m, order, q)
    bad = check(got, want, q)
    assert bad is None, (bad, {k: v for k, v in q.items() if k not in ("keys", "ids")})
    assert int(got["res"]["next_shard"]) == 0
    return got, want


# ---- the sequential stand-in of the map ----
BIAS = 1 << 63
EMPTY, NO_ATTR = INT64_MIN, INT64_MAX


def word_of(i):
    """the carried word of a node id: id ^ 2^63 as a signed number"""
    w = int(i) ^ BIAS
    return w - (1 << 64) if w >= BIAS else w


def id_of(w):
    return (int(w) % (1 << 64)) ^ BIAS


class MapDevice:
    def __init__(self, map_cap, signed=False):
        self.cap, self.slots, self.signed = map_cap, slots_for(map_cap), signed
        self.keys, self.words = [EMPTY] * self.slots, [NO_ATTR] * self.slots
        self.claims = self.overflow = self.counted = 0
        self.tags = set()

    def _walk(self, key, claim):
        h = home(key, self.slots)
        for p in range(self.slots):
            s = h + p
            if s >= self.slots:
                s -= self.slots; self.tags.add("wrap")
            k = self.keys[s]
            if k == EMPTY and claim:
                self.keys[s] = k = key; self.claims += 1
            if k == key:
                if p:
                    self.tags.add(("walk", p))
                return s
            if k == EMPTY:
                return None
            if claim and p & 63 == 63 and self.claims > self.cap:
                break
        return None

    def insert(self, key, node_id):
        s = self._walk(int(key), True)
        if s is None:
            self.overflow = 1; return
        w = word_of(node_id)
        if self.signed:                                    # the defect: the id itself under a signed minimum
            w = int(np.uint64(node_id).astype(np.int64)); cur = self.words[s]
            self.words[s] = w if cur == NO_ATTR else min(cur, w); return
        if self.words[s] > w:
            self.words[s] = w; self.tags.add("lowered")

    def insert_list(self, keys, ids):
        for k, i in zip(keys, ids):
            if k < -VAL_MAX or k > VAL_MAX or int(i) == NO_NODE:
                self.tags.add("skipped"); continue
            self.counted += 1
            self.insert(k, i)

    def fits(self):
        return not self.overflow and self.claims <= self.cap

    def find(self, key):
        """-> the inner id, NO_NODE when the key is none of the map's"""
        s = self._walk(int(key), False)
        if s is None:
            return NO_NODE
        return int(np.int64(self.words[s]).astype(np.uint64)) if self.signed else id_of(self.words[s])

    def pairs(self):
        return sorted((k, self.find(k)) for k in self.keys if k != EMPTY)


# ---- layouts of the tests ----
def truth_table(outer_wide=False, inner_wide=False):
    """outer nodes 40..: {selected or not} x link {a key of M, a key whose inner node is not selected, no key at all, tombstone, absent}; inner nodes 0..39: keys
    100..104, four nodes each (the smallest id wins), the cells FX / FY of the inner nodes in all three states; the four nodes of key 105 hold it as a tombstone
    (105 is no key)"""
    n = 160
    ow, iw = (WIDE if outer_wide else 0), (WIDE if inner_wide else 0)
    m = Table(streams.splitmix64_np(np.arange(1, n + 1, dtype=np.uint64) + np.uint64(81000 + 2 * outer_wide + inner_wide)))
    i = np.arange(n)
    inn, out = i[:40], i[40:]
    m.set(FI, inn, iw + 1 + inn % 3, 10 + inn)
    m.set(FK, inn[:24], 100 + inn[:24] % 6, 50 + inn[:24])
    m.set(FI, inn[24:32], iw + 9, 7); m.set(FK, inn[24:32], 110, 7)                      # inner nodes the programs below do not select
    m.set(FX, inn[inn % 3 != 0], 1000 + inn[inn % 3 != 0], 100 + inn[inn % 3 != 0])
    m.set(FY, inn[inn % 4 != 1], -5 - inn[inn % 4 != 1], 200 + inn[inn % 4 != 1])
    m.set(FB, out, ow + out % 2, 300 + out)
    lk = (out // 2) % 5
    m.set(FL, out[lk == 0], 100 + (out[lk == 0] // 10) % 5); m.set(FL, out[lk == 1], 110); m.set(FL, out[lk == 2], 5000 + out[lk == 2]); m.set(FL, out[lk == 3], 101)
    m.set(FL, out[lk == 2][:3], 105)
    m.set(F1, out, out % 7, 400 + out)
    m.set(F2, out[out % 3 != 0], out[out % 3 != 0] * 11, 500 + out[out % 3 != 0])
    tombs = {FL: out[lk == 3], FK: np.array([5, 11, 17, 23]), FX: inn[inn % 3 == 1], FY: inn[inn % 4 == 2], F2: out[out % 3 == 1]}
    return m, tombs, ow, iw


def apply_tombs(m, tombs, x=None):
    rm.apply_tombs(m, tombs, x)


# ---- the seeded suite: join_model's seeded orders and users as a Table (every cell's clock 5), and its 60 program pairs with fields to project ----
def as_table(m, ts=5):
    t = Table(m.ids)
    for f in m.val:
        t._f(f)
        t.val[f][:] = m.val[f]; t.st[f][:] = m.st[f]; t.clk[f][:] = np.where(m.st[f] == ABSENT, NO_CLOCK, ts)
    return t


def seeded_model():
    import join_model as jm
    m, tombs = jm.seeded_model()
    return as_table(m), tombs


def seeded_pairs(count=60):
    """-> [query]: 0..8 fields on either side (the base, link and key fields, program fields, a field nobody holds, repeats), with and without clocks, every third
    an inner join"""
    import join_model as jm
    po = [jm.FB, jm.FL, jm.F1, jm.FM, jm.F2, NOBODY, jm.FL, jm.FM]
    pi = [jm.FA, jm.FK, jm.FI, jm.F1, NOBODY, jm.FA, jm.F2, jm.FK]
    out = []
    for k, q in enumerate(jm.seeded_pairs(count)):
        fields = [po[(k + j) % 8] for j in range(k % 9)]
        in_fields = [pi[(2 * k + j) % 8] for j in range((k * 5 + 1) % 9)]
        out.append(Q(q["base"], q["clauses"], q["link"], fields, q["inner_base"], q["inner_clauses"], q["key"], in_fields, k % 2 == 0, k % 3 == 1, 0, 1 << 15, 1024))
    return out


# ---- the sharded forms ----
def comm_answer(m, orders, q, start_shard=0):
    """what a communicator over shards whose outer indexes hold `orders` delivers: the map is the union, the shards deliver one after the other from the cursor
    (start_shard, q['start']) on, each in its own index order, into the room that is left -> answer()'s dictionary with next_shard set"""
    M = map_of(m, q)
    N = len(orders)
    if len(M[0]) > map_cap_of(q):
        w = answer(m, orders[-1], q, M)
        w["res"]["next_shard"] = N - 1
        return w
    parts, room, cut, tot = [], q["cap"], False, None
    for g in range(start_shard, N):
        w = answer(m, orders[g], dict(q, start=q["start"] if g == start_shard else 0, cap=room), M)
        r = w["res"]
        room -= int(r["n_out"])
        parts.append(w)
        if tot is None:
            tot = r.copy(); tot["n_match"] = tot["n_out"] = tot["n_joined"] = 0
        tot["n_match"] += r["n_match"]; tot["n_out"] += r["n_out"]; tot["n_joined"] += r["n_joined"]
        if not cut:
            tot["next_shard"] = g; tot["next_pos"] = r["next_pos"]
            cut = int(r["n_match"]) > int(r["n_out"])
    out = {k: np.concatenate([p[k] for p in parts], axis=(0 if k.endswith("ids") else 1)) for k in ("ids", "vals", "ts", "in_ids", "in_vals", "in_ts")}
    out["res"] = tot
    return out
