"""A numpy model of the semi-joins (include/bmx_semi.h, csrc/semi_kernels.h), shared by test_semi_model.py (CPU) and the GPU tests (helper, not a test). The table
and the selection are watch_model.Model's (a state per field and node: absent, data, tombstone); mask(base, clauses) is bmx_scan_where's truth.

Two halves:

expected(...) : the brute-force answer. inner_set(): the inner selection -> numpy.unique of the keys that are present; list_set(): the given values inside the
    domain. selected(): the outer selection AND numpy.isin on the links that are present, or its complement. The overflow rule (more distinct values than
    set_cap: flag, n_match 0, no ids), n_inner and set_size. check() is every comparison the GPU tests make against a pattern-filled buffer.

Device : a sequential stand-in of k_semi_build / k_semi_insert / PredSemi / k_semi_finish on group_model's home() (the table is the group table's: same hash,
    linear probing with wrap, INT64_MIN = empty). It tags every insert: ('present',) the key was there, ('home',) claimed at its home slot, ('walk', n) claimed
    n steps on, ('wrap', n) the same past the last slot, ('giveup',) a walk ended without a slot, ('skipped',) a listed value outside the domain. Built with
    defect=... it is wrong in one way each, which test_semi_model.py shows that check() notices.

The seeded suite: seeded_model() — "orders" that link to "users" by a sparse key, some links dangling, absent or tombstoned — and seeded_pairs(), 60 pairs of an
outer and an inner program with their link and key fields."""
import numpy as np

import group_model as gm
import where_agg_model as wam
from oracle import streams
from watch_model import ABSENT, DATA, TOMB, Model  # noqa: F401

SEMI_RES_DTYPE = np.dtype([("n_match", "<u8"), ("set_size", "<u8"), ("n_inner", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])
OVERFLOW, ANTI, MAX_SET = 1, 1, 1 << 20
VAL_MAX = (1 << 53) - 1
EMPTY = -(1 << 63)
FILL = 0x5A
FILL64 = int(np.full(8, FILL, np.uint8).view(np.uint64)[0])
PAD = 8                       # words of the caller's buffer behind out_ids[cap] that the checks watch

FB, FL, FI, FK, F1, F2, NOBODY = (streams.fnv1a32(s) for s in ("semi.base", "semi.link", "semi.inner", "semi.key", "semi.one", "semi.two", "semi.nobody"))
ALL_FIELDS = [FB, FL, FI, FK, F1, F2]
EVERY = [[(NOBODY, 0, 0, True)]]     # a negated literal on a field nobody has: true for every candidate

slots_for, home, keys_with_home = gm.slots_for, gm.home, gm.keys_with_home


# ---- the brute-force answer ----
def inner_set(m, inner_base, inner_clauses, key):
    """-> (the distinct keys, ascending; n_inner)"""
    sel = m.mask(inner_base, inner_clauses)
    m._f(key)
    have = sel & (m.st[key] == DATA)
    return np.unique(m.val[key][have]), int(sel.sum())


def list_set(values):
    v = np.asarray(values, np.int64).ravel()
    ok = (v >= -VAL_MAX) & (v <= VAL_MAX)
    return np.unique(v[ok]), int(ok.sum())


def selected(m, base, clauses, link, S, anti=False):
    """-> a mask over the model's nodes"""
    sel = m.mask(base, clauses)
    m._f(link)
    inside = (m.st[link] == DATA) & np.isin(m.val[link], S)
    return sel & (~inside if anti else inside)


class Expected:
    def __init__(self, ids, n_match, set_size, n_inner, flags):
        self.ids, self.n_match, self.set_size, self.n_inner, self.flags = ids, n_match, set_size, n_inner, flags

    def __repr__(self):
        return "Expected(%d ids, n_match=%d, set_size=%d, n_inner=%d, flags=%d)" % (len(self.ids), self.n_match, self.set_size, self.n_inner, self.flags)


def expected(m, pos_nodes, base, clauses, link, S, n_inner, anti=False, set_cap=None):
    """pos_nodes: the node numbers of the base index's positions, in position order (None: node order — for answers compared as sets). S: the distinct values.
    On overflow set_size is the TRUE number of distinct values: the device reports some number in (set_cap, set_size]."""
    if set_cap is not None and len(S) > set_cap:
        return Expected(np.zeros(0, np.uint64), 0, len(S), n_inner, OVERFLOW)
    sel = selected(m, base, clauses, link, S, anti)
    order = np.arange(m.N) if pos_nodes is None else np.asarray(pos_nodes)
    ids = m.ids[order[sel[order]]]
    assert len(ids) == int(sel.sum()), "a selected node is missing from the index"
    return Expected(ids, len(ids), len(S), n_inner, 0)


def expected_semijoin(m, pos_nodes, base, clauses, link, inner_base, inner_clauses, key, anti=False, set_cap=65536):
    S, n_inner = inner_set(m, inner_base, inner_clauses, key)
    return expected(m, pos_nodes, base, clauses, link, S, n_inner, anti, set_cap)


def expected_in(m, pos_nodes, base, clauses, link, values, anti=False):
    S, n_inner = list_set(values)
    return expected(m, pos_nodes, base, clauses, link, S, n_inner, anti, None)


def check(buf, res, want, cap, set_cap=None, ordered=True):
    """every comparison the GPU tests make -> None or what differs. buf: the caller's whole buffer of cap + PAD words, pattern-filled before the call"""
    buf = np.asarray(buf, np.uint64)
    if int(res["reserved"]) != 0:
        return ("reserved", int(res["reserved"]))
    if int(res["n_inner"]) != want.n_inner:
        return ("n_inner", int(res["n_inner"]), want.n_inner)
    if want.flags & OVERFLOW:
        if int(res["flags"]) != OVERFLOW or int(res["n_match"]) != 0 or not (set_cap < int(res["set_size"]) <= want.set_size):
            return ("overflow", int(res["flags"]), int(res["n_match"]), int(res["set_size"]), want.set_size)
        return None if (buf == FILL64).all() else ("out_ids written on overflow",)
    if (int(res["flags"]), int(res["n_match"]), int(res["set_size"])) != (0, want.n_match, want.set_size):
        return ("flags / n_match / set_size", int(res["flags"]), int(res["n_match"]), int(res["set_size"]), want)
    k = min(want.n_match, cap)
    if not (buf[k:] == FILL64).all():
        return ("written at or beyond out_ids[min(n_match, cap)]",)
    if ordered:
        if not np.array_equal(buf[:k], want.ids[:k]):
            bad = np.nonzero(buf[:k] != want.ids[:k])[0]
            return ("ids", int(bad[0]), int(buf[bad[0]]), int(want.ids[bad[0]]))
    elif cap >= want.n_match and not np.array_equal(np.sort(buf[:k]), np.sort(want.ids)):
        return ("id set",)
    elif not np.isin(buf[:k], want.ids).all() or len(np.unique(buf[:k])) != k:
        return ("ids outside the answer",)
    return None


# ---- helpers of the GPU tests: raw calls into pattern-filled buffers ----
def _buffers(cap):
    return np.full(cap + PAD, FILL64, np.uint64), np.full(32, FILL, np.uint8)


def raw_semijoin(x, base, clauses, link, inner_base, inner_clauses, key, anti=False, cap=0, set_cap=65536):
    """x: an Engine or a Comm -> (the whole buffer of cap + PAD words, the result record)"""
    import bmx
    buf, res = _buffers(cap)
    args = (*bmx._where_args(base, clauses), int(link), ANTI if anti else 0, *bmx._where_args(inner_base, inner_clauses), int(key), int(set_cap),
            bmx._ptr(buf) if cap else None, int(cap), bmx._ptr(res))
    x._chk(x.L.bmx_where_semijoin(x.h, *args, bmx.MEM_HOST) if isinstance(x, bmx.Engine) else x.L.bmx_comm_where_semijoin(x.h, *args))
    return buf, res.view(SEMI_RES_DTYPE)[0]


def raw_in(x, base, clauses, link, values, anti=False, cap=0):
    import bmx
    buf, res = _buffers(cap)
    v = np.ascontiguousarray(values, np.int64)
    args = (*bmx._where_args(base, clauses), int(link), ANTI if anti else 0, bmx._ptr(v), len(v), bmx._ptr(buf) if cap else None, int(cap), bmx._ptr(res))
    x._chk(x.L.bmx_where_in(x.h, *args, bmx.MEM_HOST) if isinstance(x, bmx.Engine) else x.L.bmx_comm_where_in(x.h, *args))
    return buf, res.view(SEMI_RES_DTYPE)[0]


def pos_nodes(e, m, base):
    return m.index_of(e.index_ids(base))


def ask_semijoin(e, m, base, clauses, link, inner_base, inner_clauses, key, anti=False, cap=None, set_cap=65536, pn=None):
    """one engine's answer checked against the model -> the expectation"""
    pn = pos_nodes(e, m, base) if pn is None else pn
    want = expected_semijoin(m, pn, base, clauses, link, inner_base, inner_clauses, key, anti, set_cap)
    cap = len(pn) if cap is None else cap
    buf, res = raw_semijoin(e, base, clauses, link, inner_base, inner_clauses, key, anti, cap, set_cap)
    bad = check(buf, res, want, cap, set_cap)
    assert bad is None, (bad, want, dict(base=base, clauses=clauses, link=link, inner_base=inner_base, inner_clauses=inner_clauses, key=key, anti=anti, cap=cap, set_cap=set_cap))
    return want


def ask_in(e, m, base, clauses, link, values, anti=False, cap=None, pn=None):
    pn = pos_nodes(e, m, base) if pn is None else pn
    want = expected_in(m, pn, base, clauses, link, values, anti)
    cap = len(pn) if cap is None else cap
    buf, res = raw_in(e, base, clauses, link, values, anti, cap)
    bad = check(buf, res, want, cap, len(values))
    assert bad is None, (bad, want, dict(base=base, clauses=clauses, link=link, nvalues=len(values), anti=anti, cap=cap))
    return want


# ---- the sequential stand-in ----
DEFECTS = ("lost_wrap", "tomb_key", "absent_link_plain", "absent_link_anti", "write_on_overflow", "write_behind_cap")


class Device:
    """build / insert_list, then probe, then finish — as the kernels do it, one row after the other in position order"""

    def __init__(self, set_cap, defect=None):
        assert defect is None or defect in DEFECTS
        self.cap, self.slots, self.defect = set_cap, slots_for(set_cap), defect
        self.table = [EMPTY] * self.slots
        self.claims = self.n_inner = self.overflow = 0
        self.tags = []

    def insert(self, key):
        key = int(key)
        h = home(key, self.slots)
        for p in range(self.slots):
            s = h + p
            if s >= self.slots:
                if self.defect == "lost_wrap":
                    break                                             # the walk falls off the table's end
                s -= self.slots
            k = self.table[s]
            if k == key:
                self.tags.append(("present",)); return
            if k == EMPTY:
                self.table[s] = key; self.claims += 1
                self.tags.append(("home",) if p == 0 else (("wrap", p) if h + p >= self.slots else ("walk", p))); return
            if p & 63 == 63 and self.claims > self.cap:
                break
        self.overflow = 1
        self.tags.append(("giveup",))

    def build(self, m, pn, inner_base, inner_clauses, key):
        """pn: the inner base index's positions as node numbers"""
        sel = m.mask(inner_base, inner_clauses)
        m._f(key)
        for i in pn:
            if not sel[i]:
                continue
            self.n_inner += 1
            if m.st[key][i] == DATA or (self.defect == "tomb_key" and m.st[key][i] == TOMB):
                self.insert(m.val[key][i])                                            # (the defect inserts the value the row held before its tombstone)

    def insert_list(self, values):
        for v in np.asarray(values, np.int64).tolist():
            if v < -VAL_MAX or v > VAL_MAX:
                self.tags.append(("skipped",)); continue
            self.n_inner += 1
            self.insert(v)

    def has(self, key):
        h = home(int(key), self.slots)
        for p in range(self.slots):
            s = h + p
            if s >= self.slots:
                if self.defect == "lost_wrap":
                    return False
                s -= self.slots
            k = self.table[s]
            if k == int(key):
                return True
            if k == EMPTY:
                return False
        return False

    def fits(self):
        return not self.overflow and self.claims <= self.cap

    def probe(self, m, pn, base, clauses, link, anti, buf, cap):
        """-> the count; ids go into buf[:cap]"""
        sel = m.mask(base, clauses)
        m._f(link)
        n = 0
        if not self.fits() and self.defect != "write_on_overflow":
            return 0
        for i in pn:
            if not sel[i]:
                continue
            have = m.st[link][i] == DATA
            inside = bool(have and self.has(m.val[link][i]))
            if self.defect == "absent_link_plain" and not have and not anti:
                inside = True
            if self.defect == "absent_link_anti" and not have and anti:
                inside = True
            if inside != bool(anti):
                if n < cap or (self.defect == "write_behind_cap" and n == cap):
                    buf[n] = m.ids[i]
                n += 1
        return n

    def finish(self, n_match):
        fits = self.fits()
        res = np.zeros((), SEMI_RES_DTYPE)
        res["n_match"] = n_match if fits else 0; res["set_size"] = self.claims; res["n_inner"] = self.n_inner; res["flags"] = 0 if fits else OVERFLOW
        self.table = [EMPTY] * self.slots; self.claims = self.n_inner = self.overflow = 0
        return res


def device_semijoin(m, base, clauses, link, inner_base, inner_clauses, key, anti=False, cap=None, set_cap=65536, defect=None):
    """the stand-in's answer into a pattern-filled buffer -> (buf, res, the device: its tags)"""
    cap = m.N if cap is None else cap
    buf = np.full(cap + PAD, FILL64, np.uint64)
    d = Device(set_cap, defect)
    d.build(m, np.arange(m.N), inner_base, inner_clauses, key)
    n = d.probe(m, np.arange(m.N), base, clauses, link, anti, buf, cap)
    return buf, d.finish(n), d


def device_in(m, base, clauses, link, values, anti=False, cap=None, defect=None):
    cap = m.N if cap is None else cap
    buf = np.full(cap + PAD, FILL64, np.uint64)
    d = Device(max(len(values), 1), defect)
    d.insert_list(values)
    n = d.probe(m, np.arange(m.N), base, clauses, link, anti, buf, cap)
    return buf, d.finish(n), d


# ---- the seeded suite ----
N_SEED, N_USERS, SEED = 8192 + 611, 3000, 20260311     # more than one 8192-row block of orders; the first N_USERS nodes are users too


def uid(j):
    """user j's key: sparse over both signs, far outside any window"""
    return np.asarray(j, np.int64) * 1000003 - 10**9


def seeded_model():
    """-> (model, {field: nodes to tombstone after the load})"""
    rng = np.random.default_rng(SEED)
    m = Model(wam.node_ids(N_SEED, 52000))
    everyone, users = np.arange(N_SEED), np.arange(N_USERS)
    m.set(FB, everyone, rng.integers(0, 100, N_SEED))
    for f, pr in ((F1, 0.8), (F2, 0.5)):
        idx = everyone[rng.random(N_SEED) < pr]
        m.set(f, idx, rng.integers(0, 10, len(idx)))
    m.set(FI, users, rng.integers(0, 200, N_USERS))                               # the inner base: overlaps FB's 0..99, so FB can link to it
    ku = users[rng.random(N_USERS) < 0.9]
    m.set(FK, ku, uid(rng.integers(0, 800, len(ku))))                             # 800 distinct keys at most, shared by several users
    lk = everyone[rng.random(N_SEED) < 0.8]
    target = rng.integers(0, 1000, len(lk))                                       # 800..999: keys no user holds (dangling links)
    m.set(FL, lk, uid(target))
    tombs = {}
    for f, k in ((FL, 500), (FK, 200), (FB, 60), (FI, 40), (F1, 100)):
        tombs[f] = rng.choice(np.nonzero(m.st[f] == DATA)[0], k, replace=False)
    return m, tombs


def seeded_pairs(count=60):
    """-> [(outer clauses, link, inner clauses, key, anti)]; the outer base is FB, the inner base FI"""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for k in range(count):
        lo = int(rng.integers(0, 70))
        outer = [[(FB, lo, lo + int(rng.integers(10, 50)))]]
        if k % 3 == 1:
            outer[0].append((F1, 2, int(rng.integers(3, 9)), bool(k % 2)))
        if k % 4 == 3:
            outer.append([(F2, 0, int(rng.integers(0, 4))), (FB, 0, 99)])
        ilo = int(rng.integers(0, 150))
        inner = [[(FI, ilo, ilo + int(rng.integers(5, 60)))]]
        if k % 5 == 2:
            inner[0].append((F1, 0, 6))
        if k % 6 == 5:
            inner.append([(F2, 8, 9)])
        link, key = (FB, FI) if k % 5 == 4 else (FL, FK)
        out.append((outer, link, inner, key, bool((k // 2) % 2)))
    return out


# ---- the edge layouts: small tables on which every rule of the header can go wrong; run by the stand-in (CPU) and by the library (GPU) ----
WIDE = 1 << 40                # a base value beyond int32 switches the index to its int64 column
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def Q(base, clauses, link, inner_base, inner_clauses, key, anti=False, set_cap=64):
    return dict(kind="semijoin", base=base, clauses=clauses, link=link, inner_base=inner_base, inner_clauses=inner_clauses, key=key, anti=anti, set_cap=set_cap)


def QIN(base, clauses, link, values, anti=False):
    return dict(kind="in", base=base, clauses=clauses, link=link, values=[int(v) for v in values], anti=anti)


def both(q):
    return [dict(q, anti=False), dict(q, anti=True)]


def truth_table(outer_wide=False, inner_wide=False):
    """{outer selected or not} x {link data in S, data not in S, tombstone, absent}, several nodes each; the first 16 nodes are the inner side with keys 100..103"""
    n = 64
    ow, iw = (WIDE if outer_wide else 0), (WIDE if inner_wide else 0)
    m = Model(wam.node_ids(n, 61000 + 2 * outer_wide + inner_wide))
    i = np.arange(n)
    m.set(FB, i, ow + i % 2)
    kind = (i // 2) % 4
    m.set(FL, i[kind == 0], 100 + i[kind == 0] % 4); m.set(FL, i[kind == 1], 500 + i[kind == 1]); m.set(FL, i[kind == 2], 100 + i[kind == 2] % 4)
    m.set(F1, i, i % 5)
    m.set(FI, i[:16], iw + 1 + i[:16] % 3); m.set(FK, i[:16], 100 + i[:16] % 4)
    m.set(FI, i[16:24], iw + 9); m.set(FK, i[16:20], 100 + i[16:20] % 4)   # inner nodes the programs below do not select; 20..23 have no key at all
    m.set(FI, i[24:26], iw + 2); m.set(FK, i[24:26], 104); m.set(FL, i[kind == 1][:4], 104)          # a selected inner node whose key row is a tombstone: 104 is no key
    tombs = {FL: i[kind == 2], FK: i[24:26]}
    sel = [[(FB, ow + 1, ow + 1)]]
    inner = [[(FI, iw + 1, iw + 3)]]
    qs = both(Q(FB, sel, FL, FI, inner, FK))                                                       # link and key: unnamed fields
    qs += both(Q(FB, [[(FB, ow + 1, ow + 1)], [(FL, 100, 101)]], FL, FI, [[(FI, iw + 1, iw + 3), (FK, 100, 102)]], FK))   # ... fields their programs probe
    qs += both(Q(FB, EVERY, FL, FI, [[(FI, iw + 9, iw + 9)]], FK))                                 # inner nodes without a key count in n_inner
    qs += both(Q(FB, sel, FL, FI, [[(FI, iw + 50, iw + 60)]], FK))                                 # an empty inner selection
    qs += both(Q(FB, sel, FL, FI, inner, NOBODY))                                                  # every key absent
    qs += both(Q(FB, sel, NOBODY, FI, inner, FK))                                                  # every link absent
    qs += both(Q(FB, [[(FB, ow + 7, ow + 8)]], FL, FI, inner, FK))                                 # nothing selected
    return m, tombs, qs


def base_links():
    """link = the outer base field, key = the inner base field, and both programs over ONE base field"""
    n = 300
    m = Model(wam.node_ids(n, 62000))
    i = np.arange(n)
    m.set(FB, i, i % 50); m.set(FI, i[:120], (i[:120] * 7) % 90); m.set(F1, i, i % 6); m.set(FK, i[::3], i[::3] % 11)
    tombs = {FB: i[5::40], FI: i[3:120:25]}
    qs = both(Q(FB, EVERY, FB, FI, [[(FI, 10, 60)]], FI))                                          # column against column
    qs += both(Q(FB, [[(F1, 0, 2)]], FB, FB, [[(FB, 0, 9)], [(F1, 5, 5)]], FB))                    # one base field on both sides: S = its values on the inner selection
    qs += both(Q(FB, [[(FB, 0, 30)]], FB, FB, [[(FB, 20, 49)]], FK))                               # the same index, key probed
    qs += both(Q(FB, [[(FB, 0, 30)]], FK, FI, [[(FI, 0, 40)]], FI))                                # link probed, key from the column
    return m, tombs, qs


def key_values():
    keys = np.array([0, 1, -1, VAL_MAX, -VAL_MAX, 1 << 31, -(1 << 31), (1 << 32) + 5, 7], np.int64)
    n = 6 * len(keys)
    m = Model(wam.node_ids(n, 63000))
    i = np.arange(n)
    m.set(FB, i, i); m.set(FL, i, keys[i % len(keys)])
    m.set(FI, i[:len(keys)], i[:len(keys)]); m.set(FK, i[:len(keys)], keys)
    qs = []
    for lo, hi in ((0, 8), (0, 4), (3, 4), (0, 0), (5, 8)):
        qs += both(Q(FB, EVERY, FL, FI, [[(FI, lo, hi)]], FK))
    qs += both(QIN(FB, EVERY, FL, [VAL_MAX, -VAL_MAX, 0]))
    qs += both(QIN(FB, EVERY, FL, [7, 7, 7, 1, 7, 1]))                                            # duplicates
    qs += both(QIN(FB, EVERY, FL, [VAL_MAX + 1, -VAL_MAX - 1, INT64_MIN, INT64_MAX, -1]))         # outside the domain: skipped, not counted
    qs += both(QIN(FB, EVERY, FL, [INT64_MIN]))                                                   # an empty set from a list
    qs += both(QIN(FB, EVERY, FL, [1 << 31]))                                                     # nvalues = 1
    qs += both(QIN(FB, [[(FB, 10, 30)]], FB, [11, 12, 29, 31, -4]))                               # the link is the base column
    return m, {}, qs


def table_edges():
    """set_cap <= 32, 64 slots: 32 keys that share one home; a cluster that wraps from slot 63 to 0; links to absent keys that walk the whole cluster to its
    empty word; D = set_cap and set_cap + 1; 70 keys against set_cap 32 (the table fills up: walks give up)"""
    same = keys_with_home(5, 64, 33)                                  # 32 in the set, one more with the same home that is not
    wrap = keys_with_home(62, 64, 7, start=10**6)                     # 6 in the set: slots 62, 63, 0, 1, 2, 3
    many = [int(uid(j)) for j in range(70)]
    n = 200
    m = Model(wam.node_ids(n, 64000))
    i = np.arange(n)
    m.set(FB, i, i)
    m.set(FI, i, i)
    kv = np.array(same[:32] + wrap[:6] + many + [0] * (n - 108), np.int64)
    m.set(FK, i[:108], kv[:108])
    lv = np.array(same + wrap + many[:40] + [12345] * (n - 80), np.int64)   # links: every key of the two clusters, the two absent ones, 40 of the many
    m.set(FL, i, lv)
    qs = []
    qs += both(Q(FB, EVERY, FL, FI, [[(FI, 0, 31)]], FK, set_cap=32))                             # one home, D = set_cap
    qs += both(Q(FB, EVERY, FL, FI, [[(FI, 32, 37)]], FK, set_cap=6))                             # the wrapping cluster
    qs += both(Q(FB, EVERY, FL, FI, [[(FI, 0, 37)]], FK, set_cap=38))                             # both (128 slots)
    qs += both(Q(FB, EVERY, FL, FI, [[(FI, 0, 32)]], FK, set_cap=32))                             # D = 32 + a key already there... (node 32 is the first wrap key: D = 33)
    qs += both(Q(FB, EVERY, FL, FI, [[(FI, 38, 107)]], FK, set_cap=32))                           # 70 keys into 64 slots
    qs += both(Q(FB, EVERY, FL, FI, [[(FI, 38, 107)]], FK, set_cap=69))
    qs += both(Q(FB, EVERY, FL, FI, [[(FI, 38, 107)]], FK, set_cap=70))
    qs += both(QIN(FB, EVERY, FL, same[:32] + same[:32]))
    return m, {}, qs


def edge_layouts():
    yield ("truth table",) + truth_table()
    yield ("truth table, int64 outer column",) + truth_table(outer_wide=True)
    yield ("truth table, int64 inner column",) + truth_table(inner_wide=True)
    yield ("truth table, int64 on both sides",) + truth_table(True, True)
    yield ("base links",) + base_links()
    yield ("key values",) + key_values()
    yield ("table edges",) + table_edges()


def apply_tombs(m, tombs):
    for f, idx in tombs.items():
        m.tomb(f, idx)


def want_of(m, pn, q):
    if q["kind"] == "in":
        return expected_in(m, pn, q["base"], q["clauses"], q["link"], q["values"], q["anti"])
    return expected_semijoin(m, pn, q["base"], q["clauses"], q["link"], q["inner_base"], q["inner_clauses"], q["key"], q["anti"], q["set_cap"])


def set_cap_of(q):
    return len(q["values"]) if q["kind"] == "in" else q["set_cap"]


def device_of(m, q, cap=None, defect=None):
    if q["kind"] == "in":
        return device_in(m, q["base"], q["clauses"], q["link"], q["values"], q["anti"], cap, defect)
    return device_semijoin(m, q["base"], q["clauses"], q["link"], q["inner_base"], q["inner_clauses"], q["key"], q["anti"], cap, q["set_cap"], defect)


def raw_of(x, q, cap):
    if q["kind"] == "in":
        return raw_in(x, q["base"], q["clauses"], q["link"], q["values"], q["anti"], cap)
    return raw_semijoin(x, q["base"], q["clauses"], q["link"], q["inner_base"], q["inner_clauses"], q["key"], q["anti"], cap, q["set_cap"])


def caps_of(n_match, n):
    return sorted({c for c in (0, 1, n_match - 1, n_match, n) if c >= 0})
