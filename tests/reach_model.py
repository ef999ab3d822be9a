"""A numpy model of the graph traversal (include/bmx_reach.h, csrc/reach_kernels.h), shared by test_reach_model.py (CPU) and the GPU tests (helper, not a test).
The table and the selection are watch_model.Model's (a state per field and node: absent, data, tombstone); mask(base, clauses) is bmx_scan_where's truth.

Two halves:

literal(...) / answer(...) : the brute force. literal() follows the header's definition word for word — level(v) = 0 for a seed value, otherwise the minimum of
    depth(x) over the edge nodes x with key(x) == v; depth(x) = 1 + level(link(x)) — by relaxing until nothing changes, in no particular order. answer() is the
    same least fixed point computed level by level with numpy (test_reach_model.py holds the two against each other), cut at max_depth, with set_size, n_seed,
    n_edges, rounds, MORE and the overflow rule. check() is every comparison the GPU tests make against pattern-filled buffers; levels_bad() compares a map's
    levels with the definition's.

Device : a sequential stand-in of k_reach_seed / k_reach_list / k_reach_prepare / k_reach_round / the mask and emit / k_reach_finish on join_model.Device's map
    (same hash, linear probing with wrap, INT64_MIN = empty, INT64_MAX = no level yet), one position after the other in position order. It tags its paths:
    join_model's 'present', 'claim', ('walk', n), 'wrap', 'giveup', and 'lowered' / 'min_skipped' the minimum, 'reached', 'same_round' a link found at this
    round's own level (not reached yet), 'keyless' a reached node without key, 'no_edge' a selected node without link, 'early_out' a round that returned at once,
    'skipped' a listed value outside the domain. Built with defect=... it is wrong in one way each, which test_reach_model.py shows that check() or levels_bad()
    notices."""
import numpy as np

import join_model as jm
import semi_model as sm
import where_agg_model as wam
from oracle import streams
from watch_model import ABSENT, DATA, TOMB, Model  # noqa: F401

REACH_RES_DTYPE = np.dtype([("n_match", "<u8"), ("set_size", "<u8"), ("n_seed", "<u8"), ("n_edges", "<u8"), ("rounds", "<u4"), ("flags", "<u4")])
OVERFLOW, MORE, MAX_SET, MAX_DEPTH = 1, 2, 1 << 20, 255
VAL_MAX = (1 << 53) - 1
EMPTY, NO_LEVEL = jm.EMPTY, jm.NO_ATTR
FILL, FILL64, PAD = sm.FILL, sm.FILL64, sm.PAD
WIDE = 1 << 40

FB, FL, FK, FI, F1, F2, NOBODY, EVERY = sm.FB, sm.FL, sm.FK, sm.FI, sm.F1, sm.F2, sm.NOBODY, sm.EVERY      # base, link, key; FI: the seed side's base
FS = streams.fnv1a32("reach.seed")
ALL_FIELDS = [FB, FL, FK, FI, F1, F2, FS]


def Q(base, clauses, link, key, seed_base, seed_clauses, seed_field, max_depth=MAX_DEPTH, set_cap=4096):
    return dict(kind="reach", base=base, clauses=clauses, link=link, key=key, seed_base=seed_base, seed_clauses=seed_clauses, seed_field=seed_field,
                max_depth=max_depth, set_cap=set_cap)


def QFROM(base, clauses, link, key, values, max_depth=MAX_DEPTH, set_cap=4096):
    return dict(kind="from", base=base, clauses=clauses, link=link, key=key, values=np.asarray(values, np.int64), max_depth=max_depth, set_cap=set_cap)


def as_list(m, q):
    """the list form of a program-form query: the seed side's present values, every one twice, and two values outside the domain"""
    S, _ = seeds_of(m, q)
    return QFROM(q["base"], q["clauses"], q["link"], q["key"], np.concatenate([S, [EMPTY, VAL_MAX + 1], S]).astype(np.int64), q["max_depth"], q["set_cap"])


# ---- the brute force ----
def seeds_of(m, q):
    """-> (the distinct seed values, n_seed)"""
    if q["kind"] == "from":
        v = q["values"][(q["values"] >= -VAL_MAX) & (q["values"] <= VAL_MAX)]
        return np.unique(v), len(v)
    sel = m.mask(q["seed_base"], q["seed_clauses"]); m._f(q["seed_field"])
    return np.unique(m.val[q["seed_field"]][sel & (m.st[q["seed_field"]] == DATA)]), int(sel.sum())


def edges_of(m, q):
    """-> (edge: the selected nodes whose link holds data, has_key, link values, key values)"""
    sel = m.mask(q["base"], q["clauses"]); m._f(q["link"]); m._f(q["key"])
    return sel & (m.st[q["link"]] == DATA), m.st[q["key"]] == DATA, m.val[q["link"]], m.val[q["key"]]


def literal(m, q):
    """the definition, relaxed until nothing changes -> ({value: level}, {node: depth}), not cut at max_depth"""
    S, _ = seeds_of(m, q)
    edge, has_key, lv, kv = edges_of(m, q)
    level = {int(v): 0 for v in S}
    depth = {}
    nodes = [int(i) for i in np.nonzero(edge)[0]]
    changed = True
    while changed:
        changed = False
        for x in reversed(nodes):                                  # (an order that is not the device's)
            if int(lv[x]) not in level:
                continue
            d = 1 + level[int(lv[x])]
            if depth.get(x, 1 << 30) > d:
                depth[x] = d; changed = True
            if has_key[x] and level.get(int(kv[x]), 1 << 30) > depth[x]:
                level[int(kv[x])] = depth[x]; changed = True
    return level, depth


def closure(m, q):
    """the same least fixed point level by level -> (depth per node (0: not reached), [the values of level 0, 1, ...])"""
    S, _ = seeds_of(m, q)
    edge, has_key, lv, kv = edges_of(m, q)
    depth = np.zeros(m.N, np.int64)
    known, levels, r = S, [S], 1
    while True:
        reach = edge & (depth == 0) & np.isin(lv, known)
        if not reach.any():
            return depth, levels
        depth[reach] = r
        new = np.setdiff1d(kv[reach & has_key], known)
        levels.append(new); known = np.union1d(known, new); r += 1


class Expected:
    def __init__(self, ids, depth, set_size, n_seed, n_edges, rounds, flags, level):
        self.ids, self.depth, self.n_match, self.set_size, self.n_seed, self.n_edges, self.rounds, self.flags, self.level = (
            ids, depth, len(ids), set_size, n_seed, n_edges, rounds, flags, level)

    def __repr__(self):
        return "Expected(n_match %d, set_size %d, n_seed %d, n_edges %d, rounds %d, flags %d)" % (self.n_match, self.set_size, self.n_seed, self.n_edges, self.rounds, self.flags)


def answer(m, pos_nodes, q):
    """pos_nodes: the node numbers of the base index's positions, in position order"""
    D, set_cap = q["max_depth"], q["set_cap"]
    _, n_seed = seeds_of(m, q)
    edge = edges_of(m, q)[0]
    depth, levels = closure(m, q)
    levels = levels[:D + 1]
    set_size = sum(len(v) for v in levels)
    level = {int(v): r for r, vs in enumerate(levels) for v in vs}
    if set_size > set_cap:
        return Expected(np.zeros(0, np.uint64), np.zeros(0, np.uint8), set_size, n_seed, int(edge.sum()), 0, OVERFLOW, level)
    pn = np.asarray(pos_nodes)
    inside = pn[(depth[pn] >= 1) & (depth[pn] <= D)]
    assert len(inside) == int(((depth >= 1) & (depth <= D)).sum()), "a reached node is missing from the index"
    more = len(levels) > D and len(levels[D]) > 0
    return Expected(m.ids[inside], depth[inside].astype(np.uint8), set_size, n_seed, int(edge.sum()), int(depth[inside].max()) if len(inside) else 0,
                    MORE if more else 0, level)


def check(ids, dep, res, want, cap, set_cap):
    """every comparison the GPU tests make -> None or what differs. ids / dep: the caller's whole buffers of cap + PAD entries, pattern-filled before the call"""
    ids, dep = np.asarray(ids, np.uint64), np.asarray(dep, np.uint8)
    if (int(res["n_seed"]), int(res["n_edges"])) != (want.n_seed, want.n_edges):
        return ("n_seed / n_edges", int(res["n_seed"]), int(res["n_edges"]), want)
    if want.flags & OVERFLOW:
        if int(res["flags"]) != OVERFLOW or int(res["n_match"]) != 0 or int(res["rounds"]) != 0 or not (set_cap < int(res["set_size"]) <= want.set_size):
            return ("overflow", int(res["flags"]), int(res["n_match"]), int(res["rounds"]), int(res["set_size"]), want)
        return None if (ids == FILL64).all() and (dep == FILL).all() else ("written on overflow",)
    got = (int(res["flags"]), int(res["n_match"]), int(res["set_size"]), int(res["rounds"]))
    if got != (want.flags, want.n_match, want.set_size, want.rounds):
        return ("flags / n_match / set_size / rounds", got, want)
    k = min(want.n_match, cap)
    if not (ids[k:] == FILL64).all() or not (dep[k:] == FILL).all():
        return ("written at or beyond [min(n_match, cap)]",)
    if not np.array_equal(ids[:k], want.ids[:k]):
        bad = np.nonzero(ids[:k] != want.ids[:k])[0]
        return ("ids", int(bad[0]), int(ids[bad[0]]), int(want.ids[bad[0]]))
    if not np.array_equal(dep[:k], want.depth[:k]):
        bad = np.nonzero(dep[:k] != want.depth[:k])[0]
        return ("depth", int(bad[0]), int(dep[bad[0]]), int(want.depth[bad[0]]))
    return None


def levels_bad(got, want):
    """a map's {value: level} against the definition's, cut at max_depth -> None or what differs"""
    return None if got == want.level else ("levels", sorted(set(got.items()) ^ set(want.level.items()))[:4])


# ---- helpers of the GPU tests: raw calls into pattern-filled buffers ----
def _buffers(cap):
    return np.full(cap + PAD, FILL64, np.uint64), np.full(cap + PAD, FILL, np.uint8), np.full(40, FILL, np.uint8)


def raw_of(x, q, cap):
    """x: an Engine or a Comm -> (ids: the whole buffer of cap + PAD words, depths: likewise bytes, the result record)"""
    import bmx
    ids, dep, res = _buffers(cap)
    out = (int(q["max_depth"]), int(q["set_cap"]), bmx._ptr(ids) if cap else None, bmx._ptr(dep) if cap else None, int(cap), bmx._ptr(res))
    head = (*bmx._where_args(q["base"], q["clauses"]), int(q["link"]), int(q["key"]), 0)
    one = isinstance(x, bmx.Engine)
    if q["kind"] == "from":
        v = np.ascontiguousarray(q["values"], np.int64)
        args = (*head, bmx._ptr(v), len(v), *out)
        x._chk(x.L.bmx_where_reach_from(x.h, *args, bmx.MEM_HOST) if one else x.L.bmx_comm_where_reach_from(x.h, *args))
    else:
        args = (*head, *bmx._where_args(q["seed_base"], q["seed_clauses"]), int(q["seed_field"]), *out)
        x._chk(x.L.bmx_where_reach(x.h, *args, bmx.MEM_HOST) if one else x.L.bmx_comm_where_reach(x.h, *args))
    return ids, dep, res.view(REACH_RES_DTYPE)[0]


pos_nodes = sm.pos_nodes


def caps_of(n_match, n):
    return sorted({0, 1, max(n_match - 1, 0), n_match, n})


def ask(x, m, q, cap=None, pn=None, want=None):
    """one engine's answer checked against the model -> the expectation"""
    pn = pos_nodes(x, m, q["base"]) if pn is None else pn
    want = answer(m, pn, q) if want is None else want
    cap = len(pn) if cap is None else cap
    ids, dep, res = raw_of(x, q, cap)
    bad = check(ids, dep, res, want, cap, q["set_cap"])
    assert bad is None, (bad, want, {k: v for k, v in q.items() if k != "values"}, cap)
    return want


def load(x, m, fields=None, tombs=()):
    wam.load(x, m, ALL_FIELDS if fields is None else fields)
    for f, idx in tombs:
        wam.tombstone(x, m, f, idx)


# ---- the sequential stand-in ----
DEFECTS = ("le_r", "no_min", "overwrite_depth", "drop_keyless", "more_from_reached", "unselected_passes")


class Device:
    def __init__(self, set_cap, defect=None):
        assert defect is None or defect in DEFECTS
        self.map, self.defect = jm.Device(set_cap), defect
        self.new_keys = [0] * (MAX_DEPTH + 1)
        self.n_seed = self.n_edges = self.rounds = 0
        self.reached_at = [0] * (MAX_DEPTH + 1)

    @property
    def tags(self):
        return self.map.tags

    def insert(self, key, level):
        before = self.map.claims
        s = self.map._walk(int(key), True)
        if s is None:
            self.map.overflow = 1; self.tags.add("giveup"); return
        if self.map.claims > before:
            self.new_keys[level] += 1
        if self.defect == "no_min":
            self.map.vals[s] = level
        elif self.map.vals[s] > level:
            self.map.vals[s] = level; self.tags.add("lowered")
        else:
            self.tags.add("min_skipped")

    def seed(self, m, pn, q):
        """pn: the SEED base index's positions as node numbers"""
        sel = m.mask(q["seed_base"], q["seed_clauses"]); m._f(q["seed_field"])
        for i in pn:
            if sel[i]:
                self.n_seed += 1
                if m.st[q["seed_field"]][i] == DATA:
                    self.insert(m.val[q["seed_field"]][i], 0)

    def seed_list(self, values, level=0, count=True):
        for v in np.asarray(values, np.int64).tolist():
            if v < -VAL_MAX or v > VAL_MAX:
                self.tags.add("skipped"); continue
            self.n_seed += 1 if count else 0
            self.insert(v, level)

    def prepare(self, m, pn, q):
        sel = m.mask(q["base"], q["clauses"]); m._f(q["link"]); m._f(q["key"])
        self.m, self.pn, self.q, self.sel = m, pn, q, sel
        self.link, self.depth = [EMPTY] * len(pn), [0] * len(pn)
        for p, i in enumerate(pn):
            have = m.st[q["link"]][i] == DATA
            if sel[i] and not have:
                self.tags.add("no_edge")
            if sel[i] and have:
                self.n_edges += 1
            if have and (sel[i] or self.defect == "unselected_passes"):
                self.link[p] = int(m.val[q["link"]][i])

    def round(self, r):
        if not self.map.fits() or self.new_keys[r - 1] == 0:
            self.tags.add("early_out"); return
        m, q = self.m, self.q
        for p, i in enumerate(self.pn):
            if self.link[p] == EMPTY or (self.depth[p] != 0 and self.defect != "overwrite_depth"):
                continue
            s = self.map._walk(self.link[p], False)
            if s is None:
                continue
            if self.map.vals[s] > (r if self.defect == "le_r" else r - 1):
                self.tags.add("same_round"); continue
            have = m.st[q["key"]][i] == DATA
            if not have:
                self.tags.add("keyless")
            if have or self.defect != "drop_keyless":
                self.depth[p] = r; self.tags.add("reached"); self.rounds = max(self.rounds, r); self.reached_at[r] += 1
            if have:
                self.insert(m.val[q["key"]][i], r)

    def levels(self):
        return {k: v for k, v in zip(self.map.keys, self.map.vals) if k != EMPTY}

    def finish(self, cap):
        """mask, emit and finish -> (ids, depths: the caller's buffers of cap + PAD entries, the result record)"""
        ids, dep, res = np.full(cap + PAD, FILL64, np.uint64), np.full(cap + PAD, FILL, np.uint8), np.zeros((), REACH_RES_DTYPE)
        fits, D = self.map.fits(), self.q["max_depth"]
        hit = [p for p in range(len(self.pn)) if self.depth[p] != 0 and self.sel[self.pn[p]]] if fits else []
        for k, p in enumerate(hit[:cap]):
            ids[k] = self.m.ids[self.pn[p]]; dep[k] = self.depth[p]
        more = self.reached_at[D] if self.defect == "more_from_reached" else self.new_keys[D]
        res["n_match"] = len(hit); res["set_size"] = self.map.claims; res["n_seed"] = self.n_seed; res["n_edges"] = self.n_edges
        res["rounds"] = self.rounds if fits else 0
        res["flags"] = (MORE if more else 0) if fits else OVERFLOW
        return ids, dep, res


def device_of(m, q, cap=None, defect=None, pn=None, seed_pn=None):
    """the stand-in's answer into pattern-filled buffers -> (ids, depths, res, the map's levels, the device: its tags)"""
    pn = np.arange(m.N) if pn is None else pn
    d = Device(q["set_cap"], defect)
    if q["kind"] == "from":
        d.seed_list(q["values"])
    else:
        d.seed(m, np.arange(m.N) if seed_pn is None else seed_pn, q)
    d.prepare(m, pn, q)
    for r in range(1, q["max_depth"] + 1):
        d.round(r)
    lv = d.levels()
    ids, dep, res = d.finish(len(pn) if cap is None else cap)
    return ids, dep, res, lv, d


# ---- the shapes the tests share ----
def uid(j):
    """a sparse key for number j (semi_model's)"""
    return sm.uid(j)


def graph(n, links, keys, base=None, salt=0, seeds=()):
    """a model of n nodes: links / keys are {node: value} (a node left out has no such row), base values default to the node number; `seeds`: nodes n.. carry the
    seed side (FI = its number, FS = the value) -> the model with n + len(seeds) nodes"""
    m = Model(wam.node_ids(n + len(seeds), 77000 + salt))
    i = np.arange(n)
    m.set(FB, i, i if base is None else np.asarray(base))
    for f, d in ((FL, links), (FK, keys)):
        if d:
            idx = np.array(sorted(d)); m.set(f, idx, np.array([d[k] for k in sorted(d)], np.int64))
        else:
            m._f(f)
    m._f(FI); m._f(FS); m._f(F1); m._f(F2)
    if len(seeds):
        j = np.arange(n, n + len(seeds))
        m.set(FI, j, np.arange(len(seeds))); m.set(FS, j, np.asarray(seeds, np.int64))
    return m


SEEDS_ALL = [[(FI, 0, 1 << 30)]]


def chain(n, seed=500):
    """node i links to the key of node i - 1; node 0 to the seed value"""
    return graph(n, {i: (seed if i == 0 else 1000 + i - 1) for i in range(n)}, {i: 1000 + i for i in range(n)}, seeds=[seed])


CUT = [[(FB, 0, 90)]]                                      # the program that cuts the zoo's nodes with base value 99
HAS_LINK, HAS_KEY = [[(FL, -VAL_MAX, VAL_MAX)]], [[(FK, -VAL_MAX, VAL_MAX)]]     # programs that probe the link / the key field themselves
ZOO_N = 54


def zoo(wide=False):
    """every small structure in one table (the comments give the depths from the seed value 500) -> (model, tombstones). wide: one more node whose values lie
    beyond int32, so every index over it switches to its int64 column."""
    V = VAL_MAX
    L = {0: 500, 1: 1000, 2: 1001,                                   # a chain: depths 1, 2, 3
         3: 1002, 4: 2002, 5: 2000, 6: 2001,                         # 3 enters a 3-ring 4 -> 5 -> 6 -> 4 at depth 4: 4 is reached once, at 5
         7: 3000, 8: 3001, 9: 1000,                                  # 7: a self-loop nobody enters; 8: a self-loop entered through 9's key: depths -, 3, 2
         10: 500, 11: 1001, 12: 4000,                                # 10 and 11 share the key 4000 at depths 1 and 3: 12 is at depth 2
         13: 500, 14: 500, 15: 5000, 16: 5001, 17: 5002,             # a diamond: depths 1, 1, 2, 2, 3
         18: 1000,                                                   # a keyless leaf at depth 2
         20: 500, 21: 500, 22: 6002,                                 # 19 has no link; 20's link is tombstoned; 21's key is: it is reached, 22 is not
         23: 500, 24: 7000,                                          # 23 has base value 99: CUT cuts it and 24 with it
         25: 500, 26: 0, 27: 1, 28: -1, 29: V, 30: -V}               # the keys 0, 1, -1, 2^53 - 1, -(2^53 - 1)
    K = {0: 1000, 1: 1001, 2: 1002, 3: 2002, 4: 2000, 5: 2001, 6: 2002, 7: 3000, 8: 3001, 9: 3001, 10: 4000, 11: 4000, 12: 4001, 13: 5000, 14: 5001, 15: 5002,
         16: 5002, 17: 5003, 19: 6000, 20: 6001, 21: 6002, 22: 6003, 23: 7000, 24: 7001, 25: 0, 26: 1, 27: -1, 28: V, 29: -V, 30: 8000}
    for i in range(31, 53):                                          # a star below the chain's end: depth 4
        L[i] = 1002; K[i] = 10000 + i
    n = ZOO_N if wide else ZOO_N - 1
    if wide:
        L[53] = WIDE; K[53] = WIDE + 1
    base = np.arange(n) % 90
    base[23] = 99
    if wide:
        base[53] = WIDE
    m = graph(n, L, K, base=base, salt=1 if wide else 0, seeds=[500, 501, 0, 0])       # 501: a seed nobody links to
    m.st[FS][n + 2] = ABSENT                                         # a seed node without seed value: counted, adds nothing
    return m, [(FL, np.array([20])), (FK, np.array([21])), (FS, np.array([n + 3]))]


def zoo_queries(m):
    """the program-form queries over zoo(); the set_cap cases are worked out from the model's own answer"""
    full = Q(FB, EVERY, FL, FK, FI, SEEDS_ALL, FS)
    K = answer(m, np.arange(m.N), full).set_size
    qs = [dict(full, max_depth=D) for D in (MAX_DEPTH, 1, 2, 3, 4, 5, 6)]
    qs += [dict(full, clauses=CUT), dict(full, clauses=HAS_LINK), dict(full, clauses=HAS_KEY)]                   # a cut subtree; link / key probed by the program too
    qs += [dict(full, base=FL), dict(full, base=FK), dict(full, base=FL, clauses=CUT)]                           # the link / the key from the column
    qs += [dict(full, link=FK, key=FL, seed_clauses=[[(FI, 3, 3)]]), dict(full, seed_clauses=[[(FI, 1, 1)]]),    # (a tombstoned seed) / a seed nobody links to
           dict(full, seed_clauses=[[(FI, 100, 200)]]), dict(full, seed_base=FS, seed_clauses=[[(FS, 500, 500)]])]   # an empty seed side; the seed value from the column
    qs += [dict(full, set_cap=K), dict(full, set_cap=K - 1), dict(full, set_cap=1), dict(full, set_cap=2, max_depth=1), dict(full, set_cap=7, max_depth=2)]
    return qs


def zoo_lists():
    """list-form queries over zoo(): the ancestors of two deep nodes (link and key swapped), duplicates and values outside the domain"""
    return [QFROM(FB, EVERY, FK, FL, [5003, 2001, 5003, EMPTY, VAL_MAX + 1]), QFROM(FB, EVERY, FK, FL, [10040], 3), QFROM(FB, CUT, FL, FK, [500] * 5 + [-VAL_MAX - 1]),
            QFROM(FB, EVERY, FL, FK, [VAL_MAX + 1, EMPTY]), QFROM(FB, EVERY, FL, FK, np.arange(400, 600), set_cap=199), QFROM(FB, EVERY, FL, FK, np.arange(400, 600), set_cap=300)]


def forest(n=2000, seed=20261020):
    """a random parent-pointer forest: key = the node's own sparse id, link = its parent's; some links dangle, some are absent, some get tombstoned, a few
    cycles, some keys absent; a third of the nodes fall outside the program [(FB, 0, 69)] -> (model, tombstones [(field, nodes)])"""
    rng = np.random.default_rng(seed)
    parent = np.where(np.arange(n) < 20, -1, (np.arange(n) * rng.random(n) * 0.999).astype(np.int64))    # parent < child, the first 20 are roots
    links = {i: int(uid(parent[i])) for i in range(n) if parent[i] >= 0}
    for i in rng.choice(n, 60, replace=False):
        links[int(i)] = int(uid(n + 5 + int(i)))                    # dangling
    for i in rng.choice(n, 60, replace=False):
        links.pop(int(i), None)                                     # absent
    for a in rng.choice(np.arange(100, n), 6, replace=False):       # cycles: an ancestor points down to a descendant
        b = int(a)
        for _ in range(3):
            b = int(parent[b]) if parent[b] >= 0 else b
        links[b] = int(uid(int(a)))
    keys = {i: int(uid(i)) for i in range(n)}
    for i in rng.choice(n, 80, replace=False):
        keys.pop(int(i))
    m = graph(n, links, keys, base=rng.integers(0, 100, n), salt=seed % 1000, seeds=[int(uid(r)) for r in range(20)] + [int(uid(n - 1 - 7 * r)) for r in range(20)])   # 20 roots, 20 deep nodes
    m.set(F1, np.arange(n), rng.integers(0, 10, n))
    tombs = [(FL, rng.choice(np.array(sorted(links)), 40, replace=False)), (FK, rng.choice(np.array(sorted(keys)), 40, replace=False))]
    return m, tombs


def apply_tombs(m, tombs):
    for f, idx in tombs:
        m.tomb(f, idx)


def forest_queries(count=60, n=2000, seed=20261021):
    """`count` (program-form query) over forest(): seeds from 1..20 roots or from inner nodes, varying max_depth, set_cap and edge programs; every fourth swaps
    link and key (the ancestors)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        lo = int(rng.integers(0, 15)) + (20 if k % 4 == 3 else 0); hi = lo + int(rng.integers(0, 6))     # (the ancestors: from the deep nodes)
        edge = [EVERY, [[(FB, 0, 69)]], [[(F1, 0, 7), (FB, 10, 99)], [(FB, 0, 4)]]][k % 3]
        D = [MAX_DEPTH, 1, 2, 3, 5, 8][k % 6]
        cap = 4096 if k % 5 else int(rng.integers(2, 60))
        q = Q(FB, edge, FL, FK, FI, [[(FI, lo, hi)]], FS, D, cap)
        if k % 4 == 3:
            q["link"], q["key"] = FK, FL
        out.append(q)
    return out
