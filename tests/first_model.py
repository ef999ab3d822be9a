"""A model of the first node per group (include/bmx_first.h, csrc/first_kernels.h), shared by test_first_model.py (CPU) and the GPU tests (helper, not a test).
The table and the selection are where_agg_model's (a state per field and node: absent, data, tombstone).

Three parts:

answer(m, base, clauses, group, order, fields, desc, cap, with_ts, clock) : the brute force, through Python dicts and ints (ids compare as unsigned Python
    ints) -> (records sorted by key, vals, ts, result record); on overflow no records. clock(f, node) -> the clock of a cell that is not absent; the default is
    what where_agg_model.load / tombstone write (5 for data, 9 for a tombstone).

Device(...) : a sequential stand-in of the three kernels. Pass 1 is group_model.Device with the order value as the measure (the cache, the bypass, the flush, the
    walks and their tags are its own), plus the wave's count combine ('combine'). Pass 2 walks the finished table with plain reads ('resolve_home',
    'resolve_walk', 'resolve_wrap'), compares with the key's extreme and lowers the id word ('resolve_first', 'resolve_tie' for every further contender on the
    extreme, 'resolve_skip' for a contender off it). Pass 3 ranks, writes and resets. The id words outlive a query, as the scratch does. defect: None or one of
    DEFECTS, each of which some edge layout exposes (test_first_model.py asserts it).

edge_layouts(wide) : group_model.edge_layouts with order values on top, and the layouts that pin the winner's place."""
import numpy as np

import group_model as gm
import where_agg_model as wam
from where_agg_model import DATA, TOMB, Model  # noqa: F401

FIRST_DTYPE = np.dtype([("key", "<i8"), ("id", "<u8"), ("val", "<i8"), ("n_match", "<u8"), ("n", "<u8")])
FIRST_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("flags", "<u4"), ("reserved", "<u4"), ("total", "<u8"), ("absent", "<u8"), ("n_ordered", "<u8")])
OVERFLOW, MAX_CAP, DESC, TS = 1, 1 << 20, 2, 1
NO_NODE = (1 << 64) - 1
VAL_DELETED = -(1 << 63)
NO_CLOCK = -1
FILL = 0x5A
DEFECTS = ("signed_id", "desc_flips_id", "noncontender_wins", "unselected_wins", "idw_not_reset")


def default_clock(m):
    return lambda f, i: 5 if m.st[f][i] == DATA else 9


def cell(m, f, i, clock):
    """(value, clock) of field f on node i (None: no node) in the three states of bmx_rows.h"""
    if i is None:
        return VAL_DELETED, NO_CLOCK
    m._f(f)
    st = m.st[f][i]
    if st == DATA:
        return int(m.val[f][i]), int(clock(f, i))
    if st == TOMB:
        return VAL_DELETED, int(clock(f, i))
    return VAL_DELETED, NO_CLOCK


def before(a, b, desc):
    """does (val, id) a come before b? val ascending (descending with desc), then id ascending as an unsigned number (Python ints)"""
    if a[0] != b[0]:
        return a[0] > b[0] if desc else a[0] < b[0]
    return a[1] < b[1]


def _pack(groups, winners, m, fields, with_ts, clock, cap, total, absent):
    """groups: {key: [n_match, n, (val, id) or None]}; winners: {key: node or None}"""
    res = np.zeros((), FIRST_RES_DTYPE)
    res["total"] = total; res["absent"] = absent; res["n_ordered"] = sum(g[1] for g in groups.values()); res["n_groups"] = len(groups)
    nf = len(fields)
    if len(groups) > cap:
        res["flags"] = OVERFLOW
        return np.zeros(0, FIRST_DTYPE), np.zeros((nf, 0), np.int64), np.zeros((nf, 0), np.int64) if with_ts else None, res
    keys = sorted(groups)
    out = np.zeros(len(keys), FIRST_DTYPE)
    vals = np.zeros((nf, len(keys)), np.int64); ts = np.zeros((nf, len(keys)), np.int64)
    for r, k in enumerate(keys):
        nm, n, best = groups[k]
        out[r] = (k, best[1] if best else NO_NODE, best[0] if best else VAL_DELETED, nm, n)
        for j, f in enumerate(fields):
            vals[j, r], ts[j, r] = cell(m, f, winners[k], clock)
    return out, vals, ts if with_ts else None, res


def answer(m, base, clauses, group, order, fields=(), desc=False, cap=65536, with_ts=False, clock=None):
    clock = clock or default_clock(m)
    sel = m.mask(base, clauses)
    m._f(group); m._f(order)
    groups, winners = {}, {}
    total = absent = 0
    for i in np.nonzero(sel)[0]:
        i = int(i)
        total += 1
        if m.st[group][i] != DATA:
            absent += 1
            continue
        k = int(m.val[group][i])
        g = groups.setdefault(k, [0, 0, None]); winners.setdefault(k, None)
        g[0] += 1
        if m.st[order][i] == DATA:
            g[1] += 1
            c = (int(m.val[order][i]), int(m.ids[i]))
            if g[2] is None or before(c, g[2], desc):
                g[2] = c; winners[k] = i
    return _pack(groups, winners, m, fields, with_ts, clock, cap, total, absent)


def invariant(recs, res):
    return int(recs["n_match"].sum()) + int(res["absent"]) == int(res["total"]) and int(recs["n"].sum()) == int(res["n_ordered"])


def check(got, want, cap, nf, with_ts, host=True):
    """got: (whole record buffer of cap + 1 records, vals buffer (nf, cap + 1) or None, ts buffer or None, result record), all pattern-filled before the call;
    want: answer(). Every byte of every record and of res, every cell and clock, the sorted order, the pattern behind row D and on overflow -> None or what
    differs."""
    grecs, gvals, gts, gres = got
    wrecs, wvals, wts, wres = want
    grecs = np.asarray(grecs, FIRST_DTYPE)
    cols = [c for c in ((gvals,) if nf else ()) + ((gts,) if nf and with_ts else ())]
    for k in ("total", "absent", "n_ordered"):
        if int(gres[k]) != int(wres[k]):
            return (k, int(gres[k]), int(wres[k]))
    if int(gres["reserved"]) != 0:
        return ("reserved", int(gres["reserved"]))
    if int(wres["flags"]) & OVERFLOW:
        if int(gres["flags"]) != OVERFLOW or not (cap < int(gres["n_groups"]) <= int(wres["n_groups"])):
            return ("overflow", int(gres["flags"]), int(gres["n_groups"]))
        if not (grecs.view(np.uint8) == FILL).all() or not all((c.view(np.uint8) == FILL).all() for c in cols):
            return ("written on overflow",)
        return None
    if gres.tobytes() != wres.tobytes():
        return ("res", gres, wres)
    d = len(wrecs)
    if not (grecs[d:].view(np.uint8) == FILL).all() or not all((c[:, d:].view(np.uint8) == FILL).all() for c in cols):
        return ("written at or beyond row D",)
    if nf and not with_ts and gts is not None and not (gts.view(np.uint8) == FILL).all():
        return ("out_ts written without BMX_ROWS_TS",)
    g = grecs[:d]
    if host and not np.array_equal(g["key"], np.sort(g["key"])):
        return ("host records not sorted by key",)
    o = np.argsort(g["key"], kind="stable")
    g = g[o]
    if g.tobytes() != wrecs.tobytes():
        bad = [i for i in range(d) if g[i].tobytes() != wrecs[i].tobytes()]
        return ("record", bad[0], g[bad[0]], wrecs[bad[0]])
    if nf and not np.array_equal(gvals[:, :d][:, o], wvals):
        return ("cells", gvals[:, :d][:, o], wvals)
    if nf and with_ts and not np.array_equal(gts[:, :d][:, o], wts):
        return ("clocks", gts[:, :d][:, o], wts)
    if not invariant(g, gres):
        return ("invariant",)
    return None


def merge(lists, desc):
    """bmx.first_merge"""
    import bmx
    return bmx.first_merge(lists, desc)


# ---- the sequential stand-in of the three kernels ----
def _signed(x):
    return x - (1 << 64) if x >= (1 << 63) else x


class Device:
    """Queries over columns laid out by position, on one scratch (the id words persist between run() calls as they do on the device)."""

    def __init__(self, defect=None, cus=256):
        assert defect is None or defect in DEFECTS
        self.defect, self.cus = defect, cus
        self.idw = {}                                  # slot -> id word below NO_NODE
        self.tags = set(); self.row_tags = {}

    def _id_less(self, a, b, desc):
        if self.defect == "signed_id":
            return _signed(a) < _signed(b)
        if self.defect == "desc_flips_id" and desc:
            return a > b
        return a < b

    def run(self, n, E, cap, sel, gkey, oval, ids, desc=False):
        """sel[pos]: bool; gkey[pos] / oval[pos]: int or None; ids[pos]: int. -> (records in table order as [key, id, val, n_match, n, winner pos or None],
        fits, n_groups, total, absent, n_ordered)"""
        sel = np.asarray(sel, bool)
        # pass 1: group_model.Device with measure = order value
        d = gm.Device(n, E, cap, True, self.cus)
        d.run(sel, gkey, oval)
        self.tags |= d.tags; self.row_tags = d.row_tags
        wg, wave, lane, step = gm.place(np.arange(n), n, E, self.cus)
        calls = {}                                     # one call of the row code by one wave -> [(lane, key)] of its rows that go to a record
        for p in range(n):
            if sel[p] and gkey[p] is not None:
                calls.setdefault((int(wg[p]), int(wave[p]), int(step[p])), []).append((int(lane[p]), gkey[p]))
        for rows in calls.values():
            rows.sort()
            if any(k == rows[0][1] for _, k in rows[1:]):
                self.tags.add("combine")               # lanes that hold the first lane's key add their count once
        fits = d.claims <= cap and not d.overflow
        slot_of = {k: s for s, k in d.table.items()}
        who = {}
        # pass 2: plain reads of the finished table
        if fits or self.defect == "idw_not_reset":
            for p in range(n):
                k, v = gkey[p], oval[p]
                cont = sel[p] and k is not None and v is not None
                if self.defect == "unselected_wins":
                    cont = k is not None and v is not None and k in slot_of
                if self.defect == "noncontender_wins" and sel[p] and k in slot_of and v is None and d.acc[slot_of[k]].vals:
                    cont = True; v = (max if desc else min)(d.acc[slot_of[k]].vals)
                if not cont or k not in slot_of:
                    continue
                h = gm.home(k, d.slots)
                for q in range(d.slots):
                    s = (h + q) & (d.slots - 1)
                    if d.table.get(s) == k:
                        self.tags.add("resolve_home" if q == 0 else ("resolve_wrap" if h + q >= d.slots else "resolve_walk"))
                        break
                vals = d.acc[s].vals
                if not vals or v != (max if desc else min)(vals):
                    self.tags.add("resolve_skip")
                    continue
                self.tags.add("resolve_tie" if s in who else "resolve_first")
                who.setdefault(s, None)
                if s not in self.idw or self._id_less(int(ids[p]), self.idw[s], desc):
                    self.idw[s] = int(ids[p]); who[s] = p
        # pass 3
        recs = []
        if fits:
            for s, k in d.table.items():
                a = d.acc[s]
                nn = len(a.vals)
                recs.append([k, self.idw.get(s, NO_NODE) if nn else NO_NODE, (max if desc else min)(a.vals) if nn else VAL_DELETED, a.nm, nn, who.get(s) if nn else None])
        if fits or self.defect != "idw_not_reset":
            self.idw = {}
        return recs, fits, d.claims, d.total.nm, d.absent.nm, len(d.total.vals) - len(d.absent.vals)


def device_answer(dev, m, node, n, E, cap, base, clauses, group, order, fields=(), desc=False, with_ts=False, clock=None):
    """one query of the stand-in over the model's table in position order (node: node numbers of the positions) -> what answer() returns"""
    clock = clock or default_clock(m)
    sel, gk, ov = gm.rows_of(m, base, clauses, group, order, node)
    ids = [int(x) for x in m.ids[node]]
    recs, fits, claims, total, absent, n_ordered = dev.run(n, E, cap, sel, gk, ov, ids, desc)
    res = np.zeros((), FIRST_RES_DTYPE)
    res["total"] = total; res["absent"] = absent; res["n_ordered"] = n_ordered; res["n_groups"] = claims
    nf = len(fields)
    if not fits:
        res["flags"] = OVERFLOW
        return np.zeros(0, FIRST_DTYPE), np.zeros((nf, 0), np.int64), np.zeros((nf, 0), np.int64) if with_ts else None, res
    recs.sort(key=lambda r: r[0])
    out = np.zeros(len(recs), FIRST_DTYPE)
    vals = np.zeros((nf, len(recs)), np.int64); ts = np.zeros((nf, len(recs)), np.int64)
    by_id = {int(x): i for i, x in enumerate(m.ids)}
    for r, x in enumerate(recs):
        out[r] = tuple(x[:5])
        for j, f in enumerate(fields):
            vals[j, r], ts[j, r] = cell(m, f, by_id.get(x[1]), clock)
    return out, vals, ts if with_ts else None, res


def same_answer(a, b):
    return (a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and (a[2] is None) == (b[2] is None) and (a[2] is None or np.array_equal(a[2], b[2]))
            and a[3].tobytes() == b[3].tobytes())


# ---- helpers of the GPU tests ----
def raw_first(x, base, clauses, group, order, fields=(), desc=False, with_ts=False, cap=64, flags=None):
    """bmx_where_group_first (Engine) / bmx_comm_where_group_first (Comm), host memory, into pattern-filled buffers of cap + 1 rows -> (records, vals, ts, res)"""
    import bmx
    nf = len(fields)
    out = np.full(40 * (cap + 1), FILL, np.uint8).view(FIRST_DTYPE)
    vals = np.full((max(nf, 1), cap + 1), FILL * 0x0101010101010101, np.int64)
    ts = np.full((max(nf, 1), cap + 1), FILL * 0x0101010101010101, np.int64)
    res = np.full(40, FILL, np.uint8).view(FIRST_RES_DTYPE)
    tail = list(bmx._first_tail(group, order, fields, desc, with_ts))
    if flags is not None:
        tail[4] = flags
    # the columns have stride cap: hand the library views of cap columns, keep the (cap + 1)-th column of the buffers as the guard
    v2 = np.full((max(nf, 1) * cap + cap + 1,), FILL * 0x0101010101010101, np.int64); t2 = v2.copy()
    args = (*bmx._where_args(base, clauses), *tail, int(cap), bmx._ptr(out), bmx._ptr(v2), bmx._ptr(t2) if with_ts else None, bmx._ptr(res))
    x._chk(x.L.bmx_where_group_first(x.h, *args, bmx.MEM_HOST) if isinstance(x, bmx.Engine) else x.L.bmx_comm_where_group_first(x.h, *args))
    assert (v2[nf * cap:] == FILL * 0x0101010101010101).all() and (t2[nf * cap:] == FILL * 0x0101010101010101).all(), "nothing is written behind the last column"
    for f in range(nf):
        vals[f, :cap] = v2[f * cap:(f + 1) * cap]; ts[f, :cap] = t2[f * cap:(f + 1) * cap]
    return out, vals[:nf], ts[:nf], res[0]


def ask(x, m, base, clauses, group, order, fields=(), desc=False, with_ts=False, cap=64, clock=None):
    """one query checked against the brute force -> answer()'s tuple"""
    got = raw_first(x, base, clauses, group, order, fields, desc, with_ts, cap)
    want = answer(m, base, clauses, group, order, fields, desc, cap, with_ts, clock)
    bad = check(got, want, cap, len(fields), with_ts)
    assert bad is None, (clauses, group, order, fields, desc, with_ts, cap, bad)
    return want


# ---- the edge suite: columns laid out by position ----
def edge_layouts(wide):
    """-> [dict(name, n, cap, keys, present, sel, oval, has_o (all by position), tags (what the stand-in must reach), winner (None, or {key: position}))]"""
    E = 2 if wide else 4
    rnd = gm.THREADS * gm.U * E
    start = gm.WIDE if wide else 1
    L = []
    for lay in gm.edge_layouts(wide):
        n = lay["n"]
        pos = np.arange(n)
        lay = dict(lay)
        lay["oval"] = (pos * 7) % 5 - 2                # few values: every key with several members ties on its extreme
        lay["has_o"] = pos % 6 != 1
        lay["tags"] = {t for t in lay["tags"]} | ({"resolve_first"} if lay["sel"].any() and "noroom" not in lay["tags"] and ("len", 63) not in lay["tags"] and n > 1 else set())
        lay["winner"] = None
        L.append(lay)

    def add(name, n, keys, oval, win, tags=(), cap=8, sel=None, has_o=None, fix=None):
        L.append(dict(name=name, n=n, cap=cap, keys=np.asarray(keys, np.int64), present=np.ones(n, bool), sel=np.ones(n, bool) if sel is None else sel,
                      oval=np.asarray(oval, np.int64), has_o=np.ones(n, bool) if has_o is None else has_o, tags=set(tags) | {"resolve_first"}, winner=win, base=False, fix=fix))

    n = 64 * E * 3
    lane = gm.place(np.arange(n), n, E)[2]
    for ln in (0, 63):
        p = int(np.nonzero(lane == ln)[0][E + 1])
        ov = np.full(n, 10); ov[p] = -3
        add("winner_lane_%d" % ln, n, np.full(n, start + 2), ov, {start + 2: p}, {"resolve_skip", "combine"})
    for name, n, p in (("winner_first_pos", rnd + 1, 0), ("winner_last_pos", rnd + 1, rnd), ("winner_ragged_unit", 64 * E + 1, 64 * E)):
        ov = 100 + np.arange(n) % 9; ov[p] = 99
        add(name, n, start + np.arange(n) % 3, ov, {start + p % 3: p}, {"resolve_skip"})
    n = 4 * rnd + 1 + 64 * E
    wg = gm.place(np.arange(n), n, E)[0]
    assert gm.grid(n, E) == 2
    a, b = int(np.nonzero(wg == 0)[0][77]), int(np.nonzero(wg == 1)[0][5])
    ov = np.full(n, 50); ov[[a, b]] = 7
    add("extreme_in_two_workgroups", n, np.full(n, start + 4), ov, None, {"resolve_tie"})
    ks = gm.keys_with_set(9, 6, start)
    pos = np.arange(300)
    add("extreme_cached_and_bypass", 300, np.array(ks)[pos % 6], 40 - pos // 6, None, {"hit", "bypass", "resolve_skip"})
    n = 64 * E
    add("wave_all_tie", n, np.full(n, start + 9), np.full(n, -(2**53 - 1)), None, {"resolve_tie", "combine"})
    ov = np.full(n, 3)
    add("member_without_order_first", n, np.full(n, start), ov, None, {"resolve_tie"}, has_o=np.arange(n) % 2 == 1, fix="no_order")
    add("unselected_ties", n, np.full(n, start), ov, None, {"resolve_tie"}, sel=np.arange(n) % 2 == 0, fix="unselected")
    return L


# ---- names, layouts as models, the seeded suite ----
def names():
    from oracle import streams
    f = {k: streams.fnv1a32("first." + k) for k in ("base", "group", "order", "select", "nobody", "one", "two", "three", "extra")}
    return f


def lay_fill(m, lay, node, F):
    """the layout's columns onto the model's nodes; node[pos]: the node at index position pos (the base field is set by the caller). fix: the node with the
    smallest id loses its order value ('no_order') or its selection ('unselected'): it would win if it counted. -> (sel, has_o) by position as laid out"""
    pr, sel, has_o = lay["present"], lay["sel"].copy(), lay["has_o"].copy()
    if lay.get("fix"):
        p = int(np.argmin(m.ids[node]))
        (has_o if lay["fix"] == "no_order" else sel)[p] = False
    m.set(F["group"], node[pr], lay["keys"][pr])
    if sel.any():
        m.set(F["select"], node[sel], np.ones(int(sel.sum()), np.int64))
    m.set(F["order"], node[has_o], lay["oval"][has_o])
    return sel, has_o


N_SEED, SEED_TABLE, SEED_PROGS, N_PROGS = 2000, 424242, 20251020, 60
BIG = 2**53 - 1


def seeded_model():
    """2000 nodes: a base field 0..11, three probed fields 0..5 in all three states, a group field of 40 sparse values over +-(2^53 - 1) (among them 0, +-1,
    +-(2^53 - 1)) in all three states, and an order field of few values (ties) that the members of four of the group values never hold (n == 0)."""
    F = names()
    rng = np.random.default_rng(SEED_TABLE)
    n = N_SEED
    m = Model(wam.node_ids(n, 515000))
    m.set(F["base"], np.arange(n), rng.integers(0, 12, n))
    tombs = {}
    for k, pr in (("one", 0.9), ("two", 0.6), ("three", 0.4)):
        idx = np.nonzero(rng.random(n) < pr)[0]
        m.set(F[k], idx, rng.integers(0, 6, len(idx))); tombs[F[k]] = idx[rng.random(len(idx)) < 0.1]
    pool = np.concatenate([[0, 1, -1, BIG, -BIG], rng.integers(-BIG, BIG, 35)])
    idx = np.nonzero(rng.random(n) < 0.85)[0]
    gi = rng.integers(0, len(pool), len(idx))
    m.set(F["group"], idx, pool[gi]); tombs[F["group"]] = idx[rng.random(len(idx)) < 0.08]
    has = idx[(gi >= 4) & (rng.random(len(idx)) < 0.8)]          # the members of pool[0 .. 3] never hold the order field
    m.set(F["order"], has, rng.choice(np.array([0, 1, -1, BIG, -BIG, 7, 7, 7]), len(has))); tombs[F["order"]] = has[rng.random(len(has)) < 0.1]
    return m, tombs


def has_tie_and_empty(m, base, p, group, order, desc):
    """does the brute force see a group with two contenders on its extreme, and a group with members and no contender?"""
    recs, _, _, res = answer(m, base, p, group, order, (), desc, 1 << 20)
    if not len(recs) or not (recs["n"] == 0).any():
        return False
    sel = m.mask(base, p) & (m.st[group] == DATA) & (m.st[order] == DATA)
    for r in recs[recs["n"] >= 2]:
        if int((sel & (m.val[group] == r["key"]) & (m.val[order] == r["val"])).sum()) >= 2:
            return True
    return False


def seeded_queries(m):
    """-> N_PROGS x (clauses, group field, order field, desc): seeded programs, kept only if they give the brute force a tie on an extreme and a group with
    n == 0 (m: seeded_model()'s table with its tombstones applied). The programs name the base field, three probed fields and, some of them, the group and the
    order field; every other one is descending."""
    F = names()
    probed = [F[k] for k in ("one", "two", "three")]
    out, seed = [], SEED_PROGS
    while len(out) < N_PROGS:
        for p in wam.random_programs(8, seed, F["base"], probed + [F["group"], F["order"]], [F["extra"], F["select"], F["nobody"]])[:7]:
            k = len(out)
            desc = k % 2 == 1
            if k < N_PROGS and has_tie_and_empty(m, F["base"], p, F["group"], F["order"], desc):
                out.append((p, F["group"], F["order"], desc))
        seed += 1
    return out
