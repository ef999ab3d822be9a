"""A model of the first N nodes per group (include/bmx_group_top.h, csrc/gtop_kernels.h), shared by test_gtop_model.py (CPU) and the GPU tests (helper, not a
test). The table and the selection are where_agg_model's, the cells, the order and pass 1 first_model's, the table walk group_model's.

Parts:

ranked(m, base, clauses, group, order, desc) : per key the members, the contenders and the contenders in order, through Python dicts and ints.
answer(m, base, clauses, group, order, per, fields, desc, cap, with_ts, clock) : the brute force -> (groups sorted by key, rows (D, per), vals (nf, D, per), ts,
    result record); on overflow no groups.

Device(...) : a sequential stand-in of the round kernels. Round 0 is first_model.Device (pass 1, the resolve pass and their tags are its own); then per round
    the value sweep, the id sweep and the advance over the per-key state (previous winner, round extreme, rank counter, winner pairs), which outlives a query
    as the scratch does. Path tags: 'round_first' (a round's first candidate on the extreme), 'tie_kept' (a candidate on the round's extreme that does not win:
    it is kept for the next round), 'at_prev' / 'before_prev' / 'after_prev' (a contender at, before and after the previous winner), 'exhausted' (a group that
    a round gives nothing), 'padding' (a row without a node). defect: None or one of DEFECTS, each of which some edge layout exposes (test_gtop_model.py asserts
    it).

check() : every byte of groups, rows, cells, clocks and res, the fill pattern behind group D and on overflow, the sorted order.
edge_layouts(wide) : first_model.edge_layouts with per = 3, and the layouts that pin the ranks' places in the round kernels' geometry.
seeded_queries(m, per) : 60 seeded programs per `per`, each with a tie at the cut, a short group, a group with n = 0 and a tie on an extreme."""
import functools

import numpy as np

import first_model as fm
import group_model as gm
import where_agg_model as wam
from first_model import NO_NODE, VAL_DELETED, NO_CLOCK, cell, default_clock, names, seeded_model, lay_fill  # noqa: F401
from where_agg_model import DATA, TOMB, Model  # noqa: F401

GRP_DTYPE = np.dtype([("key", "<i8"), ("n_match", "<u8"), ("n", "<u8"), ("n_rows", "<u8")])
ROW_DTYPE = np.dtype([("id", "<u8"), ("val", "<i8")])
RES_DTYPE = np.dtype([("n_groups", "<u8"), ("flags", "<u4"), ("per", "<u4"), ("total", "<u8"), ("absent", "<u8"), ("n_ordered", "<u8"), ("n_rows", "<u8")])
OVERFLOW, MAX_CAP, MAX_PER, MAX_ROWS, DESC, TS = 1, 1 << 20, 16, 1 << 22, 2, 1
FILL = 0x5A
FILL64 = FILL * 0x0101010101010101
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
ROUND_THREADS = 256                              # k_gtop_value / k_gtop_id: positions 2q and 2q + 1 run on lane q % 64 of workgroup (q // 256) % grid
DEFECTS = ("signed_id", "desc_flips_id", "after_value_only", "after_not_strict", "ext_not_reset", "exhausted_repeats", "noncontender_wins", "unselected_wins",
           "state_not_reset")
TAGS = {"round_first", "tie_kept", "at_prev", "before_prev", "after_prev", "exhausted", "padding"}


def round_grid(n, cus=256):
    return max(1, min((n + 8 * ROUND_THREADS - 1) // (8 * ROUND_THREADS), 2 * cus))


def round_place(pos, n, cus=256):
    """where position pos runs in the round kernels -> (workgroup, lane)"""
    q = np.asarray(pos, np.int64) // 2
    return (q // ROUND_THREADS) % round_grid(n, cus), q % 64


def order_key(val, nid, desc):
    """the total order as a Python sort key: the value ascending (descending with desc), then the id ascending as an unsigned number"""
    return (-val if desc else val, nid)


def ranked(m, base, clauses, group, order, desc):
    """-> ({key: [n_match, n, [(val, id, node) in order]]}, total, absent)"""
    sel = m.mask(base, clauses)
    m._f(group); m._f(order)
    groups = {}
    total = absent = 0
    for i in np.nonzero(sel)[0]:
        i = int(i)
        total += 1
        if m.st[group][i] != DATA:
            absent += 1
            continue
        g = groups.setdefault(int(m.val[group][i]), [0, 0, []])
        g[0] += 1
        if m.st[order][i] == DATA:
            g[1] += 1
            g[2].append((int(m.val[order][i]), int(m.ids[i]), i))
    for g in groups.values():
        g[2].sort(key=lambda c: order_key(c[0], c[1], desc))
    return groups, total, absent


def _pack(groups, m, per, fields, with_ts, clock, cap, total, absent):
    """groups: {key: [n_match, n, [(val, id, node or None) in order, at least min(per, n) of them]]}"""
    res = np.zeros((), RES_DTYPE)
    res["total"] = total; res["absent"] = absent; res["n_ordered"] = sum(g[1] for g in groups.values()); res["n_groups"] = len(groups); res["per"] = per
    nf = len(fields)
    if len(groups) > cap:
        res["flags"] = OVERFLOW
        return np.zeros(0, GRP_DTYPE), np.zeros((0, per), ROW_DTYPE), np.zeros((nf, 0, per), np.int64), np.zeros((nf, 0, per), np.int64) if with_ts else None, res
    keys = sorted(groups)
    out = np.zeros(len(keys), GRP_DTYPE)
    rows = np.zeros((len(keys), per), ROW_DTYPE)
    rows["id"] = NO_NODE; rows["val"] = VAL_DELETED
    vals = np.full((nf, len(keys), per), VAL_DELETED, np.int64); ts = np.full((nf, len(keys), per), NO_CLOCK, np.int64)
    for r, k in enumerate(keys):
        nm, n, cont = groups[k]
        nr = min(per, len(cont))
        out[r] = (k, nm, n, nr)
        for j in range(nr):
            rows[r, j] = (cont[j][1], cont[j][0])
            for f, fld in enumerate(fields):
                vals[f, r, j], ts[f, r, j] = cell(m, fld, cont[j][2], clock)
    res["n_rows"] = int(out["n_rows"].sum())
    return out, rows, vals, ts if with_ts else None, res


def answer(m, base, clauses, group, order, per, fields=(), desc=False, cap=65536, with_ts=False, clock=None):
    clock = clock or default_clock(m)
    groups, total, absent = ranked(m, base, clauses, group, order, desc)
    return _pack(groups, m, per, fields, with_ts, clock, cap, total, absent)


def invariant(grps, rows, res):
    return (int(grps["n_match"].sum()) + int(res["absent"]) == int(res["total"]) and int(grps["n"].sum()) == int(res["n_ordered"])
            and int(grps["n_rows"].sum()) == int(res["n_rows"]) == int((rows["id"] != np.uint64(NO_NODE)).sum())
            and (grps["n_rows"] == np.minimum(grps["n"], np.uint64(int(res["per"])))).all())


def same_answer(a, b):
    return (a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]) and (a[3] is None) == (b[3] is None)
            and (a[3] is None or np.array_equal(a[3], b[3])) and a[4].tobytes() == b[4].tobytes())


def check(got, want, cap, per, nf, with_ts, host=True):
    """got: (group buffer of cap + 1 groups, row buffer of (cap + 1) * per rows, vals buffer (nf, (cap + 1) * per) or None, ts buffer or None, result record), all
    pattern-filled before the call; want: answer(). Every byte of every group, row and of res, every cell and clock, the sorted order, the pattern behind group D
    and on overflow -> None or what differs."""
    ggrp, grow, gvals, gts, gres = got
    wgrp, wrow, wvals, wts, wres = want
    ggrp = np.asarray(ggrp, GRP_DTYPE); grow = np.asarray(grow, ROW_DTYPE).reshape(-1)
    cols = [c for c in ((gvals,) if nf else ()) + ((gts,) if nf and with_ts else ())]
    for k in ("total", "absent", "n_ordered", "per"):
        if int(gres[k]) != int(wres[k]):
            return (k, int(gres[k]), int(wres[k]))
    if int(wres["flags"]) & OVERFLOW:
        if int(gres["flags"]) != OVERFLOW or not (cap < int(gres["n_groups"]) <= int(wres["n_groups"])) or int(gres["n_rows"]) != 0:
            return ("overflow", int(gres["flags"]), int(gres["n_groups"]), int(gres["n_rows"]))
        if not (ggrp.view(np.uint8) == FILL).all() or not (grow.view(np.uint8) == FILL).all() or not all((c.view(np.uint8) == FILL).all() for c in cols):
            return ("written on overflow",)
        return None
    if gres.tobytes() != wres.tobytes():
        return ("res", gres, wres)
    d = len(wgrp)
    if not (ggrp[d:].view(np.uint8) == FILL).all() or not (grow[d * per:].view(np.uint8) == FILL).all() or not all((c[:, d * per:].view(np.uint8) == FILL).all() for c in cols):
        return ("written at or beyond group D",)
    if nf and not with_ts and gts is not None and not (gts.view(np.uint8) == FILL).all():
        return ("out_ts written without BMX_ROWS_TS",)
    g = ggrp[:d]
    if host and not np.array_equal(g["key"], np.sort(g["key"])):
        return ("host groups not sorted by key",)
    o = np.argsort(g["key"], kind="stable")
    g = g[o]
    if g.tobytes() != wgrp.tobytes():
        bad = [i for i in range(d) if g[i].tobytes() != wgrp[i].tobytes()]
        return ("group", bad[0], g[bad[0]], wgrp[bad[0]])
    r = grow[:d * per].reshape(d, per)[o]
    if r.tobytes() != wrow.tobytes():
        bad = [i for i in range(d) if r[i].tobytes() != wrow[i].tobytes()]
        return ("rows", bad[0], g[bad[0]], r[bad[0]], wrow[bad[0]])
    if nf and not np.array_equal(gvals[:, :d * per].reshape(nf, d, per)[:, o], wvals):
        return ("cells", gvals[:, :d * per].reshape(nf, d, per)[:, o], wvals)
    if nf and with_ts and not np.array_equal(gts[:, :d * per].reshape(nf, d, per)[:, o], wts):
        return ("clocks", gts[:, :d * per].reshape(nf, d, per)[:, o], wts)
    if not invariant(g, r, gres):
        return ("invariant",)
    return None


def merge(lists, per, desc):
    """bmx.gtop_merge"""
    import bmx
    return bmx.gtop_merge(lists, per, desc)


# ---- the sequential stand-in of the round kernels ----
class _Slot:
    __slots__ = ("pv", "pid", "ext", "rank", "win", "idw", "who")

    def __init__(self):
        self.pv, self.pid, self.ext, self.rank, self.win, self.idw, self.who = I64MIN, 0, I64MAX, 0, {}, None, None


class Device:
    """Queries over columns laid out by position, on one scratch (the per-key state persists between run() calls as the per-slot state does on the device: a
    key keeps its slot as long as the table keeps its size)."""

    def __init__(self, defect=None, cus=256):
        assert defect is None or defect in DEFECTS
        self.defect, self.cus = defect, cus
        self.first = fm.Device(defect if defect in ("signed_id", "desc_flips_id") else None, cus)
        self.state = {}                                # key -> _Slot that is not at rest
        self.tags = set(); self.first_tags = set()

    def _id_less(self, a, b, desc):
        return self.first._id_less(a, b, desc)

    def _after(self, ov, nid, st, desc):
        """is (ov, nid) strictly after the slot's previous winner?"""
        if ov != st.pv:
            self.tags.add("after_prev" if ov > st.pv else "before_prev")
            return ov > st.pv
        if nid == st.pid:
            self.tags.add("at_prev")
            return self.defect == "after_not_strict"
        later = self._id_less(st.pid, nid, desc)
        self.tags.add("after_prev" if later else "before_prev")
        return later and self.defect != "after_value_only"

    def run(self, n, E, cap, per, sel, gkey, oval, ids, desc=False):
        """sel[pos]: bool; gkey[pos] / oval[pos]: int or None; ids[pos]: int. -> (groups in table order as [key, n_match, n, n_rows, [(id, val, pos)] * per with
        None for padding], fits, n_groups, total, absent, n_ordered)"""
        sel = np.asarray(sel, bool)
        recs, fits, claims, total, absent, n_ordered = self.first.run(n, E, cap, sel, gkey, oval, ids, desc)
        self.first_tags |= self.first.tags
        keys = {r[0] for r in recs}
        cont = []                                      # what the words of pass 1 say, per position: (pos, key, ov, id)
        for p in range(n):
            k, v = gkey[p], oval[p]
            ok = bool(sel[p]) and k is not None and v is not None
            if self.defect == "unselected_wins":
                ok = k is not None and v is not None
            if self.defect == "noncontender_wins" and sel[p] and k is not None and v is None:
                ok = True; v = None                    # (its value: the previous winner's, below)
            if ok and k in keys:
                cont.append((p, k, None if v is None else (-v if desc else v), int(ids[p])))
        given = 0
        for round_ in range(per if fits else 0):
            if round_ and not given:
                break                                  # (uniform) nothing can follow
            if round_ == 0:
                for r in recs:                         # the table's extreme and k_first_resolve's id word
                    if r[4]:
                        st = self.state.setdefault(r[0], _Slot())
                        st.idw, st.ext, st.who = r[1], (-r[2] if desc else r[2]), r[5]
            else:
                for sweep in ("value", "id"):
                    first_on = set()
                    for p, k, ov, nid in cont:
                        st = self.state.setdefault(k, _Slot())
                        if ov is None:
                            if not st.rank:
                                continue
                            ov = st.pv
                        if not self._after(ov, nid, st, desc):
                            continue
                        if sweep == "value":
                            st.ext = min(st.ext, ov)
                        elif ov == st.ext:
                            self.tags.add("tie_kept" if k in first_on else "round_first")
                            first_on.add(k)
                            if st.idw is None or self._id_less(nid, st.idw, desc):
                                st.idw, st.who = nid, p
            given = 0
            for k in keys:                             # the advance
                st = self.state.setdefault(k, _Slot())
                if st.idw is None:
                    self.tags.add("exhausted")
                    if self.defect == "exhausted_repeats" and 0 < st.rank < per:
                        st.win[st.rank] = st.win[st.rank - 1]; st.rank += 1
                    continue
                if st.rank < per:
                    st.win[st.rank] = (st.idw, -st.ext if desc else st.ext, st.who)
                st.pv, st.pid, st.rank, st.idw, st.who = st.ext, st.idw, st.rank + 1, None, None
                if self.defect != "ext_not_reset":
                    st.ext = I64MAX
                given += 1
        out = []
        if fits:
            for key, _, _, nm, nn, _ in recs:
                st = self.state.get(key) or _Slot()
                rows = [st.win.get(j) if j < st.rank else None for j in range(per)]
                if None in rows:
                    self.tags.add("padding")
                out.append([key, nm, nn, st.rank, rows])
        if self.defect != "state_not_reset":
            self.state = {}
        return out, fits, claims, total, absent, n_ordered


def device_answer(dev, m, node, n, E, cap, per, base, clauses, group, order, fields=(), desc=False, with_ts=False, clock=None):
    """one query of the stand-in over the model's table in position order (node: node numbers of the positions) -> what answer() returns"""
    clock = clock or default_clock(m)
    sel, gk, ov = gm.rows_of(m, base, clauses, group, order, node)
    ids = [int(x) for x in m.ids[node]]
    grps, fits, claims, total, absent, n_ordered = dev.run(n, E, cap, per, sel, gk, ov, ids, desc)
    res = np.zeros((), RES_DTYPE)
    res["total"] = total; res["absent"] = absent; res["n_ordered"] = n_ordered; res["n_groups"] = claims; res["per"] = per
    nf = len(fields)
    if not fits:
        res["flags"] = OVERFLOW
        return np.zeros(0, GRP_DTYPE), np.zeros((0, per), ROW_DTYPE), np.zeros((nf, 0, per), np.int64), np.zeros((nf, 0, per), np.int64) if with_ts else None, res
    grps.sort(key=lambda g: g[0])
    out = np.zeros(len(grps), GRP_DTYPE)
    rows = np.zeros((len(grps), per), ROW_DTYPE)
    rows["id"] = NO_NODE; rows["val"] = VAL_DELETED
    vals = np.full((nf, len(grps), per), VAL_DELETED, np.int64); ts = np.full((nf, len(grps), per), NO_CLOCK, np.int64)
    by_id = {int(x): i for i, x in enumerate(m.ids)}
    for r, g in enumerate(grps):
        out[r] = tuple(g[:4])
        for j, w in enumerate(g[4]):
            if w is None:
                continue
            rows[r, j] = (w[0], w[1])
            for f, fld in enumerate(fields):
                vals[f, r, j], ts[f, r, j] = cell(m, fld, by_id.get(w[0]), clock)
    res["n_rows"] = int((rows["id"] != np.uint64(NO_NODE)).sum())
    return out, rows, vals, ts if with_ts else None, res


# ---- helpers of the GPU tests ----
def raw_gtop(x, base, clauses, group, order, per, fields=(), desc=False, with_ts=False, cap=64, flags=None):
    """bmx_where_group_top (Engine) / bmx_comm_where_group_top (Comm), host memory, into pattern-filled buffers with room for cap + 1 groups -> (groups, rows,
    vals (nf, (cap + 1) * per), ts, res)"""
    import bmx
    nf = len(fields)
    out = np.full(32 * (cap + 1), FILL, np.uint8).view(GRP_DTYPE)
    rows = np.full(16 * (cap + 1) * per, FILL, np.uint8).view(ROW_DTYPE)
    res = np.full(48, FILL, np.uint8).view(RES_DTYPE)
    tail = list(bmx._gtop_tail(group, order, per, fields, desc, with_ts))
    if flags is not None:
        tail[5] = flags
    # the columns have stride cap * per: hand the library nf columns and keep one more block of per cells behind them as the guard
    stride = cap * per
    v2 = np.full((max(nf, 1) * stride + per,), FILL64, np.int64); t2 = v2.copy()
    args = (*bmx._where_args(base, clauses), *tail, int(cap), bmx._ptr(out), bmx._ptr(rows), bmx._ptr(v2), bmx._ptr(t2) if with_ts else None, bmx._ptr(res))
    x._chk(x.L.bmx_where_group_top(x.h, *args, bmx.MEM_HOST) if isinstance(x, bmx.Engine) else x.L.bmx_comm_where_group_top(x.h, *args))
    assert (v2[nf * stride:] == FILL64).all() and (t2[nf * stride:] == FILL64).all(), "nothing is written behind the last column"
    vals = np.full((nf, stride + per), FILL64, np.int64); ts = vals.copy()
    for f in range(nf):
        vals[f, :stride] = v2[f * stride:(f + 1) * stride]; ts[f, :stride] = t2[f * stride:(f + 1) * stride]
    return out, rows, vals, ts, res[0]


def ask(x, m, base, clauses, group, order, per, fields=(), desc=False, with_ts=False, cap=64, clock=None):
    """one query checked against the brute force -> answer()'s tuple"""
    got = raw_gtop(x, base, clauses, group, order, per, fields, desc, with_ts, cap)
    want = answer(m, base, clauses, group, order, per, fields, desc, cap, with_ts, clock)
    bad = check(got, want, cap, per, len(fields), with_ts)
    assert bad is None, (clauses, group, order, per, fields, desc, with_ts, cap, bad)
    return want


# ---- the edge suite: columns laid out by position ----
def edge_layouts(wide):
    """-> first_model.edge_layouts' dicts with per (3 for first_model's own), gtags (what the stand-in of the rounds must reach) and ranks (None, or {key:
    [positions of ranks 0, 1, ... ascending]})"""
    E = 2 if wide else 4
    start = gm.WIDE if wide else 1
    L = []
    for lay in fm.edge_layouts(wide):
        lay = dict(lay)
        lay["per"], lay["gtags"], lay["ranks"] = 3, set(), None
        L.append(lay)

    def add(name, n, per, keys, oval, ranks=None, gtags=(), cap=8, sel=None, has_o=None):
        L.append(dict(name=name, n=n, cap=cap, per=per, keys=np.asarray(keys, np.int64), present=np.ones(n, bool), sel=np.ones(n, bool) if sel is None else sel,
                      oval=np.asarray(oval, np.int64), has_o=np.ones(n, bool) if has_o is None else has_o, tags={"resolve_first"}, gtags=set(gtags) | {"round_first"},
                      winner=None, ranks=ranks, base=False, fix=None))

    key = start + 2
    n = 64 * E * 3
    for ln in (0, 63):                                 # ranks 1 and 2 on lane ln of the round kernels, rank 0 elsewhere
        p = [int(x) for x in np.nonzero(round_place(np.arange(n), n)[1] == ln)[0][[1, 2]]]
        ov = np.full(n, 10); ov[17] = -5; ov[p[0]] = -4; ov[p[1]] = -3
        add("ranks_on_lane_%d" % ln, n, 3, np.full(n, key), ov, {key: [17, p[0], p[1]]}, {"before_prev", "after_prev", "at_prev"})
    rnd = gm.THREADS * gm.U * E
    for name, n, p1, p2 in (("ranks_first_and_last_pos", rnd + 1, 0, rnd), ("ranks_in_ragged_unit", 64 * E + 1, 64 * E, 5)):
        ov = 100 + np.arange(n) % 9; ov[n // 2] = 90; ov[p1] = 91; ov[p2] = 92
        add(name, n, 3, np.full(n, key), ov, {key: [n // 2, p1, p2]}, {"before_prev", "after_prev"})
    n = 8 * ROUND_THREADS + 300
    assert round_grid(n) == 2
    wg = round_place(np.arange(n), n)[0]
    a, b, c = int(np.nonzero(wg == 0)[0][5]), int(np.nonzero(wg == 1)[0][9]), int(np.nonzero(wg == 0)[0][300])
    ov = np.full(n, 50); ov[c] = 5; ov[[a, b]] = 7     # ranks 1 and 2 tie on the value, one in each workgroup
    add("ranks_in_two_workgroups", n, 4, np.full(n, key), ov, None, {"tie_kept"})
    add("wave_all_tie_per_16", 128, 16, np.full(128, key), np.full(128, -(2**53 - 1)), None, {"tie_kept", "at_prev", "before_prev", "after_prev"})
    add("seventeen_contenders_per_16", 17, 16, np.full(17, key), 40 - np.arange(17), {key: list(range(16, 0, -1))}, {"after_prev"})
    n = 22
    add("exhausted_in_round_2_and_16_rounds", n, 16, np.where(np.arange(n) < 2, key, key + 1), np.arange(n) % 4, None, {"exhausted", "padding", "tie_kept"})
    n = 64 * 4                                         # per group the values 0, 1, 1, 2: the cut falls inside the tie
    add("lanes_on_64_groups", n, 2, start + (np.arange(n) % 64) * 3, (np.arange(n) // 64 + 1) // 2, None, {"tie_kept"}, cap=64)
    n = 64 * E
    add("member_without_order_later", n, 5, np.full(n, key), np.full(n, 3), None, {"tie_kept"}, has_o=np.arange(n) % 2 == 1)
    add("unselected_later", n, 5, np.full(n, key), np.full(n, 3), None, {"tie_kept"}, sel=np.arange(n) % 2 == 0)
    add("short_groups", 40, 4, start + np.arange(40) % 8, np.arange(40) % 3, None, {"padding", "exhausted"}, has_o=np.arange(40) % 8 <= np.arange(40) // 8)
    return L


# ---- the seeded suite ----
N_PROGS, SEED_PROGS = 60, 20261020
PERS = (2, 3, 5)


def conditions(m, base, p, group, order, desc, per):
    """what the brute force sees -> (a group with n > per whose ranks per and per + 1 hold the same value, a group with 0 < n < per, a group with n == 0, a tie on
    a group's extreme)"""
    groups = ranked(m, base, p, group, order, desc)[0]
    cut = short = empty = tie = False
    for nm, n, cont in groups.values():
        cut = cut or (n > per and cont[per - 1][0] == cont[per][0])
        short = short or 0 < n < per
        empty = empty or n == 0
        tie = tie or (n >= 2 and cont[0][0] == cont[1][0])
    return cut, short, empty, tie


def _seeded(m, per):
    F = names()
    probed = [F[k] for k in ("one", "two", "three")]
    out, seed, drawn = [], SEED_PROGS, 0
    while len(out) < N_PROGS:
        for p in wam.random_programs(8, seed, F["base"], probed + [F["group"], F["order"]], [F["extra"], F["select"], F["nobody"]])[:7]:
            k = len(out)
            desc = k % 2 == 1
            drawn += k < N_PROGS
            if k < N_PROGS and all(conditions(m, F["base"], p, F["group"], F["order"], desc, per)):
                out.append((p, F["group"], F["order"], desc))
        seed += 1
    return out, drawn


@functools.lru_cache(maxsize=None)
def _seeded_cached(per):
    m, tombs = seeded_model()
    gm.apply_tombs(m, tombs)
    return _seeded(m, per)


def seeded_queries(m, per):
    """-> N_PROGS x (clauses, group field, order field, desc) for this `per`: seeded programs, kept only if the brute force sees all four of conditions() (m:
    seeded_model()'s table with its tombstones applied; the list depends on nothing else, so it is computed once per `per`). Every other one is descending."""
    return list(_seeded_cached(per)[0])


def seeded_drawn(per):
    """how many candidate programs seeded_queries(per) drew for its N_PROGS"""
    return _seeded_cached(per)[1]
