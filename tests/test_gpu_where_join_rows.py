"""GPU: join projection (include/bmx_join_rows.h bmx_where_join_rows, bmx_where_map_rows). Every answer is compared exactly with join_rows_model's brute force
over the rows the test itself loaded: the ids, out_in_ids, every cell and clock of both sides and every word of the result record. Every buffer handed to the
library held 0x5A bytes and is checked untouched behind n_out in every column (join_rows_model.raw).

The tables are the smallest on which each rule can go wrong: the truth table of link state x key state x inner-cell state on both column widths of both sides;
link and key from the column, from a field the program probes and from a field it does not name; an inner field equal to key_field or in_base_field; keys 0,
+-1, +-(2^53 - 1); ids 0, 1, 2^63 - 1, 2^63, 2^64 - 2 sharing one key; empty and keyless inner sides; left against inner join; the caps around n_match; pages;
map_cap = K and K - 1; the list form of every query; 60 seeded pairs; the device mode; older queries interleaved on one context; a living table. The geometry
of the kernels is test_gpu_where_join_rows_kernel_edges.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import group_model as gm
import join_model as jm
import join_rows_model as jrm
import rows_model as rm
import semi_model as sm
import where_agg_model as wam
from join_rows_model import EVERY, F1, F2, FB, FI, FK, FL, FX, FY, NO_NODE, NOBODY, Q, QMAP, Table


def _engine(m, tombs, fields=jrm.ALL_FIELDS, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    jrm.apply_tombs(m, tombs, e)
    return e


def _both_joins(e, m, q, order=None):
    """the left and the inner join of one query, and its list form -> the left join's (got, want)"""
    left = jrm.ask(e, m, dict(q, inner=False), order)
    inner = jrm.ask(e, m, dict(q, inner=True), order)
    g, gi = left[0], inner[0]
    if not int(g["res"]["flags"]) and q["start"] == 0 and q["cap"] >= int(g["res"]["n_match"]):
        keep = g["in_ids"] != np.uint64(NO_NODE)
        assert np.array_equal(gi["ids"], g["ids"][keep]) and np.array_equal(gi["in_ids"], g["in_ids"][keep]), "the inner join is the left join's joined rows"
        assert np.array_equal(gi["vals"], g["vals"][:, keep]) and np.array_equal(gi["in_vals"], g["in_vals"][:, keep])
        assert int(gi["res"]["n_match"]) == int(g["res"]["n_joined"]) == int(keep.sum())
    if q["kind"] == "join":
        ql = jrm.as_list(m, q)
        if ql is not None:
            for inner_join in (False, True):
                a, b = jrm.ask(e, m, dict(ql, inner=inner_join), order)[0], (gi if inner_join else g)
                if not int(b["res"]["flags"]):
                    assert all(np.array_equal(a[k], b[k]) for k in ("ids", "vals", "ts", "in_ids", "in_vals", "in_ts")), "the list form of the inner side's pairs is the same query"
                    assert all(int(a["res"][k]) == int(b["res"][k]) for k in ("n_match", "n_out", "next_pos", "n_joined", "map_size", "n_keyed", "layout"))
    return left


# ---- 1. the truth table, on both column widths of both sides ----
@pytest.mark.parametrize("outer_wide,inner_wide", [(False, False), (True, False), (False, True), (True, True)])
def test_truth_table(outer_wide, inner_wide):
    m, tombs, ow, iw = jrm.truth_table(outer_wide, inner_wide)
    sel, inner = [[(FB, ow + 1, ow + 1)]], [[(FI, iw + 1, iw + 3)]]
    with _engine(m, tombs) as e:
        order = e.index_ids(FB)
        assert len(order) == 120
        qs = [Q(FB, sel, FL, [F1, F2], FI, inner, FK, [FX, FY])]                                             # link and key: fields the programs do not name
        qs += [Q(FB, EVERY, FL, [FB, FL, F2, F2], FI, inner, FK, [FK, FI, FX, NOBODY])]                      # fields = base / link; in_fields = key / inner base
        qs += [Q(FB, [[(FB, ow + 1, ow + 1), (FL, 100, 110)], [(F2, 0, 10**6, True)]], FL, [FL, F1], FI, [[(FI, iw + 1, iw + 3), (FK, 100, 103)], [(FX, 1030, 1040)]], FK, [FY, FX])]   # probed by the programs
        qs += [Q(FB, sel, FL, [], FI, inner, FK, [])]                                                        # out_in_ids alone is the join
        qs += [Q(FB, sel, FL, [F1], FI, [[(FI, iw + 9, iw + 9)]], FK, [FX])]                                 # key 110 alone
        qs += [Q(FB, sel, FL, [F1], FI, [[(FI, iw + 50, iw + 60)]], FK, [FX])]                               # an empty inner selection
        qs += [Q(FB, sel, FL, [F1], FI, inner, NOBODY, [FX])]                                                # every key absent
        qs += [Q(FB, sel, NOBODY, [F1], FI, inner, FK, [FX])]                                                # every link absent
        qs += [Q(FB, [[(FB, ow + 7, ow + 8)]], FL, [F1], FI, inner, FK, [FX])]                               # nothing selected
        qs += [Q(FI, inner, FI, [FK], FI, inner, FI, [FI, FK])]                                              # link and key from the columns, one index on both sides
        qs += [Q(FB, sel, FB, [F1], FI, inner, FI, [FX])]                                                    # link from the outer column (values iw + 1 .. 3 against ow + 1)
        states, joined = set(), set()
        for q0 in qs:
            for with_ts in (True, False):
                got, want = _both_joins(e, m, dict(q0, with_ts=with_ts), order if q0["base"] == FB else None)
                joined |= {bool(x) for x in (got["in_ids"] != np.uint64(NO_NODE)).tolist()}
                if with_ts and len(q0["in_fields"]):
                    states |= {("data" if v != jrm.VAL_DELETED else ("tomb" if t != jrm.NO_CLOCK else "absent")) for v, t in zip(got["in_vals"].ravel().tolist(), got["in_ts"].ravel().tolist())}
        assert states == {"data", "tomb", "absent"} and joined == {True, False}
        # map_cap at K and K - 1: K - 1 overflows and nothing is written
        K = int(jrm.ask(e, m, qs[0], order)[0]["res"]["map_size"])
        assert K == 5
        for inner_join in (False, True):
            ok, _ = jrm.ask(e, m, dict(qs[0], map_cap=K, inner=inner_join), order)
            over, _ = jrm.ask(e, m, dict(qs[0], map_cap=K - 1, inner=inner_join), order)
            assert not int(ok["res"]["flags"]) and int(over["res"]["flags"]) == jrm.MAP_OVERFLOW and int(over["res"]["n_out"]) == 0 and int(over["res"]["next_pos"]) == 120
            jrm.ask(e, m, dict(qs[0], map_cap=K - 1, cap=0, inner=inner_join), order)
        jrm.ask(e, m, qs[0], order)                                                                          # the scratch is clean behind an overflow
        # the Python driver
        r = e.where_join_rows(FB, sel, FL, [F1, F2], FI, inner, FK, [FX, FY], with_ts=True)
        w = jrm.answer(m, order, qs[0])
        assert all(np.array_equal(getattr(r, k), w[k]) for k in ("ids", "vals", "ts", "in_ids", "in_vals", "in_ts"))
        assert (r.n_match, r.n_out, r.next_pos, r.n_joined, r.map_size, r.n_inner, r.n_keyed, r.flags, r.next_shard) == tuple(int(w["res"][k]) for k in ("n_match", "n_out", "next_pos", "n_joined", "map_size", "n_inner", "n_keyed", "flags", "next_shard"))
        r = e.where_join_rows(FB, sel, FL, [F1], FI, inner, FK, [FX], inner=True, cap=3, map_cap=4)
        assert r.map_overflow and r.n_out == 0 and r.ts is None and r.in_vals.shape == (1, 0)
        k, i, _ = jrm.inner_pairs(m, FI, inner, FK)
        r = e.where_map_rows(FB, sel, FL, [F1, F2], k, i, [FX, FY], with_ts=True)
        assert all(np.array_equal(getattr(r, k), w[k]) for k in ("ids", "vals", "ts", "in_ids", "in_vals", "in_ts")) and r.n_inner == r.n_keyed == len(k)


# ---- 2. keys and ids at the ends of their domains ----
def test_key_values_and_unsigned_ids():
    """keys 0, +-1, +-(2^53 - 1); the ids 0, 1, 2^63 - 1, 2^63 and 2^64 - 2 share one key, and the inner program peels them off one after the other: the smallest
    UNSIGNED id must win (a signed comparison prefers 2^63 and 2^64 - 2)"""
    vals = np.array([0, 1, -1, jrm.VAL_MAX, -jrm.VAL_MAX, 1 << 31, -(1 << 31), (1 << 32) + 5, 7], np.int64)
    special = np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 2], np.uint64)
    nv, n = len(vals), 6 * len(vals)
    ids = np.concatenate([wam.node_ids(n, 83000), special])
    m = Table(ids)
    i = np.arange(n)
    m.set(FB, i, i, 5); m.set(FL, i, vals[i % nv], 6); m.set(F1, i, vals[(i * 5) % nv], 7)
    m.set(FI, i[:nv], i[:nv], 8); m.set(FK, i[:nv], vals, 9); m.set(FX, i[:nv], vals[::-1], 10)
    s = n + np.arange(5)
    m.set(FI, s, 100 + np.arange(5), 11); m.set(FK, s, 7, 12); m.set(FX, s, 500 + np.arange(5), 13)
    with _engine(m, {}) as e:
        order = e.index_ids(FB)
        for lo, hi in ((0, 8), (0, 4), (3, 4), (0, 0), (5, 7)):
            _both_joins(e, m, Q(FB, EVERY, FL, [FL, F1], FI, [[(FI, lo, hi)]], FK, [FX, FK]), order)
        for first, winner in enumerate(special.tolist()):
            got, _ = _both_joins(e, m, Q(FB, EVERY, FL, [FL], FI, [[(FI, 100 + first, 104)]], FK, [FX, FI]), order)
            hit = got["vals"][0] == 7
            assert hit.sum() == 6 and set(got["in_ids"][hit].tolist()) == {winner} and set(got["in_vals"][0][hit].tolist()) == {500 + first}
            assert int(got["res"]["map_size"]) == 1 and int(got["res"]["n_keyed"]) == 5 - first
        for perm in ([4, 3, 2], [2, 3, 4], [3, 4, 2], [4, 1, 0, 3]):                                            # the same through the list form, in several orders
            got, _ = jrm.ask(e, m, QMAP(FB, EVERY, FL, [FL], [7] * len(perm), special[perm].tolist(), [FX]), order)
            assert set(got["in_ids"][got["vals"][0] == 7].tolist()) == {int(special[perm].min())}
        qs = [QMAP(FB, EVERY, FL, [FL], [jrm.VAL_MAX, -jrm.VAL_MAX, 0, 1, -1], ids[[0, 1, 2, n, n + 4]].tolist(), [FX, FK])]
        qs += [QMAP(FB, EVERY, FL, [], [7, 7, 7, 1, 7, 1, 0, 0], [int(ids[5]), int(ids[3]), 9, NO_NODE, int(ids[3]), 2**63 + 5, NO_NODE, NO_NODE], [FX])]   # duplicates; an id that is no node; key 0: skipped pairs only
        qs += [QMAP(FB, EVERY, FL, [FL], [jrm.VAL_MAX + 1, -jrm.VAL_MAX - 1, jrm.INT64_MIN, jrm.INT64_MAX, -1], [1, 2, 3, 4, 5], [FX])]                      # keys outside: skipped
        qs += [QMAP(FB, EVERY, FL, [FL], [jrm.INT64_MIN], [NO_NODE], [FX])]                                     # an empty map from a list
        qs += [QMAP(FB, EVERY, FL, [FL], [1 << 31], [0], [FX])]                                                 # npairs = 1, the id 0
        qs += [QMAP(FB, [[(FB, 10, 30)]], FB, [FB], [11, 12, 29, 31, -4], ids[[n, 1, 2, 3, 4]].tolist(), [FI])]   # the link is the base column
        for q in qs:
            _both_joins(e, m, q, order)


# ---- 3. caps, pages, cursors ----
@pytest.mark.parametrize("wide", [False, True])
def test_caps_pages_and_cursors(wide):
    n, nin = 2 * 8192 + 300, 900
    off = jrm.WIDE if wide else 0
    rng = np.random.default_rng(4711)
    m = Table(wam.node_ids(n + nin, 84000))
    o, u = np.arange(n), n + np.arange(nin)
    m.set(FB, o, off + rng.integers(0, 12, n), rng.integers(1, 50, n))
    lk = o[rng.random(n) < 0.8]
    m.set(FL, lk, rng.integers(0, 1200, len(lk)), rng.integers(1, 50, len(lk)))
    m.set(F1, o, rng.integers(0, 6, n), rng.integers(1, 50, n))
    m.set(FI, u, off + rng.integers(0, 9, nin), 3); m.set(FK, u, rng.integers(0, 1000, nin), 4)
    fx = u[rng.random(nin) < 0.7]
    m.set(FX, fx, rng.integers(-jrm.VAL_MAX, jrm.VAL_MAX, len(fx)), rng.integers(1, 50, len(fx)))
    tombs = {FL: lk[::11], FX: fx[::5], FB: o[17::97]}
    with _engine(m, tombs, cap=8 * (n + nin)) as e:
        order = e.index_ids(FB)
        N = len(order)
        assert N == n
        base = Q(FB, [[(FB, off + 3, off + 5), (F1, 1, 5)]], FL, [F1, FL], FI, [[(FI, off + 0, off + 6)]], FK, [FX, FK], cap=n)
        for inner_join in (False, True):
            q = dict(base, inner=inner_join)
            one, _ = jrm.ask(e, m, q, order)
            nm, layout = int(one["res"]["n_match"]), int(one["res"]["layout"])
            assert nm > 600 and 0 < int(one["res"]["n_joined"]) and (inner_join or int(one["res"]["n_joined"]) < nm)
            for cap in (0, 1, nm - 1, nm, nm + 1):
                got, _ = jrm.ask(e, m, dict(q, cap=cap), order)
                assert int(got["res"]["n_out"]) == min(cap, nm) and int(got["res"]["layout"]) == layout
            first = int(jrm.ask(e, m, dict(q, cap=0, fields=[], in_fields=[]), order)[0]["res"]["next_pos"])
            assert order[first] == one["ids"][0], "cap 0: the position of the first selected node"
            for cap in (1, 7, 1000):
                parts, start, pages = [], 0, 0
                if cap == 1:
                    start = int(jrm.answer(m, order, dict(q, cap=nm - 40))["res"]["next_pos"])      # (cap 1: the last 40 rows, not thousands of calls)
                while start < N:
                    g, _ = jrm.ask(e, m, dict(q, start=start, cap=cap), order)
                    assert int(g["res"]["layout"]) == layout
                    parts.append(g); pages += 1
                    start = int(g["res"]["next_pos"])
                k = 40 if cap == 1 else nm
                for name in ("ids", "in_ids"):
                    assert np.array_equal(np.concatenate([p[name] for p in parts]), one[name][nm - k:])
                for name in ("vals", "ts", "in_vals", "in_ts"):
                    assert np.array_equal(np.concatenate([p[name] for p in parts], axis=1), one[name][:, nm - k:])
                assert pages == -(-k // cap) and sum(int(p["res"]["n_joined"]) for p in parts) == int((one["in_ids"][nm - k:] != np.uint64(NO_NODE)).sum())
            for start in (N - 1, N, N + 5, 1 << 40):
                g, _ = jrm.ask(e, m, dict(q, start=start, cap=4), order)
                if start >= N:
                    assert (int(g["res"]["next_pos"]), int(g["res"]["n_match"]), int(g["res"]["n_out"])) == (N, 0, 0), "a cursor beyond the index selects nothing"
        ql = jrm.as_list(m, base)
        g, _ = jrm.ask(e, m, dict(ql, start=8190, cap=300, inner=True), order)
        assert int(g["res"]["n_out"]) == 300


# ---- 4. the seeded suite ----
@pytest.fixture(scope="module")
def seeded():
    m, tombs = jrm.seeded_model()
    with _engine(m, tombs, fields=jm.ALL_FIELDS, cap=16 * m.N) as e:
        yield e, m, e.index_ids(jm.FB)


def test_seeded_pairs(seeded):
    """60 program pairs, every fourth with an overflowing query directly in front of it: an overflowing query leaves the scratch clean for the next"""
    e, m, order = seeded
    hits = 0
    for k, q in enumerate(jrm.seeded_pairs()):
        if k % 4 == 2:
            over, _ = jrm.ask(e, m, dict(q, map_cap=4), order)
            assert int(over["res"]["flags"]) == jrm.MAP_OVERFLOW
        got, _ = jrm.ask(e, m, q, order)
        assert not int(got["res"]["flags"])
        if not q["inner"]:
            assert int(got["res"]["n_match"]) == e.scan_where(jm.FB, q["clauses"], count_only=True)
        hits += int(got["res"]["n_joined"]) > 0
        ql = jrm.as_list(m, q)                                         # the list form of the pair's inner side, a page from the middle of the index
        if ql is not None:
            jrm.ask(e, m, dict(ql, cap=50, start=len(order) // 3), order)
    assert hits >= 45


# ---- 5. device memory ----
def test_device_memory_back_to_back(seeded):
    """device mode into poisoned buffers: six queries enqueued back to back (a left and an inner join, one cut off by its cap, a map overflow, the list form with
    device lists, cap 0), one synchronisation at the end; the records and the columns equal host mode and nothing is written where nothing belongs"""
    e, m, order = seeded
    dev = torch.device("cuda", 0)
    outer, inner = [[(jm.FB, 5, 80)], [(jm.F1, 0, 1, True), (jm.FB, 90, 99)]], [[(jm.FI, 0, 150)]]
    base = Q(jm.FB, outer, jm.FL, [jm.FM, jm.FL, jm.FB], jm.FI, inner, jm.FK, [jm.FA, jm.FK], True, False, 0, len(order), 1024)
    k, i, _ = jrm.inner_pairs(m, jm.FI, inner, jm.FK)
    keys = np.concatenate([k, [jrm.INT64_MIN, jrm.VAL_MAX + 1, k[0]]]).astype(np.int64)
    nodes = np.concatenate([i, np.array([5, 6, NO_NODE], np.uint64)])
    jobs = [base, dict(base, inner=True, with_ts=False), dict(base, cap=100, start=700), dict(base, map_cap=16), dict(base, map_cap=16, inner=True),
            QMAP(jm.FB, outer, jm.FL, base["fields"], keys, nodes, base["in_fields"], True, True, 0, 333), dict(base, cap=0, inner=True)]
    PAT = 0x5A5A5A5A5A5A5A5A

    def poisoned(words):
        return torch.full((words + 1,), PAT, dtype=torch.int64, device=dev)

    host = [jrm.raw(e, q) for q in jobs]
    bufs = [(poisoned(q["cap"]), poisoned(3 * q["cap"]), poisoned(3 * q["cap"]), poisoned(q["cap"]), poisoned(2 * q["cap"]), poisoned(2 * q["cap"]), poisoned(9)) for q in jobs]
    dk, dn = torch.from_numpy(keys).to(dev), torch.from_numpy(nodes.view(np.int64)).to(dev)
    for q, b in zip(jobs, bufs):
        ts = (b[2], b[5]) if q["with_ts"] else (None, None)
        if q["kind"] == "map":
            e.where_map_rows_dev(jm.FB, outer, jm.FL, q["fields"], dk, dn, len(keys), q["in_fields"], q["cap"], b[0], b[1], ts[0], b[3], b[4], ts[1], b[6], inner=q["inner"], start=q["start"])
        else:
            e.where_join_rows_dev(jm.FB, outer, jm.FL, q["fields"], jm.FI, inner, jm.FK, q["in_fields"], q["cap"], b[0], b[1], ts[0], b[3], b[4], ts[1], b[6], inner=q["inner"],
                                  start=q["start"], map_cap=q["map_cap"])
    e.sync()
    flags = []
    for q, b, h in zip(jobs, bufs, host):
        raw_res = b[6].cpu().numpy()
        assert raw_res[:9].tobytes() == h["res"].tobytes() and raw_res[9] == PAT, "the same record as in host mode, nothing behind it"
        n, cap = int(h["res"]["n_out"]), q["cap"]
        flags.append(int(h["res"]["flags"]))
        for name, buf, nf in (("ids", b[0], 0), ("vals", b[1], 3), ("ts", b[2], 3), ("in_ids", b[3], 0), ("in_vals", b[4], 2), ("in_ts", b[5], 2)):
            a = buf.cpu().numpy()
            if name.endswith("ts") and not q["with_ts"]:
                assert (a == PAT).all(), "without clocks no clock is written"
                continue
            if nf == 0:
                assert np.array_equal(a[:n].view(np.uint64), h[name]) and (a[n:] == PAT).all(), name
                continue
            for j in range(nf):
                assert np.array_equal(a[j * cap:j * cap + n], h[name][j]) and (a[j * cap + n:(j + 1) * cap] == PAT).all(), name
            assert (a[nf * cap:] == PAT).all(), name
        assert jrm.check(h, jrm.answer(m, order, q), q) is None
    assert flags == [0, 0, 0, jrm.MAP_OVERFLOW, jrm.MAP_OVERFLOW, 0, 0]
    assert (dk.cpu().numpy() == keys).all() and (dn.cpu().numpy().view(np.uint64) == nodes).all()
    jrm.ask(e, m, base, order)


# ---- 6. the map's table is bmx_where_join_group's; the mask and the staging are bmx_where_rows's ----
def test_interleaved_with_older_queries(seeded):
    e, m, order = seeded
    outer, inner = [[(jm.FB, 0, 60)]], [[(jm.FI, 10, 150)]]
    q = Q(jm.FB, outer, jm.FL, [jm.FM, jm.FL], jm.FI, inner, jm.FK, [jm.FA, jm.FK], True, False, 0, len(order), 1024)
    qg = jm.Q(jm.FB, outer, jm.FL, jm.FI, inner, jm.FK, jm.FA, jm.FM, cap=512, map_cap=1024)
    pn = sm.pos_nodes(e, m, jm.FB)

    def older():
        jm.ask(e, m, qg)
        jm.ask(e, m, dict(qg, map_cap=4))                             # the lookup join overflows its map
        sm.ask_semijoin(e, m, jm.FB, outer, jm.FL, jm.FI, inner, jm.FK, False, set_cap=1024, pn=pn)
        got = rm.raw_rows(e, jm.FB, outer, [jm.FM, jm.FL], True, 0, 300)
        assert rm.same(got, rm.rows(m, order, jm.FB, outer, [jm.FM, jm.FL], True, 0, 300)) is None
        gm.ask(e, m, jm.FB, outer, jm.F1, jm.FM, cap=64)

    older()
    for small in (q, dict(q, inner=True), dict(q, map_cap=4), dict(q, cap=2, inner=True), dict(q, map_cap=4, inner=True), q):
        jrm.ask(e, m, small, order)
        older()
    jrm.ask(e, m, q, order)


# ---- 7. a living table ----
def test_a_living_table():
    """after a merge that moves keys, links and inner cells and creates nodes, after a growth (a new layout), with tombstones, with value-ordered views on both
    base fields (left as they were), and after both indexes have switched to their int64 columns"""
    rng = np.random.default_rng(81)
    N0, EXTRA, NIN = 8192 + 5, 300, 400
    m = Table(wam.node_ids(N0 + EXTRA + NIN, 85000))
    old, new, users = np.arange(N0), np.arange(N0, N0 + EXTRA), N0 + EXTRA + np.arange(NIN)
    m.set(FB, old, rng.integers(0, 12, N0)); m.set(FL, old[rng.random(N0) < 0.8], 0)
    m.set(FL, np.nonzero(m.st[FL] == jrm.DATA)[0], rng.integers(0, 500, int((m.st[FL] == jrm.DATA).sum())))
    m.set(F1, old, rng.integers(0, 6, N0))
    m.set(FI, users, rng.integers(0, 9, NIN)); m.set(FK, users, rng.integers(0, 450, NIN)); m.set(FX, users[::2], rng.integers(0, 1000, NIN // 2 + NIN % 2))
    progs = [Q(FB, [[(F1, 1, 3), (FB, 2, 9)]], FL, [F1, FL], FI, [[(FI, 0, 6)]], FK, [FX, FK], inner=False),
             Q(FB, [[(F1, 0, 1)], [(FB, 0, 5), (FL, 0, 250)]], FL, [FB], FI, [[(FI, 2, 8), (FX, 0, 1000, True)], [(FK, 0, 100)]], FK, [FX], inner=True)]

    def ask(e):
        out = [jrm.ask(e, m, q)[0] for q in progs]
        assert all(not int(g["res"]["flags"]) and int(g["res"]["n_joined"]) > 0 for g in out)
        return out

    def same(a, b):
        return all(all(np.array_equal(x[k], y[k]) for k in ("ids", "vals", "ts", "in_ids", "in_vals", "in_ts")) for x, y in zip(a, b))

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.asarray(vals, np.int64), insert_mode=bmx.INSERT_DELTA, want_flags=False)
        m.set(f, idx, vals, ts)

    with _engine(m, {}, fields=[FB, FL, F1, FI, FK, FX], cap=8 * m.N) as e:
        first = ask(e)
        layout = int(first[0]["res"]["layout"])
        idx = old[::3]; merge(e, FL, idx, rng.integers(0, 500, len(idx)), 100)                               # links move, and appear where there was none
        idx = users[::2]; merge(e, FK, idx, rng.integers(300, 500, len(idx)), 100)                            # keys move
        idx = users[1::3]; merge(e, FX, idx, rng.integers(0, 1000, len(idx)), 100)                            # inner cells move and appear
        merge(e, FB, new, rng.integers(0, 12, EXTRA), 101); merge(e, F1, new, rng.integers(0, 6, EXTRA), 101); merge(e, FL, new, rng.integers(0, 500, EXTRA), 101)
        second = ask(e)
        assert not same(first, second) and all(int(g["res"]["layout"]) == layout for g in second), "a refresh from the log keeps the layout"
        e.reserve(32 * m.N)                                                                                  # growth: a new layout
        third = ask(e)
        assert all(int(g["res"]["layout"]) != layout for g in third)
        assert all(sorted(zip(x["ids"].tolist(), x["in_ids"].tolist())) == sorted(zip(y["ids"].tolist(), y["in_ids"].tolist())) for x, y in zip(second, third))
        rm.tombstone(e, m, FL, np.nonzero(m.st[FL] == jrm.DATA)[0][::9], ts=200)
        rm.tombstone(e, m, FK, np.nonzero(m.st[FK] == jrm.DATA)[0][::7], ts=200)
        rm.tombstone(e, m, FX, np.nonzero(m.st[FX] == jrm.DATA)[0][::5], ts=200)
        rm.tombstone(e, m, FI, np.nonzero(m.st[FI] == jrm.DATA)[0][5::40], ts=200)
        fourth = ask(e)
        assert not same(third, fourth)
        for f in (FB, FI):                                                                                   # value-ordered views on both base fields
            e.index_set_ordered(f, 1)
            e.scan_range(f, 2, 9)
            assert e.index_ordered_info(f)[1], "the view answers"
        s0 = [e.index_ordered_stats(f) for f in (FB, FI)]
        assert same(ask(e), fourth)
        assert [e.index_ordered_stats(f) for f in (FB, FI)] == s0 and all(e.index_ordered_info(f)[1] for f in (FB, FI)), "the calls leave the views as they were"
        for f in (FB, FI):
            e.index_set_ordered(f, 0)
        merge(e, FI, users[[7]], [jrm.WIDE], 2000)                                                            # each index switches to its int64 column
        ask(e)
        merge(e, FB, old[[9, 11]], [jrm.WIDE, -(2**35)], 2000)
        ask(e)
        got, _ = jrm.ask(e, m, Q(FB, [[(FB, 2**39, jrm.INT64_MAX)]], FB, [FB], FI, [[(FI, 2**39, jrm.INT64_MAX)]], FI, [FI]))
        assert got["ids"].tolist() == [int(m.ids[9])] and got["in_ids"].tolist() == [int(m.ids[users[7]])] and got["in_vals"].tolist() == [[jrm.WIDE]]
