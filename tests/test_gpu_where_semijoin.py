"""GPU: semi-joins (include/bmx_semi.h bmx_where_semijoin, bmx_where_in). Every answer is compared exactly with semi_model's brute force — the inner selection,
numpy.unique of its present keys, numpy.isin on the present links, or the complement: the ids in position order of the base index, n_match, set_size, n_inner,
flags, reserved, and the fill pattern behind out_ids[min(n_match, cap)] (on overflow: in the whole buffer).

The tables are the smallest on which each rule can go wrong (semi_model.edge_layouts, which test_semi_model.py runs through a sequential stand-in of the
kernels): the truth table of {outer selected or not} x {link in S, not in S, tombstone, absent} x {plain, anti} on both column widths of both sides, links and
keys that come from the column, from a field the program probes and from a field it does not name, one base field on both sides, the keys 0, +-1, +-(2^53 - 1),
empty sets, lists with duplicates and values outside the domain. The seeded suite has more than one 8192-row block."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import semi_model as sm
import where_agg_model as wam
from semi_model import EVERY, F1, F2, FB, FI, FK, FL

LAYOUTS = {name: (m, tombs, qs) for name, m, tombs, qs in sm.edge_layouts() if name != "table edges"}      # (those: test_gpu_where_semijoin_kernel_edges.py)
FILL64 = sm.FILL64                               # (below 2^63: the same number as an int64)


def _engine(m, tombs, fields=sm.ALL_FIELDS, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    for f, idx in tombs.items():
        wam.tombstone(e, m, f, idx)
    return e


# ---- 1. the edge layouts ----
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_edge_layouts(name):
    m, tombs, qs = LAYOUTS[name]
    with _engine(m, dict(tombs)) as e:
        pn = {b: sm.pos_nodes(e, m, b) for b in {q["base"] for q in qs}}
        seen = set()
        for q in qs:
            want = sm.want_of(m, pn[q["base"]], q)
            for cap in sm.caps_of(want.n_match, len(pn[q["base"]])):
                buf, res = sm.raw_of(e, q, cap)
                bad = sm.check(buf, res, want, cap, sm.set_cap_of(q))
                assert bad is None, (name, q, cap, bad, want)
            seen.add((want.flags, want.n_match > 0))
            if q["kind"] == "semijoin" and not want.flags:
                # the list form with the inner side's values (duplicates, absent rows left out) is the same query
                sel = m.mask(q["inner_base"], q["inner_clauses"]); m._f(q["key"])
                vals = m.val[q["key"]][sel & (m.st[q["key"]] == sm.DATA)]
                if len(vals):
                    b2, r2 = sm.raw_in(e, q["base"], q["clauses"], q["link"], vals, q["anti"], len(pn[q["base"]]))
                    b1, r1 = sm.raw_of(e, q, len(pn[q["base"]]))
                    assert b1.tobytes() == b2.tobytes() and (int(r1["n_match"]), int(r1["set_size"])) == (int(r2["n_match"]), int(r2["set_size"])), (name, q)
            if q["kind"] == "semijoin" and q["anti"] and not want.flags and want.set_size == 0:
                assert np.array_equal(want.ids, e.scan_where(q["base"], q["clauses"])), "an empty set: the anti form is scan_where"
        assert (0, True) in seen


# ---- 2. the seeded suite ----
def test_seeded_pairs():
    """the 60 pairs of semi_model.seeded_pairs (test_semi_model.py asserts what they select), each with room for every key and every fourth also with set_cap = 4
    directly in front of it: an overflowing query leaves the scratch clean for the next"""
    m, tombs = sm.seeded_model()
    with _engine(m, tombs, cap=16 * m.N) as e:
        pn = sm.pos_nodes(e, m, FB)
        assert len(pn) == m.N
        overflows = 0
        for k, (outer, link, inner, key, anti) in enumerate(sm.seeded_pairs()):
            if k % 4 == 2:
                want = sm.ask_semijoin(e, m, FB, outer, link, FI, inner, key, anti, cap=64, set_cap=4, pn=pn)
                overflows += want.flags
            cap = None if k % 3 else 100
            want = sm.ask_semijoin(e, m, FB, outer, link, FI, inner, key, anti, cap=cap, set_cap=1024, pn=pn)
            assert not want.flags
            other = sm.expected_semijoin(m, pn, FB, outer, link, FI, inner, key, not anti, 1024)
            assert want.n_match + other.n_match == e.scan_where(FB, outer, count_only=True), (k, "plain + anti = the outer selection")
            r = e.where_semijoin(FB, outer, link, FI, inner, key, anti=anti, set_cap=1024, count_only=True)
            assert (r.n_match, r.set_size, r.n_inner, len(r.ids)) == (want.n_match, want.set_size, want.n_inner, 0)
        assert overflows >= 8
        r = e.where_semijoin(FB, EVERY, FL, FI, EVERY, FK)
        want = sm.expected_semijoin(m, pn, FB, EVERY, FL, FI, EVERY, FK)
        assert np.array_equal(r.ids, want.ids) and (r.n_match, r.set_size, r.n_inner, r.overflow) == (want.n_match, want.set_size, want.n_inner, False)
        r = e.where_in(FB, EVERY, FL, sm.uid(np.arange(5)), anti=True, cap=10)
        want = sm.expected_in(m, pn, FB, EVERY, FL, sm.uid(np.arange(5)), True)
        assert np.array_equal(r.ids, want.ids[:10]) and r.n_match == want.n_match > 10


# ---- 3. device memory ----
def test_device_memory_back_to_back():
    """device mode into poisoned buffers: five queries enqueued back to back (a deep one, one whose cap cuts the ids, an overflowing one, the list form with a
    device list, a count without ids), one synchronisation at the end; the answers are the model's, and nothing is written where nothing belongs"""
    m, tombs = sm.seeded_model()
    dev = torch.device("cuda", 0)
    outer, inner = [[(FB, 5, 80)], [(F1, 0, 1, True), (FB, 90, 99)]], [[(FI, 0, 150)]]
    vals = np.concatenate([sm.uid(np.arange(0, 900, 3)), [sm.INT64_MIN, sm.VAL_MAX + 1], sm.uid(np.arange(0, 30, 3))]).astype(np.int64)
    with _engine(m, tombs, cap=16 * m.N) as e:
        pn = sm.pos_nodes(e, m, FB)
        n = len(pn)
        jobs = [("semijoin", False, n, 1024), ("semijoin", True, 37, 1024), ("semijoin", False, n, 16), ("in", True, n, None), ("semijoin", True, 0, 1024)]
        outs = [torch.full((cap + sm.PAD,), FILL64, dtype=torch.int64, device=dev) for _, _, cap, _ in jobs]
        ress = [torch.full((4,), FILL64, dtype=torch.int64, device=dev) for _ in jobs]
        dvals = torch.from_numpy(vals).to(dev)
        for (kind, anti, cap, set_cap), o, r in zip(jobs, outs, ress):
            if kind == "in":
                e.where_in_dev(FB, outer, FL, dvals, len(vals), o, cap, r, anti=anti)
            else:
                e.where_semijoin_dev(FB, outer, FL, FI, inner, FK, o if cap else None, cap, r, anti=anti, set_cap=set_cap)
        e.sync()
        for (kind, anti, cap, set_cap), o, r in zip(jobs, outs, ress):
            want = sm.expected_in(m, pn, FB, outer, FL, vals, anti) if kind == "in" else sm.expected_semijoin(m, pn, FB, outer, FL, FI, inner, FK, anti, set_cap)
            res = r.cpu().numpy().view(sm.SEMI_RES_DTYPE)[0]
            bad = sm.check(o.cpu().numpy().view(np.uint64), res, want, cap, set_cap if kind != "in" else len(vals))
            assert bad is None, (kind, anti, cap, set_cap, bad, want)
        assert (dvals.cpu().numpy() == vals).all()
        # the scratch is clean behind the overflow and behind everything else: host mode right after
        sm.ask_semijoin(e, m, FB, outer, FL, FI, inner, FK, False, set_cap=1024, pn=pn)


# ---- 4. set sizes: a smaller set_cap behind a larger one ----
def test_a_smaller_set_cap_uses_the_head_of_a_larger_clean_table():
    n = 6000
    m = sm.Model(wam.node_ids(n, 66000))
    i = np.arange(n)
    m.set(FB, i, i % 100); m.set(FI, i, i); m.set(FK, i[:5000], sm.uid(i[:5000])); m.set(FK, i[5000:], sm.uid(i[5000:] % 7)); m.set(FL, i, sm.uid((i * 7) % 5500))
    with _engine(m, {}) as e:
        pn = sm.pos_nodes(e, m, FB)
        for set_cap, hi in ((8192, 4999), (8, 5006), (8, 5008), (4999, 4999), (5000, 4999), (1 << 17, 5999), (64, 40), (7, 5999)):
            for anti in (False, True):
                want = sm.ask_semijoin(e, m, FB, EVERY, FL, FI, [[(FI, 5000 if set_cap == 8 else 0, hi)]], FK, anti, set_cap=set_cap, pn=pn)
                assert want.flags == (set_cap in (4999, 7))
        want = sm.ask_in(e, m, FB, EVERY, FL, sm.uid(np.arange(3000)), pn=pn)
        assert want.set_size == 3000


# ---- 5. a living table ----
def test_a_living_table():
    """after a merge that changes keys and links and creates nodes, after a growth, with tombstones, with a value-ordered view on the base fields (left as it
    was), behind a deferred compaction, and after both indexes have switched to their int64 columns"""
    rng = np.random.default_rng(78)
    m, tombs = sm.seeded_model()
    N = m.N
    progs = [([[(FB, 10, 70)]], FL, [[(FI, 20, 120)]], FK), ([[(F1, 0, 4), (FB, 0, 50)], [(F2, 9, 9)]], FL, [[(FI, 0, 199), (F1, 3, 9)]], FK), (EVERY, FB, [[(FI, 0, 60)]], FI)]
    dev = torch.device("cuda", 0)

    def ask(e):
        out = []
        for outer, link, inner, key in progs:
            for anti in (False, True):
                out.append(sm.ask_semijoin(e, m, FB, outer, link, FI, inner, key, anti, set_cap=2048).n_match)
        return out

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.asarray(vals, np.int64), want_flags=False)
        m.set(f, idx, vals)

    with _engine(m, tombs, cap=8 * N) as e:
        first = ask(e)
        assert all(x > 0 for x in first)
        live = np.nonzero(m.st[FB] == sm.DATA)[0]
        idx = live[::3]; merge(e, FL, idx, sm.uid(rng.integers(0, 1000, len(idx))), 100)                 # links move, and appear where there was none
        idx = np.nonzero(m.st[FI] == sm.DATA)[0][::2]; merge(e, FK, idx, sm.uid(rng.integers(700, 1000, len(idx))), 100)   # keys move into the dangling range
        idx = live[1::5]; merge(e, FB, idx, rng.integers(0, 100, len(idx)), 100)
        second = ask(e)
        assert second != first
        e.reserve(32 * N)                                                                               # growth
        assert ask(e) == second
        wam.tombstone(e, m, FL, np.nonzero(m.st[FL] == sm.DATA)[0][::9], ts=200)
        wam.tombstone(e, m, FK, np.nonzero(m.st[FK] == sm.DATA)[0][::7], ts=200)
        wam.tombstone(e, m, FI, np.nonzero(m.st[FI] == sm.DATA)[0][5::40], ts=200)
        third = ask(e)
        assert third != second
        # value-ordered views on both base fields: the same answers, and the views' counters untouched
        for f in (FB, FI):
            e.index_set_ordered(f, 1)
            e.scan_range(f, 2, 9)
            assert e.index_ordered_info(f)[1], "the view answers"
        s0 = [e.index_ordered_stats(f) for f in (FB, FI)]
        assert ask(e) == third
        assert [e.index_ordered_stats(f) for f in (FB, FI)] == s0 and all(e.index_ordered_info(f)[1] for f in (FB, FI)), "the calls leave the views as they were"
        for f in (FB, FI):
            e.index_set_ordered(f, 0)
        # deferred compaction (switched on explicitly): a device batch large enough to defer, asked right behind it
        e.set_deferred(True)
        nb = 65_536
        fields = np.array([FB, FL, FI, FK, F1, F2, sm.streams.fnv1a32("semi.filler.a"), sm.streams.fnv1a32("semi.filler.b")], np.uint32)              # 8 x N distinct (node, field) keys >= nb
        keys = rng.permutation(len(fields) * N)[:nb]
        kn, kf = keys % N, fields[keys // N]
        kv = np.where(kf == FB, rng.integers(0, 100, nb), np.where(kf == FI, rng.integers(0, 200, nb), np.where((kf == FL) | (kf == FK), sm.uid(rng.integers(0, 1000, nb)), rng.integers(0, 10, nb)))).astype(np.int64)
        cols = (torch.from_numpy(m.ids[kn].view(np.int64)).to(dev), torch.from_numpy(kf.view(np.int32)).to(dev),
                torch.full((nb,), 300, dtype=torch.int64, device=dev), torch.from_numpy(kv).to(dev))
        applied = torch.zeros(nb, dtype=torch.int32, device=dev); n_applied = torch.zeros(1, dtype=torch.int64, device=dev)
        d0 = e.deferred_counts()[0]
        e.merge_batch_dev(nb, *cols, bmx.INSERT_REFERENCE, applied=applied, n_applied=n_applied)
        for f in fields:
            m.set(int(f), kn[kf == f], kv[kf == f])
        sm.ask_semijoin(e, m, FB, progs[0][0], FL, FI, progs[0][2], FK, False, set_cap=2048)
        assert e.deferred_counts()[0] == d0 + 1 and int(n_applied.item()) == nb
        ask(e)
        # base values beyond int32 on either side: each index switches to its int64 column
        merge(e, FI, [7], [sm.WIDE], 2000)
        ask(e)
        merge(e, FB, [9, 11], [sm.WIDE, -(2**35)], 2000)
        ask(e)
        want = sm.ask_semijoin(e, m, FB, [[(FB, 2**39, sm.INT64_MAX)]], FB, FI, [[(FI, 2**39, sm.INT64_MAX)]], FI, False)
        assert (want.n_match, want.set_size, want.n_inner) == (1, 1, 1)
