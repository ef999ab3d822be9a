"""GPU: graph traversal (include/bmx_reach.h bmx_where_reach, bmx_where_reach_from). Every answer is compared exactly with reach_model's brute force — the
header's least fixed point, level by level: the ids and their depths in position order of the base index, every word of the result record (n_match, set_size,
n_seed, n_edges, rounds, flags), and the fill pattern behind [min(n_match, cap)] of both buffers (on overflow: in both whole buffers).

The tables are the smallest on which each rule can go wrong (reach_model.zoo, which test_reach_model.py runs through a sequential stand-in of the kernels and its
one-defect variants): chains that pin MORE and rounds, a star, a ring entered from a seed, self-loops, a diamond, a key shared by nodes at depths 1 and 3, a
keyless leaf, linkless and tombstoned nodes, an edge program that cuts a subtree, seeds nobody links to, an empty seed side, the keys 0, +-1, +-(2^53 - 1), link
and key each from the column, a field the program probes and a field it does not name, on both column widths, the ancestor direction, set_cap at K and K - 1,
overflow by the seeds alone, the caps 0, 1, m - 1, m, n, and the list form of every case. The seeded forest has 2 000 nodes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import reach_model as rm
from reach_model import EVERY, F1, FB, FI, FK, FL, FS, MAX_DEPTH, MORE, OVERFLOW


def _engine(m, tombs=(), cap=None):
    e = bmx.Engine(cap or max(8 * m.N * len(rm.ALL_FIELDS), 4096))
    rm.load(e, m, tombs=tombs)
    return e


# ---- 1. every small structure, both column widths, both forms, every cap ----
@pytest.mark.parametrize("wide", [False, True])
def test_zoo(wide):
    m, tombs = rm.zoo(wide)
    with _engine(m, tombs) as e:
        pns = {b: rm.pos_nodes(e, m, b) for b in (FB, FL, FK)}
        seen = set()
        qs = rm.zoo_queries(m)
        for q in qs + rm.zoo_lists() + [rm.as_list(m, q) for q in qs]:
            pn = pns[q["base"]]
            want = rm.answer(m, pn, q)
            for cap in rm.caps_of(want.n_match, len(pn)):
                rm.ask(e, m, q, cap, pn, want)
            seen.add((want.flags, want.n_match > 0))
        assert {(0, True), (MORE, True), (OVERFLOW, False), (0, False)} <= seen, seen
        # the wrapper: what ReachResult says is what the record says
        r = e.where_reach(FB, EVERY, FL, FK, FI, rm.SEEDS_ALL, FS, max_depth=3)
        want = rm.answer(m, pns[FB], dict(qs[0], max_depth=3))
        assert np.array_equal(r.ids, want.ids) and np.array_equal(r.depth, want.depth) and r.more and not r.overflow
        assert (r.n_match, r.set_size, r.n_seed, r.n_edges, r.rounds) == (want.n_match, want.set_size, want.n_seed, want.n_edges, want.rounds)
        r = e.where_reach_from(FB, EVERY, FK, FL, [5003], count_only=True)
        assert (r.n_match, r.rounds, len(r.ids), len(r.depth)) == (5, 3, 0, 0)


# ---- 2. chains: MORE and rounds; more levels than one byte of rounds could hold ----
def test_chains():
    m = rm.chain(6)
    with _engine(m) as e:
        got = [rm.ask(e, m, rm.Q(FB, EVERY, FL, FK, FI, rm.SEEDS_ALL, FS, D)) for D in (5, 6, 7)]
        assert [(w.n_match, w.rounds, w.flags) for w in got] == [(5, 5, MORE), (6, 6, MORE), (6, 6, 0)]
        got = [rm.ask(e, m, rm.QFROM(FB, EVERY, FL, FK, [500, 500], D)) for D in (5, 6, 7)]
        assert [(w.n_match, w.rounds, w.flags) for w in got] == [(5, 5, MORE), (6, 6, MORE), (6, 6, 0)]
    m = rm.chain(300)
    with _engine(m) as e:
        w = rm.ask(e, m, rm.Q(FB, EVERY, FL, FK, FI, rm.SEEDS_ALL, FS, MAX_DEPTH))
        assert (w.n_match, w.rounds, w.flags, w.set_size) == (255, 255, MORE, 256)
        w = rm.ask(e, m, rm.QFROM(FB, EVERY, FL, FK, [1000 + 44], MAX_DEPTH))          # the 255 nodes below node 44: the last one's key has level 255
        assert (w.n_match, w.rounds, w.flags) == (255, 255, MORE)
        w = rm.ask(e, m, rm.QFROM(FB, EVERY, FL, FK, [1000 + 45], MAX_DEPTH))
        assert (w.n_match, w.rounds, w.flags) == (254, 254, 0)
        w = rm.ask(e, m, rm.QFROM(FB, EVERY, FK, FL, [1000 + 299], MAX_DEPTH))          # upward from the last node
        assert (w.n_match, w.rounds, w.flags) == (255, 255, MORE)


# ---- 3. the seeded forest ----
def test_seeded_forest():
    """the 60 queries of reach_model.forest_queries (test_reach_model.py asserts what they select) over 2 000 nodes with dangling, absent and tombstoned links and a
    few cycles; an overflowing query leaves the scratch clean for the next; every third also as a list, every fifth with a cap that cuts the answer"""
    m, tombs = rm.forest()
    with _engine(m, tombs) as e:
        pn = rm.pos_nodes(e, m, FB)
        for k, q in enumerate(rm.forest_queries()):
            want = rm.answer(m, pn, q)
            rm.ask(e, m, q, None if k % 5 else max(want.n_match // 2, 1), pn, want)
            if k % 3 == 0:
                rm.ask(e, m, rm.as_list(m, q), None, pn)
            r = e.where_reach(q["base"], q["clauses"], q["link"], q["key"], FI, q["seed_clauses"], FS, max_depth=q["max_depth"], set_cap=q["set_cap"], count_only=True)
            assert (r.n_match, r.set_size > q["set_cap"], r.overflow, len(r.ids)) == (want.n_match, bool(want.flags & OVERFLOW), bool(want.flags & OVERFLOW), 0)


# ---- 4. device memory ----
def test_device_memory_back_to_back():
    """device mode into poisoned buffers: six traversals enqueued back to back (a deep one, one whose cap cuts the answer, an overflowing one, the list form with
    a device list, a count without buffers, a shallow one that leaves a frontier), one synchronisation at the end"""
    m, tombs = rm.forest()
    dev = torch.device("cuda", 0)
    vals = np.concatenate([rm.uid(np.arange(5)), [rm.EMPTY, rm.VAL_MAX + 1], rm.uid(np.arange(3))]).astype(np.int64)
    seeds = [[(FI, 0, 12)]]
    with _engine(m, tombs) as e:
        pn = rm.pos_nodes(e, m, FB)
        n = len(pn)
        jobs = [rm.Q(FB, EVERY, FL, FK, FI, seeds, FS), rm.Q(FB, [[(FB, 0, 69)]], FL, FK, FI, seeds, FS), rm.Q(FB, EVERY, FL, FK, FI, seeds, FS, set_cap=9),
                rm.QFROM(FB, EVERY, FL, FK, vals), rm.Q(FB, EVERY, FL, FK, FI, seeds, FS), rm.Q(FB, EVERY, FL, FK, FI, seeds, FS, 2)]
        caps = [n, 17, n, n, 0, n]
        ids = [torch.full((cap + rm.PAD,), rm.FILL64, dtype=torch.int64, device=dev) for cap in caps]
        deps = [torch.full((cap + rm.PAD,), rm.FILL, dtype=torch.uint8, device=dev) for cap in caps]
        ress = [torch.full((5,), rm.FILL64, dtype=torch.int64, device=dev) for _ in jobs]
        dvals = torch.from_numpy(vals).to(dev)
        for q, cap, o, d, r in zip(jobs, caps, ids, deps, ress):
            if q["kind"] == "from":
                e.where_reach_from_dev(FB, q["clauses"], FL, FK, dvals, len(vals), o, d, cap, r, max_depth=q["max_depth"], set_cap=q["set_cap"])
            else:
                e.where_reach_dev(FB, q["clauses"], FL, FK, FI, q["seed_clauses"], FS, o if cap else None, d if cap else None, cap, r, max_depth=q["max_depth"], set_cap=q["set_cap"])
        e.sync()
        flags = []
        for q, cap, o, d, r in zip(jobs, caps, ids, deps, ress):
            want = rm.answer(m, pn, q)
            res = r.cpu().numpy().view(rm.REACH_RES_DTYPE)[0]
            bad = rm.check(o.cpu().numpy().view(np.uint64), d.cpu().numpy(), res, want, cap, q["set_cap"])
            assert bad is None, (q, cap, bad, want)
            flags.append(want.flags)
        assert flags == [0, 0, OVERFLOW, 0, 0, MORE] and (dvals.cpu().numpy() == vals).all()
        rm.ask(e, m, jobs[0], None, pn)                       # host mode right after: the scratch is clean behind everything


# ---- 5. one map for joins, join projections and traversals ----
def test_interleaved_with_the_joins_on_one_context():
    m, tombs = rm.forest()
    q = rm.Q(FB, EVERY, FL, FK, FI, [[(FI, 0, 9)]], FS)
    over = dict(q, set_cap=5)
    with _engine(m, tombs) as e:
        pn = rm.pos_nodes(e, m, FB)

        def others():
            g = e.where_join_group(FB, [[(FB, 0, 49)]], FL, FB, EVERY, FK, FB, cap=256, map_cap=4096)
            j = e.where_join_rows(FB, [[(FB, 0, 9)]], FL, [FB], FB, EVERY, FK, [FB], map_cap=4096)
            s = e.where_semijoin(FB, EVERY, FL, FB, [[(FB, 0, 30)]], FK, set_cap=4096)
            return (g.records.tobytes(), g.map_size, j.ids.tobytes(), j.in_ids.tobytes(), j.n_joined, s.ids.tobytes(), s.set_size)

        first = others()
        assert first[1] > 1000 and first[4] > 0 and first[6] > 0
        rm.ask(e, m, q, None, pn)
        assert others() == first
        rm.ask(e, m, over, None, pn)                           # an overflowing traversal leaves the map empty too
        assert others() == first
        e.where_join_group(FB, EVERY, FL, FB, EVERY, FK, FB, cap=256, map_cap=64)     # a join whose map overflows, then a traversal
        rm.ask(e, m, q, None, pn)
        rm.ask(e, m, dict(q, set_cap=1 << 17), None, pn)      # the map grows
        assert others() == first
        rm.ask(e, m, q, None, pn)


# ---- 6. a living table ----
def test_a_living_table():
    """after a merge that moves links and keys and creates nodes, after a growth, with a value-ordered view on the base field (left as it was), and after the
    base index has switched to its int64 column"""
    rng = np.random.default_rng(99)
    m, tombs = rm.forest()
    n0 = 2000
    qs = [rm.Q(FB, EVERY, FL, FK, FI, [[(FI, 0, 19)]], FS), rm.Q(FB, [[(F1, 0, 7), (FB, 0, 89)]], FL, FK, FI, [[(FI, 2, 30)]], FS, 6), rm.Q(FB, EVERY, FK, FL, FI, [[(FI, 20, 39)]], FS)]

    def ask(e):
        return [rm.ask(e, m, q).n_match for q in qs]

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.asarray(vals, np.int64), want_flags=False)
        m.set(f, idx, vals)

    with _engine(m, tombs, cap=16 * m.N) as e:
        first = ask(e)
        assert all(x > 0 for x in first)
        idx = rng.choice(n0, 300, replace=False); merge(e, FL, idx, rm.uid(rng.integers(0, n0, len(idx))), 100)       # links move, and appear where there was none
        idx = rng.choice(n0, 100, replace=False); merge(e, FK, idx, rm.uid(rng.integers(0, n0, len(idx))), 100)       # keys move: shared keys
        second = ask(e)
        assert second != first
        e.reserve(64 * m.N)                                                                                           # growth
        assert ask(e) == second
        e.index_set_ordered(FB, 1)
        e.scan_range(FB, 2, 9)
        assert e.index_ordered_info(FB)[1], "the view answers"
        s0 = e.index_ordered_stats(FB)
        assert ask(e) == second
        assert e.index_ordered_stats(FB) == s0 and e.index_ordered_info(FB)[1], "the calls leave the view as it was"
        e.index_set_ordered(FB, 0)
        merge(e, FB, [9, 11], [rm.WIDE, -(2**35)], 2000)                                                              # the index switches to its int64 column
        ask(e)
        w = rm.ask(e, m, rm.Q(FB, [[(FB, 0, 2**39)]], FL, FK, FI, [[(FI, 0, 19)]], FS))
        assert w.n_match > 0
