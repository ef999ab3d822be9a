"""CPU: the model of the graph traversal (tests/reach_model.py) against itself. The level-by-level brute force equals the header's definition relaxed in another
order; the sequential stand-in of the kernels equals the brute force on every shared shape, walks every path it tags, and each one-defect variant is noticed by
check() or levels_bad() — so the comparisons the GPU tests make can tell those defects apart."""
import numpy as np
import pytest

import reach_model as rm
from reach_model import EVERY, FB, FI, FK, FL, FS, MAX_DEPTH, MORE, OVERFLOW


def _zoo(wide=False):
    m, tombs = rm.zoo(wide)
    rm.apply_tombs(m, tombs)
    return m


def _all_queries(m):
    return rm.zoo_queries(m) + rm.zoo_lists() + [rm.as_list(m, q) for q in rm.zoo_queries(m)[:4]]


def test_the_level_by_level_closure_is_the_definition():
    for m in (_zoo(), _zoo(True)):
        for q in _all_queries(m):
            level, depth = rm.literal(m, q)
            d, levels = rm.closure(m, q)
            assert {int(i): int(d[i]) for i in np.nonzero(d)[0]} == depth, q
            assert {int(v): r for r, vs in enumerate(levels) for v in vs} == level, q
    m, tombs = rm.forest(); rm.apply_tombs(m, tombs)
    for q in rm.forest_queries(8):
        level, depth = rm.literal(m, q)
        d, levels = rm.closure(m, q)
        assert {int(i): int(d[i]) for i in np.nonzero(d)[0]} == depth and {int(v): r for r, vs in enumerate(levels) for v in vs} == level


def test_what_follows_from_the_definition():
    m = _zoo()
    pn = np.arange(m.N)
    w = rm.answer(m, pn, rm.Q(FB, EVERY, FL, FK, FI, rm.SEEDS_ALL, FS))
    depth = dict(zip(m.index_of(w.ids).tolist(), w.depth.tolist()))
    assert [depth.get(i) for i in (0, 1, 2, 3, 4, 5, 6)] == [1, 2, 3, 4, 5, 6, 7], "the chain, and the ring entered once"
    assert depth.get(7) is None and (depth[9], depth[8]) == (2, 3), "a self-loop is reached only from outside"
    assert (depth[10], depth[11], depth[12]) == (1, 3, 2) and w.level[4000] == 1, "the minimum on a shared key"
    assert [depth[i] for i in (13, 14, 15, 16, 17)] == [1, 1, 2, 2, 3], "the diamond"
    assert depth[18] == 2 and 19 not in depth and 20 not in depth and depth[21] == 1 and 22 not in depth, "leaves and nodes that are no edge nodes"
    assert [depth[i] for i in range(25, 31)] == [1, 2, 3, 4, 5, 6] and all(depth[i] == 4 for i in range(31, 53))
    assert (w.n_seed, w.flags, w.rounds) == (4, 0, 7) and w.level[501] == 0 and w.n_edges == 51
    cut = rm.answer(m, pn, rm.Q(FB, rm.CUT, FL, FK, FI, rm.SEEDS_ALL, FS))
    assert cut.n_match == w.n_match - 2 and 7001 not in cut.level, "a node the program does not select passes nothing on"
    # seeds are values, not nodes: node 0's key is the seed 1000 here, and it is not in the answer
    assert rm.answer(m, pn, rm.QFROM(FB, EVERY, FL, FK, [1000])).n_match > 0 and 0 not in m.index_of(rm.answer(m, pn, rm.QFROM(FB, EVERY, FL, FK, [1000])).ids)
    # the other direction: the chain of ancestors of node 17
    up = rm.answer(m, pn, rm.QFROM(FB, EVERY, FK, FL, [5003]))
    assert sorted(zip(up.depth.tolist(), m.index_of(up.ids).tolist())) == [(1, 17), (2, 15), (2, 16), (3, 13), (3, 14)]


def test_more_and_rounds_on_a_chain_of_six():
    m = rm.chain(6)
    pn = np.arange(m.N)
    got = {D: rm.answer(m, pn, rm.Q(FB, EVERY, FL, FK, FI, rm.SEEDS_ALL, FS, D)) for D in (5, 6, 7)}
    assert [(w.n_match, w.rounds, w.flags) for w in got.values()] == [(5, 5, MORE), (6, 6, MORE), (6, 6, 0)]
    assert [w.set_size for w in got.values()] == [6, 7, 7]
    long = rm.answer(np_chain := rm.chain(300), np.arange(np_chain.N), rm.Q(FB, EVERY, FL, FK, FI, rm.SEEDS_ALL, FS, MAX_DEPTH))
    assert (long.n_match, long.rounds, long.flags, long.set_size) == (255, 255, MORE, 256)


def test_the_stand_in_equals_the_brute_force():
    tags = set()
    for m in (_zoo(), _zoo(True)):
        rng = np.random.default_rng(5)
        pn = rng.permutation(m.N)                                     # (an index lays its positions out in its own order)
        for q in _all_queries(m):
            want = rm.answer(m, pn, q)
            for cap in rm.caps_of(want.n_match, m.N):
                ids, dep, res, lv, d = rm.device_of(m, q, cap, pn=pn)
                assert rm.check(ids, dep, res, want, cap, q["set_cap"]) is None, (q, cap, want, res)
                if not want.flags & OVERFLOW:
                    assert rm.levels_bad(lv, want) is None, q
                tags |= d.tags
    m, tombs = rm.forest(); rm.apply_tombs(m, tombs)
    seen = set()
    for q in rm.forest_queries():
        want = rm.answer(m, np.arange(m.N), q)
        ids, dep, res, lv, d = rm.device_of(m, q)
        assert rm.check(ids, dep, res, want, m.N, q["set_cap"]) is None, (q, want, res)
        seen.add((want.flags, want.n_match > 0)); tags |= d.tags
    assert {(0, True), (MORE, True), (OVERFLOW, False)} <= seen, seen
    assert {"reached", "same_round", "keyless", "no_edge", "early_out", "skipped", "lowered", "min_skipped", "present", "claim"} <= tags, tags


def test_the_forest_is_worth_asking():
    m, tombs = rm.forest(); rm.apply_tombs(m, tombs)
    ws = [rm.answer(m, np.arange(m.N), q) for q in rm.forest_queries()]
    assert sum(1 for w in ws if w.flags & OVERFLOW) >= 5 and sum(1 for w in ws if w.flags & MORE) >= 10
    assert max(w.n_match for w in ws) > 200 and max(w.rounds for w in ws) >= 8 and sum(1 for w in ws if w.n_match == 0 and not w.flags) <= 10


@pytest.mark.parametrize("defect", rm.DEFECTS)
def test_each_defect_is_noticed(defect):
    noticed = 0
    m = _zoo()
    pn = np.arange(m.N)
    for q in rm.zoo_queries(m)[:8] + [rm.QFROM(FB, EVERY, FL, FK, [2001], 3)]:      # (the last: a node at depth max_depth whose key is known)
        want = rm.answer(m, pn, q)
        ids, dep, res, lv, _ = rm.device_of(m, q, defect=defect)
        bad = rm.check(ids, dep, res, want, m.N, q["set_cap"]) or (None if want.flags & OVERFLOW else rm.levels_bad(lv, want))
        noticed += bad is not None
    assert noticed, defect
