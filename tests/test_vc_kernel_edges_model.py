"""No GPU: the inputs of tests/test_gpu_vc_kernel_edges.py themselves. Every batch of every scenario goes through OracleVC alone and
 - _paths reports the multiplicities, paths, chunk counts, queue depth, workspace size, lane bounds and shared bitmap words each scenario claims
   (_play asserts them batch by batch, with or without an engine), and _paths itself is right on hand-made cases;
 - rows are independent, so the oracle's answer on the interleaved batch must equal the answer when each built row's deltas are fed alone, in index
   order, one row after the other: a builder that gave a member to the wrong key fails here;
 - every case has a delta with each flag value 0, INCOMING, CURRENT, CURRENT | HISTORICAL and (K >= 2) CONCURRENT: inputs that cannot tell one order
   of application from another are rejected on the CPU.
It proves nothing about a kernel; it proves that the GPU tests ask for what they mean to."""
import numpy as np
import pytest

import test_gpu_vc_kernel_edges as edges
from oracle.oracle import OracleVC

SCENARIOS = [(case, i) for case, makers in edges.CASES.items() for i in range(len(makers))]


def _replay_row_by_row(sc, steps):
    """a second oracle gets every merge with the deltas regrouped: the first built row's deltas in index order, then the next row's, ..., then the rest"""
    o2 = OracleVC(sc.K, sc.local)
    for (b, P, flags, upd) in steps:
        ks = b.ks
        if b.load:
            o2.load_rows(b.ids, b.fields, b.clocks, b.val, keysets=ks)
            continue
        taken = np.zeros(b.n, bool)
        seen_ids = set()
        for key, mem in b.rows:
            assert (np.diff(mem) > 0).all() and not taken[mem].any()
            taken[mem] = True
            pair = set(zip(b.ids[mem].tolist(), b.fields[mem].tolist()))
            assert len(pair) == 1 and not pair & seen_ids, key
            seen_ids |= pair
        rest = np.flatnonzero(~taken)
        assert len(set(zip(b.ids[rest].tolist(), b.fields[rest].tolist())) | seen_ids) == len(rest) + len(b.rows), "the rest are rows of one delta each"
        perm = np.concatenate([m for _, m in b.rows] + [rest])
        f, u = o2.merge_batch(b.ids[perm], b.fields[perm], b.clocks[perm], b.val[perm], keysets=None if ks is None else ks[perm])
        back = np.zeros(b.n, np.uint8); back[perm] = f
        assert np.array_equal(back, flags)
        assert np.array_equal(np.sort(perm[u]), upd)
    return o2


@pytest.mark.parametrize("case,i", SCENARIOS)
def test_scenario_claims_hold_and_rows_are_what_the_builder_meant(case, i):
    sc = edges.CASES[case][i]()
    o, steps = edges._play(sc, gpu=False)
    o2 = _replay_row_by_row(sc, steps)
    assert len(o) == len(o2)
    for b, P, _, _ in steps:
        ids = np.array([k[0] for k in P.rows], np.uint64); f = np.array([k[1] for k in P.rows], np.uint32)
        for x, y in zip(o.get_rows(ids, f), o2.get_rows(ids, f)):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("case", list(edges.CASES))
def test_every_case_produces_every_flag_value(case):
    seen = {}                       # by "one writer" / "several": one writer's clocks are never concurrent
    for make in edges.CASES[case]:
        sc = make()
        for b, P, flags, _ in edges._play(sc, gpu=False)[1]:
            if flags is not None:
                seen.setdefault(sc.K == 1, set()).update(np.unique(flags).tolist())
    assert seen[False] == edges.ALL_FLAGS, (case, sorted(seen[False]))
    assert seen.get(True, edges.ALL_FLAGS - {edges.CONC}) == edges.ALL_FLAGS - {edges.CONC}, (case, sorted(seen[True]))


def test_paths_on_hand_made_batches():
    rng = np.random.default_rng(1)
    b = edges._build(rng, 600, [(1, np.arange(16)), (2, np.arange(16, 33)), (3, np.arange(40, 40 + 257)), (4, [599])], 2)
    P = edges._paths(b)
    key = lambda k: tuple(int(x[0]) for x in edges._ids([k]))
    assert [(P.rows[key(k)].m, P.rows[key(k)].path, P.rows[key(k)].chunks) for k in (1, 2, 3, 4)] == [(16, "short", 1), (17, "long", 1), (257, "long", 2), (1, "short", 1)]
    assert P.Q == 2 and len(P.rows) == 4 + 600 - 16 - 17 - 257 - 1
    assert (P.cap, P.bitmap_words, P.per, P.last_busy, P.first_idle) == (16384, 512, 2, 255, None)
    assert P.long_words == set(range(0, 10)) and P.shared_words == {1}          # 16..32 and 40..296: both in word 1
    assert not P.rows[key(1)].resident
    P = edges._paths(b, [(16385, {key(1)}), (10, None)])
    assert (P.cap, P.bitmap_words, P.per, P.last_busy, P.first_idle) == (16640, 520, 3, 173, 174) and P.rows[key(1)].resident and not P.rows[key(2)].resident
    P = edges._paths(b, [(16385, None), (65537, None), (300, None)])
    assert (P.cap, P.bitmap_words, P.per, P.last_busy, P.first_idle) == (65792, 2056, 9, 228, 229)
    b.load = True
    P = edges._paths(b)
    assert P.Q == 0 and {r.path for r in P.rows.values()} == {"preload"}
    assert [edges._cap_after(s) for s in ([1], [16384], [16385], [16385, 16640], [16385, 16641], [70000, 5])] == [16384, 16384, 16640, 16640, 16896, 70144]
