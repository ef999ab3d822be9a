"""GPU: the pair path of PredWhere::row (csrc/where_kernels.h) at the edges of its kernels. The probed columns are written BY POSITION of the base field's index
(index_ids gives the order), so a case can say which lane of which wave probes: a lane holds E consecutive positions (E = 4 int32 or 2 int64 values per 16-byte
load), a wave 64 lanes, a mask block 8192 positions. Before a case runs on the device, the sequential stand-in (tests/where_diff_model.py) must take the path the
case is about, and its answer must be the numpy model's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import where_agg_model as wam
import where_diff_model as wdm
from where_diff_model import F1, F2, FB, I64MAX, I64MIN

BLOCK = 8192
SIZES = [1, 2, 3, 4, 5, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1]         # 1, E - 1, E, E + 1 for E = 4 and E = 2; the block edges; more than two blocks


def _run(e, m, node, clauses, tags=(), probing=None):
    """node: node numbers in position order. tags: what the stand-in must have gone through; probing: the positions whose node must be the only ones that probe"""
    seen = set()
    W = wdm.prepare(FB, clauses)
    truth = np.zeros(m.N, bool)
    probers = []
    for pos, i in enumerate(node):
        probes = []
        truth[i] = wdm.row(W, m, i, tags=seen, probes=probes)
        if probes:
            probers.append(pos)
    assert set(tags) <= seen, (clauses, set(tags) - seen)
    if probing is not None:
        assert probers == sorted(probing), (clauses, probers[:8], sorted(probing)[:8])
    assert np.array_equal(truth, m.mask(FB, clauses)), clauses
    want = m.ids[node][truth[node]]
    got = e.scan_where(FB, clauses)
    assert np.array_equal(got, want), (clauses, len(got), len(want), np.nonzero(got[:min(len(got), len(want))] != want[:min(len(got), len(want))])[0][:4])
    return np.nonzero(truth[node])[0]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_pair_path_at_the_edges(n, wide):
    E = 2 if wide else 4
    m = wdm.DiffModel(wdm.node_ids(n, 3000 + n))
    m.set(FB, np.arange(n), np.zeros(n, np.int64) + ((1 << 40) if wide else 0))
    with bmx.Engine(max(16 * n, 4096)) as e:
        wam.load(e, m, (FB,))
        node = m.index_of(e.index_ids(FB))                         # node[p]: the node at position p
        pos = np.arange(n)
        # the base column by position: 1 on lane 0 of every wave, 2 on lane 63, 0 elsewhere (+ the offset that makes the column wide)
        lane = (pos // E) % 64
        off = (1 << 40) if wide else 0
        bv = np.where(lane == 0, 1, np.where(lane == 63, 2, 0)) + off
        e.merge_batch(m.ids[node], np.full(n, FB, np.uint32), np.full(n, 6, np.int64), bv.astype(np.int64), want_flags=False)
        m.set(FB, node, bv)
        assert np.array_equal(m.index_of(e.index_ids(FB)), node), "a value update moves no position"
        # A = position, B = position except: equal to A + 1 on odd positions; so A - B is 0 on even and -1 on odd positions
        m.set(F1, node, pos); m.set(F2, node, pos + (pos % 2))
        wam.load(e, m, (F1, F2))
        P = (F1, F2)
        # every lane probes both sides
        sel = _run(e, m, node, [[(P, 0, 0)]], tags=("two_probes",), probing=pos)
        assert np.array_equal(sel, pos[pos % 2 == 0])
        # only lane 0 / only lane 63 of a wave probes: the base literal in front of the clause sends every other lane away
        _run(e, m, node, [[(FB, 1 + off, 1 + off), (P, -1, -1)]], tags=("two_probes",), probing=pos[lane == 0])
        _run(e, m, node, [[(P, 0, 0), (FB, 2 + off, 2 + off)]], probing=pos[lane == 63])
        # either side the column value: one probe per lane, A - B against the position
        _run(e, m, node, [[((FB, F1), off - 5, off - 3)]], tags=("base_a",), probing=pos)
        _run(e, m, node, [[((F2, FB), 2 - off, I64MAX, True)]], tags=("base_b",), probing=pos)
        # a pair literal that decides the first and the last position of every block, and the last position of the column
        ends = np.unique(np.concatenate([pos[pos % BLOCK == 0], pos[pos % BLOCK == BLOCK - 1], pos[-1:]]))
        m.set(F2, node[ends], pos[ends] - 7)
        e.merge_batch(m.ids[node[ends]], np.full(len(ends), F2, np.uint32), np.full(len(ends), 7, np.int64), (pos[ends] - 7).astype(np.int64), want_flags=False)
        assert np.array_equal(_run(e, m, node, [[(P, 7, 7)]]), ends)
        assert np.array_equal(_run(e, m, node, [[(FB, I64MIN, I64MAX, True)], [(P, 7, I64MAX), (P, I64MIN, 7)]], tags=("clause2_only", "slot_reused")), ends)
        assert len(_run(e, m, node, [[(P, 7, 7, True)]])) == n - len(ends)
        # B absent on every third position and tombstoned on every fifth
        third, fifth = pos[pos % 3 == 2], pos[pos % 5 == 4]
        m2 = wdm.DiffModel(m.ids)
        for f in (FB, F1):
            m2.set(f, np.arange(n), m.val[f])
        keep = np.setdiff1d(pos, third)
        m2.set(wdm.F3, node[keep], pos[keep] + 1)                  # a second B: F3, loaded without the thirds, then tombstoned on the fifths
        wam.load(e, m2, (wdm.F3,))
        dead = np.intersect1d(keep, fifth)
        if len(dead):
            wam.tombstone(e, m2, wdm.F3, node[dead])
        R = (F1, wdm.F3)
        gone = np.union1d(third, fifth)
        assert np.array_equal(_run(e, m2, node, [[(R, -1, -1)]], probing=pos), np.setdiff1d(pos, gone))
        assert np.array_equal(_run(e, m2, node, [[(R, I64MIN, I64MAX, True)]]), gone)
        assert np.array_equal(_run(e, m2, node, [[(R, -1, -1, True), (FB, off, off + 2)]]), gone)
