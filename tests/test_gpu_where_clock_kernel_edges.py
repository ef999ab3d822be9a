"""GPU: the clock literals of PredWhere::row (csrc/where_kernels.h) at the edges of its kernels. The probed columns are written BY POSITION of the base field's
index (index_ids gives the order), so a case can say which lane of which wave probes: a lane holds E consecutive positions (E = 4 int32 or 2 int64 values per
16-byte load), a wave 64 lanes, a mask block 8192 positions. The layouts are where_clock_model.edge_cases (test_where_clock_model.py shows what they expose).
Before a case runs on the device, the sequential stand-in must probe exactly the positions the case names, each slot with the probe that keeps the clock, and
its answer must be the numpy model's and the positions the case expects."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import where_clock_model as wcm
from where_clock_model import FB


def _walked(n, E):
    """the positions the sequential stand-in walks: all of a small column; of a large one the two waves at either end of every mask block (the Python walk of
    every node of every case would take the test's time; the numpy model and the device still answer for all)"""
    pos = np.arange(n)
    if n <= 1024:
        return pos
    wave = 64 * E
    return pos[(pos % 8192 < 2 * wave) | (pos % 8192 >= 8192 - 2 * wave) | (pos >= n - 2 * wave)]


def _run(e, m, node, name, clauses, want, probing, walked):
    W = wcm.prepare(FB, clauses)
    model = m.mask(FB, clauses)
    probers = []
    for pos in walked:
        probes = []
        assert wcm.row(W, m, node[pos], probes=probes) == model[node[pos]], (name, pos)
        assert all(kind == "ts" for _, kind in probes) and len(probes) == len(set(probes)), (name, probes)
        if probes:
            probers.append(pos)
    assert probers == np.intersect1d(probing, walked).tolist(), (name, probers[:8], list(probing)[:8])
    assert np.array_equal(np.nonzero(model[node])[0], want), (name, np.nonzero(model[node])[0][:8], want[:8])
    got = e.scan_where(FB, clauses)
    exp = m.ids[node][want]
    assert np.array_equal(got, exp), (name, len(got), len(exp), np.nonzero(got[:min(len(got), len(exp))] != exp[:min(len(got), len(exp))])[0][:4])


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", wcm.EDGE_SIZES)
def test_clock_literals_at_the_edges(n, wide):
    E = 2 if wide else 4
    ids = wcm.node_ids(n, 5000 + n)
    with bmx.Engine(max(32 * n, 4096)) as e:
        off = (1 << 40) if wide else 0
        e.put_rows(ids, np.full(n, FB, np.uint32), np.full(n, 6, np.int64), np.full(n, off, np.int64))
        scratch = wcm.ClockModel(ids)
        node = scratch.index_of(e.index_ids(FB))                        # node[p]: the node at position p
        m = wcm.edge_table(ids, node, E, wide)
        e.merge_batch(*m.rows(FB), want_flags=False)                    # (clock 7 over clock 6: the base values by lane)
        wcm.put(e, m, (wcm.F1, wcm.F2))
        assert np.array_equal(scratch.index_of(e.index_ids(FB)), node), "a value update moves no position"
        ran, walked = 0, _walked(n, E)
        for name, mutate, clauses, want, probing in wcm.edge_cases(m, node, E, wide):
            if mutate:
                mutate(lambda f, idx, vals, ts: wcm.write(e, m, f, idx, vals, ts))
            _run(e, m, node, name, clauses, want, probing, walked)
            ran += 1
        assert ran >= 14
