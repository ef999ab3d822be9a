"""GPU: bmx_comm_where_aggregate and bmx_comm_where_top over 1, 2 and 4 logical shards (all on device 0) against one engine holding the same rows: the aggregate
records equal byte for byte, the top-k records and n_eligible equal — and both equal the numpy model."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import where_agg_model as wam
from oracle import streams
from where_agg_model import Model

FB, F1, F2, F3, F4, F5 = (streams.fnv1a32(s) for s in ("base", "one", "two", "three", "four", "five"))
MORE = [streams.fnv1a32("extra%d" % k) for k in range(3)]
PROBED = [F1, F2, F3, F4, F5]
N = 6000


def _model():
    rng = np.random.default_rng(515)
    m = Model(wam.node_ids(N, 8800))
    m.set(FB, np.arange(N), rng.integers(0, 12, N))
    tombs = {FB: np.arange(9, N, 83)}
    for f, pr in zip(PROBED + MORE, (0.9, 0.7, 0.5, 0.3, 0.6, 0.33, 0.33, 0.33)):
        idx = np.nonzero(rng.random(N) < pr)[0]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
        tombs[f] = idx[rng.random(len(idx)) < 0.1]
    return m, tombs


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = _model()
    progs = wam.random_programs(40, 20250302, FB, PROBED, MORE)
    with bmx.Engine(16 * N) as e, bmx.Comm([0] * nshards, 16 * N) as c:
        for x in (e, c):
            wam.load(x, m, [FB] + PROBED + MORE)
        for f, idx in tombs.items():
            c.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), bmx.VAL_DELETED, np.int64))
            wam.tombstone(e, m, f, idx)
        some = 0
        for k, p in enumerate(progs[:14] + progs[-1:]):
            measure = [None, FB, PROBED[k % 5], MORE[k % 3]][k % 4]
            for group, lo, ng in ((None, 0, 0), (PROBED[(k + 1) % 5], 0, 6), (FB, 1, 1030)):
                one = wam.raw_where_agg(e, FB, p, measure, group, lo, ng)
                many = wam.raw_where_agg(c, FB, p, measure, group, lo, ng)
                assert wam.same_records(many, one) is None, (nshards, p, measure, group, wam.same_records(many, one))
                assert wam.same_records(many, wam.agg(m, FB, p, measure, group, lo, ng)) is None
            assert c.where_aggregate(FB, p, measure) == e.where_aggregate(FB, p, measure)
            n_sel = int(one["n_match"].sum())
            some += 0 < n_sel < N
            want_all = wam.top(m, FB, p, N)
            cursors = [None] + ([(int(want_all[0][n_sel // 2]), int(want_all[1][n_sel // 2]))] if n_sel else []) + [(12345, 5)]
            for desc in (False, True):
                for kk in (1, 50, 4096):
                    for after in cursors:
                        a = e.where_top(FB, p, kk, desc, after); b = c.where_top(FB, p, kk, desc, after)
                        assert a[1] == b[1] and np.array_equal(a[0], b[0]), (nshards, p, desc, kk, after)
                        assert wam.top_equals(b, wam.top(m, FB, p, kk, desc, after))
        assert some >= 4
