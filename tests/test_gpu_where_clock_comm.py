"""GPU: clock literals over shards. 1 / 2 / 4 shards on one device answer bmx_comm_scan_where, bmx_comm_where_aggregate and bmx_comm_where_rows as one engine
holding the same rows does: the same set of ids (each shard in its own index order), the same aggregate records bit for bit, the same cells and clocks per id,
the same counts — and the sets as the model says."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import where_agg_model as wam
import where_clock_model as wcm
from where_clock_model import F1, F2, F3, F4, FB, PROBED

N = 8192 + 77


def _programs():
    return [p for p in wcm.seeded_programs(60, 12) if any(wcm.is_clock(t) for c in p for t in c)][:10]


def _by_id(r):
    order = np.argsort(r.ids)
    return r.ids[order], r.vals[:, order], r.ts[:, order]


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m = wcm.seeded_table(N, salt=nshards)
    with bmx.Engine(16 * N) as e, bmx.Comm([0] * nshards, 16 * N) as c:
        wcm.put(e, m, [FB] + PROBED); wcm.put(c, m, [FB] + PROBED)
        some = 0
        for p in _programs():
            want = m.ids[m.mask(FB, p)]
            one, many = e.scan_where(FB, p), c.scan_where(FB, p)
            assert np.array_equal(np.sort(one), np.sort(want)) and np.array_equal(np.sort(many), np.sort(want)), (nshards, p)
            assert c.scan_where(FB, p, count_only=True) == len(want) == e.scan_where(FB, p, count_only=True)
            for kw in (dict(measure=F4), dict(measure=F3, group=F4, group_lo=0, ngroups=6)):
                a1, an = wam.raw_where_agg(e, FB, p, **kw), wam.raw_where_agg(c, FB, p, **kw)
                assert a1.tobytes() == an.tobytes(), (nshards, p, kw)
            r1, rn = e.where_rows(FB, p, [F1, F2, F3], with_ts=True), c.where_rows(FB, p, [F1, F2, F3], with_ts=True)
            assert r1.n_match == rn.n_match == len(want) == r1.n_out == rn.n_out
            for a, b in zip(_by_id(r1), _by_id(rn)):
                assert np.array_equal(a, b), (nshards, p)
            some += 0 < len(want) < N
        assert some >= 3
