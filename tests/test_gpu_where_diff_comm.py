"""GPU: field-to-field literals over shards. 1 / 2 / 4 shards on one device answer bmx_comm_scan_where and bmx_comm_where_rows as one engine holding the same
rows does: the same set of ids (each shard in its own index order), the same cells per id, the same counts — and both as the model says."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import where_diff_model as wdm
from where_diff_model import F1, F2, F3, FB

N = 8192 + 77


def _programs():
    return [p for p in wdm.seeded_programs(60, 11) if any(wdm.is_pair(t) for c in p for t in c)][:10]


def _by_id(r):
    order = np.argsort(r.ids)
    return r.ids[order], r.vals[:, order], r.ts[:, order]


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = wdm.seeded_table(N, salt=nshards)
    m1, _ = wdm.seeded_table(N, salt=nshards)
    with bmx.Engine(16 * N) as e, bmx.Comm([0] * nshards, 16 * N) as c:
        wdm.load_table(e, m, tombs); wdm.load_table(c, m1, tombs)
        some = 0
        for p in _programs():
            want = m.ids[m.mask(FB, p)]
            one, many = e.scan_where(FB, p), c.scan_where(FB, p)
            assert np.array_equal(np.sort(one), np.sort(want)) and np.array_equal(np.sort(many), np.sort(want)), (nshards, p)
            assert c.scan_where(FB, p, count_only=True) == len(want) == e.scan_where(FB, p, count_only=True)
            r1, rn = e.where_rows(FB, p, [F1, F2, F3], with_ts=True), c.where_rows(FB, p, [F1, F2, F3], with_ts=True)
            assert r1.n_match == rn.n_match == len(want) == r1.n_out == rn.n_out
            for a, b in zip(_by_id(r1), _by_id(rn)):
                assert np.array_equal(a, b), (nshards, p)
            some += 0 < len(want) < N
        assert some >= 3
