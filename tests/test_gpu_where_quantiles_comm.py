"""GPU: bmx_comm_where_quantiles over 1, 2 and 4 logical shards (all on device 0) against one engine holding the same rows: every byte of the records and of
the result record equal — and both equal the numpy model. The quantiles of the shards do not combine; the communicator steps one select over all of them, so
the cases put what must be shared onto different shards: the minimum on one and the maximum on another, a tie group split over the shards, a shard whose
sample is empty."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import quant_model as qm
import where_agg_model as wam
from oracle import streams
from where_agg_model import DATA, Model

FB, F1, F2, FM = (streams.fnv1a32(s) for s in ("base", "one", "two", "measure"))
NOBODY = streams.fnv1a32("nobody")
EVERY = [[(NOBODY, 0, 0, True)]]
N = 6000
EIGHT = [(1, 2), (0, 1), (99, 100), (1, 1), (1, 4), (95, 100), (1, 2), (3, 4)]


def _model():
    rng = np.random.default_rng(616)
    m = Model(wam.node_ids(N, 8900))
    m.set(FB, np.arange(N), rng.integers(-2000, 2000, N))
    for f, pr in ((F1, 0.9), (F2, 0.5)):
        idx = np.nonzero(rng.random(N) < pr)[0]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
    idx = np.nonzero(rng.random(N) < 0.8)[0]
    v = rng.integers(-(2**40), 2**40, len(idx)); v[: len(idx) // 3] = 123456789            # a tie group of ~1600, on every shard
    m.set(FM, idx, v)
    return m


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m = _model()
    owner = bmx.owner_of(m.ids, nshards)
    progs = wam.random_programs(8, 20250909, FB, (F1, F2, FM), [streams.fnv1a32("m%d" % k) for k in range(5)])
    progs += [EVERY, [[(F1, 0, 2)], [(FM, 0, 2**41, True), (FB, -500, 500)]]]
    with bmx.Engine(16 * N) as e, bmx.Comm([0] * nshards, 16 * N) as c:
        for x in (e, c):
            wam.load(x, m, [FB, F1, F2, FM])
        idx = np.nonzero(m.st[FM] == DATA)[0][::9]
        c.put_rows(m.ids[idx], np.full(len(idx), FM, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), bmx.VAL_DELETED, np.int64))
        wam.tombstone(e, m, FM, idx)
        some = 0
        for k, p in enumerate(progs):
            for measure in (FB, FM, F1):
                for qs in (EIGHT, [(1, 2)]):
                    one = qm.raw(e, FB, p, measure, qs); many = qm.raw(c, FB, p, measure, qs)
                    assert qm.same(many, one) is None, (nshards, p, measure, qs, qm.same(many, one))
                    assert qm.same(many, qm.quantiles(m, FB, p, measure, qs)) is None
                some += int(one[1]["n"]) > 0
        assert some >= 12
        recs, res = c.where_quantiles(FB, EVERY, FM, EIGHT)
        assert recs.tobytes() == e.where_quantiles(FB, EVERY, FM, EIGHT)[0].tobytes() and int(recs[0]["n_equal"]) > 1000, "the tie group, split over the shards, holds the median"
        if nshards > 1:
            # the minimum on one shard and the maximum on another; and a selection whose sample lives on one shard only (the others' samples are empty)
            a, b = int(np.nonzero((owner == 0) & (m.st[FB] == DATA))[0][3]), int(np.nonzero((owner == 1) & (m.st[FB] == DATA))[0][3])
            for x in (e, c):
                x.put_rows(m.ids[[a, b]], np.full(2, FM, np.uint32), np.full(2, 15, np.int64), np.array([-(2**45), 2**45]))
            m.set(FM, [a, b], [-(2**45), 2**45])
            one = qm.raw(e, FB, EVERY, FM, EIGHT); many = qm.raw(c, FB, EVERY, FM, EIGHT)
            assert qm.same(many, one) is None and qm.same(many, qm.quantiles(m, FB, EVERY, FM, EIGHT)) is None
            assert (int(many[1]["min"]), int(many[1]["max"])) == (-(2**45), 2**45)
            on0 = np.nonzero((owner == 0) & (m.st[FB] == DATA))[0][:700]
            for x in (e, c):
                x.put_rows(m.ids[on0], np.full(len(on0), F2, np.uint32), np.full(len(on0), 20, np.int64), np.full(len(on0), 77, np.int64))
            m.set(F2, on0, np.full(len(on0), 77))
            for measure in (FB, FM):
                one = qm.raw(e, FB, [[(F2, 77, 77)]], measure, EIGHT); many = qm.raw(c, FB, [[(F2, 77, 77)]], measure, EIGHT)
                assert qm.same(many, one) is None and qm.same(many, qm.quantiles(m, FB, [[(F2, 77, 77)]], measure, EIGHT)) is None
                assert int(many[1]["n_match"]) == 700
