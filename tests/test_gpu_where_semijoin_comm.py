"""GPU: bmx_comm_where_semijoin and bmx_comm_where_in. The same rows on 1, 2 and 4 logical shards give the set of ids and the record one engine gives; a key
held only by inner nodes of another shard than the outer node's is found (the union of the shards' sets is what every shard probes); a union above set_cap
while every shard is below it raises the flag and writes nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import semi_model as sm
import where_agg_model as wam
from semi_model import EVERY, FB, FI, FK, FL


def _load(x, m, tombs):
    wam.load(x, m, sm.ALL_FIELDS)
    for f, idx in tombs.items():
        x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), wam.VAL_DELETED, np.int64))


def _shard(c, g):
    s = bmx.Engine.__new__(bmx.Engine)
    s.L = c.L; s.h = C.c_void_p(c.L.bmx_comm_shard(c.h, g))
    return s


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = sm.seeded_model()
    with bmx.Engine(16 * m.N) as e, bmx.Comm([0] * nshards, 16 * m.N) as c:
        for x in (e, c):
            _load(x, m, tombs)
        sm.apply_tombs(m, tombs)
        pn = sm.pos_nodes(e, m, FB)
        seen = 0
        for k, (outer, link, inner, key, anti) in enumerate(sm.seeded_pairs()[::4]):
            for set_cap, cap in ((1024, m.N), (1024, 50), (3, m.N), (1024, 0)):
                want = sm.expected_semijoin(m, pn, FB, outer, link, FI, inner, key, anti, set_cap)
                one = sm.raw_semijoin(e, FB, outer, link, FI, inner, key, anti, cap, set_cap)
                many = sm.raw_semijoin(c, FB, outer, link, FI, inner, key, anti, cap, set_cap)
                assert sm.check(*one, want, cap, set_cap) is None
                bad = sm.check(*many, want, cap, set_cap, ordered=False)
                assert bad is None, (k, set_cap, cap, bad, want)
                if not want.flags:
                    assert many[1].tobytes() == one[1].tobytes(), "one engine's record, byte for byte"
                    seen += want.n_match > 0
            vals = sm.uid(np.arange(k, 900, 7))
            want = sm.expected_in(m, pn, FB, outer, link, vals, anti)
            many = sm.raw_in(c, FB, outer, link, vals, anti, m.N)
            assert sm.check(*many, want, m.N, len(vals), ordered=False) is None and many[1].tobytes() == sm.raw_in(e, FB, outer, link, vals, anti, m.N)[1].tobytes()
        assert seen >= 20
        outer, link, inner, key, anti = sm.seeded_pairs()[0]
        r, w = c.where_semijoin(FB, outer, link, FI, inner, key, anti=anti, set_cap=1024), sm.expected_semijoin(m, pn, FB, outer, link, FI, inner, key, anti, 1024)
        assert np.array_equal(np.sort(r.ids), np.sort(w.ids)) and (r.n_match, r.set_size, r.n_inner, r.overflow) == (w.n_match, w.set_size, w.n_inner, False)
        assert c.where_semijoin(FB, outer, link, FI, inner, key, set_cap=2).overflow
        r = c.where_in(FB, outer, link, sm.uid(np.arange(40)), count_only=True)
        assert r.n_match == sm.expected_in(m, pn, FB, outer, link, sm.uid(np.arange(40))).n_match and len(r.ids) == 0


def test_a_key_on_another_shard_and_a_union_that_overflows():
    n = 600
    m = sm.Model(wam.node_ids(n, 67000))
    i = np.arange(n)
    L = bmx.load_library()
    owner = np.array([L.bmx_owner_of(int(x), 2) for x in m.ids])
    per = np.bincount(owner, minlength=2)
    assert 0 < per.min()
    # every node is an inner node with its own key and an outer node that links to the key of a node on the OTHER shard
    on0, on1 = i[owner == 0], i[owner == 1]
    other = np.where(owner == 0, on1[i % len(on1)], on0[i % len(on0)])
    m.set(FB, i, i % 7); m.set(FI, i, i % 5); m.set(FK, i, sm.uid(i)); m.set(FL, i, sm.uid(other))
    with bmx.Comm([0, 0], 16 * n) as c:
        wam.load(c, m, [FB, FI, FK, FL])
        want = sm.expected_semijoin(m, None, FB, EVERY, FL, FI, EVERY, FK, False, n)
        assert want.n_match == n
        many = sm.raw_semijoin(c, FB, EVERY, FL, FI, EVERY, FK, False, n, n)
        assert sm.check(*many, want, n, n, ordered=False) is None
        for g in range(2):                                                            # on its own, a shard finds none of its links
            s = _shard(c, g)
            try:
                buf, res = sm.raw_semijoin(s, FB, EVERY, FL, FI, EVERY, FK, False, n, n)
                assert (int(res["n_match"]), int(res["set_size"]), int(res["n_inner"])) == (0, per[g], per[g])
            finally:
                s.h = None                                                            # the communicator owns the context
        anti = sm.raw_semijoin(c, FB, EVERY, FL, FI, EVERY, FK, True, n, n)
        assert sm.check(*anti, sm.expected_semijoin(m, None, FB, EVERY, FL, FI, EVERY, FK, True, n), n, n, ordered=False) is None and int(anti[1]["n_match"]) == 0
        # every shard is below set_cap, the union is above it
        set_cap = int(per.max())
        assert set_cap < n
        for a in (False, True):
            buf, res = sm.raw_semijoin(c, FB, EVERY, FL, FI, EVERY, FK, a, n, set_cap)
            assert sm.check(buf, res, sm.expected_semijoin(m, None, FB, EVERY, FL, FI, EVERY, FK, a, set_cap), n, set_cap) is None
            assert (int(res["flags"]), int(res["n_match"]), int(res["set_size"]), int(res["n_inner"])) == (bmx.SEMI_OVERFLOW, 0, n, n)
        # ... and right behind it a query that fits
        many = sm.raw_semijoin(c, FB, EVERY, FL, FI, [[(FI, 0, 0)]], FK, False, n, n)
        assert sm.check(*many, sm.expected_semijoin(m, None, FB, EVERY, FL, FI, [[(FI, 0, 0)]], FK, False, n), n, n, ordered=False) is None
