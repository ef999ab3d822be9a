"""GPU: standing queries over the shards (include/bmx_watch.h bmx_comm_watch_*): 1, 2 and 4 logical shards on device 0 replay the first rounds of the seeded run
of tests/watch_model.py next to one engine. Per poll the SETS of entered and left ids equal the single engine's (and the model's), the counts are the sums, inside
one shard the order is the position order of that shard's index, an overflowing poll commits on no shard, and a shard that was rebuilt alone reports RESET with its
whole match set."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import watch_model as wm
from watch_model import FB, PROGRAMS
from test_gpu_watch import _write

ROUNDS = 10


def _shard_engine(c, g):
    """the shard's context behind the Engine methods (not owned: the caller drops it with h = None)"""
    c.L.bmx_comm_shard.restype = C.c_void_p
    e = bmx.Engine.__new__(bmx.Engine)
    e.L, e.h, e.device, e._watch_base = c.L, C.c_void_p(c.L.bmx_comm_shard(c.h, g)), 0, {}
    return e


def _in_shard_order(c, ids):
    """ids is the shards' lists one after the other, each in the position order of its shard's index of the base field"""
    if len(ids) == 0:
        return True
    own = bmx.owner_of(ids, c.N)
    if (np.diff(own.astype(np.int64)) < 0).any():
        return False
    for g in np.unique(own):
        e = _shard_engine(c, int(g))
        try:
            pos_ids = e.index_ids(FB)
        finally:
            e.h = None
        rank = {int(i): k for k, i in enumerate(pos_ids)}
        r = [rank[int(i)] for i in ids[own == g]]
        if r != sorted(r):
            return False
    return True


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded_run(nshards):
    m, first = wm.seeded_model(ROUNDS)
    with bmx.Engine(8 * m.N) as e, bmx.Comm([0] * nshards, 8 * m.N) as c:
        cols = m.columns(first, 5)
        e.load_rows(*cols); c.load_rows(*cols); m.apply(first)
        ws = wm.Watches(m)
        w, cw = [], []
        for k, p in enumerate(PROGRAMS):
            w.append(e.watch_create(FB, p)); cw.append(c.watch_create(FB, p)); ws.create(k, FB, p)
        assert cw == [0, 1, 2]

        def poll(k, tag, **caps):
            want = ws.poll(k, m.index_of(e.index_ids(FB)), caps.get("cap_entered"), caps.get("cap_left"))
            one, many = e.watch_poll(w[k], **caps), c.watch_poll(cw[k], **caps)
            for got in (one, many):
                assert (got.n_entered, got.n_left, got.n_match, got.reset, got.overflow) == (want.n_entered, want.n_left, want.n_match, want.reset, want.overflow), (tag, k, repr(got))
            if not want.overflow:
                assert np.array_equal(one.entered, want.entered) and np.array_equal(one.left, want.left), (tag, k)
                assert np.array_equal(np.sort(many.entered), np.sort(want.entered)) and np.array_equal(np.sort(many.left), np.sort(want.left)), (tag, k)
                assert _in_shard_order(c, many.entered) and _in_shard_order(c, many.left), (tag, k)
            return many

        for k in range(3):
            poll(k, "snapshot")
        events = 0
        for r, merge, tomb in wm.seeded_rounds(m, ROUNDS):
            for x in (e, c):
                mm = m if x is c else wm.Model(m.ids)                # (the model is applied once, with the second write)
                _write(x, mm, merge, 100 + 2 * r); _write(x, mm, tomb, 101 + 2 * r)
            for k in range(3):
                if wm.polled(r, k):
                    if r == 5 and k == 0:                             # an overflowing poll commits on no shard: the next one returns everything
                        full = ws.committed[0][2].copy()
                        probe = wm.Watches(m); probe.create(0, FB, PROGRAMS[0]); probe.committed[0][2][:] = full; probe.fresh.clear()
                        t = probe.poll(0, m.index_of(e.index_ids(FB)))
                        assert t.n_entered > 1 and t.n_left > 1
                        for caps in ((t.n_entered - 1, t.n_left), (t.n_entered, t.n_left - 1), (0, 0)):
                            got = poll(0, ("short", caps), cap_entered=caps[0], cap_left=caps[1])
                            assert got.overflow and len(got.entered) <= caps[0] and len(got.left) <= caps[1]
                    got = poll(k, r)
                    events += got.n_entered + got.n_left
        assert events > 100
        # one shard alone gets a larger table: its index is laid out anew, the others keep their committed sets
        g = nshards - 1
        s = _shard_engine(c, g)
        try:
            s.reserve(32 * m.N)
        finally:
            s.h = None
        before = c.watch_poll(cw[0])                                   # (nothing was written since the last poll of watch 0)
        own = bmx.owner_of(m.ids, nshards)
        theirs = m.ids[m.mask(FB, PROGRAMS[0]) & (own == g)]
        assert before.reset and not before.overflow and before.n_left == 0 and before.n_match == int(m.mask(FB, PROGRAMS[0]).sum())
        assert np.array_equal(np.sort(before.entered), np.sort(theirs)) and _in_shard_order(c, before.entered)
        after = c.watch_poll(cw[0])
        assert (after.n_entered, after.n_left, after.reset) == (0, 0, False)
        for k in range(3):
            c.watch_destroy(cw[k])
        with pytest.raises(bmx.BmxError):
            c.watch_poll(cw[0])
        assert c.watch_create(FB, PROGRAMS[1]) == 0
