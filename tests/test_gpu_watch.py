"""GPU: standing queries (include/bmx_watch.h bmx_watch_*). Every poll is compared exactly, order included, with the numpy model of tests/watch_model.py: the
committed set of a watch is kept per NODE there, and the expected lists are index_ids(base) filtered by `now & ~committed` and `committed & ~now` (on RESET: all of
`now`, and nothing). tests/test_watch_model.py shows on the CPU that the seeded run used here holds entered, left and silent polls for every program."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import watch_model as wm
from watch_model import FB, F1, F2, PROGRAMS

FILL = 0x5A5A5A5A5A5A5A5A
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


def _engine(m, first, cap=None):
    e = bmx.Engine(cap or 8 * m.N)
    e.load_rows(*m.columns(first, 5)); m.apply(first)
    return e


def _write(x, m, batch, ts):
    """one batch (node, field, value) through merge_batch, its tombstones through put_rows; x: an Engine or a Comm"""
    node, field, val = (np.asarray(a) for a in batch)
    dead = val == wm.VAL_DELETED
    if (~dead).any():
        cols = m.columns((node[~dead], field[~dead], val[~dead]), ts)
        x.merge_batch(*cols, want_flags=False) if isinstance(x, bmx.Engine) else x.merge(*cols)
    if dead.any():
        x.put_rows(*m.columns((node[dead], field[dead], val[dead]), ts))
    m.apply((node, field, val))


def _one(node, field, val):
    return (np.array([node]).ravel(), np.full(np.size(node), field), np.array([val], np.int64).ravel() * np.ones(np.size(node), np.int64))


def _check(e, m, ws, key, w, cap_entered=None, cap_left=None, tag=None):
    pos = m.index_of(e.index_ids(FB))
    want = ws.poll(key, pos, cap_entered, cap_left)
    got = e.watch_poll(w, cap_entered, cap_left)
    assert (got.n_entered, got.n_left, got.n_match, got.reset, got.overflow) == (want.n_entered, want.n_left, want.n_match, want.reset, want.overflow), (tag, key, repr(got))
    if not want.overflow:
        assert np.array_equal(got.entered, want.entered) and np.array_equal(got.left, want.left), (tag, key)
    return got


def _raw_poll(e, w, cap_entered, cap_left, pad=4):
    ent, lft, res = np.full(cap_entered + pad, FILL, np.uint64), np.full(cap_left + pad, FILL, np.uint64), bmx.WatchRes()
    e._chk(e.L.bmx_watch_poll(e.h, w, bmx._ptr(ent), cap_entered, bmx._ptr(lft), cap_left, C.cast(C.byref(res), C.c_void_p), bmx.MEM_HOST))
    return ent, lft, res


# ---- 1. the first poll ----
def test_first_poll_is_the_snapshot():
    m, first = wm.seeded_model(0)
    with _engine(m, first) as e:
        for p in PROGRAMS:
            w = e.watch_create(FB, p)
            full = e.scan_where(FB, p)
            a = e.watch_poll(w)
            assert a.reset and not a.overflow and np.array_equal(a.entered, full) and len(a.left) == 0 and a.n_left == 0
            assert a.n_match == a.n_entered == e.scan_where(FB, p, count_only=True) == len(full) > 0
            b = e.watch_poll(w)
            assert (b.n_entered, b.n_left, b.n_match, b.reset, b.overflow) == (0, 0, len(full), False, False) and len(b.entered) == 0 and len(b.left) == 0
            c = e.watch_poll(w, 0, 0)                        # no room and nothing to report: commits trivially
            assert (c.n_entered, c.n_left, c.overflow) == (0, 0, False)
            ent, lft, res = _raw_poll(e, w, 0, 0)
            assert (ent == FILL).all() and (lft == FILL).all() and (res.n_match, res.flags, res.reserved) == (len(full), 0, 0)
            res = bmx.WatchRes()
            e._chk(e.L.bmx_watch_poll(e.h, w, None, 0, None, 0, C.cast(C.byref(res), C.c_void_p), bmx.MEM_HOST))      # NULL lists with caps of 0
            assert (res.n_entered, res.n_left, res.n_match, res.flags) == (0, 0, len(full), 0)


# ---- 2. the transition table ----
def test_transition_table():
    """14 nodes with the base field (value = node number) and two that are created later; F1 is the probed field of [[F1 in 10..20]]. One poll per case."""
    m = wm.Model(wm.node_ids(16, 77))
    ids = m.ids
    first = (np.concatenate([np.arange(14), [1, 2, 3, 4, 5, 6, 7, 8]]), np.concatenate([np.full(14, FB), np.full(8, F1)]),
             np.concatenate([np.arange(14), [15, 12, 10, 5, 11, 13, 20, 21]]).astype(np.int64))
    ts = iter(range(10, 1000))
    with _engine(m, first, 4096) as e:
        _write(e, m, _one(3, F1, wm.VAL_DELETED), next(ts))              # node 3 starts with a tombstone
        ws = wm.Watches(m)
        progs = {"in": [[(F1, 10, 20)]], "not": [[(F1, 10, 20, True)]], "never": [[(F1, 20, 10)]], "always": [[(F1, 20, 10, True)]]}
        w = {}
        for k, p in progs.items():
            w[k] = e.watch_create(FB, p); ws.create(k, FB, p)
        snap = {k: _check(e, m, ws, k, w[k], tag="snapshot") for k in progs}
        assert set(snap["in"].entered.tolist()) == set(ids[[1, 2, 5, 6, 7]].tolist()) and set(snap["not"].entered.tolist()) == set(ids[[0, 3, 4, 8, 9, 10, 11, 12, 13]].tolist())
        assert snap["never"].n_entered == 0 and snap["never"].reset and snap["always"].n_entered == 14

        def case(tag, batch, entered=(), left=(), key="in"):
            _write(e, m, batch, next(ts))
            got = _check(e, m, ws, key, w[key], tag=tag)
            assert got.entered.tolist() == ids[list(entered)].tolist() and got.left.tolist() == ids[list(left)].tolist() and not got.reset, (tag, repr(got))

        case("absent -> in range", _one(0, F1, 15), entered=[0])
        case("in -> out", _one(1, F1, 99), left=[1])
        case("in -> tombstone", _one(2, F1, wm.VAL_DELETED), left=[2])
        case("tombstone -> in", _one(3, F1, 10), entered=[3])
        case("out -> in", _one(4, F1, 20), entered=[4])
        case("in -> another value in range", _one(5, F1, 19))
        case("base row tombstoned", _one(6, FB, wm.VAL_DELETED), left=[6])
        n_before = e.index_size(FB)
        case("a new node that matches", (np.array([14, 14]), np.array([FB, F1]), np.array([14, 15], np.int64)), entered=[14])
        assert e.index_size(FB) == n_before + 1 and int(e.index_ids(FB)[-1]) == int(ids[14]), "the new node has an appended position"
        case("a new node that does not match", (np.array([15, 15]), np.array([FB, F1]), np.array([15, 50], np.int64)))
        # the negated watch has not been polled since its snapshot: this poll reports the net of everything above, then one case of its own
        got = _check(e, m, ws, "not", w["not"], tag="net")
        assert set(got.entered.tolist()) == set(ids[[1, 2, 15]].tolist()) and set(got.left.tolist()) == set(ids[[0, 3, 4]].tolist()), "node 6 was never in this watch's set"
        case("a negated literal whose field is tombstoned", _one(5, F1, wm.VAL_DELETED), entered=[5], key="not")
        got = _check(e, m, ws, "in", w["in"], tag="the same tombstone under the positive literal")
        assert got.left.tolist() == [int(ids[5])] and got.n_entered == 0
        got = _check(e, m, ws, "never", w["never"], tag="lo > hi")
        assert (got.n_entered, got.n_left, got.n_match) == (0, 0, 0)
        got = _check(e, m, ws, "always", w["always"], tag="lo > hi, negated")
        assert got.entered.tolist() == ids[[14, 15]].tolist() and got.left.tolist() == [int(ids[6])] and got.n_match == 15


# ---- 3. the seeded run ----
def test_seeded_run():
    m, first = wm.seeded_model()
    with _engine(m, first) as e:
        ws = wm.Watches(m)
        w = []
        for k, p in enumerate(PROGRAMS):
            w.append(e.watch_create(FB, p)); ws.create(k, FB, p)
        assert w == [0, 1, 2]
        builds = None
        seen = [[0, 0, 0] for _ in PROGRAMS]
        for r, merge, tomb in wm.seeded_rounds(m):
            _write(e, m, merge, 100 + 2 * r); _write(e, m, tomb, 101 + 2 * r)
            for k in range(len(PROGRAMS)):
                if wm.polled(r, k):
                    got = _check(e, m, ws, k, w[k], tag=r)
                    if not got.reset:
                        seen[k][0] += got.n_entered > 0; seen[k][1] += got.n_left > 0; seen[k][2] += got.n_entered == 0 and got.n_left == 0
            if builds is None:
                builds = e.index_refresh_counts()[0]
        assert e.index_refresh_counts()[0] == builds, "the index was maintained from the change log throughout: no poll but the first was a RESET poll"
        assert all(min(s) > 0 for s in seen), seen
        assert e.index_size(FB) == wm.N0 + wm.NEW_PER_ROUND * (wm.ROUNDS - len(wm.QUIET))


# ---- 4. overflow ----
def test_overflow_commits_nothing():
    m, first = wm.seeded_model(6)
    with _engine(m, first) as e:
        ws = wm.Watches(m)
        w = e.watch_create(FB, PROGRAMS[0]); ws.create(0, FB, PROGRAMS[0])
        # the snapshot itself overflows: RESET stays up until a poll commits
        M = e.scan_where(FB, PROGRAMS[0], count_only=True)
        ent, lft, res = _raw_poll(e, w, M - 1, 0)
        assert (res.n_entered, res.n_left, res.n_match, res.flags) == (M, 0, M, bmx.WATCH_RESET | bmx.WATCH_OVERFLOW) and (ent[M - 1:] == FILL).all() and (lft == FILL).all()
        ws.poll(0, m.index_of(e.index_ids(FB)), M - 1, 0)
        _check(e, m, ws, 0, w, tag="snapshot")
        rounds = wm.seeded_rounds(m, 6)
        r, merge, tomb = next(rounds)
        _write(e, m, merge, 100); _write(e, m, tomb, 101)
        pos = m.index_of(e.index_ids(FB))
        probe = wm.Watches(m); probe.create(0, FB, PROGRAMS[0]); probe.committed[0][2][:] = ws.committed[0][2]; probe.fresh.clear()
        want = probe.poll(0, pos)
        ne, nl = want.n_entered, want.n_left
        assert ne > 2 and nl > 2
        for ce, cl in ((ne - 1, nl), (ne, nl - 1), (ne - 1, nl - 1), (0, 0)):
            ent, lft, res = _raw_poll(e, w, ce, cl)
            assert (res.n_entered, res.n_left, res.n_match, res.flags) == (ne, nl, want.n_match, bmx.WATCH_OVERFLOW), (ce, cl)
            assert (ent[ce:] == FILL).all() and (lft[cl:] == FILL).all(), "nothing at or beyond the caps"
            ws.poll(0, pos, ce, cl)
        # a change in between: one node that entered leaves again, one that left comes back, one more enters — the next full poll reports the net
        back_out, back_in = m.index_of(want.entered[:1]), m.index_of(want.left[-1:])
        other = np.nonzero(~m.mask(FB, PROGRAMS[0]) & (m.st[FB] == wm.DATA) & ~ws.committed[0][2])[0]
        other = other[other != back_in[0]][:1]
        _write(e, m, (np.concatenate([back_out, back_in, other]), np.full(3, FB), np.array([55, 15, 12], np.int64)), 200)
        got = _check(e, m, ws, 0, w, tag="after the overflow")
        assert not got.overflow and int(want.entered[0]) not in got.entered.tolist() and int(m.ids[other[0]]) in got.entered.tolist()
        assert (got.n_entered, got.n_left) == (ne, nl - 1) and int(want.left[-1]) not in got.left.tolist()
        assert (_check(e, m, ws, 0, w).n_entered, e.watch_poll(w).n_left) == (0, 0)


# ---- 5. RESET ----
def test_reset_after_a_new_layout_and_not_after_a_widened_column():
    m, first = wm.seeded_model(6)
    with _engine(m, first, 4 * m.N) as e:
        ws = wm.Watches(m)
        w = [e.watch_create(FB, p) for p in PROGRAMS]
        for k, p in enumerate(PROGRAMS):
            ws.create(k, FB, p)
        for k in range(3):
            _check(e, m, ws, k, w[k], tag="snapshot")
        rounds = wm.seeded_rounds(m, 6)
        _, merge, tomb = next(rounds)
        _write(e, m, merge, 100); _write(e, m, tomb, 101)
        _check(e, m, ws, 0, w[0], tag="round 0")                        # watches 1 and 2 still owe the changes of round 0 when the table grows
        e.reserve(16 * m.N)
        ws.reset()
        for k in range(3):
            got = _check(e, m, ws, k, w[k], tag="after reserve")
            assert got.reset and got.n_left == 0 and np.array_equal(got.entered, e.scan_where(FB, PROGRAMS[k]))
            assert not _check(e, m, ws, k, w[k]).reset
        _, merge, tomb = next(rounds)
        _write(e, m, merge, 102); _write(e, m, tomb, 103)
        assert not _check(e, m, ws, 1, w[1], tag="round 1").reset
        e.index_drop(FB)
        ws.reset()
        for k in range(3):
            got = _check(e, m, ws, k, w[k], tag="after index_drop")
            assert got.reset and got.n_left == 0 and got.n_entered == got.n_match
        # a value beyond int32: the index switches to its int64 column, no position moves
        builds = e.index_refresh_counts()[0]
        inside = np.nonzero(m.mask(FB, PROGRAMS[0]))[0][:2]
        _write(e, m, (inside, np.full(2, FB), np.array([2**40, 15], np.int64)), 300)
        got = _check(e, m, ws, 0, w[0], tag="wide")
        assert not got.reset and got.left.tolist() == [int(m.ids[inside[0]])] and got.n_entered == 0
        _, merge, tomb = next(rounds)
        _write(e, m, merge, 302); _write(e, m, tomb, 303)
        for k in range(3):
            assert not _check(e, m, ws, k, w[k], tag="on the int64 column").reset
        assert e.index_refresh_counts()[0] == builds


# ---- 6. a value-ordered view on the base field ----
def test_with_an_ordered_view():
    m, first = wm.seeded_model(6)
    with _engine(m, first) as e:
        ws = wm.Watches(m)
        w = [e.watch_create(FB, p) for p in PROGRAMS]
        for k, p in enumerate(PROGRAMS):
            ws.create(k, FB, p)
        e.index_set_ordered(FB, 1)
        assert len(e.scan_range(FB, 10, 19)) > 0 and e.index_ordered_info(FB)[1], "the view answers the range scans"
        for k in range(3):
            _check(e, m, ws, k, w[k], tag="snapshot")
        for r, merge, tomb in wm.seeded_rounds(m, 3):
            _write(e, m, merge, 100 + 2 * r); _write(e, m, tomb, 101 + 2 * r)
            e.scan_range(FB, 10, 19)                                     # the refresh (and the view's patch) is this query's
            s0 = e.index_ordered_stats(FB)
            for k in range(3):
                assert not _check(e, m, ws, k, w[k], tag=("view", r)).reset
            assert e.index_ordered_stats(FB) == s0 and e.index_ordered_info(FB)[1], "the polls leave the view as it was"


# ---- 7. device memory ----
def _dev_poll(e, w, cap_entered, cap_left, dev):
    ent = torch.full((cap_entered + 4,), FILL, dtype=torch.int64, device=dev)
    lft = torch.full((cap_left + 4,), FILL, dtype=torch.int64, device=dev)
    res = torch.full((5,), FILL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)                  # the fills run on torch's stream, the poll on the engine's
    e.watch_poll_dev(w, ent, cap_entered, lft, cap_left, res)
    return ent, lft, res


def _dev_read(e, ent, lft, res):
    e.sync()
    r = res.cpu().numpy()
    assert int(r[4]) == FILL, "the record is 32 bytes"
    return ent.cpu().numpy().view(np.uint64), lft.cpu().numpy().view(np.uint64), (int(r[0]), int(r[1]), int(r[2]), int(r[3]) & 0xFFFFFFFF, int(r[3]) >> 32)


def test_device_mode_equals_host_mode():
    dev = torch.device("cuda", 0)
    m, first = wm.seeded_model(6)
    m2, _ = wm.seeded_model(6)
    with _engine(m, first) as e, _engine(m2, first) as twin:
        w = [e.watch_create(FB, p) for p in PROGRAMS]
        tw = [twin.watch_create(FB, p) for p in PROGRAMS]
        n = e.index_size(FB)

        def both(tag, caps=None):
            pos_ids = None
            for k in range(3):
                ce, cl = caps or (n + 64, n + 64)
                ent, lft, res = _dev_poll(e, w[k], ce, cl, dev)
                if pos_ids is None:                                          # (behind the first poll, which is to come right behind the writes)
                    pos_ids = e.index_ids(FB)
                    pos_of = np.argsort(pos_ids); sorted_pos = pos_ids[pos_of]          # id -> position in this engine's index
                assert res.is_cuda and ent.is_cuda
                h = twin.watch_poll(tw[k], ce, cl)
                ent, lft, (ne, nl, nm, flags, rsv) = _dev_read(e, ent, lft, res)
                assert (ne, nl, nm, flags, rsv) == (h.n_entered, h.n_left, h.n_match, (bmx.WATCH_RESET if h.reset else 0) | (bmx.WATCH_OVERFLOW if h.overflow else 0), 0), (tag, k)
                assert (ent[ce:] == FILL).all() and (lft[cl:] == FILL).all(), (tag, k)
                if not h.overflow:
                    # the same ids as the twin's, in the position order of THIS engine's index (two engines may lay colliding keys out in either order)
                    for got, want in ((ent[:ne], h.entered), (lft[:nl], h.left)):
                        assert np.array_equal(np.sort(got), np.sort(want)), (tag, k)
                        at = np.searchsorted(sorted_pos, got)
                        assert (sorted_pos[at] == got).all() and (np.diff(pos_of[at]) > 0).all(), (tag, k)
                    assert (ent[ne:] == FILL).all() and (lft[nl:] == FILL).all(), (tag, k)

        both("snapshot, too small", (3, 3))                              # overflows on the device: RESET | OVERFLOW, nothing committed
        both("snapshot")
        both("idle")
        for r, merge, tomb in wm.seeded_rounds(m, 3):
            for x, mm in ((e, m), (twin, m2)):
                _write(x, mm, merge, 100 + 2 * r); _write(x, mm, tomb, 101 + 2 * r)
            n = e.index_size(FB)
            both(("round", r), (2, n) if r == 1 else None)               # round 1 overflows first, then is fetched whole
            if r == 1:
                both(("round", r, "again"))
        # behind a deferred compaction: a device batch large enough to defer, polled right behind it without a synchronisation in between
        e.set_deferred(True)
        rng = np.random.default_rng(5)
        nb = 65_536
        keys = rng.permutation(3 * wm.N0)[:nb]
        kn, kf = keys % wm.N0, np.array([FB, F1, F2])[keys // wm.N0]
        kv = np.where(kf == FB, rng.integers(0, 100, nb), rng.integers(0, 10, nb)).astype(np.int64)
        cols = m.columns((kn, kf, kv), 900)
        d = (torch.from_numpy(cols[0].view(np.int64)).to(dev), torch.from_numpy(cols[1].view(np.int32)).to(dev), torch.from_numpy(cols[2]).to(dev), torch.from_numpy(cols[3]).to(dev))
        applied = torch.zeros(nb, dtype=torch.int32, device=dev); n_applied = torch.zeros(1, dtype=torch.int64, device=dev)
        twin.merge_batch(*cols, want_flags=False)
        d0 = e.deferred_counts()[0]
        e.merge_batch_dev(nb, *d, bmx.INSERT_REFERENCE, applied=applied, n_applied=n_applied)
        both("behind a deferred compaction")
        assert e.deferred_counts()[0] == d0 + 1 and int(n_applied.item()) == nb


# ---- 8. handles ----
def test_handles():
    m, first = wm.seeded_model(0)
    with _engine(m, first) as e:
        res = bmx.WatchRes()
        rp = C.cast(C.byref(res), C.c_void_p)
        for bad in (0, 5, 15, 16, 0xFFFFFFFF):
            assert e.L.bmx_watch_poll(e.h, bad, None, 0, None, 0, rp, bmx.MEM_HOST) == bmx.ERR_INVALID and e.L.bmx_watch_destroy(e.h, bad) == bmx.ERR_INVALID
        ws = [e.watch_create(FB, PROGRAMS[k % 3]) for k in range(bmx.WATCH_MAX)]
        assert ws == list(range(bmx.WATCH_MAX))
        with pytest.raises(bmx.BmxError) as ei:
            e.watch_create(FB, PROGRAMS[0])
        assert ei.value.code == bmx.ERR_INVALID
        with pytest.raises(bmx.BmxError):
            e.watch_create(FB, [[(FB, 0, 1)] * 9])                       # a refused program with a context behind it
        want = [e.scan_where(FB, p) for p in PROGRAMS]
        assert np.array_equal(e.watch_poll(3).entered, want[0]) and np.array_equal(e.watch_poll(7).entered, want[1])
        e.watch_destroy(3); e.watch_destroy(11)
        assert e.L.bmx_watch_poll(e.h, 3, None, 0, None, 0, rp, bmx.MEM_HOST) == bmx.ERR_INVALID and e.L.bmx_watch_destroy(e.h, 3) == bmx.ERR_INVALID
        ent = np.full(4, FILL, np.uint64)
        assert e.L.bmx_watch_poll(e.h, 7, None, 1, bmx._ptr(ent), 4, rp, bmx.MEM_HOST) == bmx.ERR_INVALID and e.L.bmx_watch_poll(e.h, 7, bmx._ptr(ent), 4, None, 0, rp, 9) == bmx.ERR_INVALID
        assert e.L.bmx_watch_poll(e.h, 7, bmx._ptr(ent), 4, None, 0, None, bmx.MEM_HOST) == bmx.ERR_INVALID and (ent == FILL).all()
        # a watch goes on answering while its neighbours come and go, and the freed ids are handed out again, lowest first
        node = np.nonzero(~m.mask(FB, PROGRAMS[1]) & (m.st[FB] == wm.DATA) & (m.st[F1] == wm.DATA))[0][:1]
        _write(e, m, (np.concatenate([node, node]), np.array([FB, F1]), np.array([5, 3], np.int64)), 50)
        assert e.watch_create(FB, PROGRAMS[2]) == 3 and e.watch_create(FB, PROGRAMS[2]) == 11
        got = e.watch_poll(7)
        assert got.entered.tolist() == [int(m.ids[node[0]])] and got.n_left == 0 and not got.reset
        fresh = e.watch_poll(3)
        assert fresh.reset and np.array_equal(fresh.entered, e.scan_where(FB, PROGRAMS[2])), "a reused id starts from the empty set"
