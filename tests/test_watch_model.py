"""CPU: the standing-query model's own invariants (tests/watch_model.py) on the seeded run the GPU tests replay, so that those cannot pass vacuously: per poll
entered and left are disjoint and (C + entered) - left = M; per program the run holds a poll that reports entered ids, one that reports left ids and one that
reports nothing; the net-change polls really skip over nodes that came and went; an overflowing poll leaves the committed set alone."""
import numpy as np

import watch_model as wm


def _pos(m):
    return np.nonzero(m.st[wm.FB] != wm.ABSENT)[0]


def _run(rounds=wm.ROUNDS, on_poll=None):
    m, first = wm.seeded_model(rounds)
    m.apply(first)
    ws = wm.Watches(m)
    for k, p in enumerate(wm.PROGRAMS):
        ws.create(k, wm.FB, p)
    polls = {k: [] for k in range(len(wm.PROGRAMS))}
    truth = {k: [m.mask(wm.FB, p)] for k, p in enumerate(wm.PROGRAMS)}
    for r, merge, tomb in wm.seeded_rounds(m, rounds):
        m.apply(merge); m.apply(tomb)
        for k, p in enumerate(wm.PROGRAMS):
            truth[k].append(m.mask(wm.FB, p))
            if wm.polled(r, k):
                before = ws.committed[k][2].copy()
                x = ws.poll(k, _pos(m))
                polls[k].append((r, before, x))
    return m, ws, polls, truth


def test_every_poll_keeps_the_invariants():
    m, ws, polls, truth = _run()
    for k, p in enumerate(wm.PROGRAMS):
        assert len(polls[k]) == wm.ROUNDS // wm.POLL_EVERY[k]
        for r, before, x in polls[k]:
            ent, lft = m.index_of(x.entered), m.index_of(x.left)
            assert len(np.intersect1d(ent, lft)) == 0, (k, r)
            after = before.copy(); after[ent] = True; after[lft] = False
            assert not before[ent].any() and before[lft].all(), (k, r)
            assert np.array_equal(after, truth[k][r + 1]) and x.n_match == int(after.sum()), (k, r)          # (C + entered) - left = M behind round r
        assert polls[k][0][2].reset and not any(x.reset for _, _, x in polls[k][1:])
        assert not any(x.overflow for _, _, x in polls[k])


def test_every_program_sees_every_kind_of_poll():
    _, _, polls, _ = _run()
    for k in range(len(wm.PROGRAMS)):
        later = [x for _, _, x in polls[k][1:]]                       # the first poll is the snapshot
        assert any(x.n_entered > 0 for x in later), k
        assert any(x.n_left > 0 for x in later), k
        assert any(x.n_entered == 0 and x.n_left == 0 for x in later), k
        assert all(0 < x.n_match < wm.N0 for x in later), k


def test_the_sparser_polls_report_net_changes():
    """between two polls of watch 1 or 2 some node's truth went there and back: it is in neither list"""
    m, _, polls, truth = _run()
    for k in (1, 2):
        skipped = 0
        for (r0, _, _), (r1, _, x) in zip(polls[k], polls[k][1:]):
            t = truth[k][r0 + 1:r1 + 2]                                 # the truth behind rounds r0 .. r1
            flipped = np.zeros(m.N, bool)
            for a, b in zip(t, t[1:]):
                flipped |= a != b
            back = flipped & (t[0] == t[-1])
            skipped += int(back.sum())
            both = np.concatenate([m.index_of(x.entered), m.index_of(x.left)])
            assert not back[both].any(), (k, r1)
        assert skipped > 0, k


def test_an_overflowing_poll_commits_nothing():
    m, first = wm.seeded_model(4)
    m.apply(first)
    ws = wm.Watches(m)
    ws.create(0, wm.FB, wm.PROGRAMS[0])
    snap = ws.poll(0, _pos(m))
    assert snap.reset and snap.n_entered == snap.n_match > 0 and snap.n_left == 0
    rounds = wm.seeded_rounds(m, 4)
    _, merge, tomb = next(rounds)
    m.apply(merge); m.apply(tomb)
    full = wm.Watches(m); full.create(0, wm.FB, wm.PROGRAMS[0]); full.committed[0][2][:] = ws.committed[0][2]; full.fresh.clear()
    want = full.poll(0, _pos(m))
    assert want.n_entered > 1 and want.n_left > 1
    short = ws.poll(0, _pos(m), cap_entered=want.n_entered - 1, cap_left=want.n_left)
    assert short.overflow and not short.reset and (short.n_entered, short.n_left) == (want.n_entered, want.n_left)
    again = ws.poll(0, _pos(m))
    assert not again.overflow and np.array_equal(again.entered, want.entered) and np.array_equal(again.left, want.left)
    ws.reset()
    x = ws.poll(0, _pos(m), cap_entered=0)
    assert x.reset and x.overflow and x.n_left == 0
    y = ws.poll(0, _pos(m))
    assert y.reset and not y.overflow and y.n_entered == y.n_match
    assert not ws.poll(0, _pos(m)).reset
