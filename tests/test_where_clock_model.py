"""CPU: the model of the clock literals (tests/where_clock_model.py) against itself. The brute force is the header's sentences with Python ints; the stand-in
walks a program the way where_prepare and PredWhere::row do. The seeded cases must reach every path of the stand-in, and the layouts of the kernel-edge tests
must expose each single defect the stand-in can be given.

One defect, "clock_clamped" (a clock bound clamped to +-(2^53 - 1) like a value bound), changes no answer while every stored clock lies in 0..2^53 - 1, which the
engine guarantees: it is shown on a model row whose clock lies beyond that, which no table on the device can hold."""
import numpy as np
import pytest

import bmx
import where_clock_model as wcm
from where_clock_model import ABSENT, CK, DATA, TOMB, F1, F2, F3, F4, FB, I64MAX, I64MIN, TS_MAX

N = 300


@pytest.fixture(scope="module")
def table():
    return wcm.seeded_table(N)


@pytest.fixture(scope="module")
def programs():
    return wcm.seeded_programs()


@pytest.fixture(scope="module")
def truth(table, programs):
    return [wcm.brute(table, FB, p) for p in programs]


def test_the_literal_of_the_binding():
    assert (bmx.LIT_CLOCK, bmx.LIT_CLOCK_TOMB) == (16, 32)
    assert (CK(7).flags, CK(7, "deleted").flags, CK(7, "any").flags) == (16, 32, 48)
    assert bmx.Clock(7).flags == 16 and bmx.Clock(7, data=False, tombs=True).flags == 32 and bmx.Clock(7, tombs=True).flags == 48
    with pytest.raises(ValueError):
        bmx.Clock(7, data=False)
    base, nc, lens, lits = bmx._where_args(7, [[(7, 1, 2), (CK(9), 5, I64MAX), ((9, 7), 0, 0)], [(CK(7, "deleted"), I64MIN, I64MAX, True)], [(CK(11, "any"), 3, 4, False)]])
    assert (base, nc, list(lens)) == (7, 3, [4, 1, 1])
    assert [(l.field, l.flags, l.lo, l.hi) for l in lits] == [(7, 0, 1, 2), (9, 16, 5, I64MAX), (9, 4, 0, 0), (7, 8, 0, 0), (7, 32 | 1, I64MIN, I64MAX), (11, 48, 3, 4)]


def test_the_generator_mixes_all_three_kinds(programs):
    assert len(programs) == 100
    kinds = []
    for p in programs:
        assert 1 <= len(p) <= 8 and all(1 <= wcm.entries(c) <= 8 for c in p) and sum(wcm.entries(c) for c in p) <= 32
        assert len(wcm.prepare(FB, p)["slots"]) <= 8
        kinds.append({"clock" if wcm.is_clock(t) else "pair" if wcm.is_pair(t) else "plain" for c in p for t in c})
    assert sum(len(k) == 3 for k in kinds) >= 30 and sum("clock" in k for k in kinds) >= 80
    states = {t[0].flags for p in programs for c in p for t in c if wcm.is_clock(t)}
    assert states == {16, 32, 48}
    assert any(wcm.is_clock(t) and t[0].field == FB for p in programs for c in p for t in c)


def test_the_numpy_model_is_the_brute_force(table, programs, truth):
    counts = []
    for p, want in zip(programs, truth):
        assert np.array_equal(table.mask(FB, p), want), p
        counts.append(int(want.sum()))
    ncand = int((table.st[FB] == DATA).sum())
    assert sum(0 < c < ncand for c in counts) >= 40, counts


def test_the_stand_in_is_the_brute_force_on_every_path(table, programs, truth):
    tags, probes = set(), []
    for p, want in zip(programs, truth):
        assert np.array_equal(wcm.standin(table, FB, p, tags=tags, probes=probes), want), p
    assert tags == set(wcm.TAGS), set(wcm.TAGS) - tags
    assert (FB, "ts") in probes and (FB, "val") not in probes, "the base field is probed for its clock alone"


def test_one_slot_and_one_probe_per_field():
    W = wcm.prepare(FB, [[(F1, 0, 5), (CK(F1), 3, 9), (CK(F1, "deleted"), 0, 2, True)], [(CK(F1, "any"), 0, 0), (F1, 1, 1, True), ((F1, F2), 0, 0)], [(CK(FB), 1, 2), (FB, 0, 9)]])
    assert W["slots"] == [(F1, None), (F1, F2), (FB, None)] and W["slot_clock"] == [True, False, True]
    assert W["lit"][W["cbeg"][2]][0] == 0 and W["lit"][W["cbeg"][2] + 1][0] == 3, "the base value literal in front, the base clock literal among the probed"
    m = wcm.ClockModel(wcm.node_ids(1))
    m.set(FB, [0], [4], ts=1); m.set(F1, [0], [9], ts=0); m.set(F2, [0], [8])
    probes = []
    assert wcm.standin(m, FB, [[(F1, 0, 5)], [(CK(F1), 3, 9)], [(F1, 9, 9), (CK(F1, "any"), 0, 0)]], probes=probes).tolist() == [True]
    assert probes == [(F1, "ts")], "three clauses, two kinds of literal, one probe"
    eight = [[(CK(100 + k, "any"), 0, 9) for k in range(4)], [(CK(104 + k), 0, 9) for k in range(3)] + [(CK(FB), 0, 9)]]
    assert len(wcm.prepare(FB, eight)["slots"]) == 8
    with pytest.raises(ValueError, match="8 fields"):
        wcm.prepare(FB, eight + [[(CK(200, "deleted"), 0, 9)]])


def test_the_headers_examples():
    m = wcm.ClockModel(wcm.node_ids(8))
    m.set(FB, np.arange(8), np.arange(8), ts=4)
    #    node: 0 absent, 1 data@10, 2 data@20, 3 deleted@10, 4 deleted@20, 5 data@0, 6 data@2^53-1, 7 deleted@0
    m.set(F1, [1, 2, 3, 4, 5, 6, 7], [10, 1, 1, 1, 1, 1, 1], ts=np.array([10, 20, 5, 5, 0, TS_MAX, 0]))
    m.tomb(F1, [3, 4, 7], ts=np.array([10, 20, 0]))
    every = set(range(8))

    def ask(t):
        got = wcm.brute(m, FB, [[t]])
        assert np.array_equal(got, wcm.standin(m, FB, [[t]])) and np.array_equal(got, m.mask(FB, [[t]])), t
        return set(np.nonzero(got)[0].tolist())

    assert ask((CK(F1), 11, I64MAX)) == {2, 6}, "written after clock 10"
    assert ask((CK(F1, "deleted"), 11, I64MAX)) == {4}, "deleted since 10"
    assert ask((CK(F1, "deleted"), I64MIN, I64MAX)) == {3, 4, 7}, "the field is deleted"
    assert ask((CK(F1, "any"), I64MIN, I64MAX)) == every - {0} and ask((CK(F1, "any"), I64MIN, I64MAX, True)) == {0}, "a row exists"
    assert ask((CK(F1), 10, 10)) == {1} and ask((CK(F1), 10, 10, True)) == every - {1} and ask((CK(F1, "any"), 10, 10)) == {1, 3}
    assert ask((CK(F1), 0, 0)) == {5} and ask((CK(F1, "any"), 0, 0)) == {5, 7} and ask((CK(F1), I64MIN, 0)) == {5} and ask((CK(F1), I64MIN, -1)) == set()
    assert ask((CK(F1), TS_MAX, TS_MAX)) == {6} and ask((CK(F1), TS_MAX, I64MAX)) == {6} and ask((CK(F1), TS_MAX + 1, I64MAX)) == set()
    assert ask((CK(F1), I64MIN, I64MIN)) == set() and ask((CK(F1, "any"), I64MIN, I64MIN, True)) == every, "a tombstone's value is no clock"
    assert ask((CK(F1, "any"), 20, 10)) == set() and ask((CK(F1, "any"), 20, 10, True)) == every, "lo > hi"
    assert ask((CK(FB), 4, 4)) == every and ask((CK(FB), 0, 3)) == set() and ask((CK(FB, "deleted"), I64MIN, I64MAX)) == set()
    assert ask((CK(F3, "any"), I64MIN, I64MAX, True)) == every, "a field nobody has"


def _edge_runs(defect=None):
    """the kernel-edge layouts at a size with a ragged unit, both widths -> the cases (name) whose stand-in answer differs from the truth"""
    wrong, total = [], 0
    for wide, E in ((False, 4), (True, 2)):
        n = 65
        ids = wcm.node_ids(n, 4000)
        node = np.random.default_rng(5).permutation(n)
        m = wcm.edge_table(ids, node, E, wide)
        for name, mutate, clauses, want, _ in wcm.edge_cases(m, node, E, wide):
            if mutate:
                mutate(lambda f, idx, vals, ts: m.tomb(f, idx, ts) if vals is None else m.set(f, idx, vals, ts))
            truth = wcm.brute(m, FB, clauses)
            assert np.array_equal(np.nonzero(truth[node])[0], want), (name, want[:8])
            assert np.array_equal(m.mask(FB, clauses), truth), name
            total += 1
            if not np.array_equal(wcm.standin(m, FB, clauses, defect=defect), truth):
                wrong.append(name)
    assert total >= 30
    return wrong


def test_the_edge_layouts_are_what_they_say():
    assert _edge_runs() == []


@pytest.mark.parametrize("defect", [d for d in wcm.DEFECTS if d != "clock_clamped"])
def test_the_edge_layouts_expose_each_defect(defect):
    assert len(_edge_runs(defect)) >= 2, defect


def test_a_clamped_clock_bound_shows_only_beyond_the_clock_domain(table, programs, truth):
    for p, want in zip(programs, truth):
        assert np.array_equal(wcm.standin(table, FB, p, defect="clock_clamped"), want), "clocks in 0..2^53 - 1: the clamp is invisible"
    m = wcm.ClockModel(wcm.node_ids(1))
    m.set(FB, [0], [1]); m.set(F1, [0], [1], ts=TS_MAX + 1)              # (a model row only)
    t = [[(CK(F1), TS_MAX + 1, I64MAX)]]
    assert wcm.brute(m, FB, t).tolist() == [True] and wcm.standin(m, FB, t).tolist() == [True]
    assert wcm.standin(m, FB, t, defect="clock_clamped").tolist() == [False]


@pytest.mark.parametrize("defect", [d for d in wcm.DEFECTS if d != "clock_clamped"])
def test_the_seeded_cases_expose_each_defect(table, programs, truth, defect):
    exposed = sum(not np.array_equal(wcm.standin(table, FB, p, defect=defect), want) for p, want in zip(programs, truth))
    assert exposed >= 3, (defect, exposed)
