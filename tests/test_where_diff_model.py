"""CPU: the model of the field-to-field literals (tests/where_diff_model.py) against itself. The brute force is the header's sentences with Python ints; the stand-in
walks a program the way where_prepare and PredWhere::row do. The seeded cases must reach every path of the stand-in, see every combination of states with both
outcomes, and expose each single defect the stand-in can be given."""
import numpy as np
import pytest

import where_diff_model as wdm
from where_diff_model import ABSENT, DATA, TOMB, F1, F2, F3, F4, FB, I64MAX, I64MIN, VAL_MAX

N = 300


@pytest.fixture(scope="module")
def table():
    m, tombs = wdm.seeded_table(N)
    wdm.apply_tombs(m, tombs)
    return m


@pytest.fixture(scope="module")
def programs():
    return wdm.seeded_programs()


@pytest.fixture(scope="module")
def truth(table, programs):
    return [wdm.brute(table, FB, p) for p in programs]


def test_the_generator_keeps_the_limits(programs):
    assert len(programs) == 100
    for p in programs:
        assert 1 <= len(p) <= 8 and all(1 <= wdm.entries(c) <= 8 for c in p) and sum(wdm.entries(c) for c in p) <= 32
        assert len(wdm.prepare(FB, p)["slots"]) <= 8
    mixed = sum(any(wdm.is_pair(t) for c in p for t in c) and any(not wdm.is_pair(t) for c in p for t in c) for p in programs)
    assert 3 * mixed >= len(programs), mixed
    assert any(all(not wdm.is_pair(t) for c in p for t in c) for p in programs), "plain programs stay among them"
    pairs = [{tuple(t[0]) for c in p for t in c if wdm.is_pair(t)} for p in programs]
    assert any((b, a) in s for s in pairs for (a, b) in s), "(A, B) next to (B, A)"
    assert any(FB == a for s in pairs for (a, b) in s) and any(FB == b for s in pairs for (a, b) in s)


def test_the_numpy_model_is_the_brute_force(table, programs, truth):
    counts = []
    for p, want in zip(programs, truth):
        assert np.array_equal(table.mask(FB, p), want), p
        counts.append(int(want.sum()))
    ncand = int((table.st[FB] == DATA).sum())
    assert sum(0 < c < ncand for c in counts) >= 40, counts


def test_the_stand_in_is_the_brute_force_on_every_path(table, programs, truth):
    tags, seen, probes = set(), set(), []
    for p, want in zip(programs, truth):
        assert np.array_equal(wdm.standin(table, FB, p, tags=tags, probes=probes, seen=seen), want), p
    assert tags == set(wdm.TAGS), set(wdm.TAGS) - tags
    assert seen == {(a, b, t) for a in (ABSENT, DATA, TOMB) for b in (ABSENT, DATA, TOMB) for t in (False, True)}, "9 state combinations, each true and false"
    assert FB not in probes, "the base side of a pair is the column value"


@pytest.mark.parametrize("defect", wdm.DEFECTS)
def test_the_seeded_cases_expose_each_defect(table, programs, truth, defect):
    exposed = 0
    for p, want in zip(programs, truth):
        probes = []
        got = wdm.standin(table, FB, p, defect=defect, probes=probes)
        exposed += (FB in probes) if defect == "base_from_probe" else not np.array_equal(got, want)
    assert exposed >= 3, (defect, exposed)


def test_the_headers_examples():
    """a == b, a != b, a > b, a <= b + 5, both present, lo > hi, the extremes — on hand-made nodes"""
    m = wdm.DiffModel(wdm.node_ids(9))
    m.set(FB, np.arange(9), np.arange(9))
    #    node:      0 equal, 1 a > b, 2 a < b, 3 A absent, 4 B absent, 5 A tombstoned, 6 B tombstoned, 7 max - min, 8 min - max
    m.set(F1, [0, 1, 2, 4, 5, 6, 7, 8], [4, 9, 1, 3, 3, 3, VAL_MAX, -VAL_MAX])
    m.set(F2, [0, 1, 2, 3, 5, 6, 7, 8], [4, 3, 7, 3, 3, 3, -VAL_MAX, VAL_MAX])
    m.tomb(F1, [5]); m.tomb(F2, [6])
    P = (F1, F2)

    def ask(t):
        got = wdm.brute(m, FB, [[t]])
        assert np.array_equal(got, wdm.standin(m, FB, [[t]])) and np.array_equal(got, m.mask(FB, [[t]]))
        return set(np.nonzero(got)[0].tolist())

    assert ask((P, 0, 0)) == {0} and ask((P, 0, 0, True)) == {1, 2, 3, 4, 5, 6, 7, 8}
    assert ask((P, 1, I64MAX)) == {1, 7} and ask((P, I64MIN, -1)) == {2, 8}
    assert ask((P, I64MIN, 5)) == {0, 2, 8} and ask((P, I64MIN, 6)) == {0, 1, 2, 8}
    assert ask((P, I64MIN, I64MAX)) == {0, 1, 2, 7, 8} and ask((P, I64MIN, I64MAX, True)) == {3, 4, 5, 6}
    assert ask((P, 5, 4)) == set() and ask((P, 5, 4, True)) == set(range(9))
    assert ask((P, 2 * VAL_MAX, 2 * VAL_MAX)) == {7} and ask((P, -2 * VAL_MAX, -2 * VAL_MAX)) == {8}
    assert ask((P, 2 * VAL_MAX + 1, I64MAX)) == set() and ask(((F2, F1), 2 * VAL_MAX, I64MAX)) == {8}
    assert ask(((FB, F2), 0, 0)) == {3} and ask(((F2, FB), 4, 4)) == {0}
    assert ask(((F3, F4), I64MIN, I64MAX, True)) == set(range(9)), "fields nobody has"


def test_refusals_of_the_stand_in():
    with pytest.raises(ValueError, match="minus itself"):
        wdm.prepare(FB, [[((F1, F1), 0, 0)]])
    five = [[((F1, F2), 0, 0)] * 4, [((F1, F2), 0, 0)]]
    assert len(wdm.prepare(FB, five)["slots"]) == 1 and len(wdm.prepare(FB, five)["lit"]) == 5
    with pytest.raises(ValueError, match="1..8 literals"):
        wdm.prepare(FB, [[((F1, F2), 0, 0)] * 5])
    nine = [[((100 + k, 200 + k), 0, 0) for k in range(4)], [((104 + k, 204 + k), 0, 0) for k in range(4)], [((108, 208), 0, 0)]]
    with pytest.raises(ValueError, match="no slot left"):
        wdm.prepare(FB, nine)
    assert len(wdm.prepare(FB, nine[:2])["slots"]) == 8
