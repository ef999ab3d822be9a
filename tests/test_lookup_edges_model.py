"""No GPU: the arithmetic of tests/test_gpu_lookup_edges.py itself. The probe sequence of slot.h is replayed in numpy (its Model); this asserts that every
row of every case lands in the line its case says, that every probe takes the branches its case says, and that the cases together reach the home slot, the
crossing into the next line, two crossings, the wrap from the last line to line 0, the stop at an empty slot and the slot of the same id with another field —
for the four-slot lines of the table and the two-slot lines of the vector-clock table. It proves nothing about a kernel."""
import numpy as np
import pytest

import test_gpu_lookup_edges as lk
import test_gpu_sync_kernel_edges as edges


@pytest.mark.parametrize("spl", [4, 2])
def test_every_row_lands_where_its_case_says_and_every_branch_is_reached(spl):
    cases = lk.engine_cases() if spl == 4 else lk.vc_cases()
    m = lk.lay(cases, spl)                       # asserts the lines
    seen = lk.reached(m, cases)                  # asserts every probe's own branches
    assert seen >= set(lk.TAGS), sorted(set(lk.TAGS) - seen)
    assert len({c.name for c in cases}) == len(cases)
    names = {c.name for c in cases}
    assert {"home", "cross", "wrap", "two_full", "absent_far", "absent_near"} <= names
    assert sum(len(c.writes) for c in cases) <= 64, "a handful of rows per case"


def test_the_restated_home_slot_is_the_harness_own():
    T = edges.Table(None, lk.NSLOTS)
    for s in (0, 1, 5, 4094, 4095):
        id = int(T.ids_for([s], lk.FA, 2)[0])
        assert lk.home(id, lk.FA, lk.NSLOTS, 4) == s == edges.home_slot(id, lk.FA, lk.NSLOTS)
    for line in (0, 7, 2047):
        for salt in range(3):
            id = lk.node_in_line(line, lk.NSLOTS, 2, salt)
            assert {lk.home(id, f, lk.NSLOTS, 2) // 2 for f in (lk.FA, lk.FB, lk.FZ)} == {line}


def test_wrap_case_sits_in_the_last_line_and_line_0():
    for spl, cases in ((4, lk.engine_cases()), (2, lk.vc_cases())):
        m = lk.lay(cases, spl)
        nl = lk.NSLOTS // spl
        wrap = next(c for c in cases if c.name == "wrap")
        for id, field, _ in wrap.probes:
            assert lk.home(id, field, lk.NSLOTS, spl) // spl == nl - 1
            s = m.find(id, field)[0]
            assert s is None or s // spl == 0


def test_the_model_answers_of_the_engine_cases():
    cases = lk.engine_cases()
    m = lk.lay(cases, 4)
    got = lk.matches(m, lk.TERMS)
    assert sorted(v for _, v in got) == [11, 12, 13, 14, 17, 19]
    by_name = {c.name: c for c in cases}
    node = lambda name: by_name[name].writes[-1][0]
    assert lk.value_of(m, node("tomb_term"), lk.FB) == lk.DEL and not lk.holds(m, node("tomb_term"), lk.FB, -(1 << 62), 1 << 62)
    assert lk.value_of(m, node("absent_far"), lk.FB) is None and lk.value_of(m, node("absent_near"), lk.FC) is None
    ids, fields = lk.keys_of(cases)
    assert len(ids) == len(set(zip(ids.tolist(), fields.tolist())))
    assert sorted(lk.value_of(m, i, lk.FC) for i, _ in got if lk.value_of(m, i, lk.FC) not in (None, lk.DEL)) == sorted([5, -7, 9, 1 << 40, 8])
