"""GPU: the read-only lookup of the row (id, field) — the probe loop of k_get_rows, PredFilter::rest, agg_probe (aggregates and top-k) and k_vc_get — at the
edges of its probe sequence, through every consumer: get_rows, scan_filter on a plain index and through the value-ordered view, scan_aggregate with a second term and a measure from a third field, scan_top
with two terms — and EngineVC.get_rows for the two-slot lines of the vector-clock table (ProbeSeq<2>).

Built on the slot-layout harness of tests/test_gpu_sync_kernel_edges.py: Table.ids_for gives a node id whose key starts its probe sequence in a chosen
slot. The tables are the smallest the engine makes (4096 slots: 1024 lines of 4, or 2048 lines of 2). Every row is written by a call of its own, so where it
lands is determined: Model replays the probe sequence in numpy, a case says in which line each of its rows must land, and the premise asserts that the
device table IS the model (dump_rows / index_ids, or EngineVC.scan_range, in slot order). Every answer is compared exactly with the model's.

The cases, each a handful of rows in lines of its own:
  home         a key in its home slot
  cross        the home line already holds four rows: the key sits in the next line
  wrap         the same with the last line as home: the key sits in line 0
  two_full     two full lines in a row: the key sits two lines on
  absent_far   an absent key whose home line is full and whose next line has a free slot (the node's other field sits in that line)
  absent_near  an absent key that stops at an empty slot in its home line
  two_fields   fields of one id in one line (id equal, field not): four of them fill it, the second term's row sits behind them in the next line
  tomb_term    the second term's row is a tombstone: found by get_rows, matches no term
  tomb_measure the measure's row is a tombstone: the node matches, nothing is measured
  out_of_range the second term's row exists and lies outside the term (the control: presence alone does not satisfy a term)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from bmx import synth
import test_gpu_sync_kernel_edges as edges

DEL = bmx.VAL_DELETED
M64 = (1 << 64) - 1
EMPTY = M64
NSLOTS = 4096
FA, FB, FC, FZ, FY = (synth.fnv1a32(x) for x in ("age", "score", "weight", "filler", "extra"))   # term 0 / the index, the second term, the measure, the rows that crowd a line
T0 = (0, 1000)              # term 0's range: every case's FA value lies inside, except the node `outside`
T1 = (100, 200)             # the second term's range
TAGS = ["home slot", "crossing", "two crossings", "wrap", "stop at empty", "id equal, field not"]


def field_c(field, spl):
    return ((int(field) * 0x9E3779B9) & 0xFFFFFFFF) >> (30 if spl == 4 else 31)


def home(id, field, nslots, spl):
    h = edges.node_hash(int(id))
    return ((h * (nslots // spl)) >> 64) * spl + ((field_c(field, spl) + (h & 0xFFFFFFFF)) & (spl - 1))


def node_in_line(line, nslots, spl, salt):
    """a node id whose rows start in `line` (Table.ids_for's inversion, for any line width); another salt gives another id"""
    nl = nslots // spl
    h = (((line << 64) + nl - 1) // nl) + 1 + salt
    id = ((edges.unmix64(h) - edges.NH_ADD) * edges.NH_INV) & M64
    assert home(id, 0, nslots, spl) // spl == line and id != EMPTY
    return id


class Model:
    """the table slot by slot, filled through the restated probe sequence (slot.h ProbeSeq<SPL>)"""

    def __init__(self, nslots, spl):
        self.nslots, self.spl = nslots, spl
        self.id = [EMPTY] * nslots
        self.field = [0] * nslots
        self.ts = [0] * nslots
        self.val = [0] * nslots

    def find(self, id, field):
        """-> (slot of the row or None, slot where an insert would land or None, the branches the walk took)"""
        spl, nl = self.spl, self.nslots // self.spl
        line, c = divmod(home(id, field, self.nslots, spl), spl)
        h0, tags, k = line, set(), 0
        for _ in range(self.nslots):
            s = line * spl + ((c + k) & (spl - 1))
            if line != h0:
                tags.add("crossing")
                if (line - h0) % nl >= 2:
                    tags.add("two crossings")
                if line < h0:
                    tags.add("wrap")
            if self.id[s] == EMPTY:
                tags.add("stop at empty")
                return None, s, tags
            if self.id[s] == id:
                if self.field[s] == field:
                    if s == home(id, field, self.nslots, spl):
                        tags.add("home slot")
                    return s, None, tags
                tags.add("id equal, field not")
            k += 1
            if k & (spl - 1) == 0:
                line = 0 if line + 1 == nl else line + 1
        return None, None, tags

    def put(self, id, field, ts, val):
        """stored as given: a key that has a row keeps its slot"""
        s, free, _ = self.find(id, field)
        s = free if s is None else s
        assert s is not None
        self.id[s], self.field[s], self.ts[s], self.val[s] = id, field, ts, val
        return s

    def rows(self, field=None, tombstones=True):
        """(slot, id, field, ts, val) in slot order"""
        return [(s, self.id[s], self.field[s], self.ts[s], self.val[s]) for s in range(self.nslots)
                if self.id[s] != EMPTY and (field is None or self.field[s] == field) and (tombstones or self.val[s] != DEL)]


class Case:
    def __init__(self, name):
        self.name, self.writes, self.lines, self.probes = name, [], [], []

    def row(self, id, field, val, line):
        """one row, written in this order; `line`: where it must land. A tombstone is a row written first and deleted by a second call."""
        if val == DEL:
            self.row(id, field, 1, line)
        self.writes.append((id, field, 7 + len(self.writes), val)); self.lines.append(line)
        return self

    def probe(self, id, field, expect):
        """a key the lookup is asked for, and the branches its walk must take"""
        self.probes.append((id, field, set(expect)))
        return self


def engine_cases():
    """lines 1023 / 0 / 1 belong to `wrap`; every other case has lines of its own"""
    T = edges.Table(None, NSLOTS)
    nl = NSLOTS // 4

    def node(line, salt=0):         # an id whose FA row starts in slot 4 * line + 1
        return int(T.ids_for([4 * line + 1], FA, salt)[0])

    def crowd(c, line, salt0):      # four rows of four other nodes: the line is full
        for k in range(4):
            c.row(int(T.ids_for([4 * line + k], FZ, salt0 + k)[0]), FZ, 1, line)

    out = []
    n = node(10)
    out.append(Case("home").row(n, FA, 11, 10).row(n, FB, 150, 10).row(n, FC, 5, 10).probe(n, FA, ["home slot"]))
    c = Case("cross"); n = node(20); crowd(c, 20, 1)
    out.append(c.row(n, FA, 12, 21).row(n, FB, 150, 21).row(n, FC, -7, 21).probe(n, FB, ["crossing"]).probe(n, FC, ["crossing"]))
    c = Case("wrap"); n = node(nl - 1); crowd(c, nl - 1, 1)
    out.append(c.row(n, FA, 13, 0).row(n, FB, 200, 0).row(n, FC, 9, 0).probe(n, FB, ["crossing", "wrap"]).probe(n, FC, ["crossing", "wrap"]))
    c = Case("two_full"); n = node(30); crowd(c, 30, 1); crowd(c, 31, 5)
    out.append(c.row(n, FA, 14, 32).row(n, FB, 100, 32).row(n, FC, 1 << 40, 32).probe(n, FB, ["two crossings"]).probe(n, FC, ["two crossings"]))
    c = Case("absent_far"); n = node(40); crowd(c, 40, 1)
    out.append(c.row(n, FA, 15, 41).probe(n, FB, ["crossing", "stop at empty"]).probe(n, FC, ["crossing", "stop at empty"]))
    n = node(50)
    out.append(Case("absent_near").row(n, FA, 16, 50).probe(n, FB, ["stop at empty"]).probe(n, FC, ["stop at empty"]))
    n = node(60)
    out.append(Case("two_fields").row(n, FA, 17, 60).row(n, FC, 8, 60).row(n, FZ, 1, 60).row(n, FY, 1, 60).row(n, FB, 199, 61)
               .probe(n, FB, ["id equal, field not", "crossing"]).probe(n, FC, []))
    n = node(70)
    out.append(Case("tomb_term").row(n, FA, 18, 70).row(n, FB, DEL, 70).row(n, FC, 3, 70).probe(n, FB, []))
    n = node(80)
    out.append(Case("tomb_measure").row(n, FA, 19, 80).row(n, FB, 101, 80).row(n, FC, DEL, 80).probe(n, FC, []))
    n = node(90)
    out.append(Case("out_of_range").row(n, FA, 20, 90).row(n, FB, 201, 90).row(n, FC, 4, 90).probe(n, FB, []))
    n = node(100)
    out.append(Case("outside").row(n, FA, 1001, 100).row(n, FB, 150, 100).row(n, FC, 6, 100).probe(n, FA, ["home slot"]))
    return out


def vc_cases():
    """the vector-clock table: 2048 lines of two 64-byte slots"""
    nl = NSLOTS // 2

    def node(line, salt=0):
        return node_in_line(line, NSLOTS, 2, salt)

    def crowd(c, line, salt0):
        for k in range(2):
            c.row(node(line, salt0 + k), FZ, 1, line)

    out = []
    n = node(10)
    out.append(Case("home").row(n, FA, 11, 10).row(n, FB, 16, 10).probe(n, FA, ["home slot"]).probe(n, FZ, ["id equal, field not", "crossing", "stop at empty"]))
    c = Case("cross"); n = node(20); crowd(c, 20, 1)
    out.append(c.row(n, FA, 12, 21).row(n, FB, 13, 21).probe(n, FA, ["crossing"]).probe(n, FB, ["crossing"]))
    c = Case("wrap"); n = node(nl - 1); crowd(c, nl - 1, 1)
    out.append(c.row(n, FA, 14, 0).probe(n, FA, ["crossing", "wrap"]).probe(n, FB, ["crossing", "wrap", "stop at empty"]))
    c = Case("two_full"); n = node(30); crowd(c, 30, 1); crowd(c, 31, 3)
    out.append(c.row(n, FA, 15, 32).probe(n, FA, ["two crossings"]))
    c = Case("absent_far"); n = node(40); crowd(c, 40, 1)
    out.append(c.probe(n, FA, ["crossing", "stop at empty"]))
    out.append(Case("absent_near").probe(node(50), FA, ["stop at empty"]))
    return out


def lay(cases, spl, write=None):
    """the model of the cases, written row by row (write: the device's one-row call); asserts that every row landed in the line its case says"""
    m = Model(NSLOTS, spl)
    for c in cases:
        for (id, field, ts, val), line in zip(c.writes, c.lines):
            s = m.put(id, field, ts, val)
            assert s // spl == line, (c.name, "row", hex(id), field, "landed in slot", s, "not in line", line)
            if write:
                write(id, field, ts, val)
    return m


def reached(m, cases):
    """the branches the cases' probes take in the model; asserts what every probe says of itself"""
    seen = set()
    for c in cases:
        for id, field, expect in c.probes:
            tags = m.find(id, field)[2]
            assert expect <= tags, (c.name, hex(id), field, "was meant to reach", sorted(expect), "and reached", sorted(tags))
            seen |= tags
    return seen


# ---- the model's answers ----

def keys_of(cases):
    """every key the cases name: the rows written and the keys probed"""
    ks = []
    for c in cases:
        ks += [(id, f) for id, f, _, _ in c.writes] + [(id, f) for id, f, _ in c.probes]
    ks = sorted(set(ks))                                        # (a tombstone's key was written twice)
    return np.asarray([k[0] for k in ks], np.uint64), np.asarray([k[1] for k in ks], np.uint32)


def value_of(m, id, field):
    """the row's value; None: absent"""
    s = m.find(id, field)[0]
    return None if s is None else m.val[s]


def holds(m, id, field, lo, hi):
    v = value_of(m, id, field)
    return v is not None and v != DEL and lo <= v <= hi


def matches(m, terms):
    """(id, value of term 0's field) of the nodes that satisfy every term, in index (slot) order"""
    f0, lo, hi = terms[0]
    return [(id, v) for _, id, _, _, v in m.rows(f0, tombstones=False) if lo <= v <= hi and all(holds(m, id, f, a, b) for f, a, b in terms[1:])]


def _same(got, want, what):
    edges._same(got, want, what)


# ---- the device tables, laid out once ----

class Laid:
    pass


@pytest.fixture(scope="module")
def table():
    cases = engine_cases()
    cap = edges.capacity_for(NSLOTS)
    with bmx.Engine(cap, flags=bmx.CTX_FIXED_CAPACITY, load_pct=90) as e:
        one = lambda id, f, ts, v: e.put_rows([id], [f], [ts], [v])
        t = Laid(); t.e, t.cases = e, cases
        t.m = lay(cases, 4, one)
        # the premise: the device table is the model
        assert e.info().n_slots == NSLOTS, "the table did not grow"
        rows = t.m.rows(tombstones=False)
        for g, k, col in zip(e.dump_rows(), (1, 2, 3, 4), ("id", "field", "ts", "val")):
            _same(g, np.asarray([r[k] for r in rows], g.dtype), ("dump_rows in slot order", col))
        for f in (FA, FB, FC):
            e.index_build(f)
            _same(e.index_ids(f), np.asarray([r[1] for r in t.m.rows(f)], np.uint64), ("index_ids in slot order, tombstones included", f))
        yield t


def test_get_rows(table):
    e, m = table.e, table.m
    ids, fields = keys_of(table.cases)
    ts, val, found = e.get_rows(ids, fields)
    slot = [m.find(int(i), int(f))[0] for i, f in zip(ids, fields)]
    _same(found, np.asarray([s is not None for s in slot]), "found")
    _same(ts, np.asarray([0 if s is None else m.ts[s] for s in slot], np.int64), "ts")
    _same(val, np.asarray([0 if s is None else m.val[s] for s in slot], np.int64), "val (a tombstone is found, with VAL_DELETED)")
    assert (val == DEL).sum() == 2 and (~found).sum() >= 4


TERMS = [(FA, *T0), (FB, *T1)]


def _check_queries(e, m, what):
    want = matches(m, TERMS)
    assert sorted(v for _, v in want) == [11, 12, 13, 14, 17, 19], "the cases' own arithmetic"
    _same(np.sort(e.scan_filter(TERMS)), np.sort(np.asarray([i for i, _ in want], np.uint64)), (what, "scan_filter"))
    a = e.scan_aggregate(TERMS, measure=FC)
    meas = [value_of(m, i, FC) for i, _ in want]
    meas = [v for v in meas if v is not None and v != DEL]
    assert sorted(meas) == sorted([5, -7, 9, 1 << 40, 8]), "the cases' own arithmetic"
    assert (a.n_match, a.n, a.sum, a.min, a.max) == (len(want), len(meas), sum(meas), min(meas), max(meas)), (what, "scan_aggregate")
    order = sorted(want, key=lambda r: (r[1], r[0]))
    for k in (1, 3, len(want), len(want) + 5):
        recs, ne = e.scan_top(TERMS, k)
        assert ne == len(want), (what, "scan_top n_eligible", k)
        _same(recs["id"], np.asarray([i for i, _ in order[:k]], np.uint64), (what, "scan_top ids", k))
        _same(recs["val"], np.asarray([v for _, v in order[:k]], np.int64), (what, "scan_top values", k))


def test_filter_aggregate_top_on_the_plain_index(table):
    assert table.e.index_ordered_stats(FA)["sorts"] == 0
    _check_queries(table.e, table.m, "plain index")


def test_filter_aggregate_top_through_the_ordered_view(table):
    e = table.e
    e.index_set_ordered(FA, 1)
    _check_queries(e, table.m, "ordered view")
    assert e.index_ordered_stats(FA)["sorts"] == 1, "the queries went through the view"
    e.index_set_ordered(FA, 0)


def test_vc_get_rows():
    cases = vc_cases()
    K = 2
    e = bmx.EngineVC(NSLOTS // 2, K, 0)
    try:
        one = lambda id, f, ts, v: e.load_rows([id], [f], np.asarray([[ts, 0]], np.uint32), [v])
        m = lay(cases, 2, one)
        for f in (FA, FB, FZ):      # the premise: scan_range answers in slot order
            _same(e.scan_range(f, -(1 << 53) + 1, (1 << 53) - 1), np.asarray([r[1] for r in m.rows(f)], np.uint64), ("scan_range in slot order", f))
        ids, fields = keys_of(cases)
        clocks, val, state = e.get_rows(ids, fields)
        slot = [m.find(int(i), int(f))[0] for i, f in zip(ids, fields)]
        _same(state != 0, np.asarray([s is not None for s in slot]), "state: absent or not")
        _same(val, np.asarray([0 if s is None else m.val[s] for s in slot], np.int64), "val")
        _same(clocks[:, 0], np.asarray([0 if s is None else m.ts[s] for s in slot], np.uint32), "clock of writer 0")
        _same(clocks[:, 1], np.zeros(len(ids), np.uint32), "clock of writer 1")
        assert (state == 0).sum() >= 4
    finally:
        e.close()
