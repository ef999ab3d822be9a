"""GPU: exact quantiles over boolean filters (include/bmx_quant.h bmx_where_quantiles). Every answer is compared byte for byte — all 32 bytes of every record and
of the result record, and the fill pattern behind the last record — with quant_model.quantiles: numpy.sort of the sample the test itself loaded, bmx.quant_rank
for the rank, searchsorted for n_below and n_equal.

The shapes are the smallest at which each piece can go wrong (csrc/quant_kernels.h): a digit is 11 bits, so a sample whose values span 2^12 already runs two
digit passes; one round of a workgroup is 8192 int32 rows or 4096 int64 rows; a base value >= 2^31 forces the int64 column."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import quant_model as qm
import where_agg_model as wam
from oracle import streams
from where_agg_model import ABSENT, DATA, TOMB, Model

FB, F1, F2, F3, FM = (streams.fnv1a32(s) for s in ("base", "one", "two", "three", "measure"))
MORE = [streams.fnv1a32("more%d" % k) for k in range(6)]
NOBODY = streams.fnv1a32("nobody")
EVERY = [[(NOBODY, 0, 0, True)]]            # a negated literal on a field nobody has: true for every candidate
I64MIN, I64MAX = wam.I64MIN, wam.I64MAX
BIG, WIDE = 2**53 - 1, 2**40
QUARTILES = [(1, 4), (1, 2), (3, 4)]
EIGHT = [(1, 2), (0, 1), (99, 100), (1, 1), (1, 4), (95, 100), (1, 2), (3, 4)]       # unsorted, one repeated


def _engine(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    return e


def _check(x, m, base, clauses, measure, qs):
    got = qm.raw(x, base, clauses, measure, qs)
    want = qm.quantiles(m, base, clauses, measure, qs)
    assert qm.same(got, want) is None, (clauses, measure, qs, qm.same(got, want))
    return got


def _model(n, seed, wide=False):
    """a base field on every node, three program fields and a measure in every state, the measure with a wide value span"""
    rng = np.random.default_rng(seed)
    m = Model(wam.node_ids(n, 300 * seed))
    m.set(FB, np.arange(n), (WIDE if wide else 0) + rng.integers(-300, 300, n))
    for f, pr in ((F1, 0.9), (F2, 0.6), (F3, 0.3)):
        idx = np.nonzero(rng.random(n) < pr)[0]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
    idx = np.nonzero(rng.random(n) < 0.8)[0]
    m.set(FM, idx, rng.integers(-(2**30), 2**34, len(idx)))
    return m


# ---- 1. the truth table: selection x the three cell states of the measure; the measure as base field, program field and unnamed field ----
@pytest.mark.parametrize("wide", [False, True])
def test_truth_table_and_measure_sources(wide):
    n = 600
    off = WIDE if wide else 0
    m = Model(wam.node_ids(n, 4100 + wide))
    k = np.arange(n)
    m.set(FB, k[k % 5 != 4], off + (k[k % 5 != 4] * 37) % 211)                 # a fifth of the nodes have no base row: outside every universe
    m.set(F1, k[k % 2 == 0], k[k % 2 == 0] % 7)                                # the program field: selects or not
    m.set(FM, k[k % 3 != 2], (k[k % 3 != 2] * 101) % 5000 - 2500)              # the measure: data, tombstone (below) or absent
    with _engine(m, (FB, F1, FM)) as e:
        wam.tombstone(e, m, FM, k[k % 3 == 1]); wam.tombstone(e, m, FB, k[k % 35 == 3]); wam.tombstone(e, m, F1, k[k % 22 == 0])
        sel = m.mask(FB, [[(F1, 0, 3)]])
        for s in (True, False):
            for st in (DATA, TOMB, ABSENT):
                assert ((sel == s) & (m.st[FM] == st) & (m.st[FB] == DATA)).sum() > 5, "every cell of the truth table"
        for p in ([[(F1, 0, 3)]], [[(F1, 0, 3, True)]], EVERY, [[(FB, off + 10, off + 150), (F1, 2, 6)], [(FM, 0, I64MAX)]]):
            for measure in (FB, F1, FM, NOBODY):                               # the column, a program field, an unnamed field, a field nobody has (n = 0)
                recs, res = _check(e, m, FB, p, measure, EIGHT)
                assert int(res["n_match"]) == e.scan_where(FB, p, count_only=True)
                a = e.where_aggregate(FB, p, measure=measure)
                assert (int(res["n_match"]), int(res["n"])) == (a.n_match, a.n)
                if a.n:        # 0/1 and 1/1 are the minimum and the maximum, res's and where_aggregate's
                    assert int(recs[1]["value"]) == int(res["min"]) == a.min and int(recs[3]["value"]) == int(res["max"]) == a.max
                    assert int(recs[1]["n_below"]) == 0 and int(recs[3]["n_below"]) + int(recs[3]["n_equal"]) == a.n
                else:
                    assert measure == NOBODY and (int(res["min"]), int(res["max"])) == (I64MAX, I64MIN) and not recs.view(np.uint8).any()
                assert recs[0].tobytes() == recs[6].tobytes(), "a repeated quantile gives the same record"
        # the measure is a field of the program that is ALSO probed by it, in a clause that fails early for some lanes
        _check(e, m, FB, [[(F1, 5, 6), (FM, -100, 100)], [(FM, 0, 2500)]], FM, QUARTILES)


# ---- 2. tiny samples ----
def test_empty_single_and_pair():
    n = 300
    m = Model(wam.node_ids(n, 4300))
    m.set(FB, np.arange(n), np.arange(n) % 50)
    m.set(F1, np.arange(0, 100), np.arange(100) % 4)
    m.set(FM, np.arange(200, 300), np.arange(100) - 50)
    with _engine(m, (FB, F1, FM)) as e:
        for qs in ([(1, 2)], EIGHT):
            recs, res = _check(e, m, FB, [[(FB, 100, 200)]], FB, qs)            # no match
            assert (int(res["n_match"]), int(res["n"]), int(res["min"]), int(res["max"])) == (0, 0, I64MAX, I64MIN) and not recs.view(np.uint8).any()
            recs, res = _check(e, m, FB, [[(F1, 0, 3)]], FM, qs)                # matches, none of them measured
            assert (int(res["n_match"]), int(res["n"])) == (100, 0) and not recs.view(np.uint8).any()
        # n = 1: every quantile is the one element
        m.set(F2, [17], [1])
        e.load_rows(*m.rows(F2, 6))
        for measure in (FB, F2, F1):
            recs, res = _check(e, m, FB, [[(F2, 1, 1)]], measure, EIGHT)
            assert int(res["n"]) == 1 and all(r.tobytes() == recs[0].tobytes() for r in recs) and (int(recs[0]["rank"]), int(recs[0]["n_equal"])) == (0, 1)
        # n = 2: 1/2 is the lower of the two
        m.set(F2, [250], [1])
        e.put_rows(*m.rows(F2, 7))
        for measure, lower in ((FB, min(17 % 50, 250 % 50)), (FM, None)):
            recs, res = _check(e, m, FB, [[(F2, 1, 1)]], measure, [(1, 2), (2, 4), (0, 1), (1, 1)])
            if lower is not None:
                assert int(res["n"]) == 2 and int(recs[0]["value"]) == lower == int(recs[2]["value"]) and int(recs[3]["value"]) == max(17 % 50, 250 % 50)
            assert recs[0].tobytes() == recs[1].tobytes(), "1/2 and 2/4"


# ---- 3. values at the ends of the domain; a value held 10^4 times ----
@pytest.mark.parametrize("probe", [False, True])
def test_domain_ends_and_a_large_tie_group(probe):
    vals = np.array([-1, 0, 1, BIG, -BIG, 0, 1, -1, BIG - 1, -BIG + 1], np.int64)
    n = len(vals)
    m = Model(wam.node_ids(n, 4400))
    meas = FM if probe else FB
    if probe:
        m.set(FB, np.arange(n), np.arange(n))
    m.set(meas, np.arange(n), vals)
    with _engine(m, (FB, FM)) as e:
        for qs in (EIGHT, [(k, 9) for k in range(8)], [(9, 9), (5, 9)]):
            recs, res = _check(e, m, FB, EVERY, meas, qs)
        assert (int(res["min"]), int(res["max"])) == (-BIG, BIG)
    # 10^4 copies of one value in the middle of 15000, the ranks on and around the group's edges
    n = 15000
    rng = np.random.default_rng(44)
    v = rng.integers(-(2**22), 2**22, n); v[2000:12000] = 4097
    m = Model(wam.node_ids(n, 4500))
    if probe:
        m.set(FB, np.arange(n), rng.integers(0, 9, n))
    m.set(meas, np.arange(n), v)
    first = int((v < 4097).sum())
    with _engine(m, (FB, FM)) as e:
        recs, res = _check(e, m, FB, EVERY, meas, [(first - 1, n - 1), (first, n - 1), (1, 2), (first + 9999, n - 1), (first + 10000, n - 1)])
        assert [int(x) for x in recs["n_equal"][1:4]] == [10000] * 3 and [int(x) for x in recs["n_below"][1:4]] == [first] * 3 and [int(x) for x in recs["value"][1:4]] == [4097] * 3
        assert int(recs[0]["value"]) < 4097 < int(recs[4]["value"]) and int(recs[4]["n_below"]) == first + 10000


# ---- 4. refusals on a live engine ----
def test_refusals_leave_the_buffers_alone():
    m = _model(500, 46)
    with _engine(m, (FB, F1, FM)) as e:
        out = np.full(32 * 9, 0xA5, np.uint8); res = np.full(32, 0xA5, np.uint8)
        prog = bmx._where_args(FB, [[(F1, 0, 3)]])

        def call(prog, measure, nq, qs, o, r, mem=bmx.MEM_HOST):
            arr = None if qs is None else (bmx.QuantQ * max(len(qs), 1))(*[bmx.QuantQ(a, b) for a, b in qs])
            return e.L.bmx_where_quantiles(e.h, *prog, measure, nq, arr, bmx._ptr(o), bmx._ptr(r), mem)

        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert call(prog, FM, 0, [(1, 2)], out, res, mem) == bmx.ERR_INVALID
            assert call(prog, FM, 9, [(1, 2)] * 9, out, res, mem) == bmx.ERR_INVALID
            assert call(prog, FM, 1, None, out, res, mem) == bmx.ERR_INVALID
            assert call(prog, FM, 1, [(1, 2)], None, res, mem) == bmx.ERR_INVALID
            for q in ((0, 0), (2, 1), (1, bmx.QUANT_MAX_DEN + 1)):
                assert call(prog, FM, 2, [(1, 2), q], out, res, mem) == bmx.ERR_INVALID
            assert call(bmx._where_args(FB, []), FM, 1, [(1, 2)], out, res, mem) == bmx.ERR_INVALID            # no clause
            assert call(bmx._where_args(FB, [[(F1, 0, 1)] * 9]), FM, 1, [(1, 2)], out, res, mem) == bmx.ERR_INVALID
        assert call(prog, FM, 1, [(1, 2)], out, res, 7) == bmx.ERR_INVALID
        assert (out == 0xA5).all() and (res == 0xA5).all(), "a refused call writes nothing"
        _check(e, m, FB, [[(F1, 0, 3)]], FM, QUARTILES)                          # and the engine answers as before
        got = qm.raw(e, FB, [[(F1, 0, 3)]], FM, QUARTILES, with_res=False)       # res may be NULL
        assert got[0].tobytes() == qm.quantiles(m, FB, [[(F1, 0, 3)]], FM, QUARTILES)[0].tobytes()


# ---- 5. seeded random programs x random quantiles ----
@pytest.mark.parametrize("wide", [False, True])
def test_seeded_programs(wide):
    n = 9000
    m = _model(n, 50 + wide, wide)
    rng = np.random.default_rng(60 + wide)
    for k, f in enumerate(MORE):
        idx = np.nonzero(rng.random(n) < 0.5)[0]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
    off = WIDE if wide else 0
    progs = wam.random_programs(30, 70 + wide, FB, (F1, F2, F3, FM), MORE)       # 30 per width: 60 in all
    with _engine(m, [FB, F1, F2, F3, FM] + MORE) as e:
        wam.tombstone(e, m, FM, np.nonzero(m.st[FM] == DATA)[0][::9]); wam.tombstone(e, m, FB, np.arange(5, n, 31)); wam.tombstone(e, m, F1, np.nonzero(m.st[F1] == DATA)[0][::11])
        nonempty = deep = 0
        for k, p in enumerate(progs):
            p = [[(t[0], t[1] + off, t[2] + off, *t[3:]) if t[0] == FB and abs(t[1]) < 2**60 and abs(t[2]) < 2**60 else t for t in c] for c in p]
            nq = int(rng.integers(1, 9))
            qs = [(int(a), int(b)) for b in rng.choice([1, 2, 3, 4, 10, 100, 1000, 2**20], nq) for a in [rng.integers(0, b + 1)]]
            measure = (FB, FM, F2, MORE[0], FM)[k % 5]
            recs, res = _check(e, m, FB, p, measure, qs)
            nonempty += int(res["n"]) > 0; deep += int(res["n"]) > 0 and int(res["max"]) - int(res["min"]) >= 2**11
        assert nonempty >= 15 and deep >= 4, (nonempty, deep)


# ---- 6. device memory ----
def test_device_memory_back_to_back():
    """device mode into poisoned buffers; four queries enqueued back to back (deep: five digit passes, shallow: one, empty, deep again) with one synchronisation at
    the end: each leaves the state record ready for the next; qs is overwritten as soon as each call returns"""
    n = 8192 + 700
    rng = np.random.default_rng(81)
    m = Model(wam.node_ids(n, 8100))
    m.set(FB, np.arange(n), rng.integers(0, 2000, n))
    idx = np.nonzero(rng.random(n) < 0.7)[0]; m.set(FM, idx, rng.integers(-BIG, BIG, len(idx)))
    deep = [[(FB, 100, 1800)], [(FM, 0, WIDE, True), (FB, 0, 50)]]
    queries = [(deep, FM, EIGHT), (deep, FB, QUARTILES), ([[(FB, 5000, 6000)]], FM, EIGHT), (deep, FM, [(1, 2)]), (EVERY, FM, [(2, 3), (1, 3)])]
    dev = torch.device("cuda", 0)
    with _engine(m, (FB, FM)) as e:
        host = [qm.raw(e, FB, p, me, qs) for p, me, qs in queries]
        outs = [torch.full((4 * (len(qs) + 1),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev) for _, _, qs in queries]
        ress = [torch.full((4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev) for _ in queries]
        for (p, me, qs), o, r in zip(queries, outs, ress):
            arr = (bmx.QuantQ * len(qs))(*[bmx.QuantQ(a, b) for a, b in qs])
            e._chk(e.L.bmx_where_quantiles(e.h, *bmx._where_args(FB, p), me, len(qs), arr, bmx._ptr(o), bmx._ptr(r), bmx.MEM_DEVICE))
            C.memset(arr, 0xFF, C.sizeof(arr))                                   # qs was read at call time
        e.where_quantiles_dev(FB, deep, FM, QUARTILES, outs[0][:12].clone(), None)      # res may be NULL in device mode too
        e.sync()
        for (p, me, qs), o, r, h in zip(queries, outs, ress, host):
            want = qm.quantiles(m, FB, p, me, qs)
            recs = o.cpu().numpy().view(bmx.QUANT_REC_DTYPE); res = r.cpu().numpy().view(bmx.QUANT_RES_DTYPE)[0]
            assert qm.same((recs[:len(qs)], res), want) is None and qm.same(h, want) is None, (p, me, qs)
            assert (recs[len(qs):].view(np.uint8) == 0x5A).all(), "nothing is written behind the last record"
        assert int(host[0][1]["max"]) - int(host[0][1]["min"]) >= 2**44 and int(host[2][1]["n_match"]) == 0
        recs, res = e.where_quantiles(FB, deep, FM, QUARTILES)                    # the Python surface
        assert recs.tobytes() == qm.quantiles(m, FB, deep, FM, QUARTILES)[0].tobytes() and res.n == int(host[0][1]["n"])


# ---- 7. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(91)
    N0, EXTRA = 8192 + 5, 300
    m = Model(wam.node_ids(N0 + EXTRA, 9100))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 3000, N0))
    for f, pr in ((F1, 0.9), (FM, 0.8)):
        idx = old[rng.random(N0) < pr]
        m.set(f, idx, rng.integers(0, 6, len(idx)) if f == F1 else rng.integers(-(2**25), 2**25, len(idx)))
    progs = [[[(F1, 1, 3), (FB, 200, 2900)]], [[(F1, 0, 1)], [(FM, 0, 2**24), (FB, 0, 500)]], [[(FB, 300, 400, True), (F1, 0, 5, True)], [(FB, 0, 100)]]]

    def ask(e):
        return [_check(e, m, FB, p, me, EIGHT) for p in progs for me in (FB, FM, F1)]

    def same(a, b):
        return all(qm.same(x, y) is None for x, y in zip(a, b))

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), vals, want_flags=False)
        m.set(f, idx, vals)

    with _engine(m, (FB, F1, FM), 8 * (N0 + EXTRA)) as e:
        first = ask(e)
        assert all(int(a[1]["n"]) > 100 for a in first)
        # a merge that changes measures and base rows and creates rows: the index grows, and with it the value scratch
        idx = old[::3]; merge(e, FM, idx, rng.integers(-(2**25), 2**25, len(idx)), 100)
        idx = old[1::5]; merge(e, FB, idx, rng.integers(0, 3000, len(idx)), 100)
        new = np.arange(N0, N0 + EXTRA)
        merge(e, FB, new, rng.integers(0, 3000, EXTRA), 101); merge(e, FM, new[::2], rng.integers(-(2**25), 2**25, len(new[::2])), 101); merge(e, F1, new, rng.integers(0, 6, EXTRA), 101)
        second = ask(e)
        assert e.index_size(FB) == N0 + EXTRA and not same(first, second)
        # growth
        e.reserve(32 * (N0 + EXTRA))
        assert same(ask(e), second)
        wam.tombstone(e, m, FM, np.nonzero(m.st[FM] == DATA)[0][::7], ts=200); wam.tombstone(e, m, FB, np.concatenate([old[5::40], new[1::7]]), ts=200)
        third = ask(e)
        assert not same(third, second)
        # a value-ordered view on the base field in three states — answering, patched behind a write, stale — the same answers and the view's counters untouched
        e.index_set_ordered(FB, 1)
        assert set(e.scan_range(FB, 200, 900).tolist()) == set(m.ids[m.mask(FB, [[(FB, 200, 900)]])].tolist())
        assert e.index_ordered_info(FB)[1], "the view answers"
        s0 = e.index_ordered_stats(FB)
        assert same(ask(e), third)
        assert e.index_ordered_stats(FB) == s0 and e.index_ordered_info(FB)[1], "the calls leave the view as it was"
        merge(e, FB, old[2::50], rng.integers(0, 3000, len(old[2::50])), 300)     # the next scan patches the view
        assert len(e.scan_range(FB, 200, 900)) == int(m.mask(FB, [[(FB, 200, 900)]]).sum())
        s1 = e.index_ordered_stats(FB)
        fourth = ask(e)
        assert e.index_ordered_stats(FB) == s1 and not same(fourth, third)
        e.index_set_ordered(FB, 1000)                                             # sorted again only by the 1000th query: a write leaves it stale
        merge(e, FB, old[3::60], rng.integers(0, 3000, len(old[3::60])), 400)
        e.where_top(FB, EVERY, 1)                                                 # (the columns are brought up to date by a call that leaves the view alone too)
        i0, s2 = e.index_ordered_info(FB), e.index_ordered_stats(FB)
        ask(e)
        assert e.index_ordered_info(FB) == i0 and e.index_ordered_stats(FB) == s2
        e.index_set_ordered(FB, 0)
        # a base value beyond int32: the index switches to its int64 column
        merge(e, FB, [7, N0 + 3], np.array([WIDE, -(2**35)]), 2000)
        last = ask(e)
        recs, res = _check(e, m, FB, [[(FB, 2**39, I64MAX)], [(FB, I64MIN, -(2**33))]], FB, [(0, 1), (1, 1)])
        assert recs["value"].tolist() == [-(2**35), WIDE] and int(res["n"]) == 2
        assert int(last[0][1]["n"]) > 100
