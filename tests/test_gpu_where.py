"""GPU: boolean filters (include/bmx_where.h bmx_scan_where). Every answer is compared exactly with a numpy model over the rows the test itself loaded: each field
has a state per node (absent, data, tombstone); a positive literal is "data and lo <= value <= hi", a negated one its complement, a clause the AND of its
literals, the program the OR of its clauses, and the universe the nodes with data in the base field. The expected order is index_ids(base) filtered by that mask.

The shapes are the smallest at which each piece can go wrong (csrc/select.h, csrc/where_kernels.h): one mask block is 8192 rows, one mask word is 32 rows shared
by 32 / E lanes (E = 4 int32 or 2 int64 values per lane and load), a wave is 64 lanes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
from oracle import streams

FB, F1, F2, F3, F4, F5 = (streams.fnv1a32(s) for s in ("base", "one", "two", "three", "four", "five"))
MORE = [streams.fnv1a32("extra%d" % k) for k in range(4)]
PROBED = [F1, F2, F3, F4, F5]
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
BLOCK = 8192
ABSENT, DATA, TOMB = 0, 1, 2


class Model:
    """the table as the test loaded it: val[f][i], st[f][i] (ABSENT / DATA / TOMB) of node i"""

    def __init__(self, ids):
        self.ids = np.asarray(ids, np.uint64); self.N = len(self.ids); self.val = {}; self.st = {}
        self.order = np.argsort(self.ids); self.sorted_ids = self.ids[self.order]

    def _f(self, f):
        if f not in self.val:
            self.val[f] = np.zeros(self.N, np.int64); self.st[f] = np.zeros(self.N, np.uint8)

    def set(self, f, idx, vals):
        self._f(f); self.val[f][idx] = vals; self.st[f][idx] = DATA

    def tomb(self, f, idx):
        self._f(f); self.st[f][idx] = TOMB

    def rows(self, f, ts):
        i = np.nonzero(self.st[f] == DATA)[0]
        return self.ids[i], np.full(len(i), f, np.uint32), np.full(len(i), ts, np.int64), self.val[f][i]

    def lit(self, t):
        f, lo, hi = t[0], int(t[1]), int(t[2])
        self._f(f)
        pos = (self.st[f] == DATA) & (self.val[f] >= lo) & (self.val[f] <= hi) if lo <= hi else np.zeros(self.N, bool)
        return ~pos if len(t) > 3 and t[3] else pos

    def mask(self, base, clauses):
        self._f(base)
        any_clause = np.zeros(self.N, bool)
        for c in clauses:
            all_lits = np.ones(self.N, bool)
            for t in c:
                all_lits &= self.lit(t)
            any_clause |= all_lits
        return any_clause & (self.st[base] == DATA)

    def index_of(self, ids):
        """node numbers of ids (all of them nodes of the model)"""
        k = np.searchsorted(self.sorted_ids, ids)
        assert (self.sorted_ids[k] == ids).all()
        return self.order[k]

    def want(self, e, base, clauses):
        """index_ids(base) filtered by the model's mask"""
        pos_ids = e.index_ids(base)
        return pos_ids[self.mask(base, clauses)[self.index_of(pos_ids)]]


def _ids(n, salt=0):
    return streams.splitmix64_np(np.arange(1 + salt, n + 1 + salt, dtype=np.uint64))


def _engine_with(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    for f in fields:
        if (m.st[f] == DATA).any():
            e.load_rows(*m.rows(f, 5))
    return e


def _tombstone(e, m, f, idx, ts=9):
    idx = np.asarray(idx)
    e.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.full(len(idx), bmx.VAL_DELETED, np.int64))
    m.tomb(f, idx)


def _check(e, m, base, clauses):
    want = m.want(e, base, clauses)
    got = e.scan_where(base, clauses)
    assert len(got) == len(want), (clauses, len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (clauses, bad[:4], got[bad[:4]], want[bad[:4]])
    assert e.scan_where(base, clauses, count_only=True) == len(want), clauses
    return got


# ---- 1. truth table ----
def test_truth_table():
    """12 nodes. F1 in every state: absent, tombstone, below / at the lower end of / inside / at the upper end of / above the range 10..20; the base field
    itself absent (node 10) and tombstoned (node 11): neither is ever returned."""
    m = Model(_ids(12))
    m.set(FB, np.arange(10), np.arange(10) * 10)               # 0, 10, .., 90
    m.set(FB, [11], [55])
    #            node: 0 absent, 1 tombstone, 2 below, 3 lo, 4 inside, 5 hi, 6 above, 7 far below, 8 far above, 9 absent, 10 inside (no base), 11 inside (base tombstoned)
    m.set(F1, [1, 2, 3, 4, 5, 6, 7, 8, 10, 11], [15, 9, 10, 15, 20, 21, -(2**53 - 1), 2**53 - 1, 15, 15])
    m.set(F2, [0, 1, 2, 3, 10, 11], [1, 1, 2, 2, 1, 1])
    with _engine_with(m, (FB, F1, F2)) as e:
        _tombstone(e, m, F1, [1]); _tombstone(e, m, FB, [11]); _tombstone(e, m, F2, [3])
        ids = m.ids

        def ask(clauses):
            return set(_check(e, m, FB, clauses).tolist())

        assert ask([[(F1, 10, 20)]]) == set(ids[[3, 4, 5]].tolist())
        assert ask([[(F1, 10, 20, True)]]) == set(ids[[0, 1, 2, 6, 7, 8, 9]].tolist()), "the complement inside the universe: absent and tombstoned included"
        # lo > hi: never true / always true
        assert ask([[(F1, 20, 10)]]) == set()
        assert ask([[(F1, 20, 10, True)]]) == set(ids[:10].tolist())
        assert ask([[(FB, 50, 40)]]) == set() and ask([[(FB, 50, 40, True)]]) == set(ids[:10].tolist())
        # the whole int64 range, negated: true on a tombstone and on an absent field, false on data
        assert ask([[(F1, I64MIN, I64MAX, True)]]) == set(ids[[0, 1, 9]].tolist())
        assert ask([[(F1, I64MIN, I64MAX)]]) == set(ids[[2, 3, 4, 5, 6, 7, 8]].tolist()), "presence"
        assert ask([[(F1, I64MIN, 0, True)]]) == set(ids[[0, 1, 2, 3, 4, 5, 6, 8, 9]].tolist()), "a tombstone is no small value"
        assert ask([[(F1, I64MIN, I64MIN)]]) == set() and ask([[(F1, I64MAX, I64MAX)]]) == set()
        assert ask([[(F1, -(2**53 - 1), -(2**53 - 1))]]) == {int(ids[7])} and ask([[(F1, 2**53 - 1, I64MAX)]]) == {int(ids[8])}
        # literals on the base field, both signs, and the base column's own tombstone
        assert ask([[(FB, 20, 40)]]) == set(ids[[2, 3, 4]].tolist())
        assert ask([[(FB, 20, 40, True)]]) == set(ids[[0, 1, 5, 6, 7, 8, 9]].tolist())
        assert ask([[(FB, I64MIN, I64MAX)]]) == set(ids[:10].tolist())
        assert ask([[(FB, I64MIN, I64MAX, True)]]) == set()
        # AND, OR, the same field twice, a contradiction, a tautology
        assert ask([[(F1, 10, 20), (FB, 40, 90)]]) == set(ids[[4, 5]].tolist())
        assert ask([[(F1, 10, 20)], [(F2, 1, 1)]]) == set(ids[[0, 1, 3, 4, 5]].tolist())
        assert ask([[(F1, 10, 20), (F1, 15, 30)]]) == set(ids[[4, 5]].tolist())
        assert ask([[(F1, 10, 20), (F1, 10, 20, True)]]) == set()
        assert ask([[(F1, 10, 20)], [(F1, 10, 20, True)]]) == set(ids[:10].tolist())
        assert ask([[(F2, 2, 2, True), (F1, 0, 100, True)], [(F2, 2, 2)]]) == set(ids[[0, 1, 2, 7, 8, 9]].tolist())
        # a field nobody has
        assert ask([[(MORE[0], I64MIN, I64MAX)]]) == set() and ask([[(MORE[0], 0, 0, True)]]) == set(ids[:10].tolist())


# ---- 2. the AND filter ----
@pytest.mark.parametrize("nterms", [1, 2, 8])
def test_one_positive_clause_is_scan_filter(nterms):
    n = 2 * BLOCK + 77
    rng = np.random.default_rng(nterms)
    m = Model(_ids(n, 50))
    fields = [FB, F1, F2, F3, F4, F5, MORE[0], MORE[1]]
    m.set(FB, np.arange(n), rng.integers(0, 100, n))
    for f in fields[1:]:
        idx = np.nonzero(rng.random(n) < 0.9)[0]
        m.set(f, idx, rng.integers(0, 10, len(idx)))
    with _engine_with(m, fields) as e:
        _tombstone(e, m, F1, np.arange(3, n, 17)[m.st[F1][np.arange(3, n, 17)] == DATA])
        for lo0, hi0 in ((0, 99), (10, 60), (42, 42)):
            terms = [(FB, lo0, hi0)] + [(f, 1, 8) for f in fields[1:nterms]]
            flt = e.scan_filter(terms)
            got = e.scan_where(FB, [terms])
            assert np.array_equal(got, flt), (nterms, lo0, hi0, len(got), len(flt))
            assert np.array_equal(got, m.want(e, FB, [terms]))
            assert len(got) > 0


# ---- 3. edges of the column ----
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_edges_of_the_column(n, wide):
    """only the first row, only the last, all rows, none — as a base literal, as a probed one, and in a two-clause program with a negated probed literal; on the
    int32 column and (wide: one value beyond int32 in the base field) on the int64 column"""
    m = Model(_ids(n, 1000 + n))
    v = np.arange(n, dtype=np.int64) + 1
    if wide:
        v = v + 2**40
    m.set(FB, np.arange(n), v)
    m.set(F1, np.arange(n), np.arange(n) % 7)
    vmin, vmax = int(v[0]), int(v[-1])
    with _engine_with(m, (FB, F1)) as e:
        pos_ids = e.index_ids(FB)                                  # the column's order is the table's, not the load's
        node = m.index_of(pos_ids)
        first, last = int(v[node[0]]), int(v[node[-1]])
        lastval = 2 if n > 1 else 1                                # F2: 1 on the first row of the column, 2 on the last (n == 1: the one row is both)
        m.set(F2, [node[-1]], [lastval]); m.set(F2, [node[0]], [1])
        e.load_rows(*m.rows(F2, 5))
        assert np.array_equal(e.index_ids(FB), pos_ids)
        progs = {
            "first": [[[(FB, first, first)]], [[(F2, 1, 1)]], [[(F2, 1, 1), (F1, 7, 9, True)]], [[(F1, 9, 9)], [(F2, 1, 1), (FB, vmin, vmax)]]],
            "last": [[[(FB, last, last)]], [[(F2, lastval, lastval)]], [[(F2, lastval, lastval)], [(F1, 9, 9)]], [[(FB, last, last, True), (F1, 0, 6, True)], [(FB, last, last)]]],
            "all": [[[(FB, vmin, vmax)]], [[(F1, 0, 6)]], [[(F2, 1, 1)], [(F2, 1, 1, True)]], [[(F1, 0, 3)], [(F1, 0, 3, True), (FB, vmin, vmax)]]],
            "none": [[[(FB, vmax + 1, I64MAX)]], [[(F1, 7, 100)]], [[(F2, 5, 5)], [(F1, 0, 6, True), (FB, vmin, vmax)]]],
        }
        for kind, ps in progs.items():
            for p in ps:
                got = _check(e, m, FB, p)
                want = {"first": pos_ids[:1], "last": pos_ids[-1:], "all": pos_ids, "none": pos_ids[:0]}[kind]
                assert np.array_equal(got, want), (n, kind, p)
        # two-clause programs, one literal negated and probed: the rows with F1 == 0 are out of clause 0; the last row comes in through clause 1
        _check(e, m, FB, [[(F1, 0, 0, True), (FB, vmin, vmax)], [(F2, 2, 2)]])
        _check(e, m, FB, [[(F2, 1, 2, True), (F1, 3, 5)], [(FB, last, last)]])


# ---- 4. random programs ----
N_RAND = 3 * BLOCK + 17
SEED = 20240611
PRESENCE = dict(zip(PROBED, (0.9, 0.7, 0.5, 0.1, 0.0)))


def _random_model(salt=0):
    rng = np.random.default_rng(4242)
    m = Model(_ids(N_RAND, 7000 + salt))
    m.set(FB, np.arange(N_RAND), rng.integers(0, 12, N_RAND))
    tombs = {}
    for f in PROBED:
        idx = np.nonzero(rng.random(N_RAND) < PRESENCE[f])[0]
        m._f(f)
        if len(idx):
            m.set(f, idx, rng.integers(0, 6, len(idx)))
            tombs[f] = idx[rng.random(len(idx)) < 0.05]
    for f in MORE:                                     # present on a third each: only the programs at the field limit name them
        idx = np.nonzero(rng.random(N_RAND) < 0.33)[0]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
    return m, tombs


def _load_random(x, m, tombs):
    """x: an Engine or a Comm"""
    for f in [FB] + PROBED + MORE:
        if (m.st[f] == DATA).any():
            x.load_rows(*m.rows(f, 5))
    for f, idx in tombs.items():
        x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), bmx.VAL_DELETED, np.int64))


def _apply_tombs(m, tombs):
    for f, idx in tombs.items():
        m.tomb(f, idx)


def _random_lit(rng, fields):
    f = fields[int(rng.integers(0, len(fields)))]
    top = 12 if f == FB else 6
    kind = int(rng.integers(0, 10))
    if kind == 0:
        lo, hi = I64MIN, I64MAX                        # presence / absence
    elif kind == 1:
        lo = int(rng.integers(0, top)); hi = lo - 1 - int(rng.integers(0, 3))      # an empty range
    elif kind <= 4:
        lo = hi = int(rng.integers(-1, top + 1))       # an equality
    else:
        lo = int(rng.integers(-2, top)); hi = lo + int(rng.integers(0, top))
    return (f, lo, hi, bool(rng.random() < 0.35))


def _random_programs(count=200, seed=SEED):
    rng = np.random.default_rng(seed)
    fields = [FB] + PROBED
    progs = []
    while len(progs) < count - 1:
        nc = int(rng.integers(1, 9))
        lens = [int(rng.integers(1, 9)) for _ in range(nc)]
        if rng.random() < 0.5:
            lens = [min(x, 3) for x in lens]           # half of them short clauses: long ANDs are mostly empty
        while sum(lens) > 32:
            lens[int(np.argmax(lens))] -= 1
        pool = [fields[i] for i in rng.choice(len(fields), int(rng.integers(1, len(fields) + 1)), replace=False)]   # few fields: repeated inside and across clauses
        progs.append([[_random_lit(rng, pool) for _ in range(L)] for L in lens])
    # every limit at once: 8 clauses, 32 literals, 8 probed fields (and the base field)
    eight = PROBED[:4] + MORE
    progs.append([[(eight[(c + k) % 8], 0, 3 + (k % 3), (c + k) % 5 == 0) if k < 3 else (FB, c, 11) for k in range(4)] for c in range(8)])
    return progs


def test_the_random_programs_cover_the_space():
    """(model only) both empty and non-empty answers, at least a quarter neither empty nor everything, the limits reached"""
    m, tombs = _random_model()
    _apply_tombs(m, tombs)
    progs = _random_programs()
    assert len(progs) == 200
    counts = np.array([int(m.mask(FB, p).sum()) for p in progs])
    assert (counts == 0).any() and (counts > 0).any()
    assert ((counts > 0) & (counts < N_RAND)).sum() >= 50, ((counts > 0) & (counts < N_RAND)).sum()
    assert max(len(p) for p in progs) == 8 and max(sum(len(c) for c in p) for p in progs) == 32 and max(len(c) for p in progs for c in p) == 8
    last = progs[-1]
    assert len(last) == 8 and sum(len(c) for c in last) == 32 and len({t[0] for c in last for t in c} - {FB}) == 8
    assert 0 < counts[-1] < N_RAND
    assert any(t[0] == FB for p in progs for c in p for t in c) and any(len({t[0] for t in c}) < len(c) for p in progs for c in p)
    assert all(len({t[0] for c in p for t in c} - {FB}) <= 8 for p in progs)


def test_random_programs():
    m, tombs = _random_model()
    with bmx.Engine(16 * N_RAND) as e:
        _load_random(e, m, tombs); _apply_tombs(m, tombs)
        pos_ids = e.index_ids(FB)
        node = m.index_of(pos_ids)
        for k, p in enumerate(_random_programs()):
            want = pos_ids[m.mask(FB, p)[node]]
            got = e.scan_where(FB, p)
            assert np.array_equal(got, want), (k, p, len(got), len(want))


# ---- 5. output forms ----
def test_output_forms():
    m, tombs = _random_model(1)
    dev = torch.device("cuda", 0)
    FILL = 0x5A5A5A5A5A5A5A5A
    progs = _random_programs(40, SEED + 1)
    with bmx.Engine(16 * N_RAND) as e:
        _load_random(e, m, tombs); _apply_tombs(m, tombs)
        seen_some = 0
        for p in progs[:12] + progs[-1:]:
            want = m.want(e, FB, p)
            M = len(want)
            assert e.scan_where(FB, p, count_only=True) == M, "out == NULL counts only"
            assert len(e.scan_where(FB, p, cap=0)) == 0
            for cap in sorted({1, M // 2, M - 1, M, M + 5} - {0} - set(range(-9, 0))):
                # host memory: a sentinel behind out[cap]
                args = bmx._where_args(FB, p)
                out = np.full(cap + 4, FILL, np.uint64)
                cnt = np.array([FILL], np.uint64)
                e._chk(e.L.bmx_scan_where(e.h, *args, bmx._ptr(out), cap, bmx._ptr(cnt), bmx.MEM_HOST))
                assert int(cnt[0]) == M, "n_out is the total, whatever cap"
                assert np.array_equal(out[:min(cap, M)], want[:cap]) and (out[min(cap, M):] == FILL).all(), (cap, M)
                # device memory, read after sync()
                d_out = torch.full((cap + 4,), FILL, dtype=torch.int64, device=dev)
                d_cnt = torch.full((2,), FILL, dtype=torch.int64, device=dev)
                e.scan_where_dev(FB, p, d_out, cap, d_cnt[0:1])
                e.sync()
                h = d_out.cpu().numpy().view(np.uint64); c = d_cnt.cpu().numpy()
                assert int(c[0]) == M and int(c[1]) == FILL
                assert np.array_equal(h[:min(cap, M)], want[:cap]) and (h[min(cap, M):] == FILL).all(), (cap, M)
            # cap = 0 with a buffer, and the device count-only form
            out = np.full(4, FILL, np.uint64); cnt = np.array([FILL], np.uint64)
            e._chk(e.L.bmx_scan_where(e.h, *bmx._where_args(FB, p), bmx._ptr(out), 0, bmx._ptr(cnt), bmx.MEM_HOST))
            assert int(cnt[0]) == M and (out == FILL).all()
            d_cnt = torch.full((2,), FILL, dtype=torch.int64, device=dev)
            e.scan_where_dev(FB, p, None, 0, d_cnt[0:1])
            e.sync()
            assert d_cnt.cpu().numpy().tolist() == [M, FILL]
            seen_some += M > 4
        assert seen_some >= 3


def test_refused_programs_on_a_live_engine_and_communicator():
    """the limits with a context behind them: ERR_INVALID, the output and the counter untouched, and the engine answers the next query"""
    m = Model(_ids(100, 31))
    m.set(FB, np.arange(100), np.arange(100)); m.set(F1, np.arange(100), np.arange(100) % 5)
    FILL = 0x5A5A5A5A5A5A5A5A
    nine = [[(1000 + k, 0, 1) for k in range(8)], [(1008, 0, 1)]]                  # nine fields besides the base
    bad = [nine, [[(FB, 0, 1)] * 8] * 4 + [[(FB, 0, 1)]], [[(F1, 0, 1)] * 9], [], [[(F1, 0, 1)], []], [[(FB, 0, 1)]] * 9]
    with _engine_with(m, (FB, F1)) as e, bmx.Comm([0, 0], 4096) as c:
        c.load_rows(*m.rows(FB, 5)); c.load_rows(*m.rows(F1, 5))
        good = [[(FB, 10, 50), (F1, 1, 3)]]
        want = _check(e, m, FB, good)

        def calls(args, out, cnt):
            yield e.L.bmx_scan_where(e.h, *args, bmx._ptr(out), 64, bmx._ptr(cnt), bmx.MEM_HOST)
            yield e.L.bmx_scan_where(e.h, *args, None, 0, bmx._ptr(cnt), bmx.MEM_HOST)
            yield e.L.bmx_scan_where(e.h, *args, bmx._ptr(out), 64, bmx._ptr(cnt), 7) if args[1] else bmx.ERR_INVALID
            yield c.L.bmx_comm_scan_where(c.h, *args, bmx._ptr(out), 64, bmx._ptr(cnt))

        for p in bad:
            out = np.full(64, FILL, np.uint64); cnt = np.array([FILL], np.uint64)
            for rc in calls(bmx._where_args(FB, p), out, cnt):
                assert rc == bmx.ERR_INVALID, p
            assert (out == FILL).all() and int(cnt[0]) == FILL, p
        # unknown flag bits, and a bad mem kind with a good program
        base, nc, lens, lits = bmx._where_args(FB, good)
        lits[1].flags = 2
        out = np.full(64, FILL, np.uint64); cnt = np.array([FILL], np.uint64)
        for rc in calls((base, nc, lens, lits), out, cnt):
            assert rc == bmx.ERR_INVALID
        assert e.L.bmx_scan_where(e.h, *bmx._where_args(FB, good), bmx._ptr(out), 64, bmx._ptr(cnt), 7) == bmx.ERR_INVALID
        assert (out == FILL).all() and int(cnt[0]) == FILL
        with pytest.raises(bmx.BmxError):
            e.scan_where(FB, nine)
        with pytest.raises(bmx.BmxError):
            c.scan_where(FB, nine)
        assert np.array_equal(e.scan_where(FB, good), want) and np.array_equal(np.sort(c.scan_where(FB, good)), np.sort(want))


# ---- 6. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(66)
    N0, EXTRA = 2 * BLOCK + 5, 300
    m = Model(_ids(N0 + EXTRA, 9000))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 12, N0))
    for f, pr in ((F1, 0.9), (F2, 0.5)):
        idx = old[rng.random(N0) < pr]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
    m._f(F3)
    progs = [
        [[(F1, 1, 3), (FB, 2, 9), (F2, 2, 2, True)]],                                       # two positive literals and a negated probed one
        [[(F1, 0, 1)], [(F2, 4, 5), (FB, 0, 5)]],                                          # an OR
        [[(F2, I64MIN, I64MAX, True), (F1, 2, 4)], [(FB, 11, I64MAX)], [(F3, 1, 1)]],
        [[(FB, 3, 3, True), (F1, 0, 5, True)], [(FB, 0, 1), (F2, 0, 2)]],
    ]
    dev = torch.device("cuda", 0)

    def ask(e):
        return [_check(e, m, FB, p) for p in progs]

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), vals, want_flags=False)
        m.set(f, idx, vals)

    with _engine_with(m, (FB, F1, F2), 8 * (N0 + EXTRA)) as e:
        first = ask(e)
        assert all(0 < len(a) < N0 for a in first[:2])
        # a merge that changes values of probed fields and of the base field
        for f, top in ((F1, 6), (F2, 6), (FB, 12)):
            idx = np.nonzero(m.st[f] == DATA)[0][::3]
            merge(e, f, idx, rng.integers(0, top, len(idx)), 100)
        ask(e)
        # a merge that creates new nodes: rows appended to the index from the change log, and probed rows of old and new nodes
        new = np.arange(N0, N0 + EXTRA)
        builds = e.index_refresh_counts()[0]
        merge(e, FB, new, rng.integers(0, 12, EXTRA), 101)
        merge(e, F1, new[::2], rng.integers(0, 6, len(new[::2])), 101)
        merge(e, F3, np.concatenate([old[::50], new[::3]]), np.ones(len(old[::50]) + len(new[::3]), np.int64), 101)
        got = ask(e)
        assert e.index_refresh_counts()[0] == builds, "the new rows came in through the change log, not through a rebuild"
        assert e.index_size(FB) == N0 + EXTRA and np.isin(m.ids[new], got[2]).any()
        # tombstones on the base field and on a probed field
        _tombstone(e, m, FB, np.concatenate([old[5::40], new[1::7]]), ts=200)
        _tombstone(e, m, F1, np.nonzero(m.st[F1] == DATA)[0][::9], ts=200)
        ask(e)
        # a larger table
        e.reserve(32 * (N0 + EXTRA))
        ask(e)
        # a value-ordered view on the base field: the same arrays, and the view's bookkeeping untouched
        before = ask(e)
        e.index_set_ordered(FB, 1)
        assert set(e.scan_range(FB, 2, 9).tolist()) == set(m.ids[m.mask(FB, [[(FB, 2, 9)]])].tolist())
        assert e.index_ordered_info(FB)[1], "the view answers"
        s0 = e.index_ordered_stats(FB)
        after = ask(e)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert e.index_ordered_stats(FB) == s0 and e.index_ordered_info(FB)[1], "the where calls leave the view as it was"
        e.index_set_ordered(FB, 0)
        # deferred compaction (switched on explicitly): a device batch large enough to defer, asked right behind it
        e.set_deferred(True)
        nb = 65_536
        keys = rng.permutation(4 * N0)[:nb]                       # distinct (node, field) keys over the old nodes
        kn, kf = keys % N0, np.array([FB, F1, F2, F3], np.uint32)[keys // N0]
        kv = np.where(kf == FB, rng.integers(0, 12, nb), rng.integers(0, 6, nb)).astype(np.int64)
        cols = (torch.from_numpy(m.ids[kn].view(np.int64)).to(dev), torch.from_numpy(kf.view(np.int32)).to(dev),
                torch.full((nb,), 300, dtype=torch.int64, device=dev), torch.from_numpy(kv).to(dev))
        applied = torch.zeros(nb, dtype=torch.int32, device=dev); n_applied = torch.zeros(1, dtype=torch.int64, device=dev)
        d0 = e.deferred_counts()[0]
        e.merge_batch_dev(nb, *cols, bmx.INSERT_REFERENCE, applied=applied, n_applied=n_applied)
        for f in (FB, F1, F2, F3):
            m.set(f, kn[kf == f], kv[kf == f])
        ask(e)
        assert e.deferred_counts()[0] == d0 + 1 and int(n_applied.item()) == nb
        # a base value beyond int32: the index switches to its int64 column
        merge(e, FB, [7, N0 + 3], np.array([2**40, -(2**35)]), 400)
        wide = ask(e)
        _check(e, m, FB, [[(FB, 2**39, I64MAX)], [(FB, I64MIN, -(2**33)), (F1, I64MIN, I64MAX, True)]])
        assert int(m.ids[7]) in wide[2].tolist(), "clause [(FB, 11, INT64_MAX)] sees the wide value"


# ---- 7. shards ----
@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m, tombs = _random_model(2)
    progs = _random_programs(60, SEED + 2)
    with bmx.Engine(16 * N_RAND) as e, bmx.Comm([0] * nshards, 16 * N_RAND) as c:
        _load_random(e, m, tombs); _load_random(c, m, tombs); _apply_tombs(m, tombs)
        some = 0
        for p in progs[:9] + progs[-1:]:
            one = e.scan_where(FB, p); many = c.scan_where(FB, p)
            want = m.ids[m.mask(FB, p)]
            assert np.array_equal(np.sort(one), np.sort(many)) and np.array_equal(np.sort(many), np.sort(want)), (nshards, p)
            assert c.scan_where(FB, p, count_only=True) == len(want) == e.scan_where(FB, p, count_only=True)
            some += 0 < len(want) < N_RAND
        assert some >= 3
