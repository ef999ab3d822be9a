"""GPU: aggregate queries (include/bmx.h bmx_scan_aggregate) — count, sum, min, max and group-by over the nodes a declarative filter selects, answered on the
device without delivering an id. Every comparison is exact integer equality against numpy / Python-int arithmetic over the rows the test itself loaded
(a small model of the table: per field a value and a state per node), and against the reference's own query results (tests/golden/g5_query_seeded_*.json).
Every case runs with the value-ordered view off, on, and carrying a pending patch: the three must agree with the model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
from oracle import streams
from helpers import load_golden

FA, FS, FO, FG = streams.fnv1a32("age"), streams.fnv1a32("score"), streams.fnv1a32("other"), streams.fnv1a32("grp")
VMAX = 2**53 - 1
LDS_GROUPS = 1024          # bmx.h: up to 1024 groups are accumulated in LDS, more take the slow form
ABSENT, DATA, TOMB = 0, 1, 2


class Model:
    """the table as the test loaded it: val[f][i], st[f][i] (ABSENT / DATA / TOMB) of node i"""

    def __init__(self, ids):
        self.ids = np.asarray(ids, np.uint64); self.N = len(self.ids); self.val = {}; self.st = {}

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

    def agg(self, terms, measure=None, group=None, group_lo=0, ngroups=0):
        """-> (n_match, n, min, max, sum) or the list of ngroups + 1 of them"""
        sel = np.ones(self.N, bool)
        for f, lo, hi in terms:
            self._f(f)
            sel &= (self.st[f] == DATA) & (self.val[f] >= lo) & (self.val[f] <= hi)
        gi = np.zeros(self.N, np.int64)
        if ngroups:
            self._f(group)
            d = self.val[group].astype(object) - int(group_lo) if abs(int(group_lo)) > 2**62 else self.val[group] - np.int64(group_lo)
            inw = (self.st[group] == DATA) & np.asarray(d >= 0, bool) & np.asarray(d < ngroups, bool)
            gi = np.where(inw, d, ngroups).astype(np.int64)
        nrec = ngroups + 1
        nm = np.bincount(gi[sel], minlength=nrec)
        n = np.zeros(nrec, np.int64); mn = [None] * nrec; mx = [None] * nrec; sm = [0] * nrec
        if measure is not None:
            self._f(measure)
            hm = sel & (self.st[measure] == DATA)
            g = gi[hm]; v = self.val[measure][hm]
            n = np.bincount(g, minlength=nrec)
            if len(v):
                big = int(np.abs(v).max()) * len(v) >= 2**62
                s = np.zeros(nrec, object if big else np.int64)
                np.add.at(s, g, v.astype(object) if big else v)
                lo_ = np.full(nrec, np.iinfo(np.int64).max); hi_ = np.full(nrec, np.iinfo(np.int64).min)
                np.minimum.at(lo_, g, v); np.maximum.at(hi_, g, v)
                sm = [int(x) for x in s]
                mn = [int(lo_[k]) if n[k] else None for k in range(nrec)]; mx = [int(hi_[k]) if n[k] else None for k in range(nrec)]
        else:
            n = nm
        recs = [(int(nm[k]), int(n[k]), mn[k], mx[k], sm[k]) for k in range(nrec)]
        return recs if ngroups else recs[0]


def _t(r):
    return [(x.n_match, x.n, x.min, x.max, x.sum) for x in r] if isinstance(r, list) else (r.n_match, r.n, r.min, r.max, r.sum)


def _check(e, m, terms, **kw):
    got = _t(e.scan_aggregate(terms, **kw)); want = m.agg(terms, **kw)
    assert got == want, (terms, kw, [(k, a, b) for k, (a, b) in enumerate(zip(got, want)) if a != b][:4] if isinstance(got, list) else (got, want))
    if isinstance(got, list):
        assert sum(r[0] for r in got) == _t(e.scan_aggregate(terms))[0], "the groups' n_match add up to the ungrouped n_match"
    return got


def _three_states(e, m, f0, cases, rng, ts0=1000, lo=0, hi=99, want_pending=True):
    """every case with the view of f0 off, on, and carrying a pending patch (new clocks on ~1 % of f0); -> pending keys seen"""
    e.index_set_ordered(f0, 0)
    off = [_check(e, m, t, **kw) for t, kw in cases]
    e.index_set_ordered(f0, 1)
    on = [_check(e, m, t, **kw) for t, kw in cases]
    assert on == off
    assert e.index_ordered_info(f0)[1], "the view answers"
    have = np.nonzero(m.st[f0] == DATA)[0]
    pick = rng.choice(have, max(len(have) // 100, 8), replace=False)
    nv = rng.integers(lo, hi + 1, len(pick)).astype(np.int64)
    e.merge_batch(m.ids[pick], np.full(len(pick), f0, np.uint32), np.full(len(pick), ts0, np.int64), nv, want_flags=False)
    m.set(f0, pick, nv)
    pending = 0
    patched = []
    for t, kw in cases:
        patched.append(_check(e, m, t, **kw))
        pending = max(pending, e.index_ordered_stats(f0)["pending_keys"])
    if want_pending:
        assert pending > 0 and e.index_ordered_info(f0)[1], "the pending-patch path was really taken"
    e.index_set_ordered(f0, 0)
    assert [_check(e, m, t, **kw) for t, kw in cases] == patched
    return pending


# ---- the reference's dataset (oracle/gen_golden.js genQuerySeeded, restated) ----
def _nodes(N, seed):
    rng = streams.XorShift32(seed)
    ages = np.zeros(N, np.int64); scores = np.zeros(N, np.int64)
    for i in range(N):
        ages[i] = rng() % 100
        scores[i] = rng() % 200001 - 100000
    ids = np.array([streams.fnv1a32("n/k%d" % i) | (i << 32) for i in range(N)], dtype=np.uint64)
    ts = np.array([10 + (i % 7) for i in range(N)], np.int64)
    return ids, ts, ages, scores


@pytest.mark.parametrize("name", ["g5_query_seeded_2k.json", "g5_query_seeded_100k.json"])
def test_reference_dataset(name):
    g = load_golden(name)
    N = g["N"]
    ids, ts, ages, scores = _nodes(N, g["seed"])
    m = Model(ids); m.set(FA, np.arange(N), ages); m.set(FS, np.arange(N), scores)
    with bmx.Engine(4 * N) as e:
        e.merge_batch(np.concatenate([ids, ids]), np.concatenate([np.full(N, FA, np.uint32), np.full(N, FS, np.uint32)]), np.concatenate([ts, ts]),
                      np.concatenate([ages, scores]), want_flags=False)
        by_age = e.scan_aggregate([(FA, 0, 99)], group=FA, group_lo=0, ngroups=100)
        assert len(by_age) == 101 and by_age[100].n_match == 0 and sum(r.n_match for r in by_age) == N
        seen = 0
        cases = [([(FA, 0, 99)], dict(group=FA, group_lo=0, ngroups=100)), ([(FA, 0, 99)], dict(measure=FS)), ([(FA, 10, 19)], dict(measure=FA))]
        for q in g["queries"]:
            if q["op"] in ("equals", "count") and q["field"] == "age":
                v = q["args"][0]
                assert (by_age[v].n_match if 0 <= v < 100 else 0) == q["count"], q
                seen += 1
            elif q["op"] == "filter_and":
                (a0, a1), (s0, s1) = q["args"]
                r = e.scan_aggregate([(FA, a0, a1), (FS, s0, s1)], measure=FS)
                assert r.n_match == q["count"] == r.n, q
                sel = (ages >= a0) & (ages <= a1) & (scores >= s0) & (scores <= s1)
                assert r.sum == int(scores[sel].sum()) and r.min == (int(scores[sel].min()) if sel.any() else None) and r.max == (int(scores[sel].max()) if sel.any() else None), q
                assert _t(e.scan_aggregate([(FS, s0, s1), (FA, a0, a1)], measure=FS)) == _t(r), "either term may lead"
                cases.append(([(FA, a0, a1), (FS, s0, s1)], dict(measure=FS)))
                cases.append(([(FA, a0, a1), (FS, s0, s1)], dict(measure=FS, group=FA, group_lo=a0, ngroups=min(max(a1 - a0 + 1, 1), 200))))
                seen += 1
        assert seen >= 3
        whole = e.scan_aggregate([(FA, 0, 99)], measure=FS)
        assert _t(whole) == (N, N, int(scores.min()), int(scores.max()), int(scores.sum()))
        _three_states(e, m, FA, cases[:12], np.random.default_rng(1))


def test_sum_is_exact_in_128_bits():
    n = 4096
    ids = streams.splitmix64_np(np.arange(1, 3 * n + 1, dtype=np.uint64))
    m = Model(ids)
    m.set(FA, np.arange(3 * n), np.repeat([1, 2, 3], n))
    mixed = np.where(np.arange(n) % 2 == 0, VMAX, -VMAX).astype(np.int64); mixed[:3] = [7, -2, 2**31]
    m.set(FS, np.arange(3 * n), np.concatenate([np.full(n, VMAX), np.full(n, -VMAX), mixed]))
    with bmx.Engine(8 * n) as e:
        for f in (FA, FS):
            e.load_rows(*m.rows(f, 5))
        a = e.scan_aggregate([(FA, 1, 1)], measure=FS)
        assert a.sum == n * VMAX and a.sum > 2**63 and (a.n, a.min, a.max) == (n, VMAX, VMAX)
        b = e.scan_aggregate([(FA, 2, 2)], measure=FS)
        assert b.sum == -n * VMAX and b.sum < -(2**63) and (b.min, b.max) == (-VMAX, -VMAX)
        c = e.scan_aggregate([(FA, 3, 3)], measure=FS)
        assert c.sum == int(sum(int(x) for x in mixed)) and abs(c.sum) < 2**54 and (c.min, c.max) == (-VMAX, VMAX)
        # the wide field itself leads: its index scans its int64 column, the measure comes from that column
        d = e.scan_aggregate([(FS, VMAX, VMAX)], measure=FS)
        assert d.sum == m.agg([(FS, VMAX, VMAX)], measure=FS)[4] and d.sum > 2**63
        cases = [([(FS, -2**62, 2**62)], dict(measure=FS)), ([(FS, -VMAX, -1)], dict(measure=FS)), ([(FS, 1, VMAX), (FA, 1, 3)], dict(measure=FS, group=FA, group_lo=1, ngroups=3)),
                 ([(FA, 1, 3)], dict(measure=FS, group=FA, group_lo=0, ngroups=5)), ([(FS, -VMAX, VMAX)], dict(measure=FS, group=FS, group_lo=VMAX - 1, ngroups=2)),
                 ([(FS, -VMAX, VMAX)], dict(group=FS, group_lo=-VMAX, ngroups=LDS_GROUPS + 1)), ([(FS, -VMAX, VMAX)], dict(measure=FA, group=FS, group_lo=-(2**63), ngroups=4))]
        _three_states(e, m, FS, cases, np.random.default_rng(2), lo=-VMAX, hi=VMAX)


def _sparse_model(N, seed):
    """age on every node; score absent on a third and tombstoned on some; grp absent on a fifth; other on every node"""
    rng = np.random.default_rng(seed)
    ids = streams.splitmix64_np(np.arange(1, N + 1, dtype=np.uint64))
    m = Model(ids)
    allv = np.arange(N)
    m.set(FA, allv, rng.integers(0, 100, N))
    m.set(FS, allv[allv % 3 != 0], rng.integers(-100000, 100001, N)[allv % 3 != 0])
    m.set(FG, allv[allv % 5 != 0], rng.integers(-20, 1500, N)[allv % 5 != 0])
    m.set(FO, allv, rng.integers(0, 10, N))
    return m, rng


def _load_sparse(e, m, tomb_fs, tomb_fa):
    for f in (FA, FS, FG, FO):
        e.load_rows(*m.rows(f, 5))
    for f, idx in ((FS, tomb_fs), (FA, tomb_fa)):
        e.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), bmx.VAL_DELETED, np.int64))
        m.tomb(f, idx)


def test_missing_and_tombstoned_rows():
    N = 60_000
    m, rng = _sparse_model(N, 7)
    tomb_fs = np.arange(1, N, 11); tomb_fs = tomb_fs[tomb_fs % 3 != 0]
    tomb_fa = np.arange(2, N, 97)
    with bmx.Engine(8 * N) as e:
        _load_sparse(e, m, tomb_fs, tomb_fa)
        r = _check(e, m, [(FA, 0, 99)], measure=FS)
        assert r[0] == N - len(tomb_fa) and r[1] < r[0] and r[0] - r[1] == int(((m.st[FS] != DATA) & (m.st[FA] == DATA)).sum())
        assert _t(e.scan_aggregate([(FA, -2**62, 2**62)]))[0] == N - len(tomb_fa), "a tombstoned term-0 row matches nothing"
        for t in ([(FA, 200, 300)], [(FA, 50, 49)], [(FA, 0, 99), (FS, 5, 4)], [(FA, 0, 99), (FO, 77, 78)]):
            assert _t(e.scan_aggregate(t, measure=FS)) == (0, 0, None, None, 0), t
            assert _t(e.scan_aggregate(t, measure=FS, group=FA, group_lo=0, ngroups=3)) == [(0, 0, None, None, 0)] * 4
        cases = [([(FA, 0, 99)], dict(measure=FS)), ([(FA, 10, 40)], {}), ([(FA, 10, 40)], dict(measure=FA)), ([(FA, 10, 40), (FO, 2, 5)], dict(measure=FS)),
                 ([(FS, -500, 90000)], dict(measure=FA)), ([(FS, -500, 90000), (FA, 0, 50)], dict(measure=FG)), ([(FA, 0, 99), (FS, -10**6, 10**6)], dict(measure=FS)),
                 ([(FA, 5, 5), (FO, 0, 9), (FS, -10**6, 10**6), (FG, -20, 1500)], dict(measure=FO))]
        _three_states(e, m, FA, cases, rng)
        _three_states(e, m, FS, cases[4:6], rng, ts0=2000, lo=-100000, hi=100000)


def test_grouping():
    N = 50_000
    m, rng = _sparse_model(N, 8)
    with bmx.Engine(8 * N) as e:
        _load_sparse(e, m, np.arange(1, N, 13), np.arange(2, N, 101))
        T = [(FA, 0, 99)]
        cases = []
        for lo, ng in ((10, 20), (-5, 50), (90, 30), (200, 10), (-100, 50), (0, 1), (0, 100), (0, LDS_GROUPS), (0, LDS_GROUPS + 1), (-30000, 65536)):
            cases.append((T, dict(group=FA, group_lo=lo, ngroups=ng)))                           # the single-field histogram
            cases.append((T, dict(measure=FA, group=FA, group_lo=lo, ngroups=ng)))
        for ng in (1, 100, LDS_GROUPS, LDS_GROUPS + 1, 65536):
            cases.append((T, dict(measure=FS, group=FG, group_lo=-20, ngroups=ng)))              # a group field that is neither term 0 nor the measure, absent on some nodes
            cases.append(([(FA, 20, 60), (FG, 0, 1200)], dict(measure=FS, group=FG, group_lo=100, ngroups=ng)))    # ... and one that a term probes anyway
        cases.append(([(FS, -50000, 50000)], dict(measure=FO, group=FA, group_lo=0, ngroups=100)))
        cases.append(([(FA, 30, 30)], dict(measure=FS, group=FO, group_lo=3, ngroups=4)))
        over = _check(e, m, T, group=FG, group_lo=0, ngroups=10)
        assert over[10][0] > N // 5, "absent, tombstoned and out-of-window group values land in the last record"
        _three_states(e, m, FA, cases, rng)


def test_freshness_growth_and_device_memory():
    N = 30_000
    m, rng = _sparse_model(N, 9)
    dev = torch.device("cuda", 0)
    cases = [([(FA, 0, 99)], dict(measure=FS)), ([(FA, 0, 49)], dict(group=FA, group_lo=0, ngroups=100)), ([(FA, 10, 80), (FO, 1, 8)], dict(measure=FS, group=FG, group_lo=0, ngroups=1400)),
             ([(FA, 0, 99)], dict(measure=FG, group=FO, group_lo=0, ngroups=2000))]
    with bmx.Engine(4 * N) as e:
        _load_sparse(e, m, np.arange(1, N, 13), np.arange(2, N, 101))
        for t, kw in cases:
            _check(e, m, t, **kw)
        # a merge: changed values, tombstoned rows that live again
        pick = rng.choice(N, 3000, replace=False); nv = rng.integers(0, 100, 3000)
        e.merge_batch(m.ids[pick], np.full(3000, FA, np.uint32), np.full(3000, 50, np.int64), nv, want_flags=False)
        m.st[FA][pick] = DATA; m.val[FA][pick] = nv
        for t, kw in cases:
            _check(e, m, t, **kw)
        # a growth
        e.reserve(16 * N)
        for t, kw in cases:
            _check(e, m, t, **kw)
        # index_drop + a rebuild
        e.index_drop(FA)
        for t, kw in cases:
            _check(e, m, t, **kw)
        # device memory: the same records, from a dirty buffer, again and again
        for t, kw in cases:
            ng = kw.get("ngroups", 0)
            want = m.agg(t, **kw)
            buf = torch.full(((ng + 1) * 6 + 6,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            for _ in range(3):
                e.scan_aggregate_dev(t, buf, **kw)
                e.sync()
                host = buf.cpu().numpy()
                assert _t(bmx.agg_results(host[:(ng + 1) * 6].view(bmx.AGG_DTYPE), ng)) == want
                assert (host[(ng + 1) * 6:] == 0x5A5A5A5A5A5A5A5A).all(), "nothing behind the last record is written"


def test_large_run():
    """20M rows, the int32 column and then the same rows in the int64 column: every workgroup of the grid many rounds deep, a ragged tail, LDS histograms
    flushed by every workgroup. (Columns beyond the cache's size, which are read with nontemporal loads, start at 33.5M int64 rows:
    bench_micro/scan_aggregate.py checks its 100M-row answers against numpy.)"""
    R = 20_000_003
    ids = streams.splitmix64_np(np.arange(1, R + 1, dtype=np.uint64))
    with np.errstate(over="ignore"):
        h = streams.splitmix64_np(ids ^ np.uint64(0xABCDEF))
    ages = (h % np.uint64(1000)).astype(np.int64)
    scores = ((h >> np.uint64(20)) % np.uint64(2_000_001)).astype(np.int64) - 1_000_000
    has_s = (h >> np.uint64(50)) % np.uint64(4) != 0
    m = Model(ids); m.set(FA, np.arange(R), ages); m.set(FS, np.nonzero(has_s)[0], scores[has_s])
    with bmx.Engine(2 * R) as e:
        for f in (FA, FS):
            i_, f_, t_, v_ = m.rows(f, 5)
            for r0 in range(0, len(i_), 5_000_000):
                sl = slice(r0, r0 + 5_000_000)
                e.load_rows(i_[sl], f_[sl], t_[sl], v_[sl])
        cases = [([(FA, 100, 199)], dict(measure=FA)), ([(FA, 100, 199)], dict(group=FA, group_lo=100, ngroups=128)), ([(FA, 100, 199)], dict(measure=FS)),
                 ([(FA, 100, 199)], dict(measure=FS, group=FA, group_lo=90, ngroups=128)), ([(FA, 0, 499), (FS, 0, 10000)], dict(measure=FS)), ([(FA, 0, 999)], {})]
        for t, kw in cases:
            _check(e, m, t, **kw)
        # the same column as int64 (one wide value switches the index)
        wide = np.array([R - 1]); m.set(FA, wide, np.array([2**40]))
        e.merge_batch(m.ids[wide], [FA], [99], [2**40], want_flags=False)
        for t, kw in cases:
            _check(e, m, t, **kw)
        assert _t(e.scan_aggregate([(FA, 2**40, 2**40)], measure=FA)) == (1, 1, 2**40, 2**40, 2**40)


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    N = 40_000
    m, rng = _sparse_model(N, 10 + nshards)
    cases = [([(FA, 0, 99)], dict(measure=FS)), ([(FA, 10, 60)], dict(group=FA, group_lo=0, ngroups=100)), ([(FA, 10, 80), (FO, 1, 8)], dict(measure=FS, group=FG, group_lo=0, ngroups=1400)),
             ([(FS, -1000, 99999), (FA, 3, 90)], dict(measure=FG)), ([(FA, 50, 49)], dict(measure=FS)), ([(FA, 0, 99)], dict(measure=FS, group=FO, group_lo=-3, ngroups=65536))]
    with bmx.Engine(8 * N) as e, bmx.Comm([0] * nshards, 8 * N) as c:
        for f in (FA, FS, FG, FO):
            e.load_rows(*m.rows(f, 5)); c.load_rows(*m.rows(f, 5))
        idx = np.arange(1, N, 13)
        tomb = (m.ids[idx], np.full(len(idx), FS, np.uint32), np.full(len(idx), 9, np.int64), np.full(len(idx), bmx.VAL_DELETED, np.int64))
        e.put_rows(*tomb); c.put_rows(*tomb); m.tomb(FS, idx)
        for view in (0, 1):
            c.index_set_ordered(FA, view)
            for t, kw in cases:
                one = _t(e.scan_aggregate(t, **kw)); many = _t(c.scan_aggregate(t, **kw))
                assert one == many == m.agg(t, **kw), (nshards, view, t, kw)
