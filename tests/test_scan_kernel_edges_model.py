"""No GPU: the arithmetic of tests/test_gpu_scan_kernel_edges.py itself — its by-position harness, its layouts, its caps and fill checks, its aggregate
arithmetic and the branches its model says the layouts reach — run against a stand-in engine in plain numpy that answers every query from a table it keeps
itself (rows by (id, field) with last-writer-wins merges, an index as a fixed shuffle of the rows plus appended ones). It proves nothing about a kernel; it
proves that the GPU tests ask for what they mean to and that every expected branch tag is reached by some layout, at a few sizes of every test."""
import numpy as np
import pytest

import bmx
import test_gpu_scan_kernel_edges as edges

TOMB = edges.TOMB


class R:
    pass


class Fld:
    def __init__(self):
        self.row = {}; self.ts = np.zeros(0, np.int64); self.val = np.zeros(0, np.int64); self.ids = np.zeros(0, np.uint64); self.perm = None


class Fake:
    def __init__(self, cap, *a, **k):
        self.f = {}

    def __enter__(self): return self
    def __exit__(self, *a): pass
    def sync(self): pass

    def _write(self, id, field, ts, val, merge):
        id = np.asarray(id, np.uint64); field = np.asarray(field, np.uint32); ts = np.asarray(ts, np.int64); val = np.asarray(val, np.int64)
        assert len(set(field.tolist())) <= 1
        if not len(id): return np.zeros(0, np.uint32)
        F = self.f.setdefault(int(field[0]), Fld())
        assert len(set(id.tolist())) == len(id)
        r = np.array([F.row.get(i, -1) for i in id.tolist()], np.int64)
        new = r < 0
        k = int(new.sum())
        if k:
            base = len(F.ids)
            for j, i in enumerate(id[new].tolist()): F.row[i] = base + j
            F.ids = np.concatenate([F.ids, id[new]]); F.ts = np.concatenate([F.ts, ts[new]]); F.val = np.concatenate([F.val, val[new]])
            if F.perm is not None: F.perm = np.concatenate([F.perm, np.arange(base, base + k)])
        old = ~new
        win = new.copy()
        w = old & ((ts > F.ts[np.maximum(r, 0)]) | (not merge))
        F.ts[r[w]] = ts[w]; F.val[r[w]] = val[w]
        win |= w
        return np.flatnonzero(win).astype(np.uint32)

    def load_rows(self, id, field, ts, val): self._write(id, field, ts, val, False)
    put_rows = load_rows

    def merge_batch(self, id, field, ts, val, *a, **k): return self._write(id, field, ts, val, True), None, None

    def index_build(self, f):
        F = self.f.setdefault(int(f), Fld())
        if F.perm is None: F.perm = np.random.default_rng(1).permutation(len(F.ids))

    def index_ids(self, f): self.index_build(f); F = self.f[int(f)]; return F.ids[F.perm].copy()
    def index_size(self, f): return len(self.index_ids(f))

    def _vals(self, f):
        F = self.f[int(f)]; return F.val[F.perm]

    def _match(self, f, lo, hi):
        self.index_build(f)
        v = self._vals(f)
        lo = max(lo, -(1 << 63) + 1); hi = min(hi, (1 << 63) - 1)
        if lo > hi: return np.zeros(0, np.int64)
        return np.flatnonzero((v != TOMB) & (v >= lo) & (v <= hi))

    def scan_range_pos(self, f, lo, hi, cap=None):
        m = self._match(f, lo, hi); return m[:cap].astype(np.uint32)

    def scan_range(self, f, lo, hi, cap=None):
        m = self._match(f, lo, hi); return self.index_ids(f)[m][:cap]

    def scan_count(self, f, lo, hi): return len(self._match(f, lo, hi))

    def scan_range_dev(self, f, lo, hi, out, cap, n_out):
        ids = self.scan_range(f, lo, hi)
        n_out[0] = len(ids)
        k = min(len(ids), cap)
        out.numpy()[:k] = ids[:k].view(np.int64)

    def scan_filter(self, terms, cap=None):
        f, lo, hi = terms[0]
        m = self._match(f, lo, hi); ids = self.index_ids(f)[m]
        keep = []
        for i in ids.tolist():
            ok = True
            for g, a, b in terms[1:]:
                G = self.f.get(int(g)); r = G.row.get(i, -1) if G else -1
                ok = ok and r >= 0 and G.val[r] != TOMB and a <= G.val[r] <= b
            if ok: keep.append(i)
        return np.array(keep, np.uint64)[:cap]

    def scan_aggregate(self, terms, measure=None, group=None, group_lo=0, ngroups=0):
        f, lo, hi = terms[0]
        m = self._match(f, lo, hi); v = self._vals(f)[m].astype(object)
        recs = [R() for _ in range(ngroups + 1 if ngroups else 1)]
        for r in recs: r.n_match = r.n = r.sum = 0; r.min = r.max = None
        for x in v.tolist():
            g = x - group_lo if ngroups and 0 <= x - group_lo < ngroups else ngroups
            r = recs[g]; r.n_match += 1; r.n += 1; r.sum += x
            r.min = x if r.min is None else min(r.min, x); r.max = x if r.max is None else max(r.max, x)
        return recs if ngroups else recs[0]


@pytest.fixture
def standin(monkeypatch):
    monkeypatch.setattr(bmx, "Engine", Fake)
    monkeypatch.setattr(edges, "DEVICE", "cpu")
    return monkeypatch


@pytest.mark.parametrize("wide,n", [(False, 5), (True, 129), (True, 2049), (False, 8193)])
def test_layouts_under_the_default_switches(standin, wide, n):
    edges.test_every_layout_under_the_default_switches(wide, n)


@pytest.mark.parametrize("form", list(edges.FORMS))
@pytest.mark.parametrize("wide,n", [(False, 1), (True, 2049), (False, 8193)])
def test_reduced_layouts_under_each_switch(standin, form, wide, n):
    edges.test_reduced_layouts_under_each_switch(standin, wide, form, n)


@pytest.mark.parametrize("wide,n", [(False, 8193), (True, 8193)])
def test_eight_blocks_per_workgroup(standin, wide, n):
    edges.test_eight_blocks_per_workgroup(standin, wide, n)
    edges.test_eight_blocks_per_workgroup_with_the_stream_forced_and_off(standin, wide, 1, n)
    edges.test_eight_blocks_per_workgroup_with_the_stream_forced_and_off(standin, wide, edges.NEVER, n)


@pytest.mark.parametrize("n", [65535, 65536, 65537, 131075])
def test_the_larger_sizes_of_eight_blocks_per_workgroup_reach_their_branches(n):
    """without any engine: the tags of the layouts alone"""
    seen = set()
    for name, m, dead in edges._layouts_sub8(n, np.random.default_rng(300 + n)):
        for odd in (0, 1):
            seen |= edges._branches(np.flatnonzero(m), n, sub8_blocks=1, out_odd=odd) if m.any() else set()
    edges._expect(seen, edges._sub8_tags(n), n)


@pytest.mark.parametrize("wide,n", [(False, 7), (True, 7), (True, 1), (False, 8195)])
def test_extreme_values_and_bounds(standin, wide, n):
    edges.test_extreme_values_in_the_last_lane_group_and_the_query_bounds(wide, n)


@pytest.mark.parametrize("wide,n", [(False, 1), (True, 33), (False, 2049)])
def test_filter(standin, wide, n):
    edges.test_filter_of_two_terms_in_column_order(standin, wide, n)


@pytest.mark.parametrize("kind", ["int32", "int64 shifted", "int64 by one -2^31"])
@pytest.mark.parametrize("n", [1, 5, 4097])
def test_aggregates(standin, kind, n):
    edges.test_aggregates_of_short_columns_and_at_the_sweeps_round(kind, n)


def test_the_model_of_the_branches_on_hand_made_cases():
    B = edges.BLOCK
    t = edges._branches(np.arange(101, 101 + 2399), B)
    assert t == {"gather"}
    t = edges._branches(np.arange(101, 101 + 2400), B)          # groups of 411, 512, 512, 512, 453: the second starts at the odd rank 411
    assert {"stream", "T == 0", "T == 512", "T > 1", "stream, a wave without a match", "odd rest", "pairs", "head"} <= t and "gather" not in t
    assert "head" not in edges._branches(np.arange(0, 2400), B) and "head" in edges._branches(np.arange(0, 2400), B, out_odd=1)
    assert edges._branches(np.array([B]), B + 1, stream_min=1, out_odd=1) >= {"gather, empty block", "stream, one-row block", "head only", "T == 1", "T == 0"}
    assert edges._branches(np.arange(0, 8 * B, 8), 8 * B + 1, sub8_blocks=1) == {"sub8 fast path", "sub8 fast path, %d matches" % B, "sub8 fast path, 0 matches", "sub8 workgroup of 1 block"}
    t = edges._branches(np.concatenate([np.arange(0, 8 * B, 8), [4099]]).astype(np.int64), 8 * B, sub8_blocks=1)
    assert "sub8 fall-through, %d matches" % (B + 1) in t and "sub8 gather" in t and "sub8 stream" not in t
    assert edges._branches(np.array([8 * B - 1]), 8 * B, sub8_blocks=1) >= {"sub8 fast path, local offset 65535", "sub8 fast path, 1 matches"}
    assert edges._branches(np.arange(8), 2 * B, sub8_blocks=1, stream_min=1) >= {"sub8 fall-through", "sub8 stream", "sub8 gather, empty block"}
    assert edges._branches(np.arange(7), 2 * B, sub8_blocks=1, stream_min=1) == {"sub8 fast path", "sub8 workgroup of 2 blocks"}
    assert edges._dense_cap(np.array([0, 5, 6, 7, 8, 9, 20])) in (3, 5) and edges._dense_cap(np.array([1, 3, 5])) is None
