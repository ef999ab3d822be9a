"""No GPU: the arithmetic of tests/test_gpu_top_kernel_edges.py itself. tests/top_select_model.py — `want` against a brute-force Python sort, `select` against its
own invariants on a few hundred small seeded cases with the constants scaled down — and every layout builder of the GPU file run against a stand-in engine in
plain numpy that answers every query from a table it keeps itself. It proves nothing about a kernel; it proves that the GPU tests ask for what they mean to and
that every tag of top_select_model.TAGS is reached by some layout, in both directions and on both column widths."""
import numpy as np
import pytest

import bmx
import top_select_model as model
import test_gpu_top_kernel_edges as edges

# what the 4-byte column cannot reach: its key word (key - kmin) has at most 32 bits, three digits of 11 (bmx_top.inc top_launch enqueues 3 + 6 rounds for it).
# A condition of the coverage test below, not something to tune.
INT32_CANNOT = {model.value_passes(4), model.value_passes(5)}


# ---- the model ----

def _brute(vals, ids, k, desc, after):
    rows = [(-int(v) if desc else int(v), int(i), int(v)) for v, i in zip(vals, ids)]
    if after is not None:
        a = (-int(after[1]) if desc else int(after[1]), int(after[0]))
        rows = [r for r in rows if (r[0], r[1]) > a]
    rows.sort()
    return [r[1] for r in rows[:k]], [r[2] for r in rows[:k]], len(rows)


def _small_case(rng, G):
    n = int(rng.integers(0, 60))
    kind = int(rng.integers(0, 5))
    span = [1, 2, 1 << G.digit_bits, 1 << (2 * G.digit_bits), 1 << (G.value_bits - 1)][kind]
    vals = rng.integers(0, span, n) - int(rng.integers(0, span))
    if kind == 4 and n > 2:
        vals[:2] = [vals.min(), vals.min() + (1 << G.value_bits) - 1]           # the widest key word the column allows
    if int(rng.integers(0, 2)):
        ids = np.arange(1, n + 1, dtype=np.uint64) + np.uint64(rng.integers(0, (1 << G.id_bits) - n - 1, dtype=np.uint64) if int(rng.integers(0, 2)) else 0)
    elif G.id_bits <= 16:
        ids = rng.choice(np.arange(1, 1 << G.id_bits, dtype=np.uint64), n, replace=False)
    else:
        ids = np.unique(rng.integers(1, (1 << G.id_bits) - 1, 2 * n + 2, dtype=np.uint64))[:n]; rng.shuffle(ids)
    return vals.astype(np.int64), ids.astype(np.uint64)


def test_want_is_a_sort():
    rng = np.random.default_rng(1)
    for case in range(300):
        vals, ids = _small_case(rng, model.Geom(3, 8, 8, 2, 8))
        for desc in (False, True):
            for after in (None, (int(ids[0]), int(vals[0])) if len(ids) else (5, 0), (0, -(1 << 63)), (2**64 - 1, (1 << 63) - 1), (3, (1 << 63) - 1 if desc else -(1 << 63))):
                for k in (1, 7, 100):
                    wi, wv, wne = model.want(vals, ids, k, desc, after)
                    bi, bv, bne = _brute(vals, ids, k, desc, after)
                    assert wne == bne and wi.tolist() == bi and wv.tolist() == bv, (case, desc, after, k)


@pytest.mark.parametrize("geom", [(3, 8, 8, 2, 8), (2, 4, 7, 4, 5), (4, 16, 6, 8, 9), (11, 16, 64, 8, 54)])
def test_select_admits_the_first_rows_of_the_order(geom):
    """the rows the traced boundary admits are exactly the first below + in_bin of the sorted order, they contain rank k, and they fit the candidate list"""
    G = model.Geom(*geom)
    rng = np.random.default_rng(sum(geom))
    tags = set()
    for case in range(300):
        vals, ids = _small_case(rng, G)
        for desc in (False, True):
            for k in sorted({1, 2, G.cand // 2, G.cand - 1, G.cand}):
                S = model.select(vals, ids, k, desc, G)
                tags |= S.tags
                n = len(vals)
                assert model.OUT_OF_PASSES not in S.tags and S.rounds <= G.passes
                assert model.value_passes(0) in S.tags or not S.all
                order = np.lexsort((ids, -vals if desc else vals))
                first = np.zeros(n, bool); first[order[:S.n_admitted]] = True
                assert np.array_equal(first, S.admitted), (case, desc, k)
                assert min(k, n) <= S.n_admitted <= max(G.cand, 0) or n == 0, (case, desc, k, S.n_admitted)
                if not S.all and n:
                    assert S.n_admitted == S.below + S.in_bin and S.below < S.kk <= S.below + S.in_bin
    if geom[0] < 11:
        assert {model.SWITCH, model.ONE_VALUE, model.DONE_V, model.DONE_I, model.ALL, model.SELECT, model.BIN_0, model.ONE_BIN} <= tags, sorted(tags)


def test_select_on_hand_made_cases():
    seq = lambda n: np.arange(1, n + 1, dtype=np.uint64)
    t = model.trace(np.full(5000, 3), seq(5000), 4096)
    assert {model.ONE_VALUE, model.value_passes(0), model.id_passes(6), model.SHORT_I, model.DONE_I} <= t
    assert model.id_passes(5) in model.trace(np.full(5000, 3), seq(5000), 4095)
    assert model.trace(np.arange(4096), seq(4096), 5) >= {model.ALL, model.ELIG_CAND} and model.trace(np.arange(4097), seq(4097), 5) >= {model.SELECT, model.ELIG_CAND1}
    far = (1 << 31) - 1
    t = model.trace(np.concatenate([[0], np.arange(2, 8193), [far]]), seq(8193), 4096, geom=model.GEOM32)
    assert {model.value_passes(3), model.id_passes(0), model.DONE_V, model.SHORT_V} <= t and model.SWITCH not in t
    assert model.DONE_CAND in model.trace(np.concatenate([np.arange(8192), [far]]), seq(8193), 4096)
    # the two directions mirror each other: descending over -v is ascending over v
    v = np.random.default_rng(2).integers(-10**6, 10**6, 9000)
    for k in (1, 1000, 4096):
        assert model.trace(v, seq(9000), k, False) == model.trace(-v, seq(9000), k, True)
    with pytest.raises(AssertionError):
        model.trace(np.array([0, 1 << 40] * 3000), seq(6000), 5, geom=model.GEOM32)       # not a column of int32


# ---- the stand-in engine ----

class Fld:
    def __init__(self):
        self.row = {}; self.ts = np.zeros(0, np.int64); self.val = np.zeros(0, np.int64); self.ids = np.zeros(0, np.uint64); self.perm = None


class Fake:
    """rows by (id, field) with last-writer-wins merges; an index is a fixed shuffle of the field's rows plus appended ones (Fake of test_scan_kernel_edges_model.py)"""

    def __init__(self, cap, *a, **k):
        self.f = {}

    def __enter__(self): return self
    def __exit__(self, *a): pass
    def sync(self): pass

    def _write(self, id, field, ts, val, merge):
        id = np.asarray(id, np.uint64); field = np.asarray(field, np.uint32); ts = np.asarray(ts, np.int64); val = np.asarray(val, np.int64)
        win = np.zeros(len(id), bool)
        for f in np.unique(field).tolist():
            sel = np.flatnonzero(field == f)
            F = self.f.setdefault(int(f), Fld())
            i, t, v = id[sel], ts[sel], val[sel]
            assert len(np.unique(i)) == len(i)
            r = np.array([F.row.get(x, -1) for x in i.tolist()], np.int64)
            new = r < 0
            k = int(new.sum())
            if k:
                base = len(F.ids)
                for j, x in enumerate(i[new].tolist()): F.row[x] = base + j
                F.ids = np.concatenate([F.ids, i[new]]); F.ts = np.concatenate([F.ts, t[new]]); F.val = np.concatenate([F.val, v[new]])
                if F.perm is not None: F.perm = np.concatenate([F.perm, np.arange(base, base + k)])
            w = ~new & ((t > F.ts[np.maximum(r, 0)]) | (not merge))
            F.ts[r[w]] = t[w]; F.val[r[w]] = v[w]
            win[sel] = new | w
        return np.flatnonzero(win).astype(np.uint32)

    def load_rows(self, id, field, ts, val): self._write(id, field, ts, val, False)
    def merge_batch(self, id, field, ts, val, *a, **k): return self._write(id, field, ts, val, True), None, None

    def index_build(self, f):
        F = self.f.setdefault(int(f), Fld())
        if F.perm is None: F.perm = np.random.default_rng(1).permutation(len(F.ids))

    def index_ids(self, f): self.index_build(f); F = self.f[int(f)]; return F.ids[F.perm].copy()

    def scan_top(self, terms, k, desc=False, after=None):
        """a brute-force sort in Python ints, nothing shared with top_select_model.want"""
        f, lo, hi = terms[0]
        F = self.f.get(int(f), Fld())
        rows = []
        for i, v in zip(F.ids.tolist(), F.val.tolist()):
            ok = lo <= v <= hi
            for g, a, b in terms[1:]:
                G = self.f.get(int(g)); r = G.row.get(i, -1) if G else -1
                ok = ok and r >= 0 and a <= int(G.val[r]) <= b
            if ok: rows.append((-v if desc else v, i, v))
        if after is not None:
            a = (-int(after[1]) if desc else int(after[1]), int(after[0]))
            rows = [r for r in rows if (r[0], r[1]) > a]
        rows.sort()
        out = np.zeros(min(k, len(rows)), bmx.TOP_DTYPE)
        out["id"] = [r[1] for r in rows[:k]]; out["val"] = [r[2] for r in rows[:k]]
        return out, len(rows)

    def scan_top_dev(self, terms, k, out, n_out=None, n_eligible=None, desc=False, after=None):
        recs, ne = self.scan_top(terms, k, desc, after)
        out.numpy()[:2 * len(recs)] = recs.view(np.int64)
        if n_out is not None: n_out[0] = len(recs)
        if n_eligible is not None: n_eligible[0] = ne


@pytest.fixture
def standin(monkeypatch):
    monkeypatch.setattr(bmx, "Engine", Fake)
    monkeypatch.setattr(edges, "DEVICE", "cpu")
    monkeypatch.setattr(edges, "SEEN", {})
    return monkeypatch


# ---- the GPU file's layouts ----

def test_no_layout_is_larger_than_40000_rows():
    assert edges.MAX_ROWS == 40_000
    for L in edges.LAYOUTS.values():
        ids, f, v = L.rows()
        per_field = np.unique(f, return_counts=True)[1]
        assert per_field.max() <= edges.MAX_ROWS and len(L.vals) > edges.CAND - 1, L.name
    for n in (33000, edges.SHARE32 + 1, edges.SHARE32 + 3, 36000):
        assert n + 1 <= edges.MAX_ROWS


def test_every_tag_is_reached_in_both_directions_on_both_widths(standin):
    """every test of the GPU file against the stand-in engine: each layout reaches the tags it claims (asserted inside, before each query), and between them the
    layouts reach every tag — no exemption beyond INT32_CANNOT"""
    for name in edges.LAYOUTS:
        edges.test_layout_in_every_form(name)
    edges.test_cursor_inside_one_value()
    edges.test_cursor_on_the_last_id_below_2_63()
    edges.test_cursor_whose_value_is_the_smallest_that_remains()
    assert INT32_CANNOT == model.INT32_CANNOT
    for w in (32, 64):
        for desc in (False, True):
            missing = model.TAGS - edges.SEEN.get((w, desc), set()) - (INT32_CANNOT if w == 32 else set())
            assert not missing, (w, desc, sorted(missing))
        assert not (edges.SEEN[(32, False)] | edges.SEEN[(32, True)]) & INT32_CANNOT, "the model lets the int32 column make more than three value passes"


@pytest.mark.parametrize("name", ["a: ids 1..5000", "b: ties under a deep value"])
def test_page_walks(standin, name):
    edges.test_page_walk(name)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [33000, edges.SHARE32 + 1, edges.SHARE32 + 3, 36000])
def test_by_position(standin, wide, n):
    edges.test_by_position(wide, n)


def test_clean_state(standin):
    edges.test_clean_state_between_deep_shallow_all_and_empty_queries()


def test_the_ballot_model_on_hand_made_cases():
    n, E = 256, 4
    p = np.arange(n)
    lane = p // E % 64
    assert edges._ballots(lane == 0, p % 7, E, n) == {edges.LANE0} and edges._ballots(lane == 63, p % 7, E, n) == {edges.LANE63}
    assert edges._ballots(p >= 0, np.zeros(n, np.int64), E, n) == {edges.SAME_BIN} and edges._ballots(p >= 0, p, E, n) == {edges.ALL_DIFFERENT}
    assert edges._ballots(p >= 0, None, E, n) == set()
    n = edges.SHARE32 + 1
    assert edges._ballots(np.arange(n) == n - 1, None, 4, n) == {edges.RAGGED_ONLY} and edges._ballots(np.arange(n) >= n - 2, None, 4, n) == set()
