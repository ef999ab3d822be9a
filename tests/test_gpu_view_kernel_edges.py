"""GPU: the value-ordered view's own kernels (csrc/view_kernels.h: k_view_tile_sort, k_view_merge_pass, k_view_merge, k_view_merge2, k_view_flag_in,
k_ordered_copy_p and the 64-ary searches) at their tile, chunk, group and window edges — small, structured, adversarial columns instead of large random ones.

Every check is exact integer equality against numpy. The index's id column (index_ids) says which row sits at every position; with the model's value of that
row the view must list the live positions in np.lexsort((position, value)) order, element for element. While a patch is pending the listing is the survivors of
the view's main run in (value, position) order followed by the pending inserted keys in (value, position) order; the model below keeps both runs the way
patch_view_t (csrc/bmx_view.inc) does, and the number of pending keys must agree too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from oracle import streams
from oracle.oracle import VAL_DELETED

FA, FS = streams.fnv1a32("age"), streams.fnv1a32("score")
LO, HI = -(1 << 60), 1 << 60            # the whole range
TOMB = VAL_DELETED                       # a tombstoned row's key value: in front of every legal value, never listed
I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)


def _enc(v, wide):
    """the column's value for the small number v: as it is (int32 column), or shifted left by 33 plus 2^32 — no such value fits int32, the order is kept"""
    v = np.asarray(v, np.int64)
    return (v << 33) + (1 << 32) if wide else v


class ViewModel:
    """One indexed field of one engine: the rows (id -> value or TOMB) as the writes of the test leave them, the index's id column as last read, and the
    view as main - pd + pi in position space (at most one key per position in each run)."""

    def __init__(self, e, f):
        self.e, self.f = e, f
        self.ids = np.zeros(0, np.uint64); self.val = np.zeros(0, np.int64)
        self.clock = 10
        self.next_id = 1
        self._by_id = None
        self.forget_index()

    def forget_index(self):
        self.col = np.zeros(0, np.uint64); self.key = np.zeros(0, np.int64)
        self.main_key = None

    def new_ids(self, k):
        ids = streams.splitmix64_np(np.arange(self.next_id, self.next_id + k, dtype=np.uint64))
        self.next_id += k
        return ids

    def _rows(self, ids):
        if self._by_id is None:
            o = np.argsort(self.ids, kind="stable"); self._by_id = (o, self.ids[o])
        o, s = self._by_id
        if len(s) == 0:
            return np.zeros(len(ids), np.int64), np.zeros(len(ids), bool)
        k = np.minimum(np.searchsorted(s, ids), len(s) - 1)
        return o[k], s[k] == ids

    def load(self, ids, vals):
        self.e.load_rows(ids, np.full(len(ids), self.f, np.uint32), np.full(len(ids), 5, np.int64), vals)
        self.ids = np.asarray(ids, np.uint64).copy(); self.val = np.asarray(vals, np.int64).copy(); self._by_id = None

    def write(self, ids, vals, put=False):
        """a merge under a newer clock than anything stored (every delta wins), or put_rows (tombstones: vals = TOMB); unknown ids are new rows"""
        ids = np.asarray(ids, np.uint64)
        vals = np.broadcast_to(np.asarray(vals, np.int64), ids.shape).copy()
        if len(ids) == 0:
            return
        assert len(np.unique(ids)) == len(ids)
        self.clock += 10
        args = (ids, np.full(len(ids), self.f, np.uint32), np.full(len(ids), self.clock, np.int64), vals)
        if put:
            self.e.put_rows(*args)
        else:
            assert len(self.e.merge_batch(*args)[0]) == len(ids), "every delta of the test wins"
        r, hit = self._rows(ids)
        self.val[r[hit]] = vals[hit]
        if not hit.all():
            self.ids = np.concatenate([self.ids, ids[~hit]]); self.val = np.concatenate([self.val, vals[~hit]]); self._by_id = None

    def refresh(self):
        """read the id column again (this brings the index, and through it the view, up to date): the key at every position, and what changed since the last time"""
        col = self.e.index_ids(self.f)
        n0 = len(self.col)
        assert len(col) == len(self.ids) and np.array_equal(col[:n0], self.col), "the test's premise: no position of the index is renumbered"
        r, hit = self._rows(col)
        assert hit.all()
        key = self.val[r]
        if self.main_key is not None:
            grow = len(col) - len(self.pd)
            self.pd = np.concatenate([self.pd, np.zeros(grow, bool)]); self.pi = np.concatenate([self.pi, np.zeros(grow, bool)])
            self.pi_key = np.concatenate([self.pi_key, np.zeros(grow, np.int64)])
            chg = np.flatnonzero(key[:n0] != self.key)
            self.pd[chg[~self.pi[chg]]] = True        # a deleted key that is a pending insert cancels it; the others are keys of main
            new = np.concatenate([chg, np.arange(n0, len(col))])
            self.pi[new] = True; self.pi_key[new] = key[new]
            self.last_run = (len(chg), len(col) - n0)
        self.col, self.key = col, key

    def rebase(self):
        """the view's main run holds every key as it is now"""
        n = len(self.key)
        self.main_key = self.key.copy(); self.main_order = np.lexsort((np.arange(n), self.key))
        self.pd = np.zeros(n, bool); self.pi = np.zeros(n, bool); self.pi_key = np.zeros(n, np.int64)

    def stats(self):
        return self.e.index_ordered_stats(self.f)

    def sync(self):
        self.refresh()
        st = self.stats()
        if st["pending_keys"] == 0:
            self.rebase()
        else:
            assert st["pending_keys"] == int(self.pd.sum()) + int(self.pi.sum()), (st, int(self.pd.sum()), int(self.pi.sum()))
        return st

    def rank_order(self):
        """positions by rank in the view (tombstones in front)"""
        return np.lexsort((np.arange(len(self.key)), self.key))

    def sorted_live(self, lo=LO, hi=HI):
        live = np.flatnonzero((self.key != TOMB) & (self.key >= lo) & (self.key <= hi))
        return live[np.lexsort((live, self.key[live]))]

    def listing(self, lo=LO, hi=HI):
        surv = self.main_order[~self.pd[self.main_order]]
        sv = self.main_key[surv]
        surv = surv[(sv != TOMB) & (sv >= lo) & (sv <= hi)]
        ins = np.flatnonzero(self.pi); iv = self.pi_key[ins]
        keep = (iv != TOMB) & (iv >= lo) & (iv <= hi)
        ins, iv = ins[keep], iv[keep]
        return np.concatenate([surv, ins[np.lexsort((ins, iv))]])


def _same(got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def _check(m, ranges=()):
    """bring the view up to date and hold the whole-range listing (positions, ids, count) and the given sub-ranges against the model"""
    st = m.sync()
    e, f = m.e, m.f
    pending = st["pending_keys"] > 0
    for lo, hi in [(LO, HI)] + list(ranges):
        fresh = m.sorted_live(lo, hi)
        want = m.listing(lo, hi) if pending else fresh
        pos = e.scan_range_pos(f, lo, hi).astype(np.int64)
        _same(pos, want, ("positions", lo, hi, st))
        _same(e.scan_range(f, lo, hi), m.col[want], ("ids", lo, hi, st))
        assert e.scan_count(f, lo, hi) == len(want), (lo, hi, st)
        if pending:
            assert np.array_equal(np.sort(pos), np.sort(fresh)), (lo, hi, st)
    return m.stats()


def _ranges(m, rng, k=3):
    """a handful of value ranges: both ends, single values, pairs, between two values, an empty one"""
    vs = np.unique(m.key[m.key != TOMB])
    if len(vs) == 0:
        return [(0, 10)]
    a, b, mid = int(vs[0]), int(vs[-1]), int(vs[len(vs) // 2])
    out = [(a, a), (b, b), (a - 3, a - 1), (b + 1, b + 3), (mid + 1, mid), (mid, b), (a, mid)]
    for _ in range(k):
        x, y = sorted(rng.choice(len(vs), 2).tolist())
        out.append((int(vs[x]) + 1, int(vs[y])))
    return out


def _engine(monkeypatch, rows, **env):
    """an engine with room for `rows` rows without a table growth, created under the given A/B switches (they are read at create)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = bmx.Engine(max(1 << 14, 4 * rows))
    for k in env:
        monkeypatch.delenv(k)
    return e


def _fresh_view(e, f, vals):
    """len(vals) rows with these values, indexed, the view sorted by the first query"""
    m = ViewModel(e, f)
    m.load(m.new_ids(len(vals)), vals)
    e.index_build(f); e.index_set_ordered(f, 1)
    e.scan_count(f, 0, 0)
    m.refresh(); m.rebase()
    st = m.stats()
    assert st["sorts"] == 1 and st["patches"] == 0 and e.index_ordered_info(f)[1], st
    return m


# ---- A. the sort kernels on structured columns ----

SIZES_A = [1, 2, 7, 8, 9, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 12288, 12289, 16385, 40961, 70001]


def _layouts(n, rng, wide):
    """value as a function of position"""
    p = np.arange(n, dtype=np.int64)
    run = np.full(n, 3, np.int64)                   # one long run of equal values, a handful of extremes at both ends (the last ones inside a ragged last tile):
    ends = np.unique(np.concatenate([p[:3], p[-3:]]))      # for the int32 column the values next to the sort's padding key and to the tombstone key
    ext = [50_000, -50_000, 49_999, -49_999] if wide else [I32_MAX, I32_MIN + 1, I32_MAX - 1, I32_MIN + 2]
    run[ends] = np.resize(np.array(ext, np.int64), len(ends))
    return [
        ("a few distinct values", rng.integers(0, 5, n).astype(np.int64)),
        ("all equal", np.full(n, 7, np.int64)),
        ("ascending", p.copy()),
        ("descending", n - 1 - p),
        ("first half high, second half low", np.where(p < n // 2, 100 + p % 5, p % 5)),
        ("sawtooth of period 4096", p % 4096),
        ("organ pipe", np.minimum(p, n - 1 - p)),
        ("one long run with extremes at both ends", run),
    ]


def _dead_positions(n, rng):
    cand = np.unique(np.concatenate([[0, n - 1, n // 2, n // 3, 4095, 4096, 8191], rng.integers(0, n, 4)]))
    cand = cand[cand < n]
    return rng.permutation(cand)[:min(len(cand), n // 2, 7)]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES_A)
def test_own_sort_of_structured_columns(monkeypatch, wide, n):
    """BMX_VIEW_SORT=own: a fresh view sorted by k_view_tile_sort + k_view_merge_pass. Sizes around the 4096-key tile and its multiples, and runs of 8192 keys and
    more (the merge-path interval then exceeds 2 * MP_WINDOW: the guessed window round, with the cut in front of it for a descending column and behind it for an
    ascending one). A few tombstones in every column: they sort in front and are not listed."""
    f = FS if wide else FA
    rng = np.random.default_rng(1000 + n)
    with _engine(monkeypatch, n, BMX_VIEW_SORT="own") as e:
        m = ViewModel(e, f)
        m.load(m.new_ids(n), np.full(n, _enc(1, wide), np.int64))
        for name, v in _layouts(n, rng, wide):
            e.index_build(f)
            m.refresh()
            m.write(m.col, _enc(v, wide))                        # value by POSITION; revives the rows the layout before tombstoned
            dead = _dead_positions(n, rng)
            m.write(m.col[dead], TOMB, put=True)
            m.refresh()
            e.index_set_ordered(f, 1)
            e.scan_count(f, 0, 0)                                # the first query sorts
            m.rebase()
            st = _check(m, _ranges(m, rng))
            assert st["sorts"] == 1 and st["patches"] == 0 and st["pending_keys"] == 0, (name, st)
            assert len(m.sorted_live()) == n - len(dead), name
            e.index_drop(f); m.forget_index()                    # the next layout gets a new index and a new view


def test_minus_two_to_the_31_makes_the_column_wide_and_the_view_is_sorted_from_it(monkeypatch):
    """an int32 column with INT32_MAX and INT32_MIN + 1 in its ragged last tile; then -(2^31) arrives, which the 4-byte column cannot tell from a tombstone:
    the index goes wide and the view is sorted again from the 8-byte column"""
    n = 4096 + 513
    rng = np.random.default_rng(31)
    v = rng.integers(-4, 5, n).astype(np.int64)
    v[[n - 1, n - 7, 4096, 0]] = [I32_MAX, I32_MIN + 1, I32_MIN + 1, I32_MAX]
    with _engine(monkeypatch, n, BMX_VIEW_SORT="own") as e:
        m = _fresh_view(e, FA, v)
        m.write(m.col[[5, n - 2]], TOMB, put=True)
        st = _check(m, [(I32_MIN, I32_MIN + 1), (I32_MAX, I32_MAX), (I32_MIN + 1, 0), (5, I32_MAX)])
        assert st["sorts"] == 1 and st["patches"] == 1, st
        m.write(m.col[[n - 3, 17]], [I32_MIN, I32_MIN + 1])
        m.refresh()
        assert e.scan_count(FA, I32_MIN, I32_MIN) == 1            # (the query sorts the wide column)
        m.rebase()
        st = _check(m, [(I32_MIN, I32_MIN), (I32_MIN, I32_MIN + 1), (I32_MIN - 5, I32_MIN - 1), (I32_MAX, I32_MAX), (0, HI)])
        assert st["sorts"] == 2 and st["pending_keys"] == 0, st


# ---- B. the streaming merge k_view_merge at small shapes: BMX_VIEW_PENDING=0, every patch rewrites main at once ----

NX_B = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 6145]
KS_B = [1, 63, 64, 65, 1024, 1025, 3000]


def _base(nx, rng):
    """multiples of 4 with duplicates: ties are decided by position, and values between two keys exist"""
    return 4 * rng.integers(0, nx // 3 + 1, nx).astype(np.int64)


def _patched_once(m, before, ranges=()):
    st = _check(m, ranges)
    assert st["patches"] == before["patches"] + 1 and st["rewrites"] == before["rewrites"] + 1 and st["pending_keys"] == 0 and st["sorts"] == 1, (before, st)
    return st


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("nx", NX_B)
def test_streaming_merge_of_appended_rows_only(monkeypatch, wide, nx):
    """c == 0: k new rows below every value (tile 0's keys in front of the view's first key), above every value (behind the last key of a ragged last tile),
    half and half; 3000 of them overflow the inserted-key window of the tile they fall into"""
    f = FS if wide else FA
    rng = np.random.default_rng(2000 + nx)
    base = _base(nx, rng)
    for k in KS_B:
        for where in ("below", "above", "both"):
            i = np.arange(k, dtype=np.int64)
            below, above = -1 - i % 3, int(base.max()) + 1 + i % 3
            v = below if where == "below" else above if where == "above" else np.where(i < k // 2, below, above)
            with _engine(monkeypatch, nx + k, BMX_VIEW_PENDING="0") as e:
                m = _fresh_view(e, f, _enc(base, wide))
                st = m.stats()
                m.write(m.new_ids(k), _enc(v, wide))
                _patched_once(m, st)
                assert m.last_run == (0, k), (k, where)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("nx", NX_B)
def test_streaming_merge_of_changed_rows_only(monkeypatch, wide, nx):
    """added == 0, one engine: a whole tile of the view moves above everything (2048 deleted keys in one tile, no survivor: the deleted-key window overflows);
    exactly 1024 keys of one tile, then 1025; the keys at the chunk and tile boundaries; every row, to the reversed order of values; every row to one value;
    every row tombstoned; every row revived"""
    f = FS if wide else FA
    rng = np.random.default_rng(3000 + nx)
    base = _base(nx, rng)
    top = int(base.max())
    with _engine(monkeypatch, nx, BMX_VIEW_PENDING="0") as e:
        m = _fresh_view(e, f, _enc(base, wide))
        st = m.stats()
        step = int(_enc(1, wide) - _enc(0, wide))

        def move(ranks, vals, put=False):
            """the keys at these ranks of the view as it is now get these values: one patch (none where no key moves, as with one row 'reversed')"""
            nonlocal st
            ranks = np.asarray(ranks, np.int64)
            ranks = np.unique(ranks[(ranks >= 0) & (ranks < nx)])
            pos = m.rank_order()[ranks]
            vals = np.broadcast_to(np.asarray(vals, np.int64), (len(vals),) if np.ndim(vals) else (len(pos),))[:len(pos)]
            moved = int((m.key[pos] != vals).sum())
            if moved:
                m.write(m.col[pos], vals, put)
                st = _patched_once(m, st, _ranges(m, rng, 1))
                assert m.last_run == (moved, 0)
            return moved

        every = np.arange(nx)
        t0 = 2048 if nx > 2048 else 0
        top += 2; assert move(np.arange(t0, t0 + 2048), _enc(top + np.arange(2048) % 2, wide)) == min(nx - t0, 2048)      # one whole tile
        top += 2; assert move(np.arange(0, 2048, 2), _enc(top, wide)) == min((nx + 1) // 2, 1024)                        # 1024 keys of tile 0 (every other one)
        top += 2; assert move(np.arange(3, 3 + 1025), _enc(top, wide)) == max(0, min(nx - 3, 1025))                      # 1025 keys of tile 0
        edge = np.array([0, 3, 4, 255, 256, 257, 2047, 2048, nx - 1])
        edge = np.unique(edge[edge < nx])
        move(edge, m.key[m.rank_order()[edge]] + step * (1 + 4 * (np.arange(len(edge)) % 2)))                            # boundary keys, a little up: behind their equals
        move(every, m.key[m.rank_order()][::-1].copy())                                                                   # c == nx: the reversed order of values
        top += 8; assert move(every, _enc(top, wide)) == nx                                                               # every row the same value
        assert move(every, TOMB, put=True) == nx                                                                          # every row tombstoned: nothing is listed
        assert len(m.sorted_live()) == 0 and e.scan_count(f, LO, HI) == 0
        assert move(every, _enc(_base(nx, rng), wide)) == nx                                                              # every row revived
        assert len(m.sorted_live()) == nx and st["patches"] >= 5


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("nx", NX_B)
def test_streaming_merge_places_new_keys_inside_a_lanes_group_of_four(monkeypatch, wide, nx):
    """a lane of k_view_merge owns four consecutive keys: new keys that land right behind its 1st, 2nd, 3rd, 4th key, behind all four, several behind one key,
    and behind a key that leaves in the same patch — in the first and last group of a chunk, of a tile and of the view. Distinct values: the key at rank r is 4r."""
    f = FS if wide else FA
    rng = np.random.default_rng(4000 + nx)
    base = 4 * rng.permutation(nx).astype(np.int64)
    groups = [g for g in sorted({0, 1, 63, 64, 511, 512, (nx - 1) // 4}) if 4 * g < nx]
    for variant in (0, 1, 2, 3, "all", "several", "gone"):
        new, leave = [], []
        for g in groups:
            for j in range(4):
                r = 4 * g + j
                if r >= nx:
                    break
                if variant == j or variant == "all":
                    new.append(4 * r + 1)
                elif variant == "several" and j == g % 4:
                    new += [4 * r + 1, 4 * r + 1, 4 * r + 2, 4 * r + 3]
                elif variant == "gone" and j == (g + 1) % 4:
                    new.append(4 * r + 1); leave.append(r)
        if not new:
            continue
        with _engine(monkeypatch, nx + len(new), BMX_VIEW_PENDING="0") as e:
            m = _fresh_view(e, f, _enc(base, wide))
            st = m.stats()
            order = m.rank_order()
            assert np.array_equal(m.key[order], _enc(4 * np.arange(nx), wide))
            m.write(m.new_ids(len(new)), _enc(new, wide))
            m.write(m.col[order[leave]], _enc(4 * nx + 8, wide))
            _patched_once(m, st)
            assert m.last_run == (len(leave), len(new)), variant


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("nx", [5, 257, 2049, 6145])
def test_streaming_merge_under_a_mix_of_all_of_it(monkeypatch, wide, nx):
    """several rounds on one engine (the two sets of view columns take turns): rows change, some to the value they have; rows are appended below, above and
    in between; rows are tombstoned; tombstoned rows come back"""
    f = FS if wide else FA
    rng = np.random.default_rng(5000 + nx)
    with _engine(monkeypatch, nx + 6 * 700, BMX_VIEW_PENDING="0") as e:
        m = _fresh_view(e, f, _enc(_base(nx, rng), wide))
        st = m.stats()
        for rnd in range(6):
            n = len(m.col)
            k = rng.choice(n, max(1, n // 3), replace=False)
            nv = _enc(4 * rng.integers(0, nx // 3 + 1, len(k)) + rng.integers(0, 2, len(k)), wide)
            keep = (np.arange(len(k)) % 5 == 0) & (m.key[k] != TOMB)
            nv[keep] = m.key[k][keep]                              # ... no key moves for these
            m.write(m.col[k], nv)
            a = int(rng.integers(1, 700))
            av = np.concatenate([np.full(a // 3, -2 - rnd), np.full(a // 3, 4 * nx + rnd), 4 * rng.integers(0, nx // 3 + 1, a - 2 * (a // 3)) + 3]).astype(np.int64)
            m.write(m.new_ids(a), _enc(av, wide))
            d = rng.choice(n, max(1, n // 7), replace=False)
            m.write(m.col[d], TOMB, put=True)
            st = _patched_once(m, st, _ranges(m, rng, 2))
            assert len(m.col) == n + a


# ---- C. the pending patch and its kernels (default switches): views of 50k rows, a patch stays pending below 65536 keys ----

R_C = 50_000


def _view_c(e, f, wide, rng):
    return _fresh_view(e, f, _enc(4 * rng.integers(0, 2000, R_C), wide))


def _pending(m, ranges=()):
    st = _check(m, ranges)
    assert st["sorts"] == 1 and st["rewrites"] == 0 and st["pending_keys"] > 0, st
    return st


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("c1,c3,added", [(1023, 3, 2), (1024, 3, 2), (1025, 3, 2), (2048, 3, 2), (2049, 3, 2),
                                         (723, 300, 1), (724, 300, 1), (725, 300, 1), (1748, 300, 1), (1749, 300, 1)])
def test_consecutive_patches_before_any_rewrite(monkeypatch, wide, c1, c3, added):
    """(i) c1 rows change: the first pending patch, k_view_merge2 with la == 0. (ii) the same rows change again: every deleted key is a pending insert (cX == 0) and
    the surviving pi run is empty before the merge. (iii) c3 other rows change or are tombstoned: no deleted key is a pending insert (cI == 0); pd and pi are
    merged with runs of c1 + c3 keys. (iv) the rows of (i) go back to the value main still holds. (v) appended rows only. The merged run lengths la + lb are
    c1, c1 + c3 and c1 + c3 + added: 1023, 1024, 1025, 2048 and 2049 among them."""
    f = FS if wide else FA
    rng = np.random.default_rng(6000 + c1)
    with _engine(monkeypatch, R_C + added) as e:
        m = _view_c(e, f, wide, rng)
        rows = rng.permutation(R_C)
        r1, r3 = rows[:c1], rows[c1:c1 + c3]
        main = m.key.copy()
        rg = lambda: _ranges(m, rng, 1)[3:]
        m.write(m.col[r1], _enc(4 * rng.integers(0, 2000, c1) + 1, wide)); st = _pending(m, rg())              # (i)
        assert st["patches"] == 1 and st["pending_keys"] == 2 * c1 and m.last_run == (c1, 0), st
        m.write(m.col[r1], _enc(4 * rng.integers(0, 2000, c1) + 2, wide)); st = _pending(m, rg())              # (ii)
        assert st["patches"] == 2 and st["pending_keys"] == 2 * c1 and m.last_run == (c1, 0), st
        m.write(m.col[r3[2:]], _enc(4 * rng.integers(0, 2000, c3 - 2) + 1, wide)); m.write(m.col[r3[:2]], TOMB, put=True)
        st = _pending(m, rg())                                                                                     # (iii)
        assert st["patches"] == 3 and st["pending_keys"] == 2 * (c1 + c3) and m.last_run == (c3, 0), st
        m.write(m.col[r1], main[r1]); st = _pending(m, rg())                                                       # (iv)
        assert st["patches"] == 4 and st["pending_keys"] == 2 * (c1 + c3) and m.last_run == (c1, 0), st
        m.write(m.new_ids(added), _enc([-1, 9000][:added], wide)); st = _pending(m, rg())                          # (v)
        assert st["patches"] == 5 and st["pending_keys"] == 2 * (c1 + c3) + added and m.last_run == (0, added), st


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("first", ["below", "above"])
def test_pending_inserts_merged_from_two_long_runs_disjoint_in_value(monkeypatch, wide, first):
    """two patches of 20000 appended rows: all below the others, then all above — or the other way round. Both runs of the pi merge are longer than
    2 * MP_WINDOW and the merge-path cut lies at one end of every interval: behind the guessed window of merge_path_wave2 one way, in front of it the other."""
    f = FS if wide else FA
    rng = np.random.default_rng(7000 + (first == "above"))
    k = 20_000
    with _engine(monkeypatch, R_C + 2 * k) as e:
        m = _view_c(e, f, wide, rng)
        i = np.arange(k, dtype=np.int64)
        vals = {"below": -1 - i % 50, "above": 8000 + i % 50}
        for n_done, where in enumerate([first, "above" if first == "below" else "below"]):
            m.write(m.new_ids(k), _enc(vals[where], wide))
            st = _pending(m, _ranges(m, rng, 1)[:4])
            assert st["patches"] == n_done + 1 and st["pending_keys"] == (n_done + 1) * k and m.last_run == (0, k), st


@pytest.mark.parametrize("wide", [False, True])
def test_truncated_answers_while_a_patch_is_pending(monkeypatch, wide):
    """k_ordered_copy_p with cap below, at and above the number of matches: the first cap elements of the full answer; the count stays the full count"""
    f = FS if wide else FA
    rng = np.random.default_rng(8000)
    with _engine(monkeypatch, R_C + 300) as e:
        m = _view_c(e, f, wide, rng)
        rows = rng.permutation(R_C)
        m.write(m.col[rows[:3000]], _enc(4 * rng.integers(0, 2000, 3000) + 1, wide))
        m.write(m.col[rows[3000:3100]], TOMB, put=True)
        m.write(m.new_ids(300), _enc(4 * rng.integers(-5, 2005, 300) + 2, wide))
        _pending(m)
        for lo, hi in [(LO, HI), (int(_enc(4 * 700, wide)), int(_enc(4 * 703 + 2, wide))), (int(_enc(-20, wide)), int(_enc(2, wide)))]:
            want = m.listing(lo, hi)
            count = len(want)
            assert count > 2 and e.scan_count(f, lo, hi) == count
            for cap in (1, count - 1, count, count + 1):
                _same(e.scan_range_pos(f, lo, hi, cap=cap).astype(np.int64), want[:cap], ("positions", lo, hi, cap))
                _same(e.scan_range(f, lo, hi, cap=cap), m.col[want[:cap]], ("ids", lo, hi, cap))
                assert e.scan_count(f, lo, hi) == count
        st = m.stats()
        assert st["sorts"] == 1 and st["rewrites"] == 0 and st["pending_keys"] == 2 * 3100 + 300, st


@pytest.mark.parametrize("wide", [False, True])
def test_a_patch_past_65536_pending_keys_makes_main_be_rewritten(monkeypatch, wide):
    """a small patch stays pending; a larger one takes the pending total past the threshold: the query that brought it about is answered from main + patch, main is
    rewritten behind its answer, and the rewritten view is one (value, position) run again"""
    f = FS if wide else FA
    rng = np.random.default_rng(9000)
    with _engine(monkeypatch, R_C) as e:
        m = _view_c(e, f, wide, rng)
        rows = rng.permutation(R_C)
        m.write(m.col[rows[:2000]], _enc(4 * rng.integers(0, 2000, 2000) + 1, wide))
        st = _pending(m, _ranges(m, rng, 1)[3:])
        assert st["pending_keys"] == 4000, st
        big = rows[1000:1000 + 32_000]                                   # (1000 of them are pending inserts already)
        m.write(m.col[big], _enc(4 * rng.integers(0, 2000, len(big)) + 2, wide))
        m.refresh()
        st = m.stats()
        assert st["patches"] == 2 and st["rewrites"] == 0 and st["pending_keys"] == int(m.pd.sum()) + int(m.pi.sum()) == 2 * 33_000, st
        fresh = m.sorted_live()
        _same(e.scan_range_pos(f, LO, HI).astype(np.int64), m.listing(), "the answer in front of the rewrite")
        e.sync()
        assert e.scan_count(f, LO, HI) == len(fresh)
        assert m.stats()["rewrites"] >= 1, m.stats()
        for _ in range(8):
            if m.stats()["pending_keys"] == 0:
                break
            assert e.scan_count(f, LO, HI) == len(fresh)
        else:
            pytest.fail("the pending patch was not folded into main within 8 queries: %r" % (m.stats(),))
        st = _check(m, _ranges(m, rng, 2))
        assert st["sorts"] == 1 and st["rewrites"] == 1 and st["pending_keys"] == 0 and st["patches"] == 2, st
