"""GPU: the ordered top-k select's own kernels (csrc/top_kernels.h: k_top_sweep0, k_top_init, k_top_digit, k_top_find, k_top_compact, k_top_finish; the chain
of csrc/bmx_top.inc) at their digit, bin and candidate edges — small, structured columns with SEQUENTIAL and CLUSTERED node ids instead of hashed ones, which
never get past the first id digit.

Every check is exact equality of the records, n_out and n_eligible with top_select_model.want (lexsort over (id, +-val) of the rows the test itself loaded).
Which path of the select a layout reaches — how many value and id digit rounds, the short last digit of either word, the switch from value to id digits, "done"
on a whole word, the bin of k_top_find the rank falls into, the candidate limits — is computed by top_select_model.select from the rows alone and asserted
BEFORE each query, never read off the answer.

A layout is loaded once per engine in every form it runs in: on the int32 column where its values allow and on the int64 column (one wide value outside term
0's range switches the index), alone and with a second term that rejects a quarter as many decoy rows as the layout has (every 5th row term 0 selects: the
mask bits decide), and mirrored (-v): the descending order over -v has the same key word (key - kmin) as the ascending one over v, so a layout's claims hold
in both directions. The two crossed directions are queried as well, without claims."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from oracle import streams
import top_select_model as model
from top_select_model import (ONE_VALUE, SWITCH, SHORT_V, FULL_V, SHORT_I, DONE_V, DONE_I, BIN_0, BIN_TOP, FIND_LAST, FIND_FIRST, ROW_FIRST, ROW_LAST,
                              ROW_LAST_OF_THREAD, ONE_BIN, ELIG_CAND, ELIG_CAND1, DONE_CAND, NOT_DONE_CAND1, ALL, SELECT, OUT_OF_PASSES, value_passes, id_passes)

DEVICE = "cuda"
CAND = 4096                        # top_kernels.h TOP_CAND == BMX_TOP_MAX_K
I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)
VMAX = model.VAL_MAX
WIDE, WIDE_ID = 1 << 40, 0x3333333333333333          # the row that makes an index scan its int64 column: outside every layout's term 0
FILL = 0x5A5A5A5A5A5A5A5A          # what a device buffer holds before a query writes into it
FO = streams.fnv1a32("top.other")  # the second term's field: 1 on a layout's rows, 0 or absent on the decoys
MAX_ROWS = 40_000
GEOM = {32: model.GEOM32, 64: model.GEOM64}
SEEN = {}                          # (width, desc) -> every tag a query of this module reached, by the model (test_top_kernel_edges_model.py reads it)


def _field(w, sign, masked):
    return streams.fnv1a32("top.%d%s%s" % (w, "+" if sign > 0 else "-", "m" if masked else ""))


class Layout:
    """rows (vals, ids) that are ALL eligible, and the queries: (k, the tags the model must yield for k)"""

    def __init__(self, name, vals, ids, queries):
        self.name = name
        self.vals = np.asarray(vals, np.int64); self.ids = np.asarray(ids, np.uint64)
        self.queries = [(int(k), set(t)) for k, t in queries]
        n = len(self.vals)
        assert n == len(self.ids) == len(np.unique(self.ids)) and n + n // 4 + 1 <= MAX_ROWS, name
        assert int(self.ids.min()) >= 1 and int(self.ids.max()) <= 2**64 - 2, "EMPTY_ID is reserved"
        assert (np.abs(self.vals) <= VMAX).all()
        self.fits32 = bool((np.abs(self.vals) <= I32_MAX).all())          # v and -v both in INT32_MIN + 1 .. INT32_MAX
        self.widths = (32, 64) if self.fits32 else (64,)
        self.lo, self.hi = int(self.vals.min()), int(self.vals.max())
        # the decoys: the value of every 4th row under an id of their own; term 0 selects them, the second term rejects them
        self.d_vals = self.vals[::4].copy()
        for flip in (1 << 62, 1 << 30, 1 << 40, 1 << 19, 0x5A5A5A5A00):       # the first bit pattern whose flip collides with no id of the layout
            self.d_ids = self.ids[::4] ^ np.uint64(flip)
            both = np.concatenate([self.ids, self.d_ids])
            if len(np.unique(both)) == len(both) and int(self.d_ids.min()) >= 1 and int(self.d_ids.max()) <= 2**64 - 2:
                break
        else:
            raise AssertionError((name, "no ids for the decoys"))
        assert not np.isin(np.uint64(WIDE_ID), both)

    def rows(self):
        """every form's rows for one load_rows: (id, field, val)"""
        I, F, V = [], [], []

        def add(ids, f, vals):
            I.append(np.asarray(ids, np.uint64)); F.append(np.full(len(ids), f, np.uint32)); V.append(np.asarray(vals, np.int64))

        for w in self.widths:
            for sign in (1, -1):
                for masked in (False, True):
                    f = _field(w, sign, masked)
                    add(self.ids, f, sign * self.vals)
                    if masked:
                        add(self.d_ids, f, sign * self.d_vals)
                    if w == 64 and self.fits32:
                        add([WIDE_ID], f, [sign * WIDE])
        add(self.ids, FO, np.ones(len(self.ids)))
        add(self.d_ids[::2], FO, np.zeros(len(self.d_ids[::2])))                 # (the other half of the decoys does not have the field at all)
        add([WIDE_ID], FO, [1])
        return np.concatenate(I), np.concatenate(F), np.concatenate(V)


def _same_recs(recs, ne, W, k, what):
    wi, wv, wne = W
    wi, wv = wi[:k], wv[:k]
    assert ne == wne, (what, "n_eligible", ne, wne)
    assert len(recs) == min(k, wne) == len(wi), (what, "n_out", len(recs), min(k, wne))
    bad = np.flatnonzero((recs["id"] != wi) | (recs["val"] != wv))
    assert len(bad) == 0, (what, len(bad), bad[:4], recs[bad[:4]], wi[bad[:4]], wv[bad[:4]])


class Loaded:
    """a layout in an engine; query() asserts the model's tags, then compares one answer"""

    def __init__(self, e, L):
        self.e, self.L = e, L
        ids, f, v = L.rows()
        e.load_rows(ids, f, np.full(len(ids), 5, np.int64), v)
        self._want, self._sel = {}, {}

    def forms(self):
        return [(w, sign, masked) for w in self.L.widths for sign in (1, -1) for masked in (False, True)]

    def terms(self, w, sign, masked):
        lo, hi = (self.L.lo, self.L.hi) if sign > 0 else (-self.L.hi, -self.L.lo)
        return [(_field(w, sign, masked), lo, hi)] + ([(FO, 1, 1)] if masked else [])

    def want(self, sign, desc, after=None):
        key = (sign, desc, after)
        if key not in self._want:
            self._want[key] = model.want(sign * self.L.vals, self.L.ids, CAND, desc, after)
        return self._want[key]

    def select(self, w, sign, k, desc, after=None):
        key = (w, sign, k, desc, after)
        if key not in self._sel:
            v = sign * self.L.vals
            el = model.eligible(v, self.L.ids, desc, after)
            self._sel[key] = model.select(v[el], self.L.ids[el], k, desc, GEOM[w])
        return self._sel[key]

    def query(self, w, sign, masked, k, desc, after=None, claims=()):
        what = (self.L.name, w, sign, masked, k, desc, after)
        S = self.select(w, sign, k, desc, after)
        assert OUT_OF_PASSES not in S.tags, what
        missing = set(claims) - S.tags
        assert not missing, (what, "the layout was meant to reach", sorted(missing), "and reaches", sorted(S.tags))
        SEEN.setdefault((w, bool(desc)), set()).update(S.tags)
        recs, ne = self.e.scan_top(self.terms(w, sign, masked), k, desc=desc, after=after)
        _same_recs(recs, ne, self.want(sign, desc, after), k, what)
        return recs

    def run(self):
        for w, sign, masked in self.forms():
            natural = sign < 0
            for k, tags in self.L.queries:
                self.query(w, sign, masked, k, natural, claims=tags)
                self.query(w, sign, masked, k, not natural)


def _engine(L):
    n = len(L.vals)
    return bmx.Engine(max(1 << 14, 4 * (4 * len(L.widths) * (n + n // 4 + 1) + 2 * n)))


# ---- the layouts ----

SEQ = lambda n: np.arange(1, n + 1, dtype=np.uint64)
PREFIX = 0xA5C396E17B2D48F0          # upper bits of the clustered ids: no digit of it is 0 or 2047
KS_A = (1, 511, 512, 4095, 4096)


def _shared(bits):
    """5000 ids that share their upper `bits` bits, differ in the 11 bits below (2 or 3 ids per digit) and in the lowest two bits"""
    j = np.arange(1, 5001, dtype=np.uint64)
    low = 64 - bits - 11
    top = np.uint64((PREFIX >> (64 - bits)) << (64 - bits)) if bits else np.uint64(0)
    return top | ((j % np.uint64(2048)) << np.uint64(low)) | (j // np.uint64(2048))


def _shared55():
    """3900 ids below a cluster of 512 that share their upper 55 bits, 700 above: rank 4096 lies in the cluster, whose bin holds 3900 + 512 rows until the last digit"""
    j = np.arange(1, 3901, dtype=np.uint64)
    return np.concatenate([j << np.uint64(50), np.uint64((PREFIX >> 9) << 9) | np.arange(512, dtype=np.uint64), np.uint64(0xF << 60) | (np.arange(700, dtype=np.uint64) << np.uint64(20))])


def _layouts_a():
    """id digits under one value"""
    one = lambda ids: np.full(len(ids), 7, np.int64)
    deep = {ONE_VALUE, value_passes(0), id_passes(6), SHORT_I, DONE_I}
    out = []

    def add(name, ids, claims):
        out.append(Layout("a: " + name, one(ids), ids, [(k, {ONE_VALUE} | claims.get(k, set())) for k in KS_A]))

    add("ids 1..5000", SEQ(5000), {4096: deep, 4095: {id_passes(5), FIND_LAST}, 1: {id_passes(5), BIN_0, ONE_BIN}})
    add("ids 2^63 - 2500 .. 2^63 + 2499", np.arange(2**63 - 2500, 2**63 + 2500, dtype=np.uint64), {511: {id_passes(1)}, 512: {id_passes(1)}, 4095: deep, 4096: deep})
    add("ids 2^64 - 2 - i", np.uint64(2**64 - 2) - np.arange(5000, dtype=np.uint64), {1: {BIN_TOP, ONE_BIN}, 4096: deep | {BIN_TOP}})
    for bits in (0, 11, 22, 33, 44):
        add("ids that share their upper %d bits" % bits, _shared(bits), {k: {id_passes(bits // 11 + 1)} for k in (1, 511, 512)})
    add("ids that share their upper 55 bits", _shared55(), {4096: deep | {ONE_BIN}})
    return out


def _span(bits, lo, seed):
    """values over a span of `bits` bits from lo: the smallest, the largest, 1000 anywhere, and a cluster of 5000 rows that differ in the LAST digit only — the
    bin of a rank inside the cluster keeps more than 4096 rows until then. -> (vals, rows below the cluster)"""
    rng = np.random.default_rng(seed)
    d = (1 << bits) - (2 if bits in (32, 54) else 1)                    # INT32_MIN + 1 .. INT32_MAX and -VAL_MAX .. VAL_MAX are two short of a power of two
    wl = bits - 11 * ((bits - 1) // 11)                                 # the last digit's width
    c0 = (((0x16B5A93C71E4D2 >> (54 - bits)) >> wl) << wl) if bits > wl else 0
    assert d.bit_length() == bits and c0 + (1 << wl) - 1 <= d
    cluster = c0 + np.arange(5000, dtype=np.int64) % (1 << wl)
    fill = rng.integers(0, d + 1, 1000, dtype=np.int64)
    off = np.concatenate([cluster, fill, [0, d]])
    return lo + off, int((off < c0).sum())


def _layouts_b():
    """value digits"""
    out = []
    for bits, lo in ((1, -1), (11, -1000), (22, -(1 << 21) - 3), (31, 0), (32, I32_MIN + 1), (33, -(1 << 31)), (44, -(1 << 40)), (54, -VMAX)):
        vals, nb = _span(bits, lo, bits)
        p = (bits + 10) // 11
        last = SHORT_V if bits % 11 else FULL_V
        if bits == 1:         # two values: the rank's bin holds half the rows
            q = [(1, {value_passes(1), SHORT_V, DONE_V, BIN_0}), (4096, {value_passes(1), SHORT_V, SWITCH})]
        else:
            inside = {value_passes(p), last, DONE_V, id_passes(0)}
            q = [(1, set()), (nb + 1, inside), (nb + 2500, inside), (4096, {value_passes(p), last})]      # (rank 4096 may sit in a bin that crosses the capacity)
        out.append(Layout("b: a span of %d bits" % bits, vals, SEQ(len(vals)), q))
    far = I32_MAX
    # (the digits run over key - kmin: 1..8192 is 0..8191 to the select — two value passes, done with exactly 4096. The row 0 in front of 2..8192 is what
    # moves rank 4096 into the next bin: three value passes, done on the whole value word, no id phase)
    out.append(Layout("b: 1..8192 and one value far out", np.concatenate([np.arange(1, 8193), [far]]), SEQ(8193),
                      [(4096, {value_passes(2), DONE_CAND, id_passes(0)}), (1, set()), (4095, set())]))
    out.append(Layout("b: 0, 2..8192 and one value far out", np.concatenate([[0], np.arange(2, 8193), [far]]), SEQ(8193),
                      [(4096, {value_passes(3), SHORT_V, DONE_V, id_passes(0), FIND_FIRST}), (1, set()), (4095, set())]))
    out.append(Layout("b: 0..8191 and one value far out", np.concatenate([np.arange(8192), [far]]), SEQ(8193),
                      [(4096, {value_passes(2), DONE_CAND, FIND_LAST, ROW_LAST, ROW_LAST_OF_THREAD}), (1, set()), (4095, set())]))
    out.append(Layout("b: 0..8191, one of them twice, and one value far out", np.concatenate([np.arange(8192), [5, far]]), SEQ(8194),
                      [(4096, {NOT_DONE_CAND1, value_passes(3)}), (4095, set())]))
    v = np.concatenate([np.arange(9000) % 3, [far]])
    deep = {value_passes(3), SHORT_V, SWITCH}
    out.append(Layout("b: ties under a deep value", v, SEQ(9001), [(1, {value_passes(3), DONE_V}), (3000, {value_passes(3), DONE_V}), (3001, deep | {id_passes(5)}), (4096, deep | {id_passes(6), SHORT_I, DONE_I})]))
    return out


def _layouts_c():
    """k_top_find's bins: one full digit, three rows per bin — the first and the last row of bin 0, of bin 7 and of bin 8 (two threads of k_top_find) — and a
    rank in bin 2047"""
    rng = np.random.default_rng(3)
    one = {value_passes(1), FULL_V, DONE_V, id_passes(0)}
    v = np.repeat(np.arange(2048), 3) - 1000
    q = [(1, {BIN_0, ROW_FIRST}), (3, {BIN_0, ROW_LAST}), (22, {FIND_LAST, ROW_FIRST}), (24, {FIND_LAST, ROW_LAST, ROW_LAST_OF_THREAD}), (25, {FIND_FIRST, ROW_FIRST}),
         (27, {FIND_FIRST, ROW_LAST})]
    # (rank 4096 is the first of its bin's three rows: 4095 below + 3 cross the capacity, and the ids of one value settle it)
    out = [Layout("c: 2048 values x 3 rows", v, rng.permutation(6144).astype(np.uint64) + np.uint64(1),
                  [(k, one | t) for k, t in q] + [(4096, {value_passes(1), FULL_V, SWITCH, ROW_FIRST}), (4095, one | {ROW_LAST})])]
    mid = np.sort(rng.choice(np.arange(1, 2047), 500, replace=False))
    v = np.concatenate([np.zeros(3000, np.int64), mid, np.full(3000, 2047)])
    out.append(Layout("c: a rank in bin 2047", v, rng.permutation(6500).astype(np.uint64) + np.uint64(1),
                      [(1, {BIN_0, value_passes(1), DONE_V}), (3500, {ROW_LAST, DONE_V}), (3501, {BIN_TOP, ROW_FIRST, SWITCH, FULL_V}), (4096, {BIN_TOP, SWITCH})]))
    return out


def _layouts_d():
    """the candidate list's capacity"""
    rng = np.random.default_rng(4)
    out = []
    for n, tag, kind in ((4096, ELIG_CAND, ALL), (4097, ELIG_CAND1, SELECT)):
        out.append(Layout("d: exactly %d eligible rows" % n, rng.integers(-300, 300, n), SEQ(n), [(k, {tag, kind}) for k in (1, 4095, 4096)]))
    return out


LAYOUTS = {L.name: L for L in _layouts_a() + _layouts_b() + _layouts_c() + _layouts_d()}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_in_every_form(name):
    """a to d: every layout ascending and descending, on the int32 column where its values allow and on the int64 column, in the single-term and the mask form"""
    L = LAYOUTS[name]
    with _engine(L) as e:
        Loaded(e, L).run()


# ---- e. cursors inside deep groups ----

def _walk(X, w, sign, masked, k, desc):
    """every page behind the last record of the one before: every id once, in order"""
    wi, wv, total = model.want(sign * X.L.vals, X.L.ids, 10**9, desc)
    pages, cur, left = [], None, total
    while left:
        recs = X.query(w, sign, masked, k, desc, after=cur)
        assert len(recs) == min(k, left)
        pages.append(recs); left -= len(recs); cur = (int(recs[-1]["id"]), int(recs[-1]["val"]))
    recs = X.query(w, sign, masked, k, desc, after=cur)
    assert len(recs) == 0
    got = np.concatenate(pages)
    assert len(got) == total and (got["id"] == wi).all() and (got["val"] == wv).all() and len(np.unique(got["id"])) == total


def _every_form(X, k, after_of, claims):
    """one cursor query per form; after_of(sign) -> (id, val); the claims hold in the layout's own direction"""
    for w, sign, masked in X.forms():
        for desc in (sign < 0, sign > 0):
            X.query(w, sign, masked, k, desc, after=after_of(sign), claims=claims if desc == (sign < 0) else ())


def test_cursor_inside_one_value():
    """ids 1..7500 under one value, the cursor on id 2500: 5000 rows remain, all of them told apart by id digits alone"""
    L = Layout("e: one value, ids 1..7500", np.full(7500, 7), SEQ(7500), [])
    with _engine(L) as e:
        X = Loaded(e, L)
        for k, claims in ((1, {ONE_VALUE, id_passes(5)}), (4096, {ONE_VALUE, id_passes(6), DONE_I})):
            _every_form(X, k, lambda sign: (2500, 7 * sign), claims)


def test_cursor_on_the_last_id_below_2_63():
    """8000 ids around 2^63 under one value, the cursor on 2^63 - 1: what remains starts at 2^63 — the ids compare unsigned"""
    L = Layout("e: ids around 2^63", np.full(8000, -3), np.arange(2**63 - 2500, 2**63 + 5500, dtype=np.uint64), [])
    with _engine(L) as e:
        X = Loaded(e, L)
        # behind 2^63 - 1 rank 4096 is id 2^63 + 4095, the last of its bin of the fifth digit: exactly 4096 at or below. One id more in front (the cursor on
        # 2^63 - 2) makes that 4097, and the sixth, short digit decides
        for k, claims, one_more in ((1, {ONE_VALUE, SELECT}, {ONE_VALUE}), (4096, {ONE_VALUE, id_passes(5), DONE_CAND}, {ONE_VALUE, NOT_DONE_CAND1, id_passes(6), SHORT_I, DONE_I})):
            _every_form(X, k, lambda sign: (2**63 - 1, -3 * sign), claims)
            _every_form(X, k, lambda sign: (2**63 - 2, -3 * sign), one_more)


def test_cursor_whose_value_is_the_smallest_that_remains():
    """the tie layout, the cursor in the middle of the group of value 1: kmin is the cursor's value, its group is cut by id"""
    L = LAYOUTS["b: ties under a deep value"]
    with _engine(L) as e:
        X = Loaded(e, L)
        assert L.vals[4501] == 1 and L.ids[4501] == 4502
        for k, claims in ((1, {SELECT}), (1499, {SELECT, DONE_V}), (1500, {SELECT, SWITCH}), (4096, {SELECT, SWITCH})):
            _every_form(X, k, lambda sign: (4502, sign), claims)       # id 4502 holds value 1: 1499 of its group remain, then 3000 of value 2 and the far one


@pytest.mark.parametrize("name", ["a: ids 1..5000", "b: ties under a deep value"])
def test_page_walk(name):
    L = LAYOUTS[name]
    with _engine(L) as e:
        X = Loaded(e, L)
        for w in L.widths:
            for sign, masked in ((1, False), (-1, True)):
                for desc in (False, True):
                    _walk(X, w, sign, masked, 333, desc)


# ---- f. by position: what one ballot of k_top_digit and k_top_compact sees ----

SHARE32 = 32768                     # bmx_top.inc top_launch: a workgroup's share, four rounds of 512 lanes x 4 loads x 16 bytes = 32768 int32 rows (16384 int64 rows)
LANE0, LANE63, SAME_BIN, ALL_DIFFERENT = "a ballot of lane 0 alone", "a ballot of lane 63 alone", "a full ballot in one bin", "a full ballot in 64 bins"
RAGGED_ONLY, TWO_FLUSHES = "eligible rows in the ragged last unit only", "more than 4096 eligible rows in two workgroups"


def _ballots(ok, digit, E, n):
    """tags of the ballots the first digit round takes: lane l's e-th element of a 16-byte unit sits at position unit * E + e, consecutive units on consecutive
    lanes. digit: per position, None when no round runs"""
    tags = set()
    share = SHARE32 * E // 4
    first = int(np.flatnonzero(ok)[0]) if ok.any() else n
    if first >= (n - 1) // E * E and n > share and n % E:
        tags.add(RAGGED_ONLY)
    if digit is None:
        return tags
    if ok.sum() > CAND and len(np.unique(np.flatnonzero(ok) // share)) >= 2:
        tags.add(TWO_FLUSHES)
    waves = -(-n // (64 * E))
    o = np.zeros(waves * 64 * E, bool); o[:n] = ok; o = o.reshape(waves, 64, E)
    g = np.zeros(waves * 64 * E, np.int64); g[:n] = digit; g = g.reshape(waves, 64, E)
    for e in range(E):
        oe, ge = o[:, :, e], g[:, :, e]
        cnt = oe.sum(1)
        if ((cnt == 1) & oe[:, 0]).any(): tags.add(LANE0)
        if ((cnt == 1) & oe[:, 63]).any(): tags.add(LANE63)
        full = cnt == 64
        if (full & (ge.max(1) == ge.min(1))).any(): tags.add(SAME_BIN)
        if (full & (np.diff(np.sort(ge, 1), axis=1) != 0).all(1)).any(): tags.add(ALL_DIFFERENT)
    return tags


class Column:
    """one indexed field laid out BY POSITION (index_ids says which node sits where), as tests/test_gpu_scan_kernel_edges.py does it; node ids 1..n"""

    def __init__(self, e, f, n):
        self.e, self.f, self.n = e, f, n
        ids = SEQ(n)
        e.load_rows(ids, np.full(n, f, np.uint32), np.full(n, 5, np.int64), np.zeros(n, np.int64))
        e.index_build(f)
        self.col = e.index_ids(f)
        assert len(self.col) == n and np.array_equal(np.sort(self.col), ids)
        self.clock = 10

    def _merge(self, f, vals):
        self.clock += 10
        won = self.e.merge_batch(self.col, np.full(self.n, f, np.uint32), np.full(self.n, self.clock, np.int64), np.asarray(vals, np.int64))[0]
        assert len(won) == self.n, "every delta of the test wins"
        assert np.array_equal(self.e.index_ids(self.f), self.col), "the test's premise: no position of the index is renumbered"

    def set(self, vals):
        self._merge(self.f, vals)

    def set_other(self, ok):
        self._merge(FO, np.where(ok, 1, 0))


def _position_layouts(n, E):
    """(name, eligible by position, value by position (in 0 .. 2^22 - 1), ballot tags the first round must show)"""
    p = np.arange(n)
    unit = p // E; lane = unit % 64; wave = unit // 64
    spread = p % 2048
    out = []
    if n == 33000:
        ok = p != 5
        v = spread.copy(); v[9] = (1 << 22) - 1
        out.append(("one bin, then 64 bins", ok, v, {SAME_BIN}))                       # the far value leaves every other row in one bin of the first round
        out.append(("64 bins", ok, spread, {ALL_DIFFERENT}))
        kind = wave % 4
        ok = ((kind == 0) & (lane == 0)) | ((kind == 1) & (lane == 63)) | (kind == 2)
        out.append(("lane 0 alone, lane 63 alone, every lane, none", ok, spread, {LANE0, LANE63, ALL_DIFFERENT}))
    elif n in (SHARE32 + 1, SHARE32 + 3):
        out.append(("the ragged last unit only", p >= (n - 1) // E * E, spread, {RAGGED_ONLY}))
    else:
        out.append(("two workgroups", (p >= 30500) & (p != 31000), spread, {TWO_FLUSHES, ALL_DIFFERENT}))
    return out


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [33000, SHARE32 + 1, SHARE32 + 3, 36000])
def test_by_position(wide, n):
    """the eligible rows chosen by position, first by term 0's range (the other positions hold -7 or 2^23), then by the second term alone (every position holds
    a value in range; the mask bits are the layout). wide: position 5, eligible in no layout, holds 2^40."""
    E = 2 if wide else 4
    w = 64 if wide else 32
    f = _field(w, 1, False)
    hi = (1 << 22) - 1
    assert n + 1 <= MAX_ROWS
    with bmx.Engine(8 * n) as e:
        c = Column(e, f, n)
        for name, ok, v, tags in _position_layouts(n, E):
            assert not ok[5]
            nodes, vals = c.col[ok], v[ok]
            for masked in (False, True):
                out = np.where(np.arange(n) % 2 == 0, -7, 1 << 23)
                col = v.copy() if masked else np.where(ok, v, out)
                if wide:
                    col[5] = WIDE
                c.set(col)
                if masked:
                    c.set_other(ok)
                terms = [(f, 0, hi)] + ([(FO, 1, 1)] if masked else [])
                for desc in (False, True):
                    S = model.select(vals, nodes, CAND, desc, GEOM[w])
                    digit = None
                    if S.first_digit is not None:
                        digit = np.zeros(n, np.int64); digit[ok] = S.first_digit
                    seen = _ballots(ok, digit, E, n)
                    assert tags <= seen, (name, n, wide, "the layout was meant to show", sorted(tags - seen))
                    W = model.want(vals, nodes, CAND, desc)
                    for k in (1, 777, CAND):
                        S = model.select(vals, nodes, k, desc, GEOM[w])
                        assert OUT_OF_PASSES not in S.tags
                        SEEN.setdefault((w, desc), set()).update(S.tags)
                        recs, ne = e.scan_top(terms, k, desc=desc)
                        _same_recs(recs, ne, W, k, (name, n, wide, masked, desc, k))


# ---- g. a clean state between queries of every depth ----

def test_clean_state_between_deep_shallow_all_and_empty_queries():
    """a six-id-pass query, a one-pass query, an `all` query and an empty one in turn: on the host path, then back to back in device mode with no synchronisation
    in between. Every answer is right, the deep query's second answer is its first, and nothing is written behind the last record."""
    import torch
    deep, shallow = LAYOUTS["a: ids 1..5000"], LAYOUTS["c: 2048 values x 3 rows"]
    fd, fs = streams.fnv1a32("top.deep"), streams.fnv1a32("top.shallow")
    with bmx.Engine(1 << 16) as e:
        for L, f in ((deep, fd), (shallow, fs)):
            e.load_rows(L.ids, np.full(len(L.ids), f, np.uint32), np.full(len(L.ids), 5, np.int64), L.vals)
        # (terms, k, rows, claims)
        few = shallow.vals <= -990
        cases = [([(fd, 7, 7)], CAND, deep, None, {id_passes(6), DONE_I}), ([(fs, -1000, 1047)], 100, shallow, None, {value_passes(1), id_passes(0)}),
                 ([(fs, -1000, -990)], 50, shallow, few, {ALL}), ([(fs, 5, 4)], 10, shallow, np.zeros(len(shallow.vals), bool), {model.EMPTY})]
        runs = []
        for terms, k, L, keep, claims in cases:
            keep = np.ones(len(L.vals), bool) if keep is None else keep
            for desc in (False, True):
                tags = model.trace(L.vals[keep], L.ids[keep], k, desc, model.GEOM32)
                assert claims <= tags, (terms, k, desc, sorted(tags))
                runs.append((terms, k, desc, model.want(L.vals[keep], L.ids[keep], k, desc)))
        runs = runs + runs
        host = []
        for terms, k, desc, W in runs:
            recs, ne = e.scan_top(terms, k, desc=desc)
            _same_recs(recs, ne, W, k, ("host", terms, k, desc))
            host.append(recs)
        half = len(runs) // 2
        assert all((a == b).all() for a, b in zip(host[:half], host[half:])), "a query's second answer is its first"
        bufs = []
        for terms, k, desc, W in runs:
            bufs.append((torch.full((2 * k + 2,), FILL, dtype=torch.int64, device=DEVICE), torch.full((3,), FILL, dtype=torch.int64, device=DEVICE)))
        if DEVICE == "cuda":
            torch.cuda.synchronize()
        for (terms, k, desc, W), (out, cnt) in zip(runs, bufs):         # every query right behind the one before on the stream
            e.scan_top_dev(terms, k, out, cnt[0:1], cnt[1:2], desc=desc)
        e.sync()
        for (terms, k, desc, W), (out, cnt), h0 in zip(runs, bufs, host):
            h = out.cpu().numpy(); c = cnt.cpu().numpy()
            m = len(W[0])
            assert int(c[0]) == m and int(c[1]) == W[2] and int(c[2]) == FILL, (terms, k, desc, c)
            recs = h[:2 * m].view(bmx.TOP_DTYPE)
            _same_recs(recs, int(c[1]), W, k, ("device", terms, k, desc))
            assert (recs == h0).all(), "host mode and device mode agree"
            assert (h[2 * m:] == FILL).all(), "nothing behind the last record is written"
