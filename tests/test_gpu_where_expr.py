"""GPU: computed measures (include/bmx_expr.h): bmx_where_aggregate_expr, bmx_where_group_expr and bmx_where_quantiles_expr. Every byte of every record, of the
result record and of the bmx_expr_res is compared with the brute force of tests/expr_model.py (Python ints, straight from the header's sentences) over the
rows the test itself loaded; the calls write into buffers that held a pattern, and nothing behind the answer may change. Each form is also checked
differentially: the expression against the plain form on a shadow field that the test loaded with the expression's values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import expr_model as xm
import where_agg_model as wam
import where_clock_model as wcm
from expr_model import ALL, BIG, DATA, F1, F2, F3, F4, FB, I64MAX, I64MIN, OPS, P1, P2, VAL_MAX

NOBODY = wcm.wdm.streams.fnv1a32("expr.nobody")
FS = wcm.wdm.streams.fnv1a32("expr.shadow")
QS = [(0, 1), (1, 4), (1, 2), (95, 100), (1, 1), (1, 2)]


def check(x, m, clauses, e, group=None, window=None, sel=None, forms="agq", cap=65536):
    """every form of the expression e over the selection, against the brute force; -> (n_undef, n_range)"""
    sel = xm.selection(m, FB, clauses) if sel is None else sel
    want = xm.brute_agg(m, FB, clauses, e, sel=sel)
    xres = want[1]
    if "a" in forms:
        got = xm.raw_agg(x, FB, clauses, e)
        assert xm.same(got, want), ("flat", e, got, want)
        assert int(got[0][0]["n_match"]) == int(got[0][0]["n"]) + xres[0] + xres[1]
        if group is not None:
            lo, ng = window or (-2, 6)
            got, want = xm.raw_agg(x, FB, clauses, e, group, lo, ng), xm.brute_agg(m, FB, clauses, e, group, lo, ng, sel=sel)
            assert xm.same(got, want), ("window", e, group, lo, ng, got, want)
            assert int(got[0]["n_match"].sum()) == int(got[0]["n"].sum()) + xres[0] + xres[1]
    if "g" in forms and group is not None:
        got, want = xm.raw_group(x, FB, clauses, e, group, cap), xm.brute_group(m, FB, clauses, e, group, cap, sel=sel)
        assert xm.same(got, want), ("group", e, group, got, want)
        assert got[2] == xres and int(got[1][0]["total"]["n_match"]) == int(got[1][0]["total"]["n"]) + xres[0] + xres[1]
    if "q" in forms:
        got, want = xm.raw_quant(x, FB, clauses, e, QS), xm.brute_quant(m, FB, clauses, e, QS, sel=sel)
        assert xm.same(got, want), ("quantiles", e, got, want)
        assert got[2] == xres and int(got[1][0]["n_match"]) == int(got[1][0]["n"]) + xres[0] + xres[1]
    return xres


# ---- 1. the classes: the 9 state pairs, the values at the edge of the range, the operands' places ----
VALUES = [(0, 0), (0, 1), (1, -1), (-1, -1), (1, 1), (VAL_MAX, 0), (0, VAL_MAX), (VAL_MAX, 1), (1, VAL_MAX), (-VAL_MAX, -1), (-VAL_MAX, 1), (VAL_MAX, -1), (-VAL_MAX, 0),
          (P1, P2), (-P1, P2), (1 << 26, 1 << 27), (-(1 << 26), 1 << 27), (94906265, 94906265), (94906266, 94906267), (VAL_MAX, VAL_MAX), (-VAL_MAX, VAL_MAX),
          (BIG, BIG + 1), (-BIG, BIG + 1), (VAL_MAX, -VAL_MAX), (3, 5)]


def _class_table(wide):
    """nodes 0..8: the 9 combinations of (absent, data, tombstone) for F1 and F2, values 6 and 7; then one node per pair of VALUES; then a node with everything
    but the base field and one whose base field is tombstoned. F3 (the group field): small values, absent on every fourth node, tombstoned on node 5."""
    st = [(a, b) for a in range(3) for b in range(3)]
    n = 9 + len(VALUES) + 2
    m = wcm.ClockModel(wcm.node_ids(n, 4100))
    off = (1 << 40) if wide else 0
    m.set(FB, np.arange(n - 2), np.arange(n - 2) - 4 + off); m.set(FB, [n - 1], [3 + off]); m.tomb(FB, [n - 1])
    for f, col in ((F1, 0), (F2, 1)):
        held = [k for k, s in enumerate(st) if s[col]]
        m.set(f, held, np.full(len(held), 6 + col)); m.tomb(f, [k for k, s in enumerate(st) if s[col] == 2])
        m.set(f, np.arange(9, 9 + len(VALUES)), [v[col] for v in VALUES]); m.set(f, [n - 2, n - 1], [2, 2])
    g = np.array([k for k in range(n) if k % 4 != 3])
    m.set(F3, g, g % 5 - 1); m.tomb(F3, [5])
    return m


@pytest.mark.parametrize("wide", [False, True])
def test_the_three_classes(wide):
    m = _class_table(wide)
    off = (1 << 40) if wide else 0
    with bmx.Engine(4096) as e:
        wcm.put(e, m, (FB, F1, F2, F3))
        sel = xm.selection(m, FB, ALL)
        assert len(sel) == m.N - 2
        for op in OPS:
            xres = check(e, m, ALL, (F1, op, F2), F3, sel=sel)
            assert xres[0] == 8, "eight of the nine state pairs lack an operand"
            check(e, m, ALL, (F2, op, F1), F3, sel=sel)
        # the header's own numbers, node by node: a program that selects one node
        node = {v: 9 + k for k, v in enumerate(VALUES)}

        def one(v, op):
            k = node[v]
            recs, x = xm.raw_agg(e, FB, [[(FB, k - 4 + off, k - 4 + off)]], (F1, op, F2))
            assert int(recs[0]["n_match"]) == 1
            return (int(recs[0]["n"]), x, int(recs[0]["min"]) if int(recs[0]["n"]) else None)
        assert one((P1, P2), "*") == (1, (0, 0), VAL_MAX) and one((-P1, P2), "*") == (1, (0, 0), -VAL_MAX)
        assert one((1 << 26, 1 << 27), "*") == (0, (0, 1), None) and one((-(1 << 26), 1 << 27), "*") == (0, (0, 1), None)
        assert one((94906265, 94906265), "*") == (1, (0, 0), 94906265 ** 2) and one((94906266, 94906267), "*") == (0, (0, 1), None)
        assert one((VAL_MAX, VAL_MAX), "*") == (0, (0, 1), None) and one((-VAL_MAX, VAL_MAX), "*") == (0, (0, 1), None)
        assert one((BIG, BIG + 1), "*") == (0, (0, 1), None), "the product whose low 64 bits are 2^32"
        assert one((-BIG, BIG + 1), "*") == (0, (0, 1), None)
        assert one((VAL_MAX, 0), "+") == (1, (0, 0), VAL_MAX) and one((VAL_MAX, 1), "+") == (0, (0, 1), None) and one((-VAL_MAX, -1), "+") == (0, (0, 1), None)
        assert one((-VAL_MAX, 1), "-") == (0, (0, 1), None) and one((VAL_MAX, -1), "-") == (0, (0, 1), None) and one((VAL_MAX, 1), "-") == (1, (0, 0), VAL_MAX - 1)
        assert one((VAL_MAX, -VAL_MAX), "+") == (1, (0, 0), 0) and one((VAL_MAX, -VAL_MAX), "-") == (0, (0, 1), None)
        assert one((0, VAL_MAX), "*") == (1, (0, 0), 0) and one((1, VAL_MAX), "*") == (1, (0, 0), VAL_MAX) and one((VAL_MAX, -1), "*") == (1, (0, 0), -VAL_MAX)
        assert one((3, 5), "-") == (1, (0, 0), -2) and one((3, 5), "*") == (1, (0, 0), 15)
        # the operands' places: the base field on either side and on both, a == b, a field nobody holds, an operand that is also a field of the program or the
        # group field
        for a, b in ((FB, F1), (F1, FB), (FB, FB), (F1, F1), (F2, F2), (NOBODY, F1), (F1, NOBODY), (NOBODY, NOBODY), (F3, F1), (F1, F3), (F3, F3)):
            for op in OPS:
                check(e, m, ALL, (a, op, b), F3, sel=sel, forms="ag" if op == "-" else "agq")
        for a, b in ((FB, F1), (F1, F2), (F1, F1)):
            check(e, m, ALL, (a, "*", b), FB, window=(off - 2, 9), sel=sel, forms="ag")
        prog = [[(F1, -VAL_MAX, 6), (FB, off, I64MAX)], [(F2, 7, 7, True), ((F1, F2), I64MIN, 0)]]
        for e2 in ((F1, "*", F2), (F2, "-", F1), (FB, "+", F2), (F1, "+", F1)):
            check(e, m, prog, e2, F3)
        if wide:
            assert check(e, m, ALL, (FB, "*", FB), F3, sel=sel) == (0, len(sel)), "every square of a base value beyond 2^40 is out of range"
            assert check(e, m, ALL, (FB, "+", FB), F3, sel=sel) == (0, 0)
        else:
            assert check(e, m, ALL, (FB, "*", FB), F3, sel=sel) == (0, 0)


# ---- 2. groups ----
def test_an_out_of_range_node_in_a_group_of_its_own_and_the_overflow_rule():
    D = 40
    n = 3 * D
    m = wcm.ClockModel(wcm.node_ids(n, 4200))
    m.set(FB, np.arange(n), np.arange(n)); m.set(F1, np.arange(n), np.arange(n) % 7 + 1); m.set(F2, np.arange(n), np.full(n, 3))
    m.set(F3, np.arange(n), np.arange(n) % D)
    lonely = [D - 1, 2 * D - 1, 3 * D - 1]                               # group D - 1: its three nodes out of range, undefined, out of range
    m.set(F1, lonely, [VAL_MAX, 5, 1 << 52]); m.tomb(F2, [2 * D - 1])
    e = (F1, "*", F2)
    with bmx.Engine(4096) as x:
        wcm.put(x, m, (FB, F1, F2, F3))
        assert check(x, m, ALL, e, F3, window=(0, D)) == (1, 2)
        recs, res, xr = xm.raw_group(x, FB, ALL, e, F3)
        g = recs[recs["key"] == D - 1][0]["agg"]
        assert (int(g["n_match"]), int(g["n"]), int(g["min"]), int(g["max"]), int(g["sum_lo"]), int(g["sum_hi"])) == (3, 0, I64MAX, I64MIN, 0, 0)
        w = xm.raw_agg(x, FB, ALL, e, F3, 0, D)[0][D - 1]
        assert w.tobytes() == g.tobytes()
        # one record too few: the overflow flag, no record, `absent`, `total` and the counters exact; the exact query right behind it
        got, want = xm.raw_group(x, FB, ALL, e, F3, D - 1), xm.brute_group(m, FB, ALL, e, F3, D - 1)
        assert want[0] is None and xm.same(got, want), (got, want)
        got, want = xm.raw_group(x, FB, ALL, e, F3, D), xm.brute_group(m, FB, ALL, e, F3, D)
        assert len(want[0]) == D and xm.same(got, want)
        assert xm.same(xm.raw_quant(x, FB, ALL, e, QS), xm.brute_quant(m, FB, ALL, e, QS))


# ---- 3. quantiles ----
def test_quantiles_of_small_samples_and_of_ties():
    T = 10_000
    pairs = [(a, 3600 // a) for a in range(1, 3601) if 3600 % a == 0] + [(-a, -(3600 // a)) for a in (2, 3, 40, 900)]      # 3600 = a * b in 49 ways
    n = T + 700
    rng = np.random.default_rng(43)
    m = wcm.ClockModel(wcm.node_ids(n, 4300))
    m.set(FB, np.arange(n), rng.integers(0, 50, n))
    k = np.arange(T) % len(pairs)
    m.set(F1, np.arange(T), np.array([p[0] for p in pairs])[k]); m.set(F2, np.arange(T), np.array([p[1] for p in pairs])[k])
    rest = np.arange(T, n)
    m.set(F1, rest, rng.integers(-30, 31, len(rest))); m.set(F2, rest, rng.integers(-30, 31, len(rest)))      # (products below 3600)
    m.set(F3, np.arange(5), [9, 9, 9, 9, 9])                              # the small samples: F3 selects 0, 1, 2 defined nodes
    m.set(F4, [0, 1, 2], [1, 2, 3]); m.tomb(F4, [0]); m.set(F4, [3], [VAL_MAX])
    with bmx.Engine(16 * n) as x:
        wcm.put(x, m, (FB, F1, F2, F3, F4))
        e = (F1, "*", F2)
        recs, res, xr = xm.raw_quant(x, FB, ALL, e, QS)
        assert xm.same((recs, res, xr), xm.brute_quant(m, FB, ALL, e, QS))
        assert int(recs[2]["value"]) == 3600 and int(recs[2]["n_equal"]) == T, "the ties hold the median"
        small = (F4, "*", F4)
        for prog, n_want in (([[(F3, 9, 9), (F4, 0, 0)]], 0), ([[(F3, 9, 9), (FB, I64MIN, I64MAX), (F4, 2, 2)]], 1), ([[(F3, 9, 9)]], 2)):
            got, want = xm.raw_quant(x, FB, prog, small, QS), xm.brute_quant(m, FB, prog, small, QS)
            assert xm.same(got, want) and int(got[1][0]["n"]) == n_want, (prog, got, want)
        got = xm.raw_quant(x, FB, [[(F3, 9, 9)]], small, QS)
        assert got[2] == (2, 1) and int(got[1][0]["n_match"]) == 5 and (int(got[1][0]["min"]), int(got[1][0]["max"])) == (4, 9)
        empty = xm.raw_quant(x, FB, [[(F3, 9, 9), (F4, VAL_MAX, VAL_MAX)]], small, QS)
        assert (empty[0].view(np.uint8) == 0).all() and empty[2] == (0, 1) and (int(empty[1][0]["min"]), int(empty[1][0]["max"])) == (I64MAX, I64MIN)


# ---- 4. seeded programs ----
N_SEEDED = 900


@pytest.fixture(scope="module", params=[False, True], ids=["int32", "int64"])
def seeded(request):
    wide = request.param
    m = xm.seeded_table(N_SEEDED, wide=wide)
    e = bmx.Engine(32 * N_SEEDED)
    wcm.put(e, m, [FB] + xm.PROBED)
    yield e, m, wide
    e.close()


def test_seeded_programs(seeded):
    e, m, wide = seeded
    progs = xm.seeded_programs(60, wide=wide)
    assert len(progs) == 60
    fields = [F1, F2, F3, F4, FB]
    for k, (clauses, (a, b)) in enumerate(progs):
        sel = xm.selection(m, FB, clauses)
        for j, op in enumerate(xm.ops_of(a, b)):
            xres = check(e, m, clauses, (a, op, b), fields[(k + j) % 5], sel=sel, forms=("ag", "aq", "agq")[(k + j) % 3])
            assert xres[0] >= 1 and xres[1] >= 1, (k, op)


def test_device_mode_into_poisoned_buffers(seeded):
    e, m, wide = seeded
    dev = torch.device("cuda", 0)
    P = 0x5A5A5A5A5A5A5A5A
    for k, (clauses, (a, b)) in enumerate(xm.seeded_programs(6, seed=77, wide=wide)):
        ex = (a, "*", b)
        sel = xm.selection(m, FB, clauses)
        x = xm.E(ex)
        # the aggregate, windowed: 7 records of 6 words, then the pattern
        d_out = torch.full((7 * 6 + 3,), P, dtype=torch.int64, device=dev); d_x = torch.full((4,), P, dtype=torch.int64, device=dev)
        e.where_aggregate_expr_dev(FB, clauses, x, d_out, d_x, group=F3, group_lo=-2, ngroups=6)
        # the group-by and the quantiles right behind it, no sync in between
        d_g = torch.full((7 * 64 + 3,), P, dtype=torch.int64, device=dev); d_gr = torch.full((14 + 2,), P, dtype=torch.int64, device=dev); d_gx = torch.full((4,), P, dtype=torch.int64, device=dev)
        e.where_group_expr_dev(FB, clauses, F3, x, d_g, d_gr, d_gx, cap=64)
        d_q = torch.full((4 * len(QS) + 3,), P, dtype=torch.int64, device=dev); d_qr = torch.full((4 + 2,), P, dtype=torch.int64, device=dev); d_qx = torch.full((4,), P, dtype=torch.int64, device=dev)
        e.where_quantiles_expr_dev(FB, clauses, x, QS, d_q, d_qr, d_qx)
        e.where_quantiles_expr_dev(FB, clauses, x, QS, d_q, None, None)                     # (res and xres may be NULL)
        e.sync()
        want = xm.brute_agg(m, FB, clauses, ex, F3, -2, 6, sel=sel)
        h = d_out.cpu().numpy()
        assert h[:42].tobytes() == want[0].tobytes() and (h[42:] == P).all()
        for d in (d_x, d_gx, d_qx):
            hx = d.cpu().numpy()
            assert (int(hx[0]), int(hx[1])) == want[1] and (hx[2:] == P).all()
        wg = xm.brute_group(m, FB, clauses, ex, F3, 64, sel=sel)
        hr = d_gr.cpu().numpy()
        assert hr[:14].tobytes() == wg[1].tobytes() and (hr[14:] == P).all()
        ng = len(wg[0])
        hg = d_g.cpu().numpy()
        assert np.sort(hg[:7 * ng].view(bmx.GROUP_DTYPE), order="key").tobytes() == wg[0].tobytes() and (hg[7 * ng:] == P).all()
        wq = xm.brute_quant(m, FB, clauses, ex, QS, sel=sel)
        hq, hqr = d_q.cpu().numpy(), d_qr.cpu().numpy()
        assert hq[:4 * len(QS)].tobytes() == wq[0].tobytes() and (hq[4 * len(QS):] == P).all()
        assert hqr[:4].tobytes() == wq[1].tobytes() and (hqr[4:] == P).all()


def test_interleaved_with_the_plain_forms(seeded):
    """one context, the expression forms and the plain forms in turn: each leaves the scratch the other finds (the accumulators, the table, the select's state,
    the counters) clean"""
    e, m, wide = seeded
    clauses, (a, b) = xm.seeded_programs(3, seed=78, wide=wide)[1]
    sel = xm.selection(m, FB, clauses)
    ex = (a, "*", b)
    plain = (wam.raw_where_agg(e, FB, clauses, F1, F3, -2, 6).tobytes(), e.where_group(FB, clauses, F3, measure=F1).records.tobytes(),
             e.where_quantiles(FB, clauses, F1, QS)[0].tobytes(), e.where_quantiles(FB, clauses, FB, QS)[0].tobytes())
    for _ in range(3):
        check(e, m, clauses, ex, F3, sel=sel)
        again = (wam.raw_where_agg(e, FB, clauses, F1, F3, -2, 6).tobytes(), e.where_group(FB, clauses, F3, measure=F1).records.tobytes(),
                 e.where_quantiles(FB, clauses, F1, QS)[0].tobytes(), e.where_quantiles(FB, clauses, FB, QS)[0].tobytes())
        assert again == plain
        r, xr = e.where_aggregate_expr(FB, clauses, xm.E(ex))
        assert (xr.n_undef, xr.n_range) == xm.brute_agg(m, FB, clauses, ex, sel=sel)[1] and r.n_match == len(sel)
    # the Python forms return what the plain forms return, plus the counters
    g, xr = e.where_group_expr(FB, clauses, F3, xm.E(ex))
    wg = xm.brute_group(m, FB, clauses, ex, F3, sel=sel)
    assert g.records.tobytes() == wg[0].tobytes() and (xr.n_undef, xr.n_range) == wg[2] and isinstance(g, bmx.GroupResult)
    recs, res, xr = e.where_quantiles_expr(FB, clauses, xm.E(ex), QS)
    wq = xm.brute_quant(m, FB, clauses, ex, QS, sel=sel)
    assert recs.tobytes() == wq[0].tobytes() and bytes(res) == wq[1].tobytes() and (xr.n_undef, xr.n_range) == wq[2]


# ---- 5. the expression against the plain form on a shadow field ----
@pytest.mark.parametrize("op", OPS)
def test_shadow_field_differential(seeded, op):
    e, m, wide = seeded
    ex = (F1, op, F2) if op != "-" else (F2, op, FB)
    xm.shadow(m, FS, ex)
    wcm.put(e, m, [FS])
    try:
        for clauses, _ in xm.seeded_programs(8, seed=79, wide=wide):
            sel = xm.selection(m, FB, clauses)
            xres = xm.brute_agg(m, FB, clauses, ex, sel=sel)[1]
            assert xm.raw_agg(e, FB, clauses, ex, F3, -2, 6)[0].tobytes() == wam.raw_where_agg(e, FB, clauses, FS, F3, -2, 6).tobytes()
            assert xm.raw_agg(e, FB, clauses, ex)[0].tobytes() == wam.raw_where_agg(e, FB, clauses, FS).tobytes()
            got, plain = xm.raw_group(e, FB, clauses, ex, F4), e.where_group(FB, clauses, F4, measure=FS)
            assert got[0].tobytes() == plain.records.tobytes() and got[2] == xres
            assert (int(got[1][0]["total"]["n"]), int(got[1][0]["total"]["n_match"])) == (plain.total.n, plain.total.n_match) and plain.total.n_match - plain.total.n == sum(xres)
            got, (recs, res) = xm.raw_quant(e, FB, clauses, ex, QS), e.where_quantiles(FB, clauses, FS, QS)
            assert got[0].tobytes() == recs.tobytes() and got[1].tobytes() == bytes(res) and got[2] == xres
    finally:
        gone = np.nonzero(m.st[FS] == DATA)[0]                              # the shadow field leaves the shared table as it came: every row tombstoned
        wcm.write(e, m, FS, gone, None, ts=50)


# ---- 6. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(97)
    N0, EXTRA = 8192 + 5, 150
    m = wcm.ClockModel(wcm.node_ids(N0 + EXTRA, 4600))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 8, N0))
    for f, pr in ((F1, 0.9), (F2, 0.7), (F3, 0.8)):
        idx = old[rng.random(N0) < pr]
        m.set(f, idx, rng.integers(-3, 8, len(idx)))
    progs = [ALL, [[(FB, 2, 6), (F1, 0, I64MAX)], [(F2, 0, 3, True)]]]
    exprs = [(F1, "*", F2), (F1, "+", FB), (F2, "-", F1), (F2, "*", F2)]

    def ask(x):
        out = []
        for p in progs:
            sel = xm.selection(m, FB, p)
            out += [check(x, m, p, ex, F3, sel=sel, forms="agq" if k == 0 else "ag") for k, ex in enumerate(exprs)]
        return out

    def merge(x, f, idx, vals, ts):
        idx = np.asarray(idx)
        x.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.asarray(vals, np.int64), want_flags=False)
        m.set(f, idx, vals, ts)

    with bmx.Engine(8 * (N0 + EXTRA)) as x:
        wcm.put(x, m, (FB, F1, F2, F3))
        first = ask(x)
        assert first[0][0] > 0 and first[0][1] == 0
        # a merge moves defined nodes out of range and back; a tombstone makes them undefined; a second merge defines them again
        both = np.nonzero((m.st[F1] == DATA) & (m.st[F2] == DATA) & (m.val[F2] != 0) & (m.val[F1] != 0))[0]
        out = both[::5]
        merge(x, F1, out, np.where(m.val[F1][out] > 0, VAL_MAX, -VAL_MAX), 100)
        moved = ask(x)
        assert moved[0][1] == int((np.abs(m.val[F2][out]) > 1).sum()) > 0
        back = out[::2]
        merge(x, F1, back, rng.integers(1, 5, len(back)), 101)
        assert ask(x)[0][1] < moved[0][1]
        dead = out[1::2]
        wcm.write(x, m, F2, dead, None, ts=102)
        after = ask(x)
        assert after[0][0] > first[0][0]
        merge(x, F2, dead[::2], np.full(len(dead[::2]), 1), 103)
        ask(x)
        wcm.write(x, m, FB, old[7::50], None, ts=104)                     # a tombstone on the base field takes the node away
        ask(x)
        # new nodes through the change log, then a larger table
        new = np.arange(N0, N0 + EXTRA)
        merge(x, FB, new, rng.integers(0, 8, EXTRA), 201); merge(x, F1, new[::2], np.full(len(new[::2]), 1 << 30), 201); merge(x, F2, new[::3], np.full(len(new[::3]), 1 << 30), 201)
        assert ask(x)[0][1] > 0
        x.reserve(32 * (N0 + EXTRA))
        before = ask(x)
        # a value-ordered view on the base field is neither read nor touched
        x.index_set_ordered(FB, 1)
        stv = x.index_ordered_stats(FB)
        assert ask(x) == before and x.index_ordered_stats(FB) == stv
        x.index_set_ordered(FB, 0)
        # a base value beyond int32: the int64 column
        merge(x, FB, [11, N0 + 3], np.array([2**40, -(2**35)]), 400)
        ask(x)
        check(x, m, ALL, (FB, "*", FB), F3)
