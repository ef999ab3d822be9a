"""CPU: the model of the computed measures (tests/expr_model.py) against itself. The brute force is the header's sentences with Python ints; the numpy model
and the lane's stand-in are held against it; the seeded generator must give every program an undefined and an out-of-range node; the layouts of the
kernel-edge tests must expose each single defect the stand-in can be given, and together with the seeded cases reach every path of the stand-in."""
import numpy as np
import pytest

import bmx
import expr_model as xm
from expr_model import DEFINED, F1, F2, F3, F4, FB, OPS, RANGE, UNDEF, VAL_MAX

N = 240
QS = [(0, 1), (1, 4), (1, 2), (95, 100), (1, 1), (1, 2)]


@pytest.fixture(scope="module")
def table():
    return xm.seeded_table(N)


@pytest.fixture(scope="module")
def programs():
    return xm.seeded_programs(60)


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_the_binding():
    e = bmx.Expr(7, "*", 9)
    assert (e.a, e.b, e.op, e.reserved) == (7, 9, bmx.EXPR_MUL, 0)
    assert [bmx.Expr(1, o, 2).op for o in OPS] == [1, 2, 3]
    with pytest.raises(ValueError):
        bmx.Expr(1, "/", 2)
    assert bmx.EXPR_RES_DTYPE.itemsize == 16 and len(bmx.EXPORTS_EXPR) == 6


def test_classify_at_the_edge_of_the_range():
    m = xm.ClockModel(xm.node_ids(12))
    a = [xm.P1, 1 << 26, 94906265, 94906266, VAL_MAX, xm.BIG, VAL_MAX, VAL_MAX, -VAL_MAX, 0, 1, -1]
    b = [xm.P2, 1 << 27, 94906265, 94906267, VAL_MAX, xm.BIG + 1, 0, 1, -1, VAL_MAX, -VAL_MAX, VAL_MAX]
    m.set(F1, np.arange(12), a); m.set(F2, np.arange(12), b)
    mul = [xm.classify(m, (F1, "*", F2), i) for i in range(6)]
    assert mul == [(DEFINED, VAL_MAX), (RANGE, None), (DEFINED, 94906265 ** 2), (RANGE, None), (RANGE, None), (RANGE, None)]
    assert ((xm.BIG * (xm.BIG + 1)) % (1 << 64)) == xm.BIG          # the product that wraps into the range
    assert [xm.classify(m, (F1, "+", F2), i) for i in (6, 7)] == [(DEFINED, VAL_MAX), (RANGE, None)]
    assert xm.classify(m, (F1, "+", F2), 8) == (RANGE, None) and xm.classify(m, (F1, "-", F2), 7)[0] == DEFINED
    assert [xm.classify(m, (F1, "*", F2), i) for i in (9, 10, 11)] == [(DEFINED, 0), (DEFINED, -VAL_MAX), (DEFINED, -VAL_MAX)]
    m.tomb(F2, [0])
    assert xm.classify(m, (F1, "*", F2), 0) == (UNDEF, None) and xm.classify(m, (F1, "-", F1), 0) == (DEFINED, 0)
    assert xm.classify(m, (F1, "*", F3), 1) == (UNDEF, None)


def test_the_generator_guarantees_both_classes(table, programs):
    assert len(programs) == 60
    seen_pairs = set()
    for clauses, (a, b) in programs:
        assert 1 <= len(clauses) <= 8 and sum(xm.wcm.entries(c) for c in clauses) <= 32 and (a, b) != (FB, FB)
        sel = xm.selection(table, FB, clauses)
        for op in xm.ops_of(a, b):
            _, (n_undef, n_range) = xm.brute_agg(table, FB, clauses, (a, op, b), sel=sel)
            assert n_undef >= 1 and n_range >= 1, (clauses, a, op, b)
        seen_pairs.add(("base" if a == FB else "probed", "base" if b == FB else "same" if b == a else "probed"))
    assert seen_pairs == {("base", "probed"), ("probed", "base"), ("probed", "same"), ("probed", "probed")}


def test_the_numpy_model_is_the_brute_force(table, programs):
    for k, (clauses, (a, b)) in enumerate(programs):
        sel = xm.selection(table, FB, clauses)
        for op in xm.ops_of(a, b):
            e = (a, op, b)
            ra, xa = xm.brute_agg(table, FB, clauses, e, sel=sel)
            ma, mxa = xm.model_agg(table, FB, clauses, e)
            assert same(ra, ma) and xa == mxa, (k, op)
            assert int(ra[0]["n_match"]) == int(ra[0]["n"]) + xa[0] + xa[1]
            if k % 3 == 0:
                g = [F1, F2, F3, F4, FB][k % 5]
                rw, xw = xm.brute_agg(table, FB, clauses, e, g, -2, 6, sel=sel)
                mw, mxw = xm.model_agg(table, FB, clauses, e, g, -2, 6)
                assert same(rw, mw) and xw == mxw == xa, (k, op, "window")
                rg, sg, xg = xm.brute_group(table, FB, clauses, e, g, sel=sel)
                mg, msg, mxg = xm.model_group(table, FB, clauses, e, g)
                assert same(rg, mg) and same(sg, msg) and xg == mxg == xa, (k, op, "group")
                assert int(sg[0]["total"]["n_match"]) == int(sg[0]["total"]["n"]) + xg[0] + xg[1]
            if k % 3 == 1:
                rq, sq, xq = xm.brute_quant(table, FB, clauses, e, QS, sel=sel)
                mq, msq, mxq = xm.model_quant(table, FB, clauses, e, QS)
                assert same(rq, mq) and same(sq, msq) and xq == mxq == xa, (k, op, "quantiles")


def test_the_stand_in_is_the_brute_force_and_reaches_its_paths(table, programs):
    tags = set()
    for clauses, (a, b) in programs[:30]:
        sel = xm.selection(table, FB, clauses)
        for op in xm.ops_of(a, b):
            probes = []
            want = xm.brute_agg(table, FB, clauses, (a, op, b), sel=sel)
            got = xm.standin_agg(table, FB, clauses, (a, op, b), tags=tags, probes=probes, sel=sel)
            assert same(want[0], got[0]) and want[1] == got[1]
            per_node = (a != FB) + (b != FB and b != a)
            assert len(probes) == per_node * len(sel) and set(probes) <= {a, b} - {FB}
    m, node = _edge_table(65, False)
    for name, mutate, e, probed in xm.edge_layouts(False, 65):
        if mutate:
            mutate(m, node)
        probes = []
        want = xm.brute_agg(m, FB, xm.ALL, e)
        got = xm.standin_agg(m, FB, xm.ALL, e, tags=tags, probes=probes)
        assert same(want[0], got[0]) and want[1] == got[1], name
        assert probes == probed * m.N, name
    assert tags == set(xm.TAGS), set(xm.TAGS) - tags


def _edge_table(n, wide):
    ids = xm.node_ids(n, 123)
    node = np.random.default_rng(5).permutation(n)
    return xm.edge_table(ids, node, wide), node


@pytest.mark.parametrize("wide", [False, True])
def test_every_defect_is_exposed_by_an_edge_layout(wide):
    exposed = {d: [] for d in xm.DEFECTS}
    m, node = _edge_table(65, wide)
    for name, mutate, e, _ in xm.edge_layouts(wide, 65):
        if mutate:
            mutate(m, node)
        want = xm.brute_agg(m, FB, xm.ALL, e)
        for d in xm.DEFECTS:
            got = xm.standin_agg(m, FB, xm.ALL, e, defect=d)
            if not (same(want[0], got[0]) and want[1] == got[1]):
                exposed[d].append(name)
    assert all(exposed.values()), [d for d, v in exposed.items() if not v]
    assert any("products" in n for n in exposed["mul_wrapped_64"]) and any("lone out-of-range" in n for n in exposed["no_range_check"])


def test_the_lone_nodes_are_alone():
    m, node = _edge_table(8193, False)
    for name, mutate, e, _ in xm.edge_layouts(False, 8193):
        if not name.startswith("lone"):
            break
        mutate(m, node)
        recs, (n_undef, n_range) = xm.model_agg(m, FB, xm.ALL, e)
        n = int(recs[0]["n"])
        if "defined" in name and "undefined" not in name:
            assert (n, n_undef, n_range) == (1, 8192, 0), name
        elif "undefined" in name:
            assert (n, n_undef, n_range) == (8192, 1, 0), name
        else:
            assert (n, n_undef, n_range) == (8192, 0, 1), name
