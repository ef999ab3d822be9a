"""GPU: the sharded forms of the computed measures (bmx_comm_where_aggregate_expr, bmx_comm_where_group_expr, bmx_comm_where_quantiles_expr) over 1, 2 and 4
logical shards (all on device 0) against one engine holding the same rows: every byte of the records, of the result record and of the bmx_expr_res equal — and
both equal the brute force of tests/expr_model.py. A node is classified by the one shard that owns it: the shards' n_undef and n_range add, and a group whose
out-of-range node lives on another shard than its other members still has one record."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import expr_model as xm
import where_clock_model as wcm
from expr_model import ALL, F1, F2, F3, F4, FB, OPS, VAL_MAX

N = 700
QS = [(1, 2), (0, 1), (99, 100), (1, 1), (1, 4)]
LONELY = 555          # a group value nobody else holds


@pytest.mark.parametrize("nshards", [1, 2, 4])
def test_sharded(nshards):
    m = xm.seeded_table(N, seed=20250601)
    owner = bmx.owner_of(m.ids, nshards)
    # three nodes of one group on as many shards as there are, the first of them out of range for F1 * F2, the second undefined
    trio = [int(np.nonzero(owner == s % nshards)[0][3 + s]) for s in range(3)]
    m.set(FB, trio, [1, 2, 3]); m.set(F3, trio, [LONELY] * 3)
    m.set(F1, trio, [VAL_MAX, 4, 4]); m.set(F2, trio, [2, 2, 5]); m.tomb(F2, [trio[1]])
    with bmx.Engine(32 * N) as e, bmx.Comm([0] * nshards, 32 * N) as c:
        for x in (e, c):
            wcm.put(x, m, [FB] + xm.PROBED)
        some = 0
        for k, (clauses, (a, b)) in enumerate(xm.seeded_programs(10, seed=20250602) + [(ALL, (F1, F2)), (ALL, (F4, F4))]):
            sel = xm.selection(m, FB, clauses)
            for op in xm.ops_of(a, b):
                ex = (a, op, b)
                want = xm.brute_agg(m, FB, clauses, ex, F3, -2, 6, sel=sel)
                one, many = xm.raw_agg(e, FB, clauses, ex, F3, -2, 6), xm.raw_agg(c, FB, clauses, ex, F3, -2, 6)
                assert xm.same(many, one) and xm.same(many, want), (nshards, k, op, "window")
                assert xm.same(xm.raw_agg(c, FB, clauses, ex), xm.brute_agg(m, FB, clauses, ex, sel=sel)), (nshards, k, op, "flat")
                want = xm.brute_group(m, FB, clauses, ex, F3, sel=sel)
                one, many = xm.raw_group(e, FB, clauses, ex, F3), xm.raw_group(c, FB, clauses, ex, F3)
                assert xm.same(many, one) and xm.same(many, want), (nshards, k, op, "group")
                want = xm.brute_quant(m, FB, clauses, ex, QS, sel=sel)
                one, many = xm.raw_quant(e, FB, clauses, ex, QS), xm.raw_quant(c, FB, clauses, ex, QS)
                assert xm.same(many, one) and xm.same(many, want), (nshards, k, op, "quantiles")
                some += want[2][0] > 0 and want[2][1] > 0
        assert some >= 20
        # the lonely group: one record, three nodes, one measured; too small a cap overflows on the union
        recs, res, xr = xm.raw_group(c, FB, ALL, (F1, "*", F2), F3)
        g = recs[recs["key"] == LONELY][0]["agg"]
        assert (int(g["n_match"]), int(g["n"]), int(g["sum_lo"])) == (3, 1, 20)
        if nshards > 1:
            assert len({int(owner[t]) for t in trio}) == min(nshards, 3)
        D = len(recs)
        got, want = xm.raw_group(c, FB, ALL, (F1, "*", F2), F3, D - 1), xm.brute_group(m, FB, ALL, (F1, "*", F2), F3, D - 1)
        assert want[0] is None and xm.same(got, want)
        # the Python forms of the communicator
        r, xres = c.where_aggregate_expr(FB, ALL, xm.E((F1, "*", F2)))
        assert (xres.n_undef, xres.n_range) == xr and r.n_match == r.n + xr[0] + xr[1]
        g2, xres = c.where_group_expr(FB, ALL, F3, xm.E((F1, "*", F2)))
        assert g2.records.tobytes() == recs.tobytes() and (xres.n_undef, xres.n_range) == xr
        q, qres, xres = c.where_quantiles_expr(FB, ALL, xm.E((F1, "*", F2)), QS)
        assert q.tobytes() == xm.brute_quant(m, FB, ALL, (F1, "*", F2), QS)[0].tobytes() and (xres.n_undef, xres.n_range) == xr and qres.n_match == r.n_match
