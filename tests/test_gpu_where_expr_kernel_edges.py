"""GPU: the computed measures (csrc/expr_kernels.h) at the edges of the three sweeps that fetch them: k_where_agg (G = 0 / 1 / 2), k_group_sweep and k_quant0.
The operand columns are written BY POSITION of the base field's index (index_ids gives the order), so a case can say which lane of which wave holds the one
node of a class: a lane holds E consecutive positions (E = 4 int32 or 2 int64 values per 16-byte load), a wave 64 lanes, a workgroup 512 lanes with 4 loads in
flight. The layouts are expr_model.edge_layouts (test_expr_model.py shows that they expose every single defect of the stand-in). Before a layout runs on the
device, the sequential stand-in must probe exactly the fields the layout names, in order, and class every walked node as the numpy model does; then every byte
of every form's answer is the brute force's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import expr_model as xm
import where_clock_model as wcm
from expr_model import ALL, F1, F2, FB, VAL_MAX

FG = wcm.wdm.streams.fnv1a32("expr.edge.group")
QS = [(0, 1), (1, 2), (1, 1), (1, 3)]


def _walked(n, E):
    """the positions the sequential stand-in walks: all of a small column; of a large one the two waves at either end of every block of 8192"""
    pos = np.arange(n)
    if n <= 1024:
        return pos
    wave = 64 * E
    return pos[(pos % 8192 < 2 * wave) | (pos % 8192 >= 8192 - 2 * wave) | (pos >= n - 2 * wave)]


def _five_keys_of_one_set():
    """five group values that fall into one set of k_group_sweep's LDS cache (4 ways): group_set = (((u32)key ^ (u32)(key >> 32)) * 0x9E3779B1) >> 24"""
    by_set = {}
    for key in range(1, 4000):
        s = ((key * 0x9E3779B1) & 0xFFFFFFFF) >> 24
        by_set.setdefault(s, []).append(key)
        if len(by_set[s]) == 5:
            return by_set[s]
    raise AssertionError("no set with five keys below 4000")


def _answers(x, m, e, sel):
    """flat aggregate, quantiles: every layout"""
    want = xm.brute_agg(m, FB, ALL, e, sel=sel)
    got = xm.raw_agg(x, FB, ALL, e)
    assert xm.same(got, want), ("flat", got, want)
    got, wq = xm.raw_quant(x, FB, ALL, e, QS), xm.brute_quant(m, FB, ALL, e, QS, sel=sel)
    assert xm.same(got, wq), ("quantiles", got, wq)
    return want[1]


def _grouped(x, m, e, sel, n):
    """the grouped sweeps: G = 1 at its last size (1024 groups, 1025 records), G = 2 right behind it and far behind it, the discovered groups"""
    for ng in (7, 1024, 1025, 4000):
        got, want = xm.raw_agg(x, FB, ALL, e, FG, 0, ng), xm.brute_agg(m, FB, ALL, e, FG, 0, ng, sel=sel)
        assert xm.same(got, want), ("window", ng)
    got, want = xm.raw_group(x, FB, ALL, e, FG, 4096), xm.brute_group(m, FB, ALL, e, FG, 4096, sel=sel)
    assert xm.same(got, want), "group"
    if n > 1100:
        got, want = xm.raw_group(x, FB, ALL, e, FG, 1029), xm.brute_group(m, FB, ALL, e, FG, 1029, sel=sel)
        assert want[0] is None and xm.same(got, want), "group, one record too few"


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", xm.EDGE_SIZES)
def test_computed_measures_at_the_edges(n, wide):
    E = 2 if wide else 4
    ids = wcm.node_ids(n, 6000 + n)
    with bmx.Engine(max(32 * n, 4096)) as x:
        off = (1 << 40) if wide else 0
        x.put_rows(ids, np.full(n, FB, np.uint32), np.full(n, 6, np.int64), np.full(n, off, np.int64))
        scratch = wcm.ClockModel(ids)
        node = scratch.index_of(x.index_ids(FB))                        # node[p]: the node at position p
        m = xm.edge_table(ids, node, wide)
        x.merge_batch(*m.rows(FB), want_flags=False)                    # (clock 7 over clock 6: the base values)
        m.set(FG, node, np.arange(n) % 1030)                            # the group field, by position: 1030 groups (or n)
        wcm.put(x, m, (F1, F2, FG))
        assert np.array_equal(scratch.index_of(x.index_ids(FB)), node), "a value update moves no position"
        sel = np.arange(n)
        walked, ran, tags = _walked(n, E), 0, set()
        for name, mutate, e, probed in xm.edge_layouts(wide, n):
            if mutate:
                mutate(m, node)
                wcm.put(x, m, (F1, F2))
            cls, _ = xm.measure(m, e)
            for pos in walked:                                          # the stand-in first
                probes = []
                got = xm.fetch(m, FB, e, node[pos], tags=tags, probes=probes)
                assert got[0] == cls[node[pos]] and probes == probed, (name, pos, probes)
            xres = _answers(x, m, e, sel)
            if name.startswith("lone"):
                assert sorted((int(xm.brute_agg(m, FB, ALL, e, sel=sel)[0][0]["n"]), xres[0], xres[1]))[:2] == ([0, 0] if n == 1 else [0, 1]), name
            if name == "a wave all out of range":
                assert xres == (0, min(n, 64 * E))
            if name in ("lone out-of-range node at %d" % (n - 1), "products at the edge", "tombstones on either side"):
                _grouped(x, m, e, sel, n)
            ran += 1
        assert ran >= 15 and {"range_mul_64", "range_add", "undef_tomb", "same_field_one_probe", "a_column", "b_column", "both_column"} <= tags
        assert n < 11 or "range_mul_128" in tags                        # (the products at the edge repeat every 11 positions)
        # five keys of one set of the group cache: the fifth bypasses the cache (and an out-of-range node among each key's rows)
        keys = _five_keys_of_one_set()
        m.set(FG, node, np.array(keys)[np.arange(n) % 5])
        m.set(F1, node, np.where(np.arange(n) % 11 == 0, VAL_MAX, 3)); m.set(F2, node, np.full(n, 2))
        wcm.put(x, m, (F1, F2, FG))
        e = (F1, "*", F2)
        got, want = xm.raw_group(x, FB, ALL, e, FG, 16), xm.brute_group(m, FB, ALL, e, FG, 16, sel=sel)
        assert xm.same(got, want) and len(want[0]) == min(n, 5)
