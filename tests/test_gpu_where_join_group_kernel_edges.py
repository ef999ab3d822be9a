"""GPU: the lookup-join kernels at the edges of their geometry (csrc/join_kernels.h k_join_build / k_join_group_sweep). A lane loads 16 bytes (4 int32 or 2 int64
values), a wave holds 2048 rows of a round, a workgroup 8192. The engine's base column is loaded first and the model's nodes are numbered by POSITION in its
index, so every other field is written by position and join_model's brute force answers for it: a pattern field selects rows at the first and last element of
a lane's load, of a wave, of a workgroup's round and of the index — on the outer side, where three lists rotate every selected position through the three
destinations (grouped, absent, unmatched), and on the inner side, where the selected positions are the map. Both value widths (wide: every base value beyond
int32, so the index sweeps its int64 column). The 64-slot maps and the LDS-cache bypass are join_model.table_edges / cache_bypass, whose walks
test_join_model.py pins on the stand-in."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import join_model as jm
import where_agg_model as wam
from oracle import streams

FB, FL, FA, FM = (streams.fnv1a32(s) for s in ("join.edge", "join.edge.link", "join.edge.attr", "join.edge.measure"))
WAVE, WORD = 2048, 32
SIZES = [1, 3, 31, 33, 2047, 2049, 8191, 8193, 2 * 8192 + 1]


def _patterns(n):
    words = np.arange(0, n, WORD)
    lanes = np.arange(0, n, 4)                             # a lane's 16-byte load: 4 int32 (or two loads of 2 int64)
    edges = np.arange(WAVE, n, WAVE)                       # wave boundaries; every fourth is a workgroup boundary
    return {
        "none": np.zeros(0, np.int64),
        "all": np.arange(n),
        "first": np.array([0]),
        "last": np.array([n - 1]),
        "lane ends": np.unique(np.concatenate([lanes, np.minimum(lanes + 3, n - 1)])),
        "word ends": np.unique(np.concatenate([words, np.minimum(words + WORD - 1, n - 1)])),
        "wave and workgroup boundaries": np.unique(np.concatenate([edges - 1, edges])) if len(edges) else np.array([n // 2]),
    }


def _by_position(e, n, base, salt):
    """the base column loaded -> a model whose node p is the index's position p"""
    ids = streams.splitmix64_np(np.arange(1 + salt + n, n + 1 + salt + n, dtype=np.uint64))
    e.load_rows(ids, np.full(n, FB, np.uint32), np.full(n, 5, np.int64), np.full(n, base, np.int64))
    m = jm.Model(e.index_ids(FB))
    assert m.N == n
    m.set(FB, np.arange(n), base)
    return m


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_both_sweeps_at_the_edges(n, wide):
    base = (2**40 if wide else 0) + 7
    with bmx.Engine(max(16 * n, 1024)) as e:
        m = _by_position(e, n, base, 400000)
        p = np.arange(n)
        pats = _patterns(n)
        fp = [streams.fnv1a32("join.edge.pattern.%d" % k) for k in range(len(pats))]
        m.set(FL, p[p % 5 != 0], 1000 + p[p % 5 != 0])                # every fifth position has no link, every tenth's is a tombstone
        m.set(FM, p[p % 4 != 1], p[p % 4 != 1] - 7)
        m.set(FA, p[p % 6 != 2], p[p % 6 != 2] % 11 - 5)
        for f, rows in zip(fp, pats.values()):
            if len(rows):
                m.set(f, rows, 1)
        wam.load(e, m, [FL, FM, FA] + fp)
        wam.tombstone(e, m, FL, p[p % 10 == 3])
        assert np.array_equal(e.index_ids(FB), m.ids), "no position moved"
        seen = set()
        for (name, rows), f in zip(pats.items(), fp):
            sel = [[(f, 1, 1)]]
            for r in range(3):                                         # the outer side: position p is grouped, absent or unmatched in turn
                grouped, absent = p[p % 3 == r], p[p % 3 == (r + 1) % 3]
                keys = np.concatenate([1000 + grouped, 1000 + absent, [5]])
                vals = np.concatenate([grouped % 7 - 3, np.full(len(absent), jm.INT64_MAX), [5]])
                recs, res = jm.ask(e, m, jm.QMAP(FB, sel, FL, keys, vals, FM, cap=16))
                assert int(res["total"]["n_match"]) == len(rows) and not int(res["flags"])
                seen |= {k for k in ("absent", "unmatched") if int(res[k]["n_match"])} | ({"grouped"} if len(recs) else set())
            # the inner side: the selected positions are the map (key: the link field, attribute: FA, FM or the key itself); the outer program selects every row
            for attr, measure in ((FA, FM), (FL, None)) if n <= 33 else ((FA, FM),):
                recs, res = jm.ask(e, m, jm.Q(FB, jm.EVERY, FL, FB, sel, FL, attr, measure, cap=64, map_cap=max(len(rows), 1)))
                assert int(res["n_inner"]) == len(rows) and not int(res["flags"]) and int(res["map_size"]) == int(res["n_keyed"])
            if len(rows) > 12:
                _, res = jm.ask(e, m, jm.Q(FB, jm.EVERY, FL, FB, sel, FL, FA, FM, cap=64, map_cap=len(rows) // 2))
                assert int(res["flags"]) == jm.MAP_OVERFLOW
        assert seen == ({"grouped", "absent", "unmatched"} if n > 3 else seen)


@pytest.mark.parametrize("name", ["table edges", "cache bypass"])
def test_small_tables(name):
    """64-slot maps: 32 keys on one home, a cluster that wraps from slot 63 to 0, links that walk a whole cluster and miss, 70 keys into 64 slots; more than four
    attributes in one LDS set; 64 keys that map to one attribute — each query also at cap = D, D - 1, map_cap = K, K - 1"""
    m, tombs, qs = {n: (m, t, q) for n, m, t, q in jm.edge_layouts()}[name]
    with bmx.Engine(8192) as e:
        wam.load(e, m, jm.ALL_FIELDS)
        for f, idx in tombs.items():
            wam.tombstone(e, m, f, idx)
        flags = set()
        for q0 in qs:
            for q in jm.variants(m, q0):
                flags.add(int(jm.ask(e, m, q)[1]["flags"]))
        assert flags == {0, jm.MAP_OVERFLOW, jm.GROUP_OVERFLOW}


@pytest.mark.parametrize("nkeys", [1, 5, 5000])
def test_many_inner_nodes_with_few_keys(nkeys):
    """10^5 inner nodes that hold nkeys keys between them, every node with a different attribute: the minimum must come out, with the keys dealt round the lanes
    and with every lane of a wave on one key (positions in runs of 2048); then every key with the same attribute: every lane of a wave reaches one record
    through a different key"""
    n, nout = 100_000, 3000
    with bmx.Engine(8 * n) as e:
        m = _by_position(e, n, 3, 500000)
        p = np.arange(n)
        m.set(FL, p[:nout], jm.uid((p[:nout] * 5) % (2 * nkeys)))       # half of the link values are keys
        m.set(FM, p[:nout], p[:nout] * 3 - 4000)
        sel = [[(FL, -jm.VAL_MAX, jm.VAL_MAX)]]                        # the outer program: the nout nodes that have a link
        key, a1, a2 = (streams.fnv1a32("join.edge.key.%d" % k) for k in range(3))
        wam.load(e, m, [FL, FM])
        unique = (p * 7919) % 100003 - 50000                           # all different
        for ts, keys, attr, f in ((5, p % nkeys, unique, a1), (6, (p // WAVE) % nkeys, unique[::-1], a2), (7, p % nkeys, np.full(n, 7), a1)):
            e.put_rows(m.ids, np.full(n, key, np.uint32), np.full(n, ts, np.int64), jm.uid(keys))
            e.put_rows(m.ids, np.full(n, f, np.uint32), np.full(n, ts, np.int64), attr.astype(np.int64))
            m.set(key, p, jm.uid(keys)); m.set(f, p, attr)
            recs, res = jm.ask(e, m, jm.Q(FB, sel, FL, FB, jm.EVERY, key, f, FM, cap=8192, map_cap=8192))
            assert (int(res["map_size"]), int(res["n_inner"]), int(res["n_keyed"]), int(res["total"]["n_match"])) == (len(np.unique(keys)), n, n, nout)
            assert (len(recs) == 1 if ts == 7 else len(recs) >= 1) and int(res["unmatched"]["n_match"]) > 0 and not int(res["flags"])
