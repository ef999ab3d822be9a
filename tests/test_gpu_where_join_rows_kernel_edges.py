"""GPU: the join-projection kernels at the edges of their geometry (csrc/join_rows_kernels.h k_jrows_build, PredJRowsFrom, k_jrows_emit). A lane loads 16 bytes
(4 int32 or 2 int64 values), a mask word holds 32 rows, a wave 2048 rows of a round, a workgroup 8192. The engine's base column is loaded first and the model's
nodes are numbered by POSITION in its index, so every other field is written by position and join_rows_model's brute force answers for it. A pattern field
selects rows at the first and last element of a lane's load, of a mask word, of a wave, of a workgroup's block and of the index — on the outer side, where
every third selected position has no inner node, so that the inner join's ranks differ from the left join's, and on the inner side, where the selected
positions are the map. Both value widths (wide: every base value beyond int32, so the index sweeps its int64 column). Caps and cursors at 8191 / 8192 / 8193 and
at a workgroup's first and last rank; 64-slot maps whose walks wrap; 10^5 inner nodes on 1 and 5 keys (every lane lowers one word); 0, 1 and 8 fields on
either side."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import join_rows_model as jrm
import where_agg_model as wam
from join_rows_model import EVERY, NO_NODE, Q, QMAP, Table
from oracle import streams

FB, FL = (streams.fnv1a32(s) for s in ("jrows.edge", "jrows.edge.link"))
FO = [streams.fnv1a32("jrows.edge.outer.%d" % k) for k in range(3)]
FN = [streams.fnv1a32("jrows.edge.inner.%d" % k) for k in range(3)]
WAVE, WORD, BLOCK = 2048, 32, 8192
SIZES = [1, 3, 31, 33, 2047, 2049, 8191, 8193, 2 * 8192 + 1]
FIELDS = {0: [], 1: [0], 8: [0, 1, 2, 1, 0, 2, 2, 0]}                  # how many fields -> which of the three (repeats)


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
    """the base column loaded -> a table whose node p is the index's position p"""
    ids = streams.splitmix64_np(np.arange(1 + salt + n, n + 1 + salt + n, dtype=np.uint64))
    e.load_rows(ids, np.full(n, FB, np.uint32), np.full(n, 5, np.int64), np.full(n, base, np.int64))
    m = Table(e.index_ids(FB))
    assert m.N == n
    m.set(FB, np.arange(n), base, 5)
    return m


def _cells(m, n):
    """a link on four positions of five (every tenth's a tombstone) and three fields per side in all three states, every cell with its own clock"""
    p = np.arange(n)
    m.set(FL, p[p % 5 != 0], 1000 + p[p % 5 != 0], 7)
    for k, f in enumerate(FO + FN):
        rows = p[(p + k) % 4 != 0]
        m.set(f, rows, rows * (k + 2) - 9, 10 + k + rows % 7)
    return {FL: p[p % 10 == 3], FO[1]: p[p % 9 == 2], FN[0]: p[p % 6 == 1], FN[2]: p[p % 8 == 5]}


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_both_passes_at_the_edges(n, wide):
    base = (2**40 if wide else 0) + 7
    with bmx.Engine(max(32 * n, 1024)) as e:
        m = _by_position(e, n, base, 600000)
        p = np.arange(n)
        pats = _patterns(n)
        fp = [streams.fnv1a32("jrows.edge.pattern.%d" % k) for k in range(len(pats))]
        tombs = _cells(m, n)
        for f, rows in zip(fp, pats.values()):
            if len(rows):
                m.set(f, rows, 1)
        wam.load(e, m, [FL] + FO + FN + fp)
        jrm.apply_tombs(m, tombs, e)
        order = e.index_ids(FB)
        assert np.array_equal(order, m.ids), "no position moved"
        joined = set()
        for k, ((name, rows), f) in enumerate(zip(pats.items(), fp)):
            sel = [[(f, 1, 1)]]
            nf, nif = (0, 1, 8)[k % 3], (8, 0, 1)[(k + k // 3) % 3]
            fields, in_fields = [FO[j] for j in FIELDS[nf]], [FN[j] for j in FIELDS[nif]]
            # the outer side: the links of the positions p % 3 != r are keys, each of another node; every third selected position has no inner node
            r = k % 3
            keyed = p[p % 3 != r]
            ql = QMAP(FB, sel, FL, fields, (1000 + keyed).tolist() + [jrm.INT64_MIN], m.ids[(keyed * 7 + 1) % n].tolist() + [NO_NODE], in_fields, with_ts=k % 2 == 0, cap=n)   # (and one pair that is skipped: npairs >= 1)
            for inner_join in (False, True):
                got, _ = jrm.ask(e, m, dict(ql, inner=inner_join), order)
                assert inner_join or int(got["res"]["n_match"]) == len(rows)
                joined |= {bool(x) for x in (got["in_ids"] != np.uint64(NO_NODE)).tolist()}
            # the inner side: the selected positions are the map (key: the link field); the outer program selects every row
            for inner_join in (False, True):
                got, _ = jrm.ask(e, m, Q(FB, EVERY, FL, fields, FB, sel, FL, in_fields, k % 2 == 1, inner_join, cap=n, map_cap=max(len(rows), 1)), order)
                assert int(got["res"]["n_inner"]) == len(rows) and not int(got["res"]["flags"]) and int(got["res"]["map_size"]) == int(got["res"]["n_keyed"])
                assert inner_join or int(got["res"]["n_match"]) == n
                assert np.array_equal(got["in_ids"][got["in_ids"] != np.uint64(NO_NODE)], got["ids"][got["in_ids"] != np.uint64(NO_NODE)]), "every node's link is its own key"
            if len(rows) > 12:
                got, _ = jrm.ask(e, m, Q(FB, EVERY, FL, fields, FB, sel, FL, in_fields, map_cap=len(rows) // 2), order)
                assert int(got["res"]["flags"]) == jrm.MAP_OVERFLOW
        assert joined == ({True, False} if n > 3 else joined)


@pytest.mark.parametrize("wide", [False, True])
def test_caps_and_cursors_at_the_block_edges(wide):
    """every row selected, every third without inner node: the left join's rank is the position, the inner join's is not; cap and start at 8191 / 8192 / 8193
    and at the first and last rank of the second workgroup"""
    n = 2 * BLOCK + 1
    base = (2**40 if wide else 0) + 7
    with bmx.Engine(32 * n) as e:
        m = _by_position(e, n, base, 700000)
        p = np.arange(n)
        tombs = _cells(m, n)
        wam.load(e, m, [FL] + FO + FN)
        jrm.apply_tombs(m, tombs, e)
        order = e.index_ids(FB)
        keyed = p[p % 3 != 1]
        q = QMAP(FB, EVERY, FL, [FO[0], FL], 1000 + keyed, m.ids[(keyed * 7 + 1) % n], [FN[0], FN[1]], cap=n)
        for inner_join in (False, True):
            qi = dict(q, inner=inner_join)
            full = jrm.answer(m, order, qi)
            sel_pos = m.index_of(full["ids"])                                  # positions of the delivered rows, in rank order
            nm = len(sel_pos)
            first_rank = int(np.searchsorted(sel_pos, BLOCK))                   # the rank of the second workgroup's first row
            last_rank = int(np.searchsorted(sel_pos, 2 * BLOCK)) - 1
            assert inner_join == (first_rank != BLOCK)
            caps = sorted({BLOCK - 1, BLOCK, BLOCK + 1, first_rank - 1, first_rank, first_rank + 1, last_rank, last_rank + 1, nm - 1, nm})
            for cap in caps:
                got, _ = jrm.ask(e, m, dict(qi, cap=cap), order)
                assert int(got["res"]["n_out"]) == min(cap, nm)
            for start in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK):
                for cap in (1, 3, BLOCK):
                    jrm.ask(e, m, dict(qi, start=start, cap=cap), order)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("blocks", [9, 17])
def test_eight_blocks_per_workgroup(monkeypatch, blocks, wide):
    """BMX_SCAN_SUB8_BLOCKS=1: the emit pass takes eight blocks per workgroup (k_jrows_emit<T, 8>); 9 and 17 blocks leave a last workgroup with one block. Sparse
    selections take its one-scan path (at most 8192 matches in eight blocks), dense ones go block by block. Every third selected row has no inner node, so the
    inner join's rank is not the left join's. Every answer equals the model's and, byte for byte, the one-block form's."""
    n = (blocks - 1) * BLOCK + 5
    base = (2**40 if wide else 0) + 7
    sparse = np.unique(np.concatenate([np.arange(0, n, 509), np.arange(BLOCK - 1, n, BLOCK), np.arange(BLOCK, n, BLOCK), [n - 1]]))
    pats = {"sparse": sparse, "dense": np.setdiff1d(np.arange(n), sparse), "exactly 8192 in the first eight blocks": np.arange(0, 8 * BLOCK, 8),
            "8193 there": np.sort(np.concatenate([np.arange(0, 8 * BLOCK, 8), [3]]))}
    fp = [streams.fnv1a32("jrows.edge.sub8.%d" % k) for k in range(len(pats))]
    with bmx.Engine(8 * n) as e:
        m = _by_position(e, n, base, 1000000 + blocks)
        p = np.arange(n)
        m.set(FL, p, 1000 + p, 7)
        m.set(FO[0], p[p % 4 != 0], p[p % 4 != 0] * 2 - 9, 10 + p[p % 4 != 0] % 7)
        m.set(FN[0], p[p % 4 != 1], p[p % 4 != 1] * 3 - 9, 11 + p[p % 4 != 1] % 7)
        for f, rows in zip(fp, pats.values()):
            m.set(f, rows, 1)
        wam.load(e, m, [FL, FO[0], FN[0]] + fp)
        jrm.apply_tombs(m, {FO[0]: p[p % 9 == 2], FN[0]: p[p % 6 == 1]}, e)
        order = e.index_ids(FB)
        assert np.array_equal(order, m.ids), "no position moved"
        for (name, rows), f in zip(pats.items(), fp):
            keyed = rows[np.arange(len(rows)) % 3 != 1]                 # every third selected row: its link is no key
            q = QMAP(FB, [[(f, 1, 1)]], FL, [FO[0]], (1000 + keyed).tolist(), m.ids[(keyed * 7 + 1) % n].tolist(), [FN[0]], with_ts=True, cap=n)
            M = jrm.map_of(m, q)
            for inner_join in (False, True):
                nm = len(keyed) if inner_join else len(rows)
                for start, cap in ((0, n), (0, 0), (0, 1), (0, nm - 1), (0, nm), (0, BLOCK), (0, 8 * BLOCK - 1), (0, 8 * BLOCK + 1), (1, nm), (8 * BLOCK - 1, 3),
                                   (8 * BLOCK + 1, n), (BLOCK, BLOCK), (nm - 1, n), (n - 1, 2)):
                    qi = dict(q, inner=inner_join, start=start, cap=cap)
                    tag = (blocks, name, inner_join, start, cap)
                    want = jrm.answer(m, order, qi, M)
                    assert start or int(want["res"]["n_match"]) == nm, tag
                    monkeypatch.setenv("BMX_SCAN_SUB8_BLOCKS", "1")
                    got8 = jrm.raw(e, qi)
                    monkeypatch.delenv("BMX_SCAN_SUB8_BLOCKS")
                    got1 = jrm.raw(e, qi)
                    for got, form in ((got8, "eight blocks per workgroup"), (got1, "one block per workgroup")):
                        assert jrm.check(got, want, qi) is None, (jrm.check(got, want, qi), tag, form)
                    assert got8["res"].tobytes() == got1["res"].tobytes(), tag
                    for k in ("ids", "vals", "ts", "in_ids", "in_vals", "in_ts"):
                        assert got8[k].tobytes() == got1[k].tobytes(), (k, tag)


def test_small_maps_whose_walks_wrap():
    """64-slot maps: 32 keys on one home, a cluster that wraps from slot 63 to 0, links that walk a whole cluster and miss; 70 keys into 64 slots give up"""
    same = jrm.keys_with_home(5, 64, 33)                               # 32 in the map, one more with the same home that is not
    wrap = jrm.keys_with_home(62, 64, 7, start=10**6)                  # 6 in the map: slots 62, 63, 0, 1, 2, 3
    many = list(range(5000, 5070))
    n = 200
    with bmx.Engine(16 * n) as e:
        m = _by_position(e, n, 3, 800000)
        i = np.arange(n)
        FI, FK = FO[0], FO[1]
        m.set(FI, i, i); m.set(FN[0], i, 7 * i, 20 + i % 5)
        kv = np.array(same[:32] + wrap[:6] + many + same[:32] + wrap[:6], np.int64)     # nodes 108..145 hold the cluster keys a second time
        m.set(FK, i[:146], kv)
        m.set(FL, i, np.array(same + wrap + many[:40] + [12345] * (n - 80), np.int64))   # links: every key of the clusters, the two absent ones, 40 of the many
        wam.load(e, m, [FI, FK, FL, FN[0]])
        order = e.index_ids(FB)
        qs = [Q(FB, EVERY, FL, [FL], FB, [[(FI, 0, 31)]], FK, [FN[0], FI], map_cap=32)]                        # one home
        qs += [Q(FB, EVERY, FL, [FL], FB, [[(FI, 32, 37)]], FK, [FN[0], FI], map_cap=6)]                       # the wrapping cluster
        qs += [Q(FB, EVERY, FL, [FL], FB, [[(FI, 0, 37)], [(FI, 108, 145)]], FK, [FN[0], FI], map_cap=38)]     # both (128 slots), every key on two nodes
        qs += [Q(FB, EVERY, FL, [FL], FB, [[(FI, 0, 31)], [(FI, 108, 139)]], FK, [FN[0], FI], map_cap=32)]     # one home, every key on two nodes
        qs += [Q(FB, EVERY, FL, [FL], FB, [[(FI, 38, 107)]], FK, [FN[0], FI], map_cap=32)]                     # 70 keys into 64 slots
        qs += [Q(FB, EVERY, FL, [FL], FB, [[(FI, 38, 107)]], FK, [FN[0], FI], map_cap=70)]
        qs += [QMAP(FB, EVERY, FL, [FL], same[:32] + same[:32], m.ids[:64][::-1], [FN[0]])]
        flags = []
        for q in qs:
            for inner_join in (False, True):
                got, _ = jrm.ask(e, m, dict(q, inner=inner_join), order)
                flags.append(int(got["res"]["flags"]))
                if q["kind"] == "join":
                    K = int(jrm.answer(m, order, dict(q, map_cap=1 << 12))["res"]["map_size"])
                    for mc in (K, max(K - 1, 1)):
                        g, _ = jrm.ask(e, m, dict(q, inner=inner_join, map_cap=mc), order)
                        assert bool(int(g["res"]["flags"])) == (mc < K)
        assert set(flags) == {0, jrm.MAP_OVERFLOW}


@pytest.mark.parametrize("nkeys", [1, 5])
def test_many_inner_nodes_with_few_keys(nkeys):
    """10^5 inner nodes that hold nkeys keys between them: the smallest unsigned id of each key must come out, with the keys dealt round the lanes and with every
    lane of a wave on one key (positions in runs of 2048)"""
    n, nout = 100_000, 3000
    with bmx.Engine(8 * n) as e:
        m = _by_position(e, n, 3, 900000)
        p = np.arange(n)
        m.set(FL, p[:nout], (p[:nout] * 7) % (2 * nkeys) + 77)           # half of the link values are keys
        m.set(FN[0], p, p * 3 - 4000, 9)
        wam.load(e, m, [FL, FN[0]])
        order = e.index_ids(FB)
        sel = [[(FL, -jrm.VAL_MAX, jrm.VAL_MAX)]]                       # the outer program: the nout nodes that have a link
        key = streams.fnv1a32("jrows.edge.key")
        for ts, keys in ((5, p % nkeys), (6, (p // WAVE) % nkeys)):
            e.put_rows(m.ids, np.full(n, key, np.uint32), np.full(n, ts, np.int64), (keys + 77).astype(np.int64))
            m.set(key, p, keys + 77, ts)
            for inner_join in (False, True):
                got, _ = jrm.ask(e, m, Q(FB, sel, FL, [FL], FB, EVERY, key, [FN[0], key], True, inner_join, map_cap=64), order)
                r = got["res"]
                assert (int(r["map_size"]), int(r["n_inner"]), int(r["n_keyed"])) == (nkeys, n, n) and not int(r["flags"])
                assert int(r["n_joined"]) == nout // 2 and int(r["n_match"]) == (nout // 2 if inner_join else nout)
                want = {int(m.ids[keys == k].min()) for k in range(nkeys)}
                assert set(got["in_ids"][got["in_ids"] != np.uint64(NO_NODE)].tolist()) == want
