"""GPU: the first N nodes per group (include/bmx_group_top.h bmx_where_group_top). Every answer is compared exactly with gtop_model.answer — a brute force through
Python dicts and ints over the rows the test itself loaded: every byte of every group, row and of res, every cell and clock, the sorted order in host mode, and
the fill pattern behind group D and, on overflow, in every buffer.

The shapes are small: the kernels' geometry (waves, workgroups, ragged units, rounds) is test_gpu_where_group_top_kernel_edges.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import first_model as fm
import group_model as gm
import gtop_model as tm
import where_agg_model as wam
from where_agg_model import DATA, Model

F = tm.names()
FB, FG, FO, FS, NOBODY, F1, F2, F3 = F["base"], F["group"], F["order"], F["select"], F["nobody"], F["one"], F["two"], F["three"]
EVERY = [[(NOBODY, 0, 0, True)]]
BIG, WIDE = fm.BIG, gm.WIDE
POISON = 0x5A5A5A5A5A5A5A5A
EDGE_IDS = np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 2], np.uint64)


def _engine(m, fields, cap=None):
    e = bmx.Engine(cap or max(4 * m.N * len(fields), 1024))
    wam.load(e, m, fields)
    return e


@pytest.fixture(scope="module")
def seeded():
    """the seeded table of first_model on one engine, shared by the tests that only ask"""
    m, tombs = tm.seeded_model()
    e = bmx.Engine(16 * m.N)
    wam.load(e, m, [FB, F1, F2, F3, FG, FO])
    for f, idx in tombs.items():
        wam.tombstone(e, m, f, idx)
    assert e.index_size(FB) == m.N
    yield e, m
    e.close()


# ---- 1. against the forms that exist ----
def test_per_1_equals_the_first_node_per_group_byte_for_byte(seeded):
    e, m = seeded
    for k, (p, group, order, desc) in enumerate(fm.seeded_queries(m)[::5]):
        fields = (order, FB, F1)[: k % 4]
        for cap in (64, 3):
            got = tm.raw_gtop(e, FB, p, group, order, 1, fields, desc, True, cap)
            assert tm.check(got, tm.answer(m, FB, p, group, order, 1, fields, desc, cap, True), cap, 1, len(fields), True) is None
            recs, fvals, fts, fres = fm.raw_first(e, FB, p, group, order, fields, desc, True, cap)
            d = 0 if int(fres["flags"]) else int(fres["n_groups"])
            grps, rows, vals, ts, res = got
            for a in ("n_groups", "flags", "total", "absent", "n_ordered"):
                assert int(res[a]) == int(fres[a])
            for a in ("key", "n_match", "n"):
                assert grps[a][:d].tobytes() == recs[a][:d].tobytes()
            assert rows["id"][:d].tobytes() == recs["id"][:d].tobytes() and rows["val"][:d].tobytes() == recs["val"][:d].tobytes()
            assert vals[:, :d].tobytes() == fvals[:, :d].tobytes() and ts[:, :d].tobytes() == fts[:, :d].tobytes()


def test_one_group_ordered_by_the_base_field_equals_where_top():
    n = 700
    rng = np.random.default_rng(3)
    m = Model(wam.node_ids(n, 81000))
    i = np.arange(n)
    m.set(FB, i, rng.integers(-5, 6, n)); m.set(FG, i, np.full(n, 42)); m.set(F1, i[::2], rng.integers(0, 4, len(i[::2])))
    with _engine(m, (FB, FG, F1)) as e:
        for p in (EVERY, [[(F1, 1, 2)]], [[(FB, -2, 3)], [(F1, 0, 0)]]):
            for desc in (False, True):
                for per in (1, 7, 16):
                    want = tm.ask(e, m, FB, p, FG, FB, per, (FB,), desc, False, 4)
                    top, eligible = e.where_top(FB, p, per, desc=desc)
                    assert int(want[0][0]["n"]) == eligible == int(want[4]["total"]) and len(top) == per
                    assert want[1][0]["id"].tolist() == top["id"].tolist() and want[1][0]["val"].tolist() == top["val"].tolist()


# ---- 2. how many a group has ----
@pytest.mark.parametrize("per", [2, 3, 16])
def test_groups_with_0_1_per_less_one_per_and_per_plus_one_contenders(per):
    sizes = [0, 1, per - 1, per, per + 1]
    m = Model(wam.node_ids(sum(s + 2 for s in sizes), 82000 + per))
    at = 0
    for g, s in enumerate(sizes):                                  # s contenders and two members without an order value per group
        idx = np.arange(at, at + s + 2)
        m.set(FB, idx, idx); m.set(FG, idx, np.full(len(idx), 10 * g - 20)); m.set(FO, idx[:s], (idx[:s] * 7) % 3)
        at += s + 2
    with _engine(m, (FB, FG, FO)) as e:
        for desc in (False, True):
            grps, rows, vals, ts, res = tm.ask(e, m, FB, EVERY, FG, FO, per, (FO, FB), desc, True, 8)
            assert grps["n"].tolist() == sizes and grps["n_rows"].tolist() == [min(per, s) for s in sizes] and grps["n_match"].tolist() == [s + 2 for s in sizes]
            assert int(res["n_rows"]) == sum(min(per, s) for s in sizes) and int(res["per"]) == per
            assert (rows[0]["id"] == np.uint64(tm.NO_NODE)).all() and (vals[:, 0] == tm.VAL_DELETED).all() and (ts[:, 0] == -1).all()


# ---- 3. ties, ids, values ----
@pytest.mark.parametrize("desc", [False, True])
def test_ties_are_decided_by_the_unsigned_id_and_the_cut_falls_inside_them(desc):
    ids = np.concatenate([EDGE_IDS, np.array([12345, 777], np.uint64)])
    m = Model(ids)
    m.set(FB, np.arange(7), np.arange(7))
    m.set(FG, np.arange(7), np.full(7, -3))
    m.set(FO, np.arange(7), [4, 4, 4, 4, 4, -9 if desc else 9, 9 if desc else -9])     # one node in front of the five that tie, one behind them
    with _engine(m, (FB, FG, FO)) as e:
        for per in (1, 2, 3, 4, 5, 6, 7, 8):                         # the cut falls in front of, inside and behind the tie
            rows = tm.ask(e, m, FB, EVERY, FG, FO, per, (FB,), desc, True, 8)[1]
            assert rows[0]["id"][:min(per, 7)].tolist() == ([777] + EDGE_IDS.tolist() + [12345])[:per], "the ids ascend as unsigned numbers, ascending AND descending"
        for first in range(5):                                      # the tie alone, from its member `first` on
            rows = tm.ask(e, m, FB, [[(FB, first, 4)]], FG, FO, 3, (), desc, False, 8)[1]
            assert rows[0]["id"][:min(3, 5 - first)].tolist() == EDGE_IDS[first:first + 3].tolist()


@pytest.mark.parametrize("wide", [False, True])
def test_keys_and_order_values_at_the_ends_of_the_domain(wide):
    vals = np.array([0, 1, -1, BIG, -BIG], np.int64)
    n = 25
    i = np.arange(n)
    m = Model(wam.node_ids(n, 83000))
    m.set(FB, i, vals[i % 5] if wide else i)
    m.set(FG, i, vals[i % 5]); m.set(FO, i, vals[i // 5])
    with _engine(m, (FB, FG, FO)) as e:
        for desc in (False, True):
            order = [-BIG, -1, 0, 1, BIG][::-1 if desc else 1]
            for per in (2, 5, 6):
                grps, rows = tm.ask(e, m, FB, EVERY, FG, FO, per, (FG, FO), desc, True, 8)[:2]
                assert grps["key"].tolist() == [-BIG, -1, 0, 1, BIG] and all(r["val"][:min(per, 5)].tolist() == order[:per] for r in rows)
                tm.ask(e, m, FB, EVERY, FO, FG, per, (), desc, False, 8)
                if wide:
                    tm.ask(e, m, FB, EVERY, FB, FB, per, (FB,), desc, False, 8)


def test_a_smaller_id_member_the_program_rejects_and_one_without_an_order_value():
    ids = np.sort(wam.node_ids(8, 84000))
    m = Model(ids)
    m.set(FB, np.arange(8), [2, 1, 1, 1, 2, 1, 1, 1])               # the smallest id and a middle one are rejected by the program
    m.set(FG, np.arange(8), np.full(8, 7))
    m.set(FO, [0, 1, 3, 4, 5, 6, 7], [5, 5, 5, 5, 5, 5, 5])         # node 2 has no order value
    with _engine(m, (FB, FG, FO)) as e:
        for desc in (False, True):
            for per in (2, 4, 6):
                grps, rows = tm.ask(e, m, FB, [[(FB, 1, 1)]], FG, FO, per, (FO,), desc, False, 8)[:2]
                assert grps.tolist() == [(7, 6, 5, min(per, 5))] and rows[0]["id"][:min(per, 5)].tolist() == [int(x) for x in ids[[1, 3, 5, 6, 7]][:per]]


# ---- 4. where the group and the order value come from ----
@pytest.mark.parametrize("wide", [False, True])
def test_group_and_order_from_column_program_and_unnamed_fields(wide):
    n = 900
    rng = np.random.default_rng(5)
    m = Model(wam.node_ids(n, 85000))
    i = np.arange(n)
    m.set(FB, i, rng.integers(0, 12, n) + (WIDE if wide else 0))
    for f, pr, top in ((F1, 0.8, 6), (F2, 0.7, 4), (FG, 0.8, 9), (FO, 0.7, 5)):
        idx = i[rng.random(n) < pr]
        m.set(f, idx, rng.integers(-2, top, len(idx)))
    lo = WIDE if wide else 0
    prog = [[(F1, 0, 4), (FB, lo + 1, lo + 10)], [(F2, 3, 3)]]
    with _engine(m, (FB, F1, F2, FG, FO)) as e:
        wam.tombstone(e, m, FG, i[::13]); wam.tombstone(e, m, FO, i[::11]); wam.tombstone(e, m, F1, i[::17])
        k = 0
        for group in (FB, F1, FG):
            for order in (FB, F1, FO, F2, group):
                k += 1
                grps, rows = tm.ask(e, m, FB, prog, group, order, (2, 3, 5)[k % 3], (order, group), k % 2 == 1, False, 64)[:2]
                assert len(grps) >= 3
                if order == group:
                    assert (grps["n"] == grps["n_match"]).all() and all((r["val"][:int(g["n_rows"])] == g["key"]).all() for g, r in zip(grps, rows)), "every member ties"


def test_zero_one_and_eight_fields_with_and_without_clocks():
    n = 300
    rng = np.random.default_rng(8)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 86000))
    m.set(FB, i, rng.integers(0, 12, n))
    m.set(FG, i[i % 7 != 0], (i % 5)[i % 7 != 0]); m.set(FO, i[i % 3 != 0], rng.integers(-4, 4, n)[i % 3 != 0]); m.set(F1, i[::2], i[::2] * 3)
    with _engine(m, (FB, FG, FO, F1)) as e:
        wam.tombstone(e, m, F1, i[::6])
        for fields in ((), (FO,), (FB, FG, FO, FO, F1, NOBODY, FB, F1)):
            for with_ts in (False, True):
                for desc, per in ((False, 3), (True, 16)):
                    tm.ask(e, m, FB, [[(FB, 2, 11)]], FG, FO, per, fields, desc, with_ts, 8)
        r = e.where_group_top(FB, EVERY, FG, FO, 4, fields=(FO, F1), with_ts=True, desc=True)
        assert r.vals.shape == (2, 5, 4) == r.ts.shape and r.rows.shape == (5, 4) and (r.vals[0] == r.rows["val"]).all() and r.total == n and r.per == 4
        assert r.n_rows == 20 and list(r.top) == [0, 1, 2, 3, 4] and all(len(v) == 4 for v in r.top.values()) and not r.overflow
        r = e.where_group_top(FB, EVERY, FG, FO, 2)
        assert r.vals.shape == (0, 5, 2) and r.ts is None and [r.top[k] for k in r.top] == [r.rows[g]["id"].tolist() for g in range(5)]


# ---- 5. fit, overflow, one context ----
def test_cap_at_d_and_below_with_an_exact_query_right_behind():
    n = 500
    rng = np.random.default_rng(7)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 87000))
    m.set(FB, i, rng.integers(0, 12, n))
    m.set(FG, i, (i % 37) * 1000003 - 10**7)
    m.set(FO, i[i % 4 != 0], rng.integers(0, 6, n)[i % 4 != 0])
    with _engine(m, (FB, FG, FO)) as e:
        d = 37
        for k, cap in enumerate((d, d - 1, 1, d, 64, 2, 70000, d - 1, d)):
            want = tm.ask(e, m, FB, EVERY, FG, FO, (3, 16, 2)[k % 3], (FO, FB), cap % 2 == 0, True, cap)
            assert int(want[4]["flags"]) == (tm.OVERFLOW if cap < d else 0) and int(want[4]["total"]) == n and int(want[4]["n_ordered"]) == int((i % 4 != 0).sum())
        # per = 16 followed by per = 1, and an overflow followed by per = 16, on one context
        tm.ask(e, m, FB, EVERY, FG, FO, 16, (FO,), False, True, 64)
        tm.ask(e, m, FB, EVERY, FG, FO, 1, (FO,), False, True, 64)
        assert int(tm.ask(e, m, FB, EVERY, FG, FO, 16, (FO,), True, True, 8)[4]["flags"]) == tm.OVERFLOW
        want = tm.ask(e, m, FB, EVERY, FG, FO, 16, (FO,), True, True, 64)
        assert (want[0]["n_rows"] >= 9).all() and (want[0]["n_rows"] < 16).all(), "every group runs out before round 16"
        assert e.where_group_top(FB, EVERY, FG, FO, 3, cap=8).overflow and e.where_group_top(FB, EVERY, FG, FO, 3, cap=8).n_rows == 0


def test_device_mode_into_poisoned_buffers():
    n = 8192 + 300
    rng = np.random.default_rng(9)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 88000))
    m.set(FB, i, rng.integers(0, 2000, n))
    idx = i[rng.random(n) < 0.8]; m.set(FG, idx, rng.integers(-BIG, BIG, 1500)[rng.integers(0, 1500, len(idx))])
    idx = i[rng.random(n) < 0.6]; m.set(FO, idx, rng.integers(-3, 3, len(idx)))
    deep = [[(FB, 100, 1800)], [(FO, 0, 3, True), (FB, 0, 50)]]
    dev = torch.device("cuda", 0)
    queries = [(deep, FG, FO, 3, (FO, FB), False, 2048), (deep, FG, FO, 5, (FO,), True, 16), ([[(FB, 5000, 6000)]], FG, FO, 2, (FO,), False, 16), (deep, FB, FG, 4, (), True, 2048)]
    with _engine(m, (FB, FG, FO)) as e:
        wam.tombstone(e, m, FG, np.nonzero(m.st[FG] == DATA)[0][::10])
        bufs = []
        for p, g, o, per, fields, desc, cap in queries:
            nf, stride = len(fields), cap * per
            bufs.append((torch.full((4 * (cap + 1),), POISON, dtype=torch.int64, device=dev), torch.full((2 * (stride + per),), POISON, dtype=torch.int64, device=dev),
                         torch.full((nf * stride + per,), POISON, dtype=torch.int64, device=dev), torch.full((nf * stride + per,), POISON, dtype=torch.int64, device=dev),
                         torch.full((6,), POISON, dtype=torch.int64, device=dev)))
        for (p, g, o, per, fields, desc, cap), (out, rows, val, ts, res) in zip(queries, bufs):   # enqueued back to back, one synchronisation at the end
            e.where_group_top_dev(FB, p, g, o, per, out, rows, val, ts, res, fields=fields, desc=desc, cap=cap)
        e.sync()
        seen = []
        for (p, g, o, per, fields, desc, cap), (out, rows, val, ts, res) in zip(queries, bufs):
            nf, stride = len(fields), cap * per
            v, t = val.cpu().numpy(), ts.cpu().numpy()
            assert (v[nf * stride:] == POISON).all() and (t[nf * stride:] == POISON).all()
            gv = np.full((nf, stride + per), POISON, np.int64); gt = gv.copy()
            for f in range(nf):
                gv[f, :stride] = v[f * stride:(f + 1) * stride]; gt[f, :stride] = t[f * stride:(f + 1) * stride]
            got = (out.cpu().numpy().view(tm.GRP_DTYPE), rows.cpu().numpy().view(tm.ROW_DTYPE), gv, gt, res.cpu().numpy().view(tm.RES_DTYPE)[0])
            want = tm.answer(m, FB, p, g, o, per, fields, desc, cap, True)
            bad = tm.check(got, want, cap, per, nf, True, host=False)
            assert bad is None, bad
            seen.append((int(want[4]["flags"]), len(want[0])))
        assert seen[0][1] > gm.CACHE and seen[1][0] == 1 and seen[2][1] == 0 and seen[3][1] > 100


def test_the_other_grouped_forms_interleaved_on_the_same_context():
    n = 2000
    rng = np.random.default_rng(10)
    i = np.arange(n)
    m = Model(wam.node_ids(n, 89000))
    m.set(FB, i, rng.integers(0, 12, n)); m.set(FG, i[i % 9 != 0], rng.integers(0, 40, n)[i % 9 != 0] * 77 - 1000); m.set(FO, i[i % 5 != 0], rng.integers(0, 8, n)[i % 5 != 0])
    m.set(F1, i, i % 40 * 77 - 1000); m.set(F2, i, (i % 40) % 5 - 2)
    p = [[(FB, 1, 9)]]
    with _engine(m, (FB, FG, FO, F1, F2)) as e:
        g0 = e.where_group(FB, p, FG, FO, cap=64).records.tobytes()
        j0 = e.where_join_group(FB, p, FG, FB, EVERY, F1, F2, measure=FO, cap=64, map_cap=4096)
        for cap in (64, 8, 64):
            tm.ask(e, m, FB, p, FG, FO, 5, (FO,), cap == 8, True, cap)
            fm.ask(e, m, FB, p, FG, FO, (FO,), cap != 8, True, cap)
            tm.ask(e, m, FB, p, FG, FO, 16, (), False, False, cap)
            recs, res = gm.ask(e, m, FB, p, FG, FO, 64)
            assert recs.tobytes() == g0
            tm.ask(e, m, FB, p, FG, FO, 2, (), True, False, cap)
            j1 = e.where_join_group(FB, p, FG, FB, EVERY, F1, F2, measure=FO, cap=64, map_cap=4096)
            assert j1.records.tobytes() == j0.records.tobytes() and len(j0.records) > 2
            assert gm.raw_group(e, FB, p, FG, FO, cap=4)[1]["flags"] == bmx.GROUP_OVERFLOW       # a group-by that overflows right in front
            tm.ask(e, m, FB, p, FG, FO, 3, (FO,), True, False, 64)
            assert int(fm.ask(e, m, FB, p, FG, FO, (), False, False, 4)[3]["flags"]) == fm.OVERFLOW   # ... and a first-node query that does
            tm.ask(e, m, FB, p, FG, FO, 3, (FO,), False, False, 64)


# ---- 6. a living table ----
def test_a_living_table():
    rng = np.random.default_rng(11)
    N0, EXTRA, PER = 8192 + 5, 200, 4
    m = Model(wam.node_ids(N0 + EXTRA, 90000))
    old = np.arange(N0)
    m.set(FB, old, rng.integers(0, 12, N0))
    pool = rng.integers(-BIG, BIG, 30)
    idx = old[rng.random(N0) < 0.8]; m.set(FG, idx, pool[rng.integers(0, 30, len(idx))])
    idx = old[rng.random(N0) < 0.7]; m.set(FO, idx, rng.integers(10, 1000, len(idx)))
    idx = old[rng.random(N0) < 0.9]; m.set(F1, idx, rng.integers(0, 6, len(idx)))
    progs = [[[(F1, 1, 3), (FB, 2, 9)]], [[(F1, 0, 1)], [(FO, 500, 1000), (FB, 0, 5)]], EVERY]
    dev = torch.device("cuda", 0)

    def ask(e):
        out = []
        for k, p in enumerate(progs):
            out += [tm.ask(e, m, FB, p, FG, FO, PER, (FO, FB), bool(k % 2), False, 64), tm.ask(e, m, FB, p, FB, FO, 2, (), not k % 2, False, 64),
                    tm.ask(e, m, FB, p, F1, FB, 3, (FG,), False, False, 8)]
        return out

    def same(a, b):
        return all(tm.same_answer(x, y) for x, y in zip(a, b))

    def merge(e, f, idx, vals, ts):
        idx = np.asarray(idx)
        e.merge_batch(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts, np.int64), np.asarray(vals, np.int64), want_flags=False)
        m.set(f, idx, vals)

    with _engine(m, (FB, FG, FO, F1), 8 * (N0 + EXTRA)) as e:
        first = ask(e)
        assert all(len(a[0]) >= 2 for a in first)
        # a merge that puts another member in front of rank 1 of one group: ranks 2 .. per are the old ranks 1 .. per - 1
        w = first[6]                                                # EVERY, ascending, grouped by FG
        g = 3
        key = int(w[0][g]["key"]); r = w[1][g]
        assert int(w[0][g]["n"]) > PER + 2
        top_nodes = m.index_of(r["id"].copy())
        members = np.nonzero((m.st[FG] == DATA) & (m.val[FG] == key) & (m.st[FB] == DATA) & ~np.isin(np.arange(m.N), top_nodes))[0]
        other = int(members[0])
        merge(e, FO, [other], [int(r[0]["val"]) - 1], 100)
        r1 = tm.ask(e, m, FB, EVERY, FG, FO, PER, (FO,), False, False, 64)[1][g]
        assert r1["id"].tolist() == [int(m.ids[other])] + r["id"].tolist()[:PER - 1]
        # a tombstone on the order field of the node that is now rank 3: everybody behind it moves up, ranks 1 and 2 stay
        wam.tombstone(e, m, FO, [int(top_nodes[1])], ts=200)
        r2 = tm.ask(e, m, FB, EVERY, FG, FO, PER, (FO,), False, False, 64)[1][g]
        assert r2["id"].tolist()[:3] == [int(m.ids[other]), int(r[0]["id"]), int(r[2]["id"])]
        # ... and one on the group field of the old rank 1: it leaves the group
        wam.tombstone(e, m, FG, [int(top_nodes[0])], ts=200)
        w3 = tm.ask(e, m, FB, EVERY, FG, FO, PER, (FO,), False, False, 64)
        assert int(r[0]["id"]) not in w3[1][g]["id"].tolist() and int(w3[4]["absent"]) == int(w[4]["absent"]) + 1
        # new rows, then growth
        new = np.arange(N0, N0 + EXTRA)
        merge(e, FB, new, rng.integers(0, 12, EXTRA), 101); merge(e, FG, new[::2], pool[rng.integers(0, 30, len(new[::2]))], 101); merge(e, FO, new, rng.integers(0, 12, EXTRA), 101)
        second = ask(e)
        assert e.index_size(FB) == N0 + EXTRA and not same(first, second)
        e.reserve(32 * (N0 + EXTRA))
        assert same(ask(e), second)
        # a value-ordered view on the base field: the same answers, and the view's counters untouched
        e.index_set_ordered(FB, 1)
        assert set(e.scan_range(FB, 2, 9).tolist()) == set(m.ids[m.mask(FB, [[(FB, 2, 9)]])].tolist())
        assert e.index_ordered_info(FB)[1], "the view answers"
        s0 = e.index_ordered_stats(FB)
        assert same(ask(e), second)
        assert e.index_ordered_stats(FB) == s0 and e.index_ordered_info(FB)[1], "the calls leave the view as it was"
        e.index_set_ordered(FB, 0)
        # deferred compaction (switched on explicitly): a device batch large enough to defer, asked right behind it
        e.set_deferred(True)
        nb = 65_536
        fields = np.array([FB, F1, FG, FO, F2, F3, FS, F["extra"]], np.uint32)      # 8 x N0 distinct (node, field) keys >= nb
        keys = rng.permutation(len(fields) * N0)[:nb]
        kn, kf = keys % N0, fields[keys // N0]
        kv = np.where(kf == FB, rng.integers(0, 12, nb), np.where(kf == FG, pool[rng.integers(0, 30, nb)] - 1, rng.integers(0, 6, nb))).astype(np.int64)
        cols = (torch.from_numpy(m.ids[kn].view(np.int64)).to(dev), torch.from_numpy(kf.view(np.int32)).to(dev),
                torch.full((nb,), 300, dtype=torch.int64, device=dev), torch.from_numpy(kv).to(dev))
        applied = torch.zeros(nb, dtype=torch.int32, device=dev); n_applied = torch.zeros(1, dtype=torch.int64, device=dev)
        d0 = e.deferred_counts()[0]
        e.merge_batch_dev(nb, *cols, bmx.INSERT_REFERENCE, applied=applied, n_applied=n_applied)
        for f in fields:
            m.set(int(f), kn[kf == f], kv[kf == f])
        tm.ask(e, m, FB, progs[1], FG, FO, PER, (FO,), True, False, 256)
        assert e.deferred_counts()[0] == d0 + 1 and int(n_applied.item()) == nb
        ask(e)
        # a base value beyond int32: the index switches to its int64 column
        merge(e, FB, [7, N0 + 3], np.array([WIDE, -(2**35)]), 2000)
        ask(e)
        grps = tm.ask(e, m, FB, [[(FB, 2**39, wam.I64MAX)], [(FB, wam.I64MIN, -(2**33))]], FB, FB, 2, (FB,), False, False, 8)[0]
        assert grps["key"].tolist() == [-(2**35), WIDE]


# ---- 7. seeded programs ----
@pytest.mark.parametrize("per", tm.PERS)
def test_seeded_programs(seeded, per):
    """the 60 programs of gtop_model.seeded_queries for this per; each has a tie at the cut, a short group, a group without a contender and a tie on an extreme
    (test_gtop_model.py asserts it on the model); every fourth also with cap = 2 directly in front: an overflowing query leaves the state clean for the next"""
    e, m = seeded
    qs = tm.seeded_queries(m, per)
    assert len(qs) == 60
    overflows = 0
    for k, (p, group, order, desc) in enumerate(qs):
        if k % 4 == 2:
            overflows += int(tm.ask(e, m, FB, p, group, order, per, (order,), desc, True, 2)[4]["flags"])
        want = tm.ask(e, m, FB, p, group, order, per, (order, FB, group)[: 1 + k % 3], desc, bool(k % 2), 64)
        assert int(want[4]["total"]) == e.scan_where(FB, p, count_only=True) and int(want[4]["flags"]) == 0
    assert overflows >= 10
