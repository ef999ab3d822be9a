"""GPU: update and delete by query (include/bmx_update.h bmx_where_update). Two checks stand side by side after every call, on rows_model.seeded_table() (300
nodes) unless a case needs its own table:
 (i)  against the numpy model of update_model.py: every word of the result record, the ids of the changed rows with their order (into a buffer that held 0x5A
      bytes, checked untouched at and behind n_applied), and the whole state read back: bmx_where_rows with clocks over a select-all program on every field,
      dump_rows and row_count;
 (ii) against a TWIN engine that takes the route that was there before (scan_where ids, get_rows of the source, numpy, then merge_batch(INSERT_DELTA) or
      put_rows): identical dumps, and n_applied equal to the twin's merge.
Every comparison is exact. The geometry of the kernels is test_gpu_where_update_kernel_edges.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
import rows_model as rm
import update_model as um
import where_agg_model as wam
from oracle import streams
from update_model import ADD, COPY, DATA, DELETE, SET, VAL_DELETED

F = rm.names()
FB, F1, F2, F3, NOBODY = F["base"], F["one"], F["two"], F["three"], F["nobody"]
EVERY_FIELD = [FB, F1, F2, F3] + F["more"]
NEVER = streams.fnv1a32("update.never")
EVERY = [[(NEVER, 0, 0, True)]]             # a negated literal on a field nobody has: true for every candidate
BIG = 2**53 - 1
PROG = [[(FB, 0, 6), (F1, 0, 3)], [(F2, 2, 5), (FB, 3, 11)]]


class Rig:
    """the engine under test, its twin and the model, loaded alike"""

    def __init__(self, m=None, tombs=None, fields=EVERY_FIELD, capacity=None, flags=0):
        if m is None:
            m, tombs = rm.seeded_table()
        self.m, self.fields = m, list(fields)
        self.keep = {FB}                      # the indexes that stay; state() drops the others it built (beyond eight indexes none is maintained from the change log)
        cap = capacity or 16 * m.N * (len(fields) + 4)
        self.e, self.twin = bmx.Engine(cap, flags=flags), bmx.Engine(cap, flags=flags)
        for x in (self.e, self.twin):
            wam.load(x, m, fields)
        if tombs:
            for f, idx in tombs.items():
                if len(idx):
                    ts = m.clk[f][idx] + 1000
                    for x in (self.e, self.twin):
                        x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), ts, np.full(len(idx), VAL_DELETED, np.int64))
                    m.tomb(f, idx, ts)

    def close(self):
        self.e.close(); self.twin.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def twin_route(self, order, base, clauses, target, op, operand, src, ts, force, start, cap):
        """ids down, get_rows, numpy, merge_batch or put_rows up -> rows the twin's merge applied"""
        t = self.twin
        ids = t.scan_where(base, clauses)
        pos = {int(i): k for k, i in enumerate(order.tolist())}
        p = np.array([pos[int(i)] for i in ids.tolist()], np.int64)
        keep = np.argsort(p, kind="stable"); keep = keep[p[keep] >= start]
        ids = ids[keep]
        if op == SET:
            vals = np.full(len(ids), operand, np.int64)
        elif op == DELETE:
            vals = np.full(len(ids), VAL_DELETED, np.int64)
        else:
            _, sv, found = t.get_rows(ids, np.full(len(ids), src, np.uint32))
            have = found & (sv != VAL_DELETED)
            ids, sv = ids[have], sv[have]
            vals = sv + (operand if op == ADD else 0)
            ok = (vals >= -BIG) & (vals <= BIG)
            ids, vals = ids[ok], vals[ok]
        ids, vals = ids[:cap], vals[:cap]
        cols = (ids, np.full(len(ids), target, np.uint32), np.full(len(ids), ts, np.int64), vals)
        if force:
            t.put_rows(*cols)
            return len(ids)
        return len(t.merge_batch(*cols, insert_mode=bmx.INSERT_DELTA, want_flags=False)[0])

    def state(self, fields=None):
        """(i) the whole state against the model, (ii) the twin's dump"""
        e, m = self.e, self.m
        fields = self.fields if fields is None else fields
        mine = um.dump_sorted(e)
        assert np.array_equal(mine, um.state_rows(m)), "dump_rows against the model"
        assert np.array_equal(mine, um.dump_sorted(self.twin)), "dump_rows against the twin"
        assert e.row_count() == um.n_rows(m) == self.twin.row_count()
        e.index_size(FB)                      # the base index first: it takes the change log before another index is built
        for f in fields:
            m._f(f)
            if (m.st[f] != um.ABSENT).any():
                order = e.index_ids(f)
                for k in range(0, len(fields), bmx.ROWS_MAX_FIELDS):
                    part = fields[k:k + bmx.ROWS_MAX_FIELDS]
                    r = e.where_rows(f, EVERY, part, with_ts=True)
                    w = rm.rows(m, order, f, EVERY, part, True)
                    assert np.array_equal(r.ids, w[0]) and np.array_equal(r.vals, w[1]) and np.array_equal(r.ts, w[2]), ("where_rows over field", f)
                if f not in self.keep:
                    e.index_drop(f)

    def update(self, base, clauses, target, op, operand=0, src=None, ts=0, force=False, start=0, cap=None, fields=None):
        e = self.e
        order = e.index_ids(base)
        cap = len(order) if cap is None else cap
        want = um.update(self.m, order, base, clauses, target, op, operand, src, ts, force, start, cap)
        got = um.raw_update(e, base, clauses, target, op, operand, src, ts, force, start, cap)
        tag = (clauses, target, op, operand, src, ts, force, start, cap)
        bad = um.same(got, want)
        assert bad is None, (tag, bad)
        assert int(got[1]["next_shard"]) == 0 and int(got[1]["layout"]) != 0
        tw = self.twin_route(order, base, clauses, target, op, operand, src, ts, force, start, cap)
        assert tw == int(got[1]["n_applied"]), (tag, "n_applied of the twin's merge", tw)
        self.m = want[0]
        if target not in self.fields:
            self.fields.append(target)
        self.state(fields)
        return got[1]


# ---- 1. the four ops x default / force, the targets, the sources, the clocks ----
@pytest.mark.parametrize("op,force", [(SET, False), (SET, True), (DELETE, True), (COPY, False), (COPY, True), (ADD, False), (ADD, True)])
def test_ops_targets_sources_and_clocks(op, force):
    """(BMX_UPD_DELETE without BMX_UPD_FORCE is a refusal: test_refusals_leave_the_table_untouched)"""
    seen = set()
    with Rig() as g:
        k = 0
        for src in (F1, FB):                                         # a probed field with all three cell states, and the column
            for target in (FB, F1, NOBODY, src, F3):                 # the base, a program field, a field nobody holds, the source itself, another field
                for ts in (0, 500, 1500, 3000 + k):                  # below, among and above the cells' clocks (1..999; tombstones 1001..1999)
                    r = g.update(FB, PROG, target, op, [3, -1, 0, 1][k % 4], src, ts, force)
                    seen.add((int(r["n_nosrc"]) > 0, int(r["n_applied"]) < int(r["n_sent"]), int(r["n_applied"]) > 0))
                    k += 1
        assert (op in (SET, DELETE)) or any(s[0] for s in seen), "a probed source without data"
        assert force or any(s[1] for s in seen), "a record that lost"
        assert any(s[2] for s in seen)


# ---- 2. equal clocks, the operands, the edges of the value range ----
def _small_table():
    m = um.Table(wam.node_ids(40, 5150))
    i = np.arange(40)
    m.set(FB, i, i % 4, 50)
    m.set(F1, i[:32], np.array([10, 11, 9, BIG - 1, BIG, -BIG + 1, -BIG, 0] * 4), 50)      # the target of the equal-clock cases and the source of the sums
    m.set(F2, i[::2], 7, 50)
    return m, {F2: i[::6]}


def test_equal_clocks_and_the_value_range():
    m, tombs = _small_table()
    with Rig(m, tombs, [FB, F1, F2]) as g:
        for operand in (10, 11, 9, 0, 1, -1, BIG, -BIG):             # clock 50 everywhere: a larger value wins, an equal or smaller one loses
            r = g.update(FB, EVERY, F1, SET, operand, None, 50)
            assert int(r["n_sent"]) == 40
        for ts in (1049, 1050, 1051):                                # a tombstone (clock 1050) loses to ts >= its clock
            r = g.update(FB, EVERY, F2, SET, 5, None, ts)
            assert int(r["n_applied"]) >= (7 if ts >= 1050 else 0)
    m, tombs = _small_table()
    with Rig(m, tombs, [FB, F1, F2]) as g:
        sv = [10, 11, 9, BIG - 1, BIG, -BIG + 1, -BIG, 0] * 4
        for operand in (0, 1, -1, 2, BIG, -BIG):
            n_range = sum(abs(v + operand) > BIG for v in sv)
            assert n_range == {0: 0, 1: 4, -1: 4, 2: 8, BIG: 20, -BIG: 8}[operand]
            for force in (False, True):                              # results exactly at +-(2^53 - 1) are written, one beyond is counted and never written
                r = g.update(FB, EVERY, F3 if force else NOBODY, ADD, operand, F1, 60, force)
                assert (int(r["n_match"]), int(r["n_nosrc"]), int(r["n_range"])) == (40, 8, n_range), (operand, r)
        r = g.update(FB, EVERY, F1, ADD, 1, F1, 70)                  # onto its own source: the snapshot decides, once
        assert int(r["n_range"]) == 4 and int(r["n_applied"]) == 28
        r = g.update(FB, EVERY, FB, ADD, BIG - 3, FB, 70, True)      # the column as source: values 0..3, the sum reaches exactly 2^53 - 1 and the column goes wide
        assert (int(r["n_nosrc"]), int(r["n_range"]), int(r["n_sent"])) == (0, 0, 40)
        r = g.update(FB, EVERY, F2, ADD, 1, FB, 80, True)
        assert int(r["n_range"]) == 10 and int(r["n_sent"]) == 30


# ---- 3. caps, cursors and pages ----
def test_caps_and_pages():
    with Rig() as g:
        order = g.e.index_ids(FB)
        n = um.update(g.m, order, FB, PROG, NOBODY, COPY, 0, F1)[1]["n_sent"]
        assert n > 20
        for k, cap in enumerate((0, 1, n - 1, n, n + 1)):
            r = g.update(FB, PROG, NOBODY, COPY, 0, F1, 100 + k, cap=cap)
            assert int(r["n_sent"]) == min(cap, n)
        first = int(g.update(FB, PROG, NOBODY, COPY, 0, F1, 0, cap=0)["next_pos"])
        assert first == um.records(g.m, order, FB, PROG, NOBODY, COPY, 0, F1)[0][0], "cap 0: the position of the first writable node"
    # pages by cursor add up to the one-shot call: target == base, and a self-selecting program ("set x = 2 where x == 1")
    for prog, target, op, operand, src in ((PROG, FB, ADD, 100, FB), ([[(FB, 1, 1)]], FB, SET, 2, None), ([[(F1, 1, 4)]], F1, ADD, 1, F1)):
        with Rig() as one, Rig() as paged:
            r1 = one.update(FB, prog, target, op, operand, src, 5000)
            start, sent, pages, layout = 0, 0, 0, None
            while True:
                r = paged.update(FB, prog, target, op, operand, src, 5000, start=start, cap=5)
                assert layout in (None, int(r["layout"]))
                layout = int(r["layout"]); sent += int(r["n_sent"]); pages += 1
                if int(r["n_match"]) - int(r["n_nosrc"]) - int(r["n_range"]) <= int(r["n_sent"]):
                    break
                start = int(r["next_pos"])
            assert sent == int(r1["n_sent"]) > 10 and pages == -(-sent // 5)
            assert np.array_equal(um.dump_sorted(one.e), um.dump_sorted(paged.e)) and np.array_equal(um.state_rows(one.m), um.state_rows(paged.m))
    with Rig() as g:
        n = len(g.e.index_ids(FB))
        for start in (n - 1, n, n + 5, 1 << 40):
            r = g.update(FB, EVERY, F3, SET, 1, None, 9000, start=start, cap=4)
            if start >= n:
                assert (int(r["next_pos"]), int(r["n_match"]), int(r["n_sent"])) == (n, 0, 0), "a cursor beyond the index selects nothing"


# ---- 4. refusals ----
def test_refusals_leave_the_table_untouched():
    with Rig() as g:
        e = g.e
        before = um.dump_sorted(e)
        rows = e.row_count()
        ids = np.full(8 * 8, 0x5A, np.uint8); res = np.full(72, 0x5A, np.uint8)
        ip, rp = C.c_void_p(ids.ctypes.data), C.c_void_p(res.ctypes.data)
        prog = bmx._where_args(FB, PROG)
        bad_prog = (FB, 0, prog[2], prog[3])
        for head, tail, code in (
            ((*bad_prog, F1, SET, 0, 1, 5, 0), (0, 8, ip, rp, 0), bmx.ERR_INVALID),
            ((*prog, F1, 4, 0, 1, 5, 0), (0, 8, ip, rp, 0), bmx.ERR_INVALID),
            ((*prog, F1, SET, 0, 1, 5, 2), (0, 8, ip, rp, 0), bmx.ERR_INVALID),
            ((*prog, F1, DELETE, 0, 1, 5, 0), (0, 8, ip, rp, 0), bmx.ERR_INVALID),
            ((*prog, F1, SET, 0, 1, 5, 0), (0, bmx.UPD_MAX_CAP + 1, ip, rp, 0), bmx.ERR_INVALID),
            ((*prog, F1, SET, 0, 1, 5, 0), (0, 8, ip, None, 0), bmx.ERR_INVALID),
            ((*prog, F1, SET, 0, 1, 5, 0), (0, 8, ip, rp, 5), bmx.ERR_INVALID),
            ((*prog, F1, SET, 0, 1, -1, 0), (0, 8, ip, rp, 0), bmx.ERR_RANGE),
            ((*prog, F1, SET, 0, 1, BIG + 1, 1), (0, 8, ip, rp, 1), bmx.ERR_RANGE),
            ((*prog, F1, SET, 0, BIG + 1, 5, 0), (0, 8, ip, rp, 0), bmx.ERR_RANGE),
            ((*prog, F1, ADD, F2, -BIG - 1, 5, 1), (0, 8, ip, rp, 0), bmx.ERR_RANGE),
        ):
            assert e.L.bmx_where_update(e.h, *head, *tail) == code, (head[4:], tail)
            assert e.L.bmx_last_error(e.h)
        with pytest.raises(bmx.BmxError):
            e.where_update(FB, PROG, F1, DELETE, ts=5)
        assert (ids == 0x5A).all() and (res == 0x5A).all(), "a refused call writes nothing"
        assert np.array_equal(um.dump_sorted(e), before) and e.row_count() == rows
        g.state()


# ---- 5. seeded programs ----
@pytest.mark.parametrize("part", [0, 1, 2])
def test_seeded_programs(part):
    cases = rm.seeded_cases(60)[part::3]
    targets = [FB, F1, NOBODY, F2, F["more"][0], F3]
    sources = [FB, F1, F2, F3]
    live = 0
    with Rig() as g:
        for k, (p, _) in enumerate(cases):
            j = 3 * k + part
            op = (SET, COPY, ADD, DELETE)[j % 4]
            force = op == DELETE or j % 3 == 0
            src = sources[(j // 4) % 4]
            target = src if j % 5 == 0 and op in (COPY, ADD) else targets[j % len(targets)]
            r = g.update(FB, p, target, op, [0, 1, -1, BIG, -BIG, 7][j % 6], src, [0, 3, 500, 999, 1500, 2500][(j // 2) % 6], force, [0, 0, 17, 150][j % 4],
                         fields=[FB, target, src] if k % 4 else None)
            live += int(r["n_match"]) > 0
    assert live >= 10


# ---- 6. device memory ----
def test_device_memory_into_poisoned_buffers():
    dev = torch.device("cuda", 0)
    PAT = 0x5A5A5A5A5A5A5A5A
    calls = [(PROG, F3, COPY, 0, F1, 2000, False, 0, 300), (PROG, FB, ADD, 5, FB, 2001, True, 10, 7), (EVERY, NOBODY, SET, 4, None, 7, False, 0, 0),
             ([[(FB, 50, 60)]], F1, SET, 1, None, 9, True, 0, 16), (EVERY, F2, DELETE, 0, None, 2500, True, 150, 300), (EVERY, F2, SET, 3, None, 2400, False, 0, 300)]
    with Rig() as g:
        for p, target, op, operand, src, ts, force, start, cap in calls:
            order = g.e.index_ids(FB)
            want = um.update(g.m, order, FB, p, target, op, operand, src, ts, force, start, cap)
            di = torch.full((cap + 1,), PAT, dtype=torch.int64, device=dev)
            dr = torch.full((10,), PAT, dtype=torch.int64, device=dev)
            g.e.where_update_dev(FB, p, target, op, cap, di, dr, operand=operand, src=src, ts=ts, force=force, start=start)
            g.e.sync()
            rec = dr.cpu().numpy()
            assert rec[9] == PAT, "72 bytes and no more"
            r = rec[:9].view(um.RES_DTYPE)[0]
            ids = di.cpu().numpy().view(np.uint64)
            k = int(r["n_applied"])
            assert um.same((ids[:k], r), want) is None, (target, op, um.same((ids[:k], r), want))
            assert (ids[k:].view(np.int64) == PAT).all() and int(r["reserved"]) == 0 and int(r["next_shard"]) == 0
            g.twin_route(order, FB, p, target, op, operand, src, ts, force, start, cap)
            g.m = want[0]
            if target not in g.fields:
                g.fields.append(target)
            g.state()
        # no ids wanted: a null pointer with room asked for
        dr = torch.full((9,), PAT, dtype=torch.int64, device=dev)
        g.e.where_update_dev(FB, EVERY, F3, SET, 300, None, dr, operand=1, ts=9999)
        g.e.sync()
        assert int(dr.cpu().numpy().view(um.RES_DTYPE)[0]["n_applied"]) == int(g.e.scan_where(FB, EVERY, count_only=True))


# ---- 7. what follows the write ----
def test_indexes_views_and_watches_follow():
    with Rig() as g:
        e, tw = g.e, g.twin
        watch_prog = [[(F3, 40, 49)], [(F3, 0, 2), (FB, 0, 5)]]
        g.keep.add(F3)
        for x in (e, tw):
            x.index_build(F3)
        assert set(e.scan_where(F3, [[(F3, 0, 3)]]).tolist()) == set(g.m.ids[g.m.mask(F3, [[(F3, 0, 3)]])].tolist())
        e.index_set_ordered(F3, 1)
        e.scan_range(F3, 0, 3)
        w = e.watch_create(F3, watch_prog)
        inside = set(e.watch_poll(w).entered.tolist())
        assert inside == set(g.m.ids[g.m.mask(F3, watch_prog)].tolist())
        g.state([FB, F3])
        builds = e.index_refresh_counts()[0]
        for k, (op, operand, src, ts, force) in enumerate(((SET, 44, None, 3000, False), (ADD, 40, F1, 3001, False), (DELETE, 0, None, 3002, True), (COPY, 0, FB, 3003, True))):
            g.update(FB, PROG if k % 2 == 0 else [[(FB, 4, 9)]], F3, op, operand, src, ts, force, fields=[FB, F3])
            for lo, hi in ((0, 3), (40, 49), (-5, 100)):
                want = set(g.m.ids[g.m.mask(F3, [[(F3, lo, hi)]])].tolist())
                assert set(e.scan_where(F3, [[(F3, lo, hi)]]).tolist()) == want, "scan_where on an index of the target"
                assert set(e.scan_range(F3, lo, hi).tolist()) == want, "the value-ordered view on the target"
            p = e.watch_poll(w)
            now = set(g.m.ids[g.m.mask(F3, watch_prog)].tolist())
            assert not p.reset and set(p.entered.tolist()) == now - inside and set(p.left.tolist()) == inside - now, "the standing query over the target"
            inside = now
        assert e.index_refresh_counts()[0] == builds, "the indexes followed through the change log: no rebuild"


# ---- 8. growth and a full table ----
def test_growth_changes_the_layout_of_the_next_call():
    m, tombs = rm.seeded_table()
    grew = 0
    with Rig(m, tombs, capacity=64) as g:
        for k in range(12):
            target = streams.fnv1a32("update.grow%d" % k)
            cap0 = int(g.e.info().capacity_rows)
            r = g.update(FB, EVERY, target, SET, k, None, 10, fields=[FB, target])
            nxt = g.update(FB, EVERY, target, SET, k, None, 5, cap=0, fields=[])      # counts only: no write, the layout as it is now
            if int(g.e.info().capacity_rows) != cap0:
                grew += 1
                assert int(nxt["layout"]) != int(r["layout"]), "the table grew during the merge: the next page's stamp differs"
            else:
                assert int(nxt["layout"]) == int(r["layout"])
            if grew >= 2:
                break
        assert grew >= 1
        g.state()


def test_a_fixed_capacity_context_is_full():
    """300 rows of capacity, never grown; two loads that each found room leave it above that: no merge fits any more, on either route"""
    m, _ = rm.seeded_table()
    with bmx.Engine(300, flags=bmx.CTX_FIXED_CAPACITY) as e:
        wam.load(e, m, [FB, F1])
        assert e.row_count() > 300
        before = um.dump_sorted(e)
        order = e.index_ids(FB)
        for force in (False, True):
            res = np.full(72, 0x5A, np.uint8)
            args = (*bmx._where_args(FB, EVERY), *bmx._upd_args(NOBODY, SET, 1, None, 5000, force), 0, 300, None, C.c_void_p(res.ctypes.data), bmx.MEM_HOST)
            assert e.L.bmx_where_update(e.h, *args) == bmx.ERR_FULL
            assert (res == 0x5A).all()
        with pytest.raises(bmx.BmxError):
            e.put_rows(m.ids[:3], np.full(3, NOBODY, np.uint32), np.full(3, 5, np.int64), np.ones(3, np.int64))
        _, r = um.raw_update(e, FB, EVERY, NOBODY, SET, 1, None, 5000, cap=0)       # counting still works
        assert int(r["n_match"]) == int((m.st[FB] == DATA).sum()) == len(order) and int(r["n_rows"]) == e.row_count()
        assert np.array_equal(um.dump_sorted(e), before)


# ---- 9. the paging helper ----
def test_where_update_all_in_pages_of_seven():
    with Rig() as g:
        order = g.e.index_ids(FB)
        for target, op, operand, src, ts, force in ((F1, ADD, 1, F1, 4000, False), (NOBODY, COPY, 0, F2, 1, False), (F2, DELETE, 0, None, 4001, True)):
            want = um.update(g.m, order, FB, PROG, target, op, operand, src, ts, force)
            r = g.e.where_update_all(FB, PROG, target, op, operand, src, ts, force, page=7)
            assert {k: getattr(r, k) for k in um.WORDS} == {**want[1], "next_pos": len(order)} and r.n_sent > 14 and r.ids is None
            g.twin_route(order, FB, PROG, target, op, operand, src, ts, force, 0, len(order))
            g.m = want[0]
            if target not in g.fields:
                g.fields.append(target)
            g.state()
        r = g.e.where_update(FB, PROG, F3, SET, 3, ts=1 << 40, want_ids=True, cap=4)
        assert r.n_sent == 4 and len(r.ids) == r.n_applied == 4 and np.array_equal(r.ids, g.e.scan_where(FB, PROG)[:4])
