"""No GPU: the arithmetic of tests/test_gpu_merge_kernel_edges.py itself — its constructed ids, its layout cases, its list positions and scenarios, its padding
records, its batches around the epoch wrap and the checks it makes — run against a stand-in engine in plain numpy and python. The stand-in places every key
by the restated probe sequence of slot.h (test_gpu_lookup_edges.Model), resolves a batch key by key in index order by the reference's rule, links the deltas
of one key through a next[] array that carries the batch epoch as the device's does (the smallest index stands for the first claimer), ranks the winners
from per-256-delta counts as the compaction does, grows by re-inserting its rows, and answers merge_batch, merge_batch_dev, merge_records_dev, put_rows,
load_rows, get_rows, get_row, dump_rows (slot order), row_count and info() from its own table.

It proves nothing about a kernel. It proves that every constructed id lands in the line its case names, that every case fits its table, that every tag of
the suite's list is reached by the cases that claim it — and, with stand-ins that carry one defect each, that the GPU suite's checks fail on a subtly wrong
engine. The batch of 2^20 + 4097 deltas is built and its arithmetic checked, but no stand-in runs it."""
import numpy as np
import pytest

import bmx
import test_gpu_sync_kernel_edges as edges
import test_gpu_lookup_edges as lk
import test_gpu_merge_kernel_edges as mk

EMPTY = lk.EMPTY
IDX_BITS, IDX_MASK, EPOCH_MAX = 24, (1 << 24) - 1, 255
INCOMING, CURRENT, HISTORICAL = bmx.FLAG_INCOMING, bmx.FLAG_CURRENT, bmx.FLAG_HISTORICAL


class Info:
    pass


class Stats:
    pass


class Fake:
    defect = None

    def __init__(self, capacity_rows, device=0, flags=0, load_pct=0):
        assert load_pct == 90 and flags in (0, bmx.CTX_FIXED_CAPACITY)
        self.cap, self.fixed = capacity_rows, bool(flags)
        self.m = lk.Model(edges.slots_for(capacity_rows, 90), 4)
        self.where = {}                                  # key -> slot
        self.epoch = 0
        self.next = np.zeros(1 << 16, np.uint32)
        self.waves, self.nrows = 8, 0

    def __enter__(self): return self
    def __exit__(self, *a): pass
    def close(self): pass
    def sync(self): pass

    def set_probe_waves(self, w):
        assert w in (8, 6, 5, 4, 3)
        self.waves = w

    def info(self):
        i = Info(); i.n_slots, i.epoch = self.m.nslots, self.epoch
        return i

    # ---- the table ----
    def _free_slot(self, id, field):
        """where a key that has no row lands; None: the defective spill found no line"""
        m = self.m
        if self.defect == "the spill stops at the last line":
            nl = m.nslots // 4
            line, c = divmod(lk.home(id, field, m.nslots, 4), 4)
            while line < nl:
                for k in range(4):
                    if m.id[line * 4 + ((c + k) & 3)] == EMPTY:
                        return line * 4 + ((c + k) & 3)
                line += 1
            return None
        if self.defect == "first empty slot, not looking past the node's other fields":
            line, c = divmod(lk.home(id, field, m.nslots, 4), 4)
            for p in range(m.nslots):                    # the first empty slot of the walk, whatever lies in front of it
                if m.id[line * 4 + ((c + p) & 3)] == EMPTY:
                    return line * 4 + ((c + p) & 3)
                if (p + 1) & 3 == 0:
                    line = 0 if line + 1 == m.nslots // 4 else line + 1
            return None
        return m.find(id, field)[1]

    def _slot(self, id, field):
        """-> the key's slot or None"""
        if self.defect == "first empty slot, not looking past the node's other fields":
            m = self.m                                   # the walk gives up looking for the key's row once it has met another field of its node
            line, c = divmod(lk.home(id, field, m.nslots, 4), 4)
            for p in range(m.nslots):
                s = line * 4 + ((c + p) & 3)
                if m.id[s] == EMPTY or (m.id[s] == id and m.field[s] != field):
                    return None
                if m.id[s] == id and m.field[s] == field:
                    return s
                if (p + 1) & 3 == 0:
                    line = 0 if line + 1 == m.nslots // 4 else line + 1
            return None
        return self.where.get((id, field))

    def _create(self, id, field):
        s = self._free_slot(id, field)
        if s is None:
            return None
        m = self.m
        m.id[s], m.field[s] = id, field
        self.where[(id, field)] = s
        self.nrows += 1
        return s

    def _rows(self):
        return self.nrows

    def _room(self, n):
        rows = self._rows()
        if rows + n < self.m.nslots and rows <= self.cap:
            return
        if self.fixed:
            raise bmx.BmxError(bmx.ERR_FULL, "full")
        old = self.m
        self.cap = max(self.cap * 2, rows + n + n // 2)
        self.m = lk.Model(edges.slots_for(self.cap, 90), 4)
        self.where = {}
        for s, id, f, ts, val in old.rows():             # k_rehash: every row again, in slot order
            k = self.m.put(id, f, ts, val)
            self.where[(id, f)] = k

    # ---- one batch ----
    def _merge(self, id, field, ts, val, imode, force=False):
        """-> (applied u32 ascending with the creation marks, flags u8[n], stats)"""
        id = np.asarray(id, np.uint64).tolist(); field = np.asarray(field, np.uint32).tolist(); ts = np.asarray(ts, np.int64).tolist(); val = np.asarray(val, np.int64).tolist()
        n = len(id)
        rule, strict, unique, mark = imode & 1, bool(imode & mk.STRICT), bool(imode & mk.UNIQUE), bool(imode & mk.MARK)
        st = Stats(); st.n_applied = st.n_conflicts = 0; st.n_rows = self._rows()
        flags = np.zeros(n, np.uint8)
        if n == 0:
            return np.zeros(0, np.uint32), flags, st
        assert all(0 <= t <= edges.TS_MAX for t in ts) and n <= 1 << IDX_BITS
        self._room(n)
        self.epoch += 1
        if self.epoch > EPOCH_MAX:
            self.epoch = 1
            if self.defect != "a stale link of the previous epoch cycle is followed":
                self.next[:] = 0
        if n > len(self.next):
            self.next = np.concatenate([self.next, np.zeros(max(n, 2 * len(self.next)) - len(self.next), np.uint32)])
        ep, nxt, m = self.epoch, self.next, self.m
        groups = {}
        for j in range(n):
            if id[j] != EMPTY:                           # a padding record takes no part
                groups.setdefault((id[j], field[j]), []).append(j)
        assert not unique or all(len(g) == 1 for g in groups.values())
        for g in groups.values():
            for a, b in zip(g, g[1:]):
                nxt[a] = (ep << IDX_BITS) | b
        winner = np.zeros(n, bool); created_by = np.zeros(n, bool)
        counts = np.zeros((n + 255) // 256, np.int64)     # winners per 256-delta block, as the probe kernel left them and the resolve pass moved them
        for key, g in groups.items():
            chain, x = [g[0]], int(nxt[g[0]])
            while x >> IDX_BITS == ep and len(chain) <= n:
                chain.append(x & IDX_MASK); x = int(nxt[x & IDX_MASK])
            chain.sort()
            s = self._slot(*key)
            cur = None if s is None else (m.ts[s], m.val[s])
            pre, owner, base = cur, None, None
            for j in chain:
                tv = (ts[j], val[j])
                if force:
                    cur, owner, fl = tv, j, INCOMING
                elif cur is None:
                    own = self.defect == "a created row stores its own clock under the reference rule"
                    cur, owner, fl = ((2 if rule == mk.REF and not own else ts[j]), val[j]), j, INCOMING
                    created_by[j] = True
                elif tv > cur:
                    cur, owner, fl = tv, j, INCOMING
                elif tv == cur:
                    fl = 0
                    if self.defect == "a tie goes to the larger index" and owner is not None:
                        owner = j
                else:
                    fl = CURRENT | (HISTORICAL if ts[j] < cur[0] else 0)
                if j < n:
                    flags[j] = fl
                if j == chain[0]:
                    base = owner                          # what the first claimer did on its own
            st.n_conflicts += len(chain) - 1 if (strict or pre is None) else max(0, sum(1 for j in chain if (ts[j], val[j]) >= pre) - 1)
            if owner is not None:
                if s is None:
                    s = self._create(*key)
                if s is not None:
                    m.ts[s], m.val[s] = cur
                winner[owner] = True
                moved = self.defect == "the winner mark moves but the block count does not" and base is not None
                counts[(base if moved else owner) >> 8] += 1
        if self.defect == "padding records are counted as winners":
            for j in range(n):
                if id[j] == EMPTY:
                    winner[j] = True; counts[j >> 8] += 1
        out = {}
        total = 0
        for blk in range((n + 4095) // 4096):            # k_compact_winners: a 4096-delta block ranks its winners behind the counts in front of it
            off = int(counts[:blk * 16].sum())
            w = np.flatnonzero(winner[blk * 4096:(blk + 1) * 4096]) + blk * 4096
            for i, j in enumerate(w.tolist()):
                out[off + i] = j
            total = off + len(w)
        applied = np.zeros(total, np.uint32)
        for p, j in out.items():
            if p < total:
                applied[p] = j | (bmx.APPLIED_CREATED if mark and created_by[j] else 0)
        st.n_applied, st.n_rows = total, self._rows()
        return applied, flags, st

    def load_rows(self, id, field, ts, val): self._merge(id, field, ts, val, mk.DELTA)
    def put_rows(self, id, field, ts, val): self._merge(id, field, ts, val, mk.DELTA | mk.UNIQUE, force=True)

    def merge_batch(self, id, field, ts, val, insert_mode=bmx.INSERT_REFERENCE, want_flags=True):
        a, fl, st = self._merge(id, field, ts, val, insert_mode)
        return a, (fl if want_flags else None), st

    def _out(self, r, applied, n_applied, flags, stats):
        a, fl, st = r
        applied.numpy()[:len(a)] = a.view(np.int32); n_applied[0] = len(a)
        flags.numpy()[:len(fl)] = fl
        stats[0], stats[1], stats[2] = int(st.n_applied), int(st.n_conflicts), int(st.n_rows)

    def merge_batch_dev(self, n, id, field, ts, val, insert_mode=bmx.INSERT_REFERENCE, applied=None, n_applied=None, flags=None, stats=None):
        self._out(self._merge(id.numpy().view(np.uint64)[:n], field.numpy().view(np.uint32)[:n], ts.numpy()[:n], val.numpy()[:n], insert_mode), applied, n_applied, flags, stats)

    def merge_records_dev(self, n, recs, insert_mode=bmx.INSERT_REFERENCE, applied=None, n_applied=None, flags=None, stats=None):
        r = recs.numpy().reshape(-1).view(bmx.DELTA_REC_DTYPE)[:n]
        self._out(self._merge(r["id"], r["field"], r["ts"], r["val"], insert_mode), applied, n_applied, flags, stats)

    # ---- reads ----
    def get_row(self, id, field):
        s = self.m.find(int(id), int(field))[0]           # (the read-only lookup is another kernel: no defect of the write path reaches it)
        return None if s is None else (self.m.ts[s], self.m.val[s])

    def get_rows(self, id, field):
        r = [self.get_row(i, f) for i, f in zip(np.asarray(id, np.uint64).tolist(), np.asarray(field, np.uint32).tolist())]
        return (np.asarray([0 if x is None else x[0] for x in r], np.int64), np.asarray([0 if x is None else x[1] for x in r], np.int64), np.asarray([x is not None for x in r], bool))

    def row_count(self): return self._rows()

    def dump_rows(self):
        r = self.m.rows(tombstones=False)
        return (np.asarray([x[1] for x in r], np.uint64), np.asarray([x[2] for x in r], np.uint32), np.asarray([x[3] for x in r], np.int64), np.asarray([x[4] for x in r], np.int64))


def _defective(what):
    return type("Wrong", (Fake,), {"defect": what})


@pytest.fixture
def standin(monkeypatch):
    monkeypatch.setattr(bmx, "Engine", Fake)
    monkeypatch.setattr(mk, "DEVICE", "cpu")
    return monkeypatch


# ---- the constructions ----

def test_every_case_lands_in_its_lines_fits_its_table_and_reaches_its_tags():
    cases = mk.layout_cases()
    assert len({c.name for c in cases}) == len(cases)
    assert {"home", "cross", "wrap", "two_full", "own_fields", "node_spill", "two_nodes", "two_nodes_2w", "same_key", "same_key_split", "resident_far"} == {c.name for c in cases}
    m = lk.lay(cases, 4)                                  # asserts the line of every resident row
    lines = {}
    seen = set()
    for c in cases:
        before = m.rows()
        created, tags = mk.place(m, c)                    # asserts the line of every created row whose line is determined
        for id, f, expect in c.probes:                    # the absent probe keys, behind the batch
            s, _, tg = m.find(id, f)
            assert s is None and expect <= tg, (c.name, "probe", sorted(expect), sorted(tg))
            assert lk.home(id, f, mk.NSLOTS, 4) // 4 in {lk.home(d[0], d[1], mk.NSLOTS, 4) // 4 for d in c.deltas}, (c.name, "the probe shares a home line with the case")
            tags |= tg
        assert c.claims <= tags, (c.name, "claims", sorted(c.claims - tags))
        seen |= tags
        mine = {r[0] // 4 for r in m.rows() if (r[1], r[2]) in set(created) | {w[:2] for w in c.writes}}
        for other, ls in lines.items():
            assert not (mine & ls), (c.name, other, "share a line")
        lines[c.name] = mine
        assert len(c.deltas) <= 300 and (c.dups or len(set(d[:2] for d in c.deltas)) == len(c.deltas))
        if c.name == "resident_far":
            assert not created and before == m.rows()
    assert len(m.rows()) <= edges.capacity_for(mk.NSLOTS) and edges.slots_for(edges.capacity_for(mk.NSLOTS), 90) == mk.NSLOTS
    assert seen >= set(mk.LAYOUT_TAGS), sorted(set(mk.LAYOUT_TAGS) - seen)
    by = {c.name: c for c in cases}
    # what the case names promise, from the model
    assert {lk.home(d[0], d[1], mk.NSLOTS, 4) // 4 for d in by["wrap"].deltas} == {mk.NL - 1} and set(by["wrap"].dlines) == {0}
    n9 = by["node_spill"].deltas
    assert len(n9) == 9 and len({d[0] for d in n9}) == 1 and sorted(m.find(d[0], d[1])[0] // 4 - 208 for d in n9) == [0] * 4 + [1] * 4 + [2]
    own = by["own_fields"]
    assert sorted(m.find(d[0], d[1])[0] // 4 - 160 for d in own.deltas[1:]) == [0, 1, 1, 1] and m.find(*own.deltas[0][:2])[0] == 4 * 160 + 2
    for name in ("two_nodes", "two_nodes_2w"):
        d = by[name].deltas[-6:]
        assert len({x[0] for x in d}) == 2 and sorted(m.find(x[0], x[1])[0] // 4 - lk.home(x[0], x[1], mk.NSLOTS, 4) // 4 for x in d) == [0, 0, 0, 0, 1, 1]
    assert [len(by[n].deltas) - 6 for n in ("two_nodes", "two_nodes_2w")] == [0, 61], "a's fields in lanes 61..63 of wave 0, b's in lanes 0..2 of wave 1"
    sk = by["same_key_split"].deltas
    assert len(set(x[:2] for x in sk[63:])) == 1 and len(sk) == 127 and sk[63][:2] not in {x[:2] for x in sk[:63]}, "the first occurrence in lane 63 of wave 0"
    assert len(by["same_key"].deltas) == 64 and len({x[:2] for x in by["same_key"].deltas}) == 1


def test_the_list_positions_scenarios_and_padding_reach_their_tags():
    seen = set()
    for name, (pos, n) in mk.POSITIONS.items():
        assert pos == sorted(set(pos)) and pos[-1] < n and n % 256 == 1
        for rule in (mk.REF, mk.DELTA):
            for sname, start, values, claims in mk.scenarios(len(pos)):
                assert len(values) == len(pos)
                tags = mk.list_tags(pos, start, values, rule)
                assert set(claims) <= tags, (name, sname, claims, tags)
                seen |= tags
        b = mk.list_batch(pos, n, mk.synth.splitmix64_np(np.arange(1, n + 1, dtype=np.uint64)), 3, 12345, mk.scenarios(len(pos))[0][2])
        assert len(set(b[0].tolist())) == n - len(pos) + 1 and 0.4 * n < (b[2] > 10).sum() < 0.6 * n
    assert mk.POSITIONS["255_256"][0] == [255, 256] and mk.POSITIONS["0_4095_4096"][0] == [0, 4095, 4096] and mk.POSITIONS["63_64_300"][0] == [63, 64, 300]
    s70 = mk.spread70()
    assert len(s70) == 70 and [p >> 8 for p in s70] == list(range(70))
    assert {257, 4097, 8193} <= {n for _, n in mk.POSITIONS.values()}
    # absent starts under the reference rule: clocks below, at and above the 2 a created row stores
    clocks = {tv[0] for _, start, values, _ in mk.scenarios(3) if start is None for tv in values}
    assert {0, 1, 2, 3} <= clocks
    pos, N = mk.pad_positions(130)
    pads = sorted(set(range(N)) - set(pos.tolist()))
    assert pads == [64, N - 1] and N == 132
    if pads[0] % 64 == 0:
        seen.add("padding at a wave border")
    assert mk.pad_positions(64)[1] == 65 and mk.pad_positions(3)[1] == 4
    assert any(len(c.deltas) > 64 for c in mk.layout_cases()), "a layout batch long enough to carry the padding at the wave border"
    if (mk.BIG_N - 1) // 4096 * 16 > mk.PREFIX_ROUND // 256 and (1 << 20) // 4096 * 16 <= mk.PREFIX_ROUND // 256:
        seen.add("prefix second round")
    assert seen >= set(mk.LIST_TAGS + mk.OTHER_TAGS), sorted(set(mk.LIST_TAGS + mk.OTHER_TAGS) - seen)
    assert set(mk.TAGS) == set(mk.LAYOUT_TAGS + mk.LIST_TAGS + mk.OTHER_TAGS)


def test_the_big_batch_and_the_epoch_batches():
    res, b = mk.big_batch()
    n = mk.BIG_N
    assert len(b[0]) == n and len(np.unique(b[0])) == n - 1 and b[0][0] == b[0][n - 1] and len(np.unique(res[0])) == n - 1
    assert np.isin(b[0], res[0]).all(), "every key is resident"
    assert ((b[2] > 10) == (np.arange(n) % 3 == 0))[1:n - 1].all() and (0 >> 8, (n - 1) >> 8) == (0, (n + 255) // 256 - 1)
    lists, u255, u1 = mk.epoch_batches()
    for u in (u255, u1):
        assert len(u[0]) == mk.EPOCH_N == len(np.unique(u[0])) and not np.isin(u[0], lists[0]).any()
    ids, cnt = np.unique(lists[0], return_counts=True)
    dup = ids[cnt > 1]
    assert len(dup) == mk.EPOCH_LISTS and (cnt[cnt > 1] == mk.EPOCH_LEN + 1).sum() + (cnt[cnt > 1] == mk.EPOCH_LEN).sum() == mk.EPOCH_LISTS
    first = [int(np.flatnonzero(lists[0] == d)[0]) for d in dup]
    assert min(first) > 4096, "every member of every list, so every first claimer, sits above index 4096"


# ---- the suite's own tests on the stand-in ----

LAYOUT = [p for p in mk.layout_params() if p.values[3] == 8 or p.values[:3] == ("recs", mk.REF, 0)]      # (the stand-in has no occupancy: the waves only pass through)


@pytest.mark.parametrize("variant,rule,mode,waves", LAYOUT)
def test_layout_cases(standin, variant, rule, mode, waves):
    mk.test_layout_cases(variant, rule, mode, waves)


@pytest.mark.parametrize("variant", mk.VARIANTS)
@pytest.mark.parametrize("rule", [mk.REF, mk.DELTA])
def test_growth(standin, variant, rule):
    mk.test_growth_moves_every_row(variant, rule)


# every position set; the larger the batch, the fewer of its modes (python resolves ~1 M deltas per second)
LISTS = [p for p in mk.list_params() if mk.POSITIONS[p.values[0]][1] < 4097 or p.values[1:] == (mk.REF, mk.MARK) or (mk.POSITIONS[p.values[0]][1] == 4097 and p.values[1:] == (mk.DELTA, mk.STRICT))]


@pytest.mark.parametrize("name,rule,mode", LISTS)
def test_list_cases(standin, name, rule, mode):
    mk.test_list_cases(name, rule, mode)


@pytest.mark.parametrize("rule,mode", [(mk.REF, 0), (mk.REF, mk.STRICT)])
def test_epoch_wrap(standin, rule, mode):
    mk.test_epoch_wrap_with_links_above_4096(rule, mode)


# ---- one defect each: the suite's checks must fail ----

WRONG = [
    ("the spill stops at the last line", lambda: mk.test_layout_cases("host", mk.REF, 0, 8)),
    ("first empty slot, not looking past the node's other fields", lambda: mk.test_layout_cases("host", mk.REF, 0, 8)),
    ("a tie goes to the larger index", lambda: mk.test_list_cases("255_256", mk.REF, mk.MARK)),
    ("a tie goes to the larger index", lambda: mk.test_layout_cases("dev", mk.DELTA, 0, 8)),
    ("a created row stores its own clock under the reference rule", lambda: mk.test_layout_cases("recs", mk.REF, mk.UNIQUE, 8)),
    ("a created row stores its own clock under the reference rule", lambda: mk.test_list_cases("63_64_300", mk.REF, mk.STRICT)),
    ("the winner mark moves but the block count does not", lambda: mk.test_list_cases("0_4095_4096", mk.DELTA, 0)),
    ("the winner mark moves but the block count does not", lambda: mk.test_list_cases("0_4095_4096_in_8193", mk.REF, mk.MARK)),
    ("a stale link of the previous epoch cycle is followed", lambda: mk.test_epoch_wrap_with_links_above_4096(mk.REF, 0)),
    ("padding records are counted as winners", lambda: mk.test_layout_cases("recs", mk.REF, 0, 8)),
]


@pytest.mark.parametrize("defect,test", WRONG, ids=["%s-%d" % (w[0], k) for k, w in enumerate(WRONG)])
def test_a_wrong_stand_in_is_caught(standin, defect, test):
    standin.setattr(bmx, "Engine", _defective(defect))
    with pytest.raises(AssertionError):
        test()
