"""GPU: the write path (csrc/merge_kernels.h: probe_or_insert and decide_and_claim in k_probe_apply and its occupancy variants, k_resolve_lists,
k_probe_link_strict, k_resolve_strict, k_rehash, k_sweep_heads; csrc/scan_kernels.h: k_compact_winners) at the edges of its probe sequence, of a wave, of the
256-delta block, of the compaction's 4096-delta block and of the 8-bit epoch — batches built delta by delta instead of seeded random ones.

Built on the slot-layout harness of tests/test_gpu_sync_kernel_edges.py (Table.ids_for inverts the probe sequence) and of tests/test_gpu_lookup_edges.py
(Model replays it, Case says where a row must land). Tables are the smallest the engine makes (4096 slots, 1024 lines of 4). The rows that crowd a line are
written one call each, so where they land is determined, and the premise asserts that the device table IS the model in slot order. Then a case's keys arrive
in ONE batch: lanes create rows concurrently. Expected state, winners and strict flags are the oracle's (oracle.oracle.Oracle); everything is exact.

Layout cases, each in lines of its own (the line after a landing line starts with a resident fence row in its first slot and the line before one is full or
ends with one, so the slot order of dump_rows says in which line a created row sits):
  home               new keys whose home line has room
  cross              the home line holds four rows of other nodes: every new key lands in the next line
  wrap               the same with the last line as home: the keys land in line 0
  two_full           two full lines in a row
  own_fields         the home line holds three fields of the same node: one new field lands in it, three in the next line (neighbouring lanes; which one is racy);
                     and a delta for a resident field that sits behind a sibling
  node_spill         9 new fields of one new node in one wave: 2 1/4 lines, the lanes lose CASes to their own node
  two_nodes          two new nodes with the same home slot, 3 fields each, in one wave (two_nodes_2w: on both sides of a wave border): which row spills is racy
  same_key           64 lanes carry one absent key whose home line is full (same_key_split: the first occurrence in lane 63 of wave 0, the rest in wave 1)
  resident_far       deltas for resident keys one and two lines from home, winning, losing and equal: no row is created

List cases: one key (field F0) whose deltas sit at chosen indices of a batch of unique filler deltas about half of which win, so that the rank of every
4096-delta block depends on the counts k_resolve_lists moves. Which member claims first is the hardware's: only the oracle's answers are asserted.

What is asserted of n_conflicts: strict mode links every valid delta (deltas - distinct keys, exact); the default mode drops a delta that is strictly below
the snapshot it saw, which for a resident row may be the pre-batch row or a value stored by the first claimer — exact where every member claims (an absent
start) or no pair can (at most one member not below the pre-batch row), otherwise between 0 and (members not below the pre-batch row) - 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from bmx import synth
from oracle import streams
from oracle.oracle import Oracle, rows_digest
import test_gpu_sync_kernel_edges as edges
import test_gpu_lookup_edges as lk

REF, DELTA = bmx.INSERT_REFERENCE, bmx.INSERT_DELTA
STRICT, UNIQUE, MARK = bmx.MERGE_STRICT_FLAGS, bmx.MERGE_UNIQUE_KEYS, bmx.MERGE_MARK_CREATED
EMPTY = lk.EMPTY
NSLOTS, NL = 4096, 1024
F0 = streams.field_hash(0)
FA, FB, FC, FZ, FY = lk.FA, lk.FB, lk.FC, lk.FZ, lk.FY
POOL = [f for f in (synth.field_hash(k) for k in range(1, 60)) if f not in (FA, FB, FC, FZ, FY, F0)]
DEVICE = "cuda"
WAVES = (8, 6, 5, 4, 3)
VARIANTS = ("host", "dev", "recs")
LAYOUT_TAGS = ["crossing", "two crossings", "wrap", "id equal, field not", "lost CAS to own node", "lost CAS to other node", "waiter in a spill line"]
LIST_TAGS = ["follower in another 256-block", "winner moved across a 4096-block", "tie with resident", "creating delta not the winner"]
OTHER_TAGS = ["padding at a wave border", "prefix second round"]
TAGS = LAYOUT_TAGS + LIST_TAGS + OTHER_TAGS
PREFIX_ROUND = 4 * 256 * 4 * 256        # k_compact_winners: one round of its prefix loop covers 4 x 256 16-byte loads = 4096 block counts = 2^20 deltas
BIG_N = (1 << 20) + 4097


def _same(got, want, what):
    edges._same(got, want, what)


# ---- one batch through one of the three entry points ----

def pad_positions(n):
    """records (AOS) carry two padding records: one in front of wave 1 (record 64) and one as the last record. -> (record index of every delta, records)"""
    pos = np.arange(n) + (np.arange(n) >= 64)
    return pos, (int(pos[-1]) + 2 if n else 1)


def run(e, b, variant, imode):
    """-> (applied: delta indices ascending, bit 31 as the device set it; flags u8[n]; (n_applied, n_conflicts, n_rows)); `recs` adds the padding records"""
    id, f, ts, val = b
    n = len(id)
    if variant == "host":
        a, fl, st = e.merge_batch(id, f, ts, val, imode)
        return a, fl, (st.n_applied, st.n_conflicts, st.n_rows)
    import torch
    dev = torch.device(DEVICE)
    pos, N = (np.arange(n), n) if variant == "dev" else pad_positions(n)
    applied = torch.zeros(N, dtype=torch.int32, device=dev); n_applied = torch.zeros(1, dtype=torch.int64, device=dev)
    flags = torch.full((N,), 0x55, dtype=torch.uint8, device=dev); stats = torch.zeros(4, dtype=torch.int64, device=dev)
    if variant == "dev":
        dcols = (torch.from_numpy(id.view(np.int64)).to(dev), torch.from_numpy(f.view(np.int32)).to(dev), torch.from_numpy(ts).to(dev), torch.from_numpy(val).to(dev))
        e.merge_batch_dev(n, *dcols, imode, applied=applied, n_applied=n_applied, flags=flags, stats=stats)
    else:
        r = np.zeros(N, bmx.DELTA_REC_DTYPE)
        r["id"] = EMPTY
        r["id"][pos], r["field"][pos], r["ts"][pos], r["val"][pos] = id, f, ts, val
        recs = torch.from_numpy(r.view(np.int64).reshape(N, 4)).to(dev)
        e.merge_records_dev(N, recs, imode, applied=applied, n_applied=n_applied, flags=flags, stats=stats)
    e.sync()
    na = int(n_applied.cpu()[0])
    assert 0 <= na <= n, ("n_applied", na, n)
    a = applied.cpu().numpy().view(np.uint32)[:na]
    inv = np.full(N, -1, np.int64); inv[pos] = np.arange(n)
    idx = inv[a & np.uint32(bmx.APPLIED_INDEX)]
    assert (idx >= 0).all(), "a padding record among the winners"
    fl = flags.cpu().numpy()
    pads = np.setdiff1d(np.arange(N), pos)
    assert (fl[pads] == 0).all(), "flags of a padding record"
    st = stats.cpu().numpy()
    return (idx.astype(np.uint32) | (a & np.uint32(bmx.APPLIED_CREATED))), fl[pos], (int(st[0]), int(st[1]), int(st[2]))


def cols(deltas):
    return (np.asarray([d[0] for d in deltas], np.uint64), np.asarray([d[1] for d in deltas], np.uint32),
            np.asarray([d[2] for d in deltas], np.int64), np.asarray([d[3] for d in deltas], np.int64))


def conflict_range(b, pre, strict):
    """(lo, hi) of stats.n_conflicts (module docstring). pre: the keys that occur more than once -> the pre-batch (ts, val), None: absent"""
    members = {}
    for i, f, t, v in zip(*(x.tolist() for x in b)):
        if (i, f) in pre:
            members.setdefault((i, f), []).append((t, v))
    lo = hi = 0
    for k, mem in members.items():
        p = pre[k]
        if strict or p is None:
            lo += len(mem) - 1; hi += len(mem) - 1
        else:
            hi += max(0, sum(1 for tv in mem if tv >= p) - 1)
    return lo, hi


# ---- the layout cases ----

class MCase(lk.Case):
    """resident rows (row: one call each), then the deltas of ONE batch. line: where the delta's row must sit afterwards; None: racy (one of the group's lines)"""

    def __init__(self, name, claims=()):
        super().__init__(name)
        self.deltas, self.dlines, self.claims, self.dups = [], [], set(claims), False

    def delta(self, id, field, ts, val, line=None):
        self.deltas.append((int(id), int(field), ts, val)); self.dlines.append(line)
        return self


def layout_cases():
    T = edges.Table(None, NSLOTS)

    def at(slot, field, salt=0):
        return int(T.ids_for([slot], field, salt)[0])

    def node(line, salt=0):
        return at(4 * line + 1, FA, salt)

    def crowd(c, line, salt0=1):
        for k in range(4):
            c.row(at(4 * line + k, FZ, salt0 + k), FZ, 1, line)

    def fence_after(c, line):
        c.row(at(4 * (line + 1), FZ, 9), FZ, 1, line + 1)

    def fence_before(c, line):
        c.row(at(4 * (line - 1) + 3, FZ, 9), FZ, 1, line - 1)

    def fillers(c, line0, count):
        """unique new keys, two per line in lines of their own: they only move the case's deltas to other lanes"""
        for k in range(count):
            line = line0 + k // 2
            c.delta(at(4 * line + 2 * (k % 2), FA, 20 + k % 2), FA, 3 + k % 3, 100 + k, line)

    def start(n, f):
        return lk.home(n, f, NSLOTS, 4) % 4

    TV = [(5, 9), (0, -3), (2, 4), (1, 1 << 40), (3, -(1 << 40)), (2, 0), (7, 7), (0, 0), (4, 1)]     # clocks below, at and above the 2 a created row stores
    out = []
    B = 16
    c = MCase("home"); n = node(B); fence_before(c, B); fence_after(c, B)
    for k, f in enumerate((FA, FB, FC)):
        c.delta(n, f, *TV[k], B)
    out.append(c.probe(n, FY, ["stop at empty"]))

    B = 64
    c = MCase("cross", ["crossing"]); n = node(B); crowd(c, B); fence_after(c, B + 1)
    for k, f in enumerate((FA, FB, FC)):
        c.delta(n, f, *TV[k + 1], B + 1)
    out.append(c.probe(n, FY, ["crossing", "stop at empty"]))

    c = MCase("wrap", ["crossing", "wrap"]); n = node(NL - 1); crowd(c, NL - 1); fence_after(c, 0)
    for k, f in enumerate((FA, FB, FC)):
        c.delta(n, f, *TV[k + 2], 0)
    out.append(c.probe(n, FY, ["crossing", "wrap", "stop at empty"]))

    B = 112
    c = MCase("two_full", ["two crossings"]); n = node(B); crowd(c, B); crowd(c, B + 1, 5); fence_after(c, B + 2)
    for k, f in enumerate((FA, FB, FC)):
        c.delta(n, f, *TV[k + 3], B + 2)
    out.append(c.probe(n, FY, ["two crossings", "stop at empty"]))

    B = 160
    c = MCase("own_fields", ["id equal, field not", "crossing", "lost CAS to own node"]); n = node(B); fence_before(c, B)
    r2 = next(f for f in POOL if start(n, f) == 1)
    r3 = next(f for f in POOL if start(n, f) == 3)
    c.row(n, FA, 11, B).row(n, r2, 12, B).row(n, r3, 13, B)          # slots 1, 2 (behind FA) and 3: slot 0 is the line's last free one
    fence_after(c, B + 1)
    new = [f for f in POOL if f not in (r2, r3)][:4]
    c.delta(n, r2, 1000, 77, B)                                       # a resident row behind its sibling: found, not created again
    for k, f in enumerate(new):
        c.delta(n, f, *TV[k])
    out.append(c.probe(n, FY, ["id equal, field not", "crossing", "stop at empty"]))

    B = 208
    c = MCase("node_spill", ["crossing", "two crossings", "id equal, field not", "lost CAS to own node"]); n = node(B); fence_before(c, B); fence_after(c, B + 2)
    for k, f in enumerate(POOL[:9]):
        c.delta(n, f, *TV[k])
    out.append(c.probe(n, FY, ["two crossings", "stop at empty"]))

    for name, B, split in (("two_nodes", 256, False), ("two_nodes_2w", 304, True)):
        c = MCase(name, ["crossing", "lost CAS to other node"]); fence_before(c, B); fence_after(c, B + 1)
        a, b = at(4 * B + 1, FA, 0), at(4 * B + 1, FA, 1)            # (a, FA) and (b, FA) start in the same slot
        if split:
            fillers(c, B + 8, 61)
        for n in (a, b):                                              # split: a in lanes 61..63 of wave 0, b in lanes 0..2 of wave 1
            for k, f in enumerate((FA, FB, FC)):
                c.delta(n, f, *TV[k + (n == b)])
        out.append(c.probe(at(4 * B + 1, FA, 2), FA, ["crossing", "stop at empty"]))

    for name, B, split in (("same_key", 352, False), ("same_key_split", 400, True)):
        c = MCase(name, ["crossing", "waiter in a spill line"]); c.dups = True; n = node(B); crowd(c, B); fence_after(c, B + 1)
        if split:
            fillers(c, B + 8, 63)
        for k in range(64):
            c.delta(n, FA, (k * 7) % 5, (k * 11) % 7 - 3, B + 1)
        out.append(c.probe(n, FY, ["crossing", "stop at empty"]))

    B = 448
    c = MCase("resident_far", ["crossing", "two crossings"]); n = node(B); crowd(c, B)
    c.row(n, FA, 21, B + 1).row(n, FB, 22, B + 1).row(n, FC, 23, B + 1).row(at(4 * (B + 1), FZ, 9), FZ, 1, B + 1)
    c.row(n, FY, 24, B + 2).row(n, FZ, 25, B + 2)
    res = {w[1]: (w[2], w[3]) for w in c.writes if w[0] == n}
    c.delta(n, FA, 1000, 5, B + 1).delta(n, FB, 1, 5, B + 1).delta(n, FC, *res[FC], B + 1)      # wins, loses, equals the row
    c.delta(n, FY, res[FY][0], res[FY][1] + 1, B + 2).delta(n, FZ, res[FZ][0], res[FZ][1] - 1, B + 2)   # the same clock: the value decides
    out.append(c.probe(n, POOL[0], ["two crossings", "stop at empty"]))
    return out


def place(m, c):
    """the model after the case's batch, key by key in index order. -> (created keys, the branches the batch reaches)"""
    tags, absent, created = set(), {}, []
    for j, (i, f, _, _) in enumerate(c.deltas):
        s, free, tg = m.find(i, f)
        tags |= tg
        if s is None:
            absent.setdefault((i, f), []).append((j, free))
    by_slot = {}
    for (i, f), occ in absent.items():
        free = occ[0][1]
        if len(occ) > 1 and free // 4 != lk.home(i, f, m.nslots, 4) // 4:
            tags.add("waiter in a spill line")
        for (i2, f2) in by_slot.get(free, []):                       # two absent keys that meet the same free slot first: one of them loses the CAS
            tags.add("lost CAS to own node" if i2 == i else "lost CAS to other node")
        by_slot.setdefault(free, []).append((i, f))
    for (i, f, _, _), line in zip(c.deltas, c.dlines):
        s, _, tg = m.find(i, f)
        tags |= tg                                                    # (the walk behind the rows the batch itself has created so far)
        if s is None:
            s = m.put(i, f, 0, 0)
            created.append((i, f))
            assert line is None or s // 4 == line, (c.name, "delta", hex(i), f, "lands in slot", s, "not in line", line)
    return created, tags


class Laid:
    """one engine with every layout case's resident rows, its oracle and its slot model"""

    def __init__(self, e, cases):
        self.e, self.cases, self.o = e, cases, Oracle()

        def one(id, f, ts, v):
            e.put_rows([id], [f], [ts], [v]); self.o.put_rows([id], [f], [ts], [v])
        self.m = lk.lay(cases, 4, one)
        self.label = {(r[1], r[2]): (r[1], r[2]) for r in self.m.rows()}
        self.check_order("the premise: the device table is the model")

    def check_order(self, what):
        """dump_rows comes in slot order: a resident row is itself, a created row is its case's line (or its racy group)"""
        gid, gf, _, _ = self.e.dump_rows()
        got = [self.label.get(k) for k in zip(gid.tolist(), gf.tolist())]
        want = [self.label[(r[1], r[2])] for r in self.m.rows()]
        assert got == want, (what, [(k, a, b) for k, (a, b) in enumerate(zip(got, want)) if a != b][:4], len(got), len(want))

    def check_state(self, what, keys=(), probes=()):
        e, o = self.e, self.o
        got, want = e.dump_rows(), o.dump_rows()
        assert len(set(zip(got[0].tolist(), got[1].tolist()))) == len(got[0]), (what, "a key has two rows")
        ga, wa = np.lexsort((got[1], got[0])), np.lexsort((want[1], want[0]))
        for g, w, col in zip(got, want, ("id", "field", "ts", "val")):
            _same(g[ga], w[wa], (what, "dump_rows", col))
        assert e.row_count() == len(o), (what, "row_count")
        if keys:
            ts, val, found = e.get_rows([k[0] for k in keys], [k[1] for k in keys])
            want = [o.get_row(*k) for k in keys]
            assert found.all() and None not in want, (what, "get_rows: a key of the case is missing")
            _same(ts, np.asarray([w[0] for w in want], np.int64), (what, "get_rows ts")); _same(val, np.asarray([w[1] for w in want], np.int64), (what, "get_rows val"))
        if probes:
            found = e.get_rows([p[0] for p in probes], [p[1] for p in probes])[2]
            assert not found.any() and all(o.get_row(p[0], p[1]) is None for p in probes), (what, "an absent key was found")

    def merge(self, b, variant, rule, mode, what):
        """one batch against the oracle: winners in order, counts, flags"""
        e, o = self.e, self.o
        seen, dup = set(), set()
        for k in zip(b[0].tolist(), b[1].tolist()):
            (dup if k in seen else seen).add(k)
        assert not (dup and mode & UNIQUE)
        pre = {k: o.get_row(*k) for k in dup}
        if mode & MARK:
            want, of = o.merge_batch_marked(*b, rule), None
        else:
            of, want = o.merge_batch(*b, rule)
        a, fl, (na, nx, nr) = run(e, b, variant, rule | mode)
        _same(a, want, (what, "applied_idx"))
        assert na == len(want) and nr == len(o), (what, "n_applied, n_rows", na, len(want), nr, len(o))
        lo, hi = conflict_range(b, pre, bool(mode & STRICT))
        assert lo <= nx <= hi, (what, "n_conflicts", nx, lo, hi)
        if of is not None and (mode & STRICT or not dup):     # (without strict mode a delta of a duplicated key answers against the snapshot it saw)
            _same(fl, of, (what, "flags"))
        elif of is not None:
            assert (fl[a & np.uint32(bmx.APPLIED_INDEX)] & 1).all(), (what, "a winner's flag")
        return a

    def run_case(self, c, variant, rule, mode):
        created, _ = place(self.m, c)
        for k, line in zip([d[:2] for d in c.deltas], c.dlines):
            if k in created:
                self.label[k] = (c.name, line)
        b = cols(c.deltas)
        keys = sorted(set([w[:2] for w in c.writes] + [d[:2] for d in c.deltas]))
        probes = [p[:2] for p in c.probes]
        for what in ("batch", "replay"):
            rows = len(self.o)
            self.merge(b, variant, rule, mode, (c.name, what))
            assert what == "batch" or len(self.o) == rows
            self.check_state((c.name, what), keys, probes)
            self.check_order((c.name, what))


def layout_params():
    for variant in VARIANTS:
        for rule in (REF, DELTA):
            for mode, waves in [(0, w) for w in WAVES] + [(UNIQUE, w) for w in WAVES] + [(STRICT, 8)]:     # (the strict path has kernels of its own: no k_probe_apply)
                yield pytest.param(variant, rule, mode, waves, id="%s-%s-%s-w%d" % (variant, "delta" if rule else "ref", {0: "default", UNIQUE: "unique", STRICT: "strict"}[mode], waves))


@pytest.mark.parametrize("variant,rule,mode,waves", list(layout_params()))
def test_layout_cases(variant, rule, mode, waves):
    cases = layout_cases()
    with bmx.Engine(edges.capacity_for(NSLOTS), flags=bmx.CTX_FIXED_CAPACITY, load_pct=90) as e:
        e.set_probe_waves(waves)
        t = Laid(e, cases)
        for c in cases:
            if not (c.dups and mode & UNIQUE):
                t.run_case(c, variant, rule, mode)
        assert e.info().n_slots == NSLOTS, "the table did not grow"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rule", [REF, DELTA])
def test_growth_moves_every_row(variant, rule):
    """cross, wrap and own_fields on a growing engine, then a batch that forces k_rehash: every row and every absent probe again, then duplicates on the moved rows"""
    cases = [c for c in layout_cases() if c.name in ("cross", "wrap", "own_fields")]
    with bmx.Engine(edges.capacity_for(NSLOTS), load_pct=90) as e:
        t = Laid(e, cases)
        for c in cases:
            t.run_case(c, variant, rule, 0)
        assert e.info().n_slots == NSLOTS
        n = 4200                                # more deltas than the table has slots
        b = (synth.splitmix64_np(np.arange(1, n + 1, dtype=np.uint64)), np.full(n, F0, np.uint32), np.arange(n, dtype=np.int64) % 5, np.arange(n, dtype=np.int64) - 7)
        t.merge(b, variant, rule, 0, "the growing batch")
        assert e.info().n_slots > NSLOTS, "the table grew"
        keys = sorted(set(k for c in cases for k in [w[:2] for w in c.writes] + [d[:2] for d in c.deltas]))
        probes = [p[:2] for c in cases for p in c.probes]
        t.check_state("after the growth", keys, probes)
        moved = keys * 3 + list(zip(b[0][:50].tolist(), b[1][:50].tolist())) * 2
        k = len(moved)
        d = (np.asarray([m[0] for m in moved], np.uint64), np.asarray([m[1] for m in moved], np.uint32), (np.arange(k, dtype=np.int64) * 7) % 6, (np.arange(k, dtype=np.int64) * 5) % 9 - 4)
        for mode in (0, STRICT):
            t.merge(d, variant, rule, mode, ("duplicates on the moved rows", mode))
            t.check_state(("duplicates on the moved rows", mode), keys, probes)


# ---- the list cases ----

def spread70():
    return [k * 256 + (k * 37) % 256 for k in range(70)]


POSITIONS = {"255_256": ([255, 256], 257), "0_4095_4096": ([0, 4095, 4096], 4097), "63_64_300": ([63, 64, 300], 4097), "0_4095_4096_in_8193": ([0, 4095, 4096], 8193),
             "63_64_300_in_8193": ([63, 64, 300], 8193), "70_blocks": (spread70(), 70 * 256 + 1)}


def scenarios(k):
    """(name, start or None, the members' (ts, val) in index order, claims) for a list of k members. Clocks sit around the 2 a created row stores."""
    lowv = [(1, 50 + j) for j in range(k)]

    def with_max(where, tv, base=None):
        v = list(base or lowv)
        for w in where:
            v[w] = tv
        return v
    mid = k // 2
    out = []
    for start in ((60, 0), None):
        s = "resident" if start else "absent"
        hi = (100, 7)
        out += [("%s, the first member wins" % s, start, with_max([0], hi), []), ("%s, the last member wins" % s, start, with_max([k - 1], hi), []),
                ("%s, a middle member wins" % s, start, with_max([mid], hi), []), ("%s, two equal maxima" % s, start, with_max(sorted({mid, k - 1} if k > 2 else {0, 1}), hi), [])]
    out.append(("a maximum equal to the resident row", (100, 7), with_max([mid, k - 1], (100, 7)), ["tie with resident"]))
    out.append(("every member below the resident row", (100, 7), with_max([0], (100, 6)), []))
    out.append(("some members below the resident row", (1, 55), with_max([mid], (100, 7)), []))
    cyc = [(1, 50), (2, 9), (0, 99)]
    out.append(("absent, the creating delta is the maximum", None, [(5, 9)] + [cyc[j % 3] for j in range(k - 1)], []))          # (2, 9) ties with the stored (2, 9)
    out.append(("absent, a delta at clock 2 beats the creating delta", None, [(0, 1)] + [[(2, 1), (2, 5), (1, 77)][(j + 1) % 3] if k > 2 else (2, 5) for j in range(k - 1)], ["creating delta not the winner"]))
    out.append(("absent, a delta above clock 2 beats the creating delta", None, [(1, 1)] + [[(1, 99), (3, -4), (2, 0)][(j + 1) % 3] if k > 2 else (3, -4) for j in range(k - 1)], ["creating delta not the winner"]))
    out.append(("absent, the creating delta stores clock 2 and holds it", None, [(9, 0)] + [[(2, -1), (0, 5), (2, 0)][j % 3] for j in range(k - 1)], []))
    return out


def list_batch(pos, n, fill_ids, bno, key, values):
    """the filler deltas (unique resident keys, every second one above what its row holds) with the list's members at `pos`"""
    j = np.arange(n, dtype=np.int64)
    win = ((j * 2654435761 + bno * 40503) >> 7) % 2 == 1
    id = fill_ids[:n].copy(); ts = np.where(win, 1000 + bno, 0).astype(np.int64); val = (j % 11 - 5 + bno).astype(np.int64)
    id[pos] = key
    ts[pos] = [v[0] for v in values]; val[pos] = [v[1] for v in values]
    return id, np.full(n, F0, np.uint32), ts, val


def list_tags(pos, start, values, rule):
    """what the members' positions and values reach, whoever claims first (module docstring)"""
    tags = set()
    if len({p >> 8 for p in pos}) > 1:
        tags.add("follower in another 256-block")
    cur, owner, creator = start, None, None
    for p, tv in zip(pos, values):
        if cur is None:
            cur, owner, creator = ((2 if rule == REF else tv[0]), tv[1]), p, p
        elif tv > cur:
            cur, owner = tv, p
    if owner is not None and len({p >> 12 for p in pos}) > 1 and sum(1 for p in pos if p >> 12 == owner >> 12) == 1:
        tags.add("winner moved across a 4096-block")     # (unless the winner happens to claim first)
    if start is not None and owner is None and max(values) == start:
        tags.add("tie with resident")
    if creator is not None and owner != creator:
        tags.add("creating delta not the winner")
    return tags


def list_params():
    for name in POSITIONS:
        for rule, mode, tag in ((REF, MARK, "ref-marked"), (REF, STRICT, "ref-strict"), (DELTA, 0, "delta-default"), (DELTA, STRICT, "delta-strict")):
            yield pytest.param(name, rule, mode, id="%s-%s" % (name, tag))


@pytest.mark.parametrize("name,rule,mode", list(list_params()))
def test_list_cases(name, rule, mode):
    pos, n = POSITIONS[name]
    fill = synth.splitmix64_np(np.arange(1, n + 1, dtype=np.uint64))
    variants = ("host", "recs") if n < 8193 else ("host",)
    with bmx.Engine(2 * n + 1000, load_pct=90) as e:
        t = Laid(e, [])
        e.load_rows(fill, np.full(n, F0, np.uint32), np.full(n, 10), np.zeros(n)); t.o.load_rows(fill, np.full(n, F0, np.uint32), np.full(n, 10), np.zeros(n))
        bno = 0
        for variant in variants:
            for sname, start, values, claims in scenarios(len(pos)):
                bno += 1
                key = int(synth.splitmix64_np(np.asarray([1_000_000 + bno], np.uint64))[0])
                if start:
                    e.load_rows([key], [F0], [start[0]], [start[1]]); t.o.load_rows([key], [F0], [start[0]], [start[1]])
                assert set(claims) <= list_tags(pos, start, values, rule) or (rule == DELTA and "creating delta not the winner" in claims), (sname, claims)
                b = list_batch(pos, n, fill, bno, key, values)
                a = t.merge(b, variant, rule, mode, (name, sname, variant))
                assert 0.3 * n < len(a) < 0.7 * n, "about half of the fillers win"
                if start and max(values) <= start:
                    assert not np.isin(np.asarray(pos, np.uint32), a & np.uint32(bmx.APPLIED_INDEX)).any(), (sname, "applied names a key nobody won")
                assert e.get_row(key, F0) == t.o.get_row(key, F0), (name, sname, variant)
        assert rows_digest(*e.dump_rows()) == t.o.digest()


def big_batch():
    """2^20 + 4097 deltas on unique resident keys, every third one a winner, and one two-member list in the first and the last 256-delta block"""
    n = BIG_N
    id = synth.splitmix64_np(np.arange(1, n + 1, dtype=np.uint64))
    j = np.arange(n, dtype=np.int64)
    ts = np.where(j % 3 == 0, 20, 5).astype(np.int64); val = j % 1001 - 500
    id[n - 1] = id[0]; ts[0], val[0] = 20, 1; ts[n - 1], val[n - 1] = 30, 2       # delta 0 beats the row, the last delta beats delta 0: the mark moves from block 0 to the last block
    return (id[:n - 1], np.full(n - 1, F0, np.uint32), np.full(n - 1, 10, np.int64), np.zeros(n - 1, np.int64)), (id, np.full(n, F0, np.uint32), ts, val)


def test_compaction_prefix_second_round():
    """the only batch whose last compaction block reads more than 4096 block counts in front of it (the second round of the 16-byte prefix loop)"""
    res, b = big_batch()
    assert (BIG_N - 1) // 4096 * 16 > PREFIX_ROUND // 256
    o = Oracle(); o.load_rows(*res)
    _, want = o.merge_batch(*b)
    assert want[-1] == BIG_N - 1 and want[0] != 0 and abs(len(want) - BIG_N // 3) < 3
    with bmx.Engine(2 * BIG_N, load_pct=90) as e:
        e.load_rows(*res)
        a, _, st = e.merge_batch(*b, want_flags=False)
        _same(a, want, "applied_idx")
        assert (st.n_applied, st.n_rows) == (len(want), len(o)) and 0 <= st.n_conflicts <= 1
        assert rows_digest(*e.dump_rows()) == o.digest()


# ---- the epoch wrap ----

EPOCH_N, EPOCH_FIRST, EPOCH_LISTS, EPOCH_LEN = 5000, 4100, 12, 70


def epoch_batches():
    """-> (the batch with long lists whose members all sit at indices above 4096, two batches of unique keys of the same size)"""
    n = EPOCH_N
    j = np.arange(n, dtype=np.int64)
    base = synth.splitmix64_np(np.arange(1, 3 * n + 1, dtype=np.uint64))
    id = base[:n].copy()
    k = np.arange(EPOCH_LISTS * EPOCH_LEN)
    id[EPOCH_FIRST + k] = base[EPOCH_FIRST + k % EPOCH_LISTS]       # EPOCH_LISTS keys, EPOCH_LEN members each, interleaved: every member's index is above 4096
    f = np.full(n, F0, np.uint32)
    return (id, f, (j * 13) % 7, j % 9 - 4), (base[n:2 * n], f, (j * 11) % 7, j % 5 - 2), (base[2 * n:], f, (j * 17) % 7, j % 7 - 3)


@pytest.mark.parametrize("rule,mode", [(REF, 0), (DELTA, 0), (REF, STRICT)])
def test_epoch_wrap_with_links_above_4096(rule, mode):
    """next[] and blk_follow[] are cleared only when the 8-bit epoch wraps: links written at epoch 1 above index 4096 must be gone at epoch 1 of the next cycle"""
    lists, u255, u1 = epoch_batches()
    with bmx.Engine(40000, load_pct=90) as e:
        t = Laid(e, [])
        t.merge(lists, "host", rule, mode, "the lists"); t.check_state("the lists")
        assert e.info().epoch == 1
        one = synth.splitmix64_np(np.arange(900_000, 900_300, dtype=np.uint64))
        k = 0
        while e.info().epoch < 254:
            t.merge((one[k:k + 1], np.full(1, F0, np.uint32), np.asarray([k % 4], np.int64), np.asarray([k], np.int64)), "host", rule, mode, ("one delta", k)); k += 1
        assert k == 253
        t.merge(u255, "host", rule, mode, "epoch 255"); t.check_state("epoch 255")
        assert e.info().epoch == 255
        t.merge(u1, "host", rule, mode, "epoch 1 of the next cycle"); t.check_state("epoch 1 of the next cycle")
        assert e.info().epoch == 1, "the epoch has wrapped"
        t.merge(lists, "host", rule, mode, "the lists again"); t.check_state("the lists again")
