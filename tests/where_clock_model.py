"""Clock literals of a boolean filter (include/bmx_where.h BMX_LIT_CLOCK / BMX_LIT_CLOCK_TOMB): the row of a field exists in a state the literal names and
lo <= its clock <= hi. Shared by test_where_clock_model.py (CPU) and the GPU tests (helper, not a test).

A literal is written as the Python binding takes it: (bmx.Clock(field, data, tombs), lo, hi[, negated]); CK(field, "data" | "deleted" | "any") builds the first part.

brute(m, base, clauses)        : the truth, node by node with Python ints, straight from the header's sentences — no slots, no bits, no order of evaluation.
ClockModel                     : where_diff_model.DiffModel with a clock per field and node next to the state and the value; its lit() also takes clock literals;
                                 numpy, for the tables of the GPU tests. test_where_clock_model.py holds it against brute().
prepare(base, clauses) / row() : a sequential stand-in of where_prepare (csrc/bmx_where.inc) and PredWhere::row (csrc/where_kernels.h) for one lane: a field's
                                 value and clock literals on ONE plain slot, a clock literal on the base field among the probed, pair slots apart. It notes in
                                 `probes` every probe as (field, "ts" | "val") — "ts": the slot has a clock literal and the probe's clock is kept — and in
                                 `tags` the PATHS a node took (TAGS). `defect` switches on ONE mistake a kernel could make (DEFECTS).
edge_cases(n, E)               : the layouts of test_gpu_where_clock_kernel_edges.py, by position; the CPU test shows that they expose the defects.
seeded_table / seeded_programs : the seeded generator of the CPU test and of the GPU tests' random programs (all three kinds of literal)."""
import numpy as np

import bmx
import where_diff_model as wdm
from where_diff_model import ABSENT, DATA, TOMB, F1, F2, F3, F4, FB, I64MAX, I64MIN, MAX_CLAUSE, MAX_LITS, MAX_SLOTS, PROBED, VAL_DELETED, VAL_MAX, is_pair, negated, node_ids  # noqa: F401

TS_MAX = (1 << 53) - 1
NOT, C_DATA, C_TOMB = 1, 2, 4          # the flags of a literal as the kernel takes it (csrc/where_kernels.h WHERE_LIT_*)

TAGS = ("clock_only_slot", "value_and_clock_one_probe", "base_clock_probed", "pair_beside_clock", "clock_reused", "decided_no_probe")
DEFECTS = ("state_dropped", "tomb_clock_as_data", "absent_not", "clock_clamped", "base_clock_from_column")


def CK(field, state="data"):
    return bmx.Clock(field, data=state in ("data", "any"), tombs=state in ("deleted", "any"))


def is_clock(t):
    return isinstance(t[0], bmx.Clock)


def names(t, state):
    """does the clock literal t name the row state `state`"""
    return bool(t[0].flags & (bmx.LIT_CLOCK if state == DATA else bmx.LIT_CLOCK_TOMB if state == TOMB else 0))


def entries(clause):
    return sum(2 if is_pair(t) else 1 for t in clause)


# ---- the truth ----
def lit_truth(m, t, i):
    if not is_clock(t):
        return wdm.lit_truth(m, t, i)
    f, lo, hi = t[0].field, int(t[1]), int(t[2])
    m._f(f)
    st = int(m.st[f][i])
    pos = st != ABSENT and names(t, st) and lo <= int(m.ts[f][i]) <= hi
    return pos != negated(t)


def brute(m, base, clauses):
    m._f(base)
    return np.array([m.st[base][i] == DATA and any(all(lit_truth(m, t, i) for t in c) for c in clauses) for i in range(m.N)], bool)


class ClockModel(wdm.DiffModel):
    """val[f][i], st[f][i], ts[f][i]: a row keeps its clock when it is tombstoned only if tomb() is told no other (the delete's clock is the row's then)"""

    def __init__(self, ids):
        wdm.DiffModel.__init__(self, ids)
        self.ts = {}

    def _f(self, f):
        wdm.DiffModel._f(self, f)
        if f not in self.ts:
            self.ts[f] = np.zeros(self.N, np.int64)

    def set(self, f, idx, vals, ts=5):
        wdm.DiffModel.set(self, f, idx, vals); self.ts[f][idx] = ts

    def tomb(self, f, idx, ts=9):
        wdm.DiffModel.tomb(self, f, idx); self.ts[f][idx] = ts

    def rows(self, f, ts=None, idx=None):
        """the rows of f that exist (of nodes idx), tombstones as VAL_DELETED, each with its own clock"""
        i = np.nonzero(self.st[f] != ABSENT)[0] if idx is None else np.asarray(idx)
        return self.ids[i], np.full(len(i), f, np.uint32), self.ts[f][i].copy(), np.where(self.st[f][i] == DATA, self.val[f][i], VAL_DELETED)

    def lit(self, t):
        if not is_clock(t):
            return wdm.DiffModel.lit(self, t)
        f, lo, hi = t[0].field, int(t[1]), int(t[2])
        self._f(f)
        state = ((self.st[f] == DATA) & names(t, DATA)) | ((self.st[f] == TOMB) & names(t, TOMB))
        pos = state & (self.ts[f] >= max(lo, I64MIN)) & (self.ts[f] <= min(hi, I64MAX)) if lo <= hi else np.zeros(self.N, bool)
        return ~pos if negated(t) else pos

    def shadow(self, s, f, state):
        """field s := the clock of f as a VALUE on exactly the nodes where f is in `state`, absent elsewhere (the differential tests' plain twin)"""
        self._f(f)
        idx = np.nonzero(self.st[f] == state)[0]
        self.val.pop(s, None); self.st.pop(s, None); self.ts.pop(s, None); self._f(s)
        self.set(s, idx, self.ts[f][idx], ts=3)


def plain_twin(clauses, f, state, s):
    """the program with every clock literal on f that names exactly `state` replaced by the same range over the value of field s"""
    want = bmx.LIT_CLOCK if state == DATA else bmx.LIT_CLOCK_TOMB
    return [[(s,) + tuple(t[1:]) if is_clock(t) and t[0].field == f and t[0].flags == want else t for t in c] for c in clauses]


def put(x, m, fields):
    """x: an Engine or a Comm; every row of `fields` that exists, stored as given"""
    for f in fields:
        m._f(f)
        if (m.st[f] != ABSENT).any():
            x.put_rows(*m.rows(f))


def write(x, m, f, idx, vals=None, ts=5):
    """rows (f, idx) := (ts, vals), or tombstones when vals is None, on the model and stored as given on x"""
    idx = np.asarray(idx)
    m.tomb(f, idx, ts) if vals is None else m.set(f, idx, vals, ts)
    if len(idx):
        x.put_rows(*m.rows(f, idx=idx))


# ---- the stand-in ----
def prepare(base, clauses):
    """-> dict: cbeg, lit [(slot, flags, lo, hi)], slots [(a, b or None)], flits, base_lits, slot_clock [bool]; ValueError where where_prepare refuses"""
    if not 1 <= len(clauses) <= 8:
        raise ValueError("1..8 clauses")
    if any(not 1 <= entries(c) <= MAX_CLAUSE for c in clauses):
        raise ValueError("1..8 literals")
    if sum(entries(c) for c in clauses) > MAX_LITS:
        raise ValueError("32 literals")
    W = dict(cbeg=[], lit=[], slots=[], flits=[], base_lits=[], slot_clock=[], base=base)
    for c in clauses:
        W["cbeg"].append(len(W["lit"]))
        for probed in (False, True):
            for t in c:
                pair, clock = is_pair(t), is_clock(t)
                f = t[0].field if clock else t[0]
                if (pair or clock or f != base) != probed:
                    continue
                lo, hi = (int(t[1]), int(t[2])) if pair or clock else (max(int(t[1]), -VAL_MAX), min(int(t[2]), VAL_MAX))
                flags = (NOT if negated(t) else 0) | ((C_DATA if names(t, DATA) else 0) | (C_TOMB if names(t, TOMB) else 0) if clock else 0)
                l = len(W["lit"])
                if not probed:
                    W["lit"].append((0, flags, lo, hi)); W["base_lits"].append(l)
                    continue
                key = (f[0], f[1]) if pair else (f, None)
                if key not in W["slots"]:
                    if len(W["slots"]) == MAX_SLOTS:
                        raise ValueError("no slot left for a field pair" if pair else "8 fields")
                    W["slots"].append(key); W["flits"].append([]); W["slot_clock"].append(False)
                s = W["slots"].index(key)
                W["slot_clock"][s] = W["slot_clock"][s] or clock
                W["lit"].append((s + 1, flags, lo, hi)); W["flits"][s].append(l)
    W["cbeg"].append(len(W["lit"]))
    return W


def _probe(m, f, i):
    """agg_probe_ts -> (found, value: VAL_DELETED for a tombstone, clock)"""
    m._f(f)
    st = m.st[f][i]
    return st != ABSENT, (int(m.val[f][i]) if st == DATA else VAL_DELETED), int(m.ts[f][i])


def row(W, m, i, defect=None, tags=None, probes=None):
    base = W["base"]
    m._f(base)
    valid = m.st[base][i] == DATA
    x = int(m.val[base][i])
    lit = W["lit"]
    truth, known = 0, 0
    for l in W["base_lits"]:
        truth |= int((lit[l][2] <= x <= lit[l][3]) != bool(lit[l][1] & NOT)) << l
    match = False
    for c in range(len(W["cbeg"]) - 1):
        alive = valid and not match
        for l in range(W["cbeg"][c], W["cbeg"][c + 1]):
            s = lit[l][0]
            if s:
                fb = 1 << (s - 1)
                a, b = W["slots"][s - 1]
                clk = W["slot_clock"][s - 1]
                if alive and (known & fb) and clk and tags is not None:
                    tags.add("clock_reused")
                if alive and not (known & fb):
                    def probe(f):
                        if probes is not None:
                            probes.append((f, "ts" if clk else "val"))
                        return _probe(m, f, i)
                    found, t = True, 0
                    if b is None:
                        found, y, t = probe(a)                       # (the base field too: its clock is in the table alone)
                        have = True
                    else:
                        ya = x if a == base else probe(a)[1]
                        yb = x if b == base else probe(b)[1]
                        have = ya != VAL_DELETED and yb != VAL_DELETED
                        if a != base and m.st[a][i] == ABSENT or b != base and m.st[b][i] == ABSENT:
                            have = False
                        y = wdm._wrap(ya - yb)
                    if tags is not None and b is None:
                        kinds = {bool(lit[j][1] & (C_DATA | C_TOMB)) for j in W["flits"][s - 1]}
                        if clk:
                            tags.add("base_clock_probed" if a == base else "value_and_clock_one_probe" if kinds == {True, False} else "clock_only_slot")
                            if any(bb is not None and a in (aa, bb) for aa, bb in W["slots"]):
                                tags.add("pair_beside_clock")
                    for j in W["flits"][s - 1]:
                        _, fl, lo, hi = lit[j]
                        if fl & (C_DATA | C_TOMB):
                            state = C_TOMB if y == VAL_DELETED else C_DATA
                            if defect == "tomb_clock_as_data":
                                state = C_DATA
                            ok = found and (defect == "state_dropped" or bool(fl & state))
                            z = t
                            if defect == "clock_clamped":
                                lo, hi = max(lo, -VAL_MAX), min(hi, VAL_MAX)
                            if defect == "base_clock_from_column" and a == base:
                                ok, z = True, x
                            inside = ok and lo <= z <= hi
                            if defect == "absent_not":
                                v = found and ((bool(fl & state) and lo <= z <= hi) != bool(fl & NOT))
                            else:
                                v = inside != bool(fl & NOT)
                        else:
                            v = (have and found and lo <= y <= hi) != bool(fl & NOT) if b is None else (have and lo <= y <= hi) != bool(fl & NOT)
                        truth |= int(v) << j
                    known |= fb
            alive = alive and bool((truth >> l) & 1)
            if not alive:
                break
        match = match or alive
        if not (valid and not match):
            break
    if tags is not None and valid and any(W["slot_clock"]) and not any((known >> s) & 1 for s in range(len(W["slots"])) if W["slot_clock"][s]):
        tags.add("decided_no_probe")
    return match


def standin(m, base, clauses, defect=None, tags=None, probes=None):
    W = prepare(base, clauses)
    return np.array([row(W, m, i, defect, tags, probes) for i in range(m.N)], bool)


# ---- the layouts of the kernel-edge tests ----
EDGE_SIZES = [1, 63, 64, 65, 8191, 8192, 8193, 2 * 8192 + 1]
LO, HI = 1000, 1999          # the window the edge programs ask for
FAR = 1 << 40                # a clock far above it, and far above any value of the edge tables


def edge_spots(n, E):
    """the positions a lone qualifying node is put at: first, last, lane 0 and lane 63 of the first and of the last wave, the ragged last unit"""
    wave = 64 * E
    last_wave = ((n - 1) // wave) * wave
    spots = {0, n - 1, min(63 * E, n - 1), last_wave, min(last_wave + 63 * E, n - 1), ((n - 1) // E) * E}
    return sorted(spots)


def edge_table(ids, node, E, wide):
    """-> ClockModel: FB on every node (base value by lane: 1 on lane 0, 2 on lane 63, else 0; + 2^40 when wide; clock 7 everywhere: the base column says nothing
    of clocks), F1 data with clock FAR everywhere, F2 data everywhere with the position as its clock offset into the window. node[p]: the node at position p."""
    n = len(ids)
    m = ClockModel(ids)
    pos = np.arange(n)
    lane = (pos // E) % 64
    off = (1 << 40) if wide else 0
    m.set(FB, node, np.where(lane == 0, 1, np.where(lane == 63, 2, 0)) + off, ts=7)
    m.set(F1, node, np.full(n, 1500), ts=FAR)       # value 1500: inside the window, where a kernel that reads the value for the clock would find it
    m.set(F2, node, np.full(n, 3), ts=LO + (pos % 64))
    return m


def edge_cases(m, node, E, wide):
    """yields (name, mutate(m, write), clauses, want positions or None, probing positions or None). mutate changes rows through write(f, nodes, vals|None, ts)."""
    n = len(node)
    pos = np.arange(n)
    lane = (pos // E) % 64
    off = (1 << 40) if wide else 0
    win = [[(CK(F1), LO, HI)]]
    prev = None
    for p in edge_spots(n, E):
        def lone(w, p=p, prev=prev):                                # (the spot before goes back to what every other node holds)
            if prev is not None:
                w(F1, node[[prev]], [1500], FAR)
            w(F1, node[[p]], [1500], LO + 1)
        fx = wdm.streams.fnv1a32("clock.edge.%d" % p)               # a field of this spot's own: every node but the one at p holds it
        yield ("lone data clock at %d" % p, lone, win, np.array([p]), pos)
        yield ("lone tombstone clock at %d" % p, lambda w, p=p: w(F1, node[[p]], None, HI), [[(CK(F1, "deleted"), LO, HI)]], np.array([p]), pos)
        yield ("lone absentee under NOT at %d" % p, lambda w, p=p, fx=fx: w(fx, np.delete(node, p), np.zeros(n - 1, np.int64), 5), [[(CK(fx, "any"), I64MIN, I64MAX, True)]], np.array([p]), pos)
        prev = p
    yield ("nobody in the window", lambda w, prev=prev: w(F1, node[[prev]], [1500], FAR), [[(CK(F1, "any"), LO, HI)]], pos[:0], pos)
    # exactly one lane of a wave needs the probe: the base literal in front sends every other lane away
    yield ("lane 0 alone probes", None, [[(FB, 1 + off, 1 + off), (CK(F2), LO, LO + 70)]], pos[lane == 0], pos[lane == 0])
    yield ("lane 63 alone probes", None, [[(CK(F2), LO, LO + 70), (FB, 2 + off, 2 + off)]], pos[lane == 63], pos[lane == 63])
    # 64 rows that differ only in clock: F2's clock is LO + position % 64
    yield ("rows differ in clock alone", None, [[(CK(F2), LO + 10, LO + 20)]], pos[(pos % 64 >= 10) & (pos % 64 <= 20)], pos)
    yield ("rows differ in clock alone, NOT", None, [[(CK(F2), LO + 10, LO + 20, True), (F2, 3, 3)]], pos[(pos % 64 < 10) | (pos % 64 > 20)], pos)
    # the base field's own clock (7 everywhere), beside a base value that lies in the window's numbers
    yield ("base clock", None, [[(CK(FB), 7, 7), (FB, off, off + 1)]], pos[lane != 63], pos[lane != 63])
    yield ("base clock outside", None, [[(CK(FB), off, off + 2)]], pos[:0], pos)
    yield ("base never deleted", None, [[(CK(FB, "deleted"), I64MIN, I64MAX)], [(CK(FB, "any"), 8, I64MAX)]], pos[:0], pos)
    # a tombstone inside the window is no data, and a data row is no tombstone
    yield ("states", lambda w: w(F2, node[::3], None, LO + 5), [[(CK(F2), LO, LO + 70)]], np.setdiff1d(pos, pos[::3]), pos)
    yield ("states, tombstones", None, [[(CK(F2, "deleted"), LO, LO + 70)]], pos[::3], pos)
    yield ("states, any", None, [[(CK(F2, "any"), LO + 5, LO + 5)]], np.union1d(pos[::3], pos[pos % 64 == 5]), pos)
    # a value literal and a clock literal of one field: one probe
    yield ("value and clock", None, [[(F2, 3, 3), (CK(F2, "any"), LO, LO + 4)], [(CK(F2, "deleted"), LO + 5, LO + 5), (F2, 3, 3, True)]], np.union1d(pos[::3], np.setdiff1d(pos[pos % 64 <= 4], pos[::3])), pos)


# ---- the seeded generator ----
def seeded_table(n, seed=20250401, salt=0):
    """-> ClockModel with FB on 90 % of the nodes (5 % absent, 5 % tombstoned), F1..F4 each data / absent / tombstoned on 60 / 25 / 15 %, values 0..5, clocks 0..9
    (a few at 0, 2^53 - 1)"""
    rng = np.random.default_rng(seed)
    m = ClockModel(node_ids(n, 70_000 + salt))
    for f, (p_data, p_tomb) in [(FB, (0.90, 0.05))] + [(f, (0.60, 0.15)) for f in PROBED]:
        u = rng.random(n)
        held = np.nonzero(u < p_data + p_tomb)[0]
        ts = rng.integers(0, 10, len(held)).astype(np.int64)
        ts[rng.random(len(held)) < 0.02] = TS_MAX
        m.set(f, held, rng.integers(0, 6, len(held)).astype(np.int64), ts=ts)
        dead = np.nonzero((u >= p_data) & (u < p_data + p_tomb))[0]
        m.tomb(f, dead, ts=m.ts[f][dead])
    return m


def _clock_lit(rng, fields):
    f = fields[int(rng.integers(0, len(fields)))]
    state = ("data", "deleted", "any")[int(rng.integers(0, 3))]
    kind = int(rng.integers(0, 8))
    if kind == 0:
        lo, hi = I64MIN, I64MAX
    elif kind == 1:
        lo, hi = int(rng.integers(0, 10)), I64MAX              # since T
    elif kind == 2:
        lo = int(rng.integers(0, 10)); hi = lo - 1             # an empty range
    elif kind == 3:
        lo, hi = TS_MAX, TS_MAX
    else:
        lo = int(rng.integers(0, 9)); hi = lo + int(rng.integers(0, 4))
    return (CK(f, state), lo, hi, bool(rng.random() < 0.35))


def seeded_programs(count=100, seed=20250402):
    """count programs of 1..4 clauses over at most 2 ordered pairs and the plain slots of FB, F1..F4 (so at most 7 slots), every kind of literal in most."""
    rng = np.random.default_rng(seed)
    fields = [FB] + PROBED
    progs = []
    while len(progs) < count:
        pairs = []
        while len(pairs) < 2:
            a, b = (fields[int(j)] for j in rng.choice(len(fields), 2, replace=False))
            if (a, b) not in pairs:
                pairs.append((a, b))
        prog, total = [], 0
        for _ in range(int(rng.integers(1, 5))):
            c, used = [], 0
            want = int(rng.integers(1, 5))
            while len(c) < want:
                u = rng.random()
                t = _clock_lit(rng, fields) if u < 0.5 else wdm._pair_lit(rng, pairs) if u < 0.7 else wdm._plain_lit(rng, fields)
                if used + (2 if is_pair(t) else 1) > MAX_CLAUSE:
                    break
                c.append(t); used += 2 if is_pair(t) else 1
            if total + used > MAX_LITS:
                break
            prog.append(c); total += used
        progs.append(prog)
    return progs
