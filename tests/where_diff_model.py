"""Field-to-field literals of a boolean filter (include/bmx_where.h BMX_LIT_MINUS): lo <= value(A) - value(B) <= hi. Shared by test_where_diff_model.py (CPU) and the
GPU tests (helper, not a test).

brute(m, base, clauses)        : the truth, node by node with Python ints, straight from the header's sentences — no slots, no bits, no order of evaluation.
DiffModel                      : watch_model.Model (a state per field and node: absent, data, tombstone) whose lit() also takes ((a, b), lo, hi[, negated]);
                                 numpy, for the tables of the GPU tests. test_where_diff_model.py holds it against brute().
prepare(base, clauses) / row() : a sequential stand-in of where_prepare (csrc/bmx_where.inc) and PredWhere::row (csrc/where_kernels.h) for one lane: the slot
                                 table with its pair bits, the literals on the base field in front of each clause, the `truth` and `known` words, one probe
                                 step per slot. It notes which PATHS a node took (TAGS), which fields it probed, and the states and outcomes it saw. `defect`
                                 switches on ONE mistake a kernel could make (DEFECTS); the seeded cases must expose each of them.
seeded_table / seeded_programs : the seeded generator of the CPU test and of the GPU tests' random programs."""
import numpy as np

from oracle import streams
from watch_model import ABSENT, DATA, TOMB, Model  # noqa: F401

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
VAL_MAX = (1 << 53) - 1
VAL_DELETED = I64MIN
MAX_SLOTS, MAX_LITS, MAX_CLAUSE = 8, 32, 8

FB, F1, F2, F3, F4 = (streams.fnv1a32(s) for s in ("diff.base", "diff.one", "diff.two", "diff.three", "diff.four"))
PROBED = [F1, F2, F3, F4]

TAGS = ("base_a", "base_b", "two_probes", "slot_reused", "clause2_only", "decided_no_probe")
DEFECTS = ("tomb_as_value", "b_minus_a", "not_before_presence", "first_lit_only", "base_from_probe")


def is_pair(t):
    return isinstance(t[0], (tuple, list))


def negated(t):
    return bool(len(t) > 3 and t[3])


def entries(clause):
    """how many bmx_lit entries a clause takes: a pair literal takes two"""
    return sum(2 if is_pair(t) else 1 for t in clause)


# ---- the truth ----
def lit_truth(m, t, i):
    """one literal on node i, Python ints"""
    lo, hi = int(t[1]), int(t[2])
    if is_pair(t):
        a, b = t[0]
        m._f(a); m._f(b)
        pos = m.st[a][i] == DATA and m.st[b][i] == DATA and lo <= int(m.val[a][i]) - int(m.val[b][i]) <= hi
    else:
        m._f(t[0])
        pos = m.st[t[0]][i] == DATA and lo <= int(m.val[t[0]][i]) <= hi
    return pos != negated(t)


def brute(m, base, clauses):
    """-> bool per node: holds data in base, and some clause has all of its literals true"""
    m._f(base)
    return np.array([m.st[base][i] == DATA and any(all(lit_truth(m, t, i) for t in c) for c in clauses) for i in range(m.N)], bool)


class DiffModel(Model):
    def lit(self, t):
        if not is_pair(t):
            return Model.lit(self, t)
        (a, b), lo, hi = t[0], int(t[1]), int(t[2])
        self._f(a); self._f(b)
        d = self.val[a] - self.val[b]                       # (|values| <= 2^53 - 1: exact in int64)
        pos = (self.st[a] == DATA) & (self.st[b] == DATA) & (d >= lo) & (d <= hi) if lo <= hi else np.zeros(self.N, bool)
        return ~pos if negated(t) else pos

    def derived(self, d, a, b):
        """field d := a - b on the nodes where both hold data, absent elsewhere (the differential tests' plain twin of the pair (a, b))"""
        self._f(a); self._f(b)
        both = np.nonzero((self.st[a] == DATA) & (self.st[b] == DATA))[0]
        self.val.pop(d, None); self.st.pop(d, None); self._f(d)
        self.set(d, both, self.val[a][both] - self.val[b][both])
        assert (np.abs(self.val[d]) <= VAL_MAX).all()


def plain_twin(clauses, pair, d):
    """the program with every literal on `pair` replaced by the same literal on field d"""
    return [[(d,) + tuple(t[1:]) if is_pair(t) and tuple(t[0]) == tuple(pair) else t for t in c] for c in clauses]


# ---- the stand-in ----
def prepare(base, clauses):
    """-> dict: cbeg, lit [(slot, neg, lo, hi)], slots [(a, b or None)], flits [[literal numbers]], base_lits; ValueError where where_prepare refuses"""
    if not 1 <= len(clauses) <= 8:
        raise ValueError("1..8 clauses")
    if any(not 1 <= entries(c) <= MAX_CLAUSE for c in clauses):
        raise ValueError("1..8 literals")
    if sum(entries(c) for c in clauses) > MAX_LITS:
        raise ValueError("32 literals")
    W = dict(cbeg=[], lit=[], slots=[], flits=[], base_lits=[], first_clause=[])
    for ci, c in enumerate(clauses):
        W["cbeg"].append(len(W["lit"]))
        for probed in (False, True):
            for t in c:
                pair = is_pair(t)
                if pair and t[0][0] == t[0][1]:
                    raise ValueError("a field minus itself")
                if (pair or t[0] != base) != probed:
                    continue
                lo, hi = (int(t[1]), int(t[2])) if pair else (max(int(t[1]), -VAL_MAX), min(int(t[2]), VAL_MAX))
                l = len(W["lit"])
                if not probed:
                    W["lit"].append((0, negated(t), lo, hi)); W["base_lits"].append(l)
                    continue
                key = (t[0][0], t[0][1]) if pair else (t[0], None)
                if key not in W["slots"]:
                    if len(W["slots"]) == MAX_SLOTS:
                        raise ValueError("no slot left for a field pair" if pair else "8 fields")
                    W["slots"].append(key); W["flits"].append([]); W["first_clause"].append(ci)
                s = W["slots"].index(key)
                W["lit"].append((s + 1, negated(t), lo, hi)); W["flits"][s].append(l)
    W["cbeg"].append(len(W["lit"]))
    W["base"] = base
    return W


def _wrap(v):
    return ((v + (1 << 63)) % (1 << 64)) - (1 << 63)


def _probe(m, f, i):
    """agg_probe: a tombstoned row IS found, with VAL_DELETED in it"""
    m._f(f)
    st = m.st[f][i]
    return (st != ABSENT), (int(m.val[f][i]) if st == DATA else VAL_DELETED)


def row(W, m, i, defect=None, tags=None, probes=None, seen=None):
    """PredWhere::row for node i. tags: a set that takes the path tags; probes: a list that takes every probed field; seen: a set that takes
    (state of A, state of B, outcome) of every pair literal whose truth bit was set."""
    base = W["base"]
    m._f(base)
    valid = m.st[base][i] == DATA
    x = int(m.val[base][i])
    lit = W["lit"]
    truth, known = 0, 0
    for l in W["base_lits"]:
        truth |= int((lit[l][2] <= x <= lit[l][3]) != lit[l][1]) << l
    match = False
    for c in range(len(W["cbeg"]) - 1):
        alive = valid and not match
        for l in range(W["cbeg"][c], W["cbeg"][c + 1]):
            s = lit[l][0]
            if s:
                fb = 1 << (s - 1)
                a, b = W["slots"][s - 1]
                if alive and (known & fb) and b is not None and tags is not None:
                    tags.add("slot_reused")
                if alive and not (known & fb):
                    def side(f):
                        if f == base and defect != "base_from_probe":
                            return True, x
                        if probes is not None:
                            probes.append(f)
                        return _probe(m, f, i)
                    if b is None:
                        have, y = side(a) if a != base else _probe(m, a, i)
                    else:
                        ha, ya = side(a)
                        hb, yb = side(b)
                        have = ha and hb
                        if defect != "tomb_as_value":
                            have = have and ya != VAL_DELETED and yb != VAL_DELETED
                        y = _wrap(yb - ya) if defect == "b_minus_a" else _wrap(ya - yb)
                        if tags is not None:
                            tags.add("base_a" if a == base else "base_b" if b == base else "two_probes")
                            if c >= 1 and W["first_clause"][s - 1] >= 1:
                                tags.add("clause2_only")
                    for j in W["flits"][s - 1][:1] if defect == "first_lit_only" and b is not None else W["flits"][s - 1]:
                        inside = lit[j][2] <= y <= lit[j][3]
                        t = (have and (inside != lit[j][1])) if defect == "not_before_presence" and b is not None else ((have and inside) != lit[j][1])
                        truth |= int(t) << j
                        if seen is not None and b is not None:
                            seen.add((DATA if a == base else int(m.st[a][i]), DATA if b == base else int(m.st[b][i]), bool(t)))
                    known |= fb
            alive = alive and bool((truth >> l) & 1)
            if not alive:
                break
        match = match or alive
        if not (valid and not match):
            break
    if tags is not None and valid and any(b is not None for _, b in W["slots"]) and not any((known >> s) & 1 for s, (_, b) in enumerate(W["slots"]) if b is not None):
        tags.add("decided_no_probe")
    return match


def standin(m, base, clauses, defect=None, tags=None, probes=None, seen=None):
    W = prepare(base, clauses)
    return np.array([row(W, m, i, defect, tags, probes, seen) for i in range(m.N)], bool)


# ---- the seeded generator ----
def node_ids(n, salt=0):
    return streams.splitmix64_np(np.arange(1 + salt, n + 1 + salt, dtype=np.uint64))


def seeded_table(n, seed=20250301, salt=0, far=0.02):
    """-> (DiffModel, tombs): FB on 90 % of the nodes (5 % absent, 5 % tombstoned), F1..F4 each data / absent / tombstoned on 60 / 25 / 15 %, values 0..5
    so that differences land on and beside the bounds, a share `far` of them at +-VAL_MAX. tombs: {field: nodes}, rows to load as data first and tombstone then."""
    rng = np.random.default_rng(seed)
    m = DiffModel(node_ids(n, 50_000 + salt))
    tombs = {}
    for f, (p_data, p_tomb) in [(FB, (0.90, 0.05))] + [(f, (0.60, 0.15)) for f in PROBED]:
        u = rng.random(n)
        held = np.nonzero(u < p_data + p_tomb)[0]
        m._f(f)
        v = rng.integers(0, 6, len(held)).astype(np.int64)
        out = rng.random(len(held)) < far
        v[out] = np.where(rng.random(int(out.sum())) < 0.5, VAL_MAX, -VAL_MAX)
        m.set(f, held, v)
        tombs[f] = np.nonzero((u >= p_data) & (u < p_data + p_tomb))[0]
    return m, tombs


def apply_tombs(m, tombs):
    for f, idx in tombs.items():
        m.tomb(f, idx)


def load_table(x, m, tombs, ts=5):
    """x: an Engine or a Comm. Every held row as data, then the tombstones on top; the model follows."""
    for f in [FB] + PROBED:
        if (m.st[f] == DATA).any():
            x.load_rows(*m.rows(f, ts))
    for f, idx in tombs.items():
        if len(idx):
            x.put_rows(m.ids[idx], np.full(len(idx), f, np.uint32), np.full(len(idx), ts + 4, np.int64), np.full(len(idx), VAL_DELETED, np.int64))
    apply_tombs(m, tombs)


def _pair_lit(rng, pairs):
    p = pairs[int(rng.integers(0, len(pairs)))]
    kind = int(rng.integers(0, 8))
    if kind == 0:
        lo, hi = I64MIN, I64MAX                              # both present
    elif kind == 1:
        lo, hi = 1, I64MAX                                   # a > b
    elif kind == 2:
        lo, hi = I64MIN, int(rng.integers(-2, 3))            # a <= b + k
    elif kind == 3:
        lo = int(rng.integers(-2, 3)); hi = lo - 1           # an empty range
    elif kind <= 5:
        lo = hi = int(rng.integers(-2, 3))                   # a == b + k
    else:
        lo = int(rng.integers(-4, 3)); hi = lo + int(rng.integers(0, 4))
    return (p, lo, hi, bool(rng.random() < 0.35))


def _plain_lit(rng, fields):
    f = fields[int(rng.integers(0, len(fields)))]
    lo = int(rng.integers(-1, 5)); hi = lo + int(rng.integers(0, 4))
    if rng.random() < 0.15:
        lo, hi = I64MIN, I64MAX
    return (f, lo, hi, bool(rng.random() < 0.35))


def seeded_programs(count=100, seed=20250302):
    """count programs of 1..4 clauses; a program names at most 4 ordered pairs and any plain fields (FB, F1..F4), so at most 8 slots; a clause takes at
    most 8 entries and a program at most 32. About a fifth are plain only, a fifth pairs only, the rest mixed."""
    rng = np.random.default_rng(seed)
    fields = [FB] + PROBED
    progs = []
    while len(progs) < count:
        style = rng.random()
        k = int(rng.integers(1, 5))
        pairs = []
        while len(pairs) < k:
            a, b = (fields[int(j)] for j in rng.choice(len(fields), 2, replace=False))
            if (a, b) not in pairs:
                pairs.append((a, b))
        if rng.random() < 0.3 and len(pairs) < 4:
            pairs.append((pairs[0][1], pairs[0][0]))         # (A, B) next to (B, A)
        plain = [fields[int(j)] for j in rng.choice(len(fields), int(rng.integers(1, 4)), replace=False)]
        p_pair = 0.0 if style < 0.2 else 1.0 if style < 0.4 else 0.5
        prog, total = [], 0
        for _ in range(int(rng.integers(1, 5))):
            c, used = [], 0
            want = int(rng.integers(1, 5))
            while len(c) < want:
                t = _pair_lit(rng, pairs) if rng.random() < p_pair else _plain_lit(rng, plain)
                if used + (2 if is_pair(t) else 1) > MAX_CLAUSE:
                    break
                c.append(t); used += 2 if is_pair(t) else 1
            if total + used > MAX_LITS:
                break
            prog.append(c); total += used
        progs.append(prog)
    return progs
