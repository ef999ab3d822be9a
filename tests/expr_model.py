"""Computed measures (include/bmx_expr.h): the measure of a selected node is value(a) op value(b), op one of + - *. Shared by test_expr_model.py (CPU) and
the GPU tests (helper, not a test). An expression is written (a, op, b) with op "+", "-" or "*"; E(e) makes the bmx.Expr of it.

brute_agg / brute_group / brute_quant : the truth, node by node with Python ints and dicts, straight from the header's sentences: the selection
                                 (where_clock_model.brute), the node's class (classify), then counts, sums, minima and maxima, or the sorted sample. No numpy
                                 arithmetic touches a value, so no integer overflow can hide in it. Each returns the bytes the call must give (records of
                                 bmx.AGG_DTYPE / GROUP_DTYPE / QUANT_REC_DTYPE, the result record, (n_undef, n_range)).
measure(m, e) and model_*      : the numpy model on the state tables of where_clock_model.ClockModel: class and value per node as arrays (the product through
                                 Python-int object arrays), the records by masks. test_expr_model.py holds it against brute.
fetch()                        : a sequential stand-in of expr_fetch + expr_value (csrc/expr_kernels.h) for one lane: ONE probe loop over a, b and the group
                                 field, b == a probed once, the overflow-checked product. It notes every probe as (field) and the PATHS a node took (TAGS).
                                 `defect` switches on ONE mistake a kernel could make (DEFECTS); standin_agg() is the flat aggregate built from it.
edge_layouts(wide)             : the tables of test_gpu_where_expr_kernel_edges.py, by position; the CPU test shows that they expose every defect.
seeded_table / seeded_programs : the seeded generator; every program it gives has at least one undefined and one out-of-range node among its selection."""
import numpy as np

import bmx
import where_clock_model as wcm
from where_clock_model import ABSENT, DATA, TOMB, EDGE_SIZES, F1, F2, F3, F4, FB, I64MAX, I64MIN, PROBED, VAL_DELETED, VAL_MAX, ClockModel, edge_spots, node_ids  # noqa: F401

OPS = ("+", "-", "*")
DEFINED, UNDEF, RANGE = 0, 1, 2
TAGS = ("both_column", "a_column", "b_column", "same_field_one_probe", "two_probes", "undef_a", "undef_b", "undef_tomb", "range_mul_128", "range_mul_64", "range_add")
DEFECTS = ("mul_wrapped_64", "no_range_check", "tomb_as_value", "n_is_match", "sub_swapped", "undef_in_range")
EMPTY_MIN, EMPTY_MAX = I64MAX, I64MIN          # what min / max of a record hold when nothing was measured


def E(e):
    return bmx.Expr(e[0], e[1], e[2])


def apply_op(op, x, y):
    return x + y if op == "+" else x - y if op == "-" else x * y


def _wrap(v):
    return ((v + (1 << 63)) % (1 << 64)) - (1 << 63)


# ---- the truth ----
def classify(m, e, i):
    """-> (DEFINED, value) | (UNDEF, None) | (RANGE, None) for node i, Python ints"""
    a, op, b = e
    m._f(a); m._f(b)
    if m.st[a][i] != DATA or m.st[b][i] != DATA:
        return UNDEF, None
    r = apply_op(op, int(m.val[a][i]), int(m.val[b][i]))
    return (DEFINED, r) if -VAL_MAX <= r <= VAL_MAX else (RANGE, None)


class Rec:
    """one bmx_agg, as Python ints"""

    def __init__(self):
        self.n_match, self.n, self.min, self.max, self.sum = 0, 0, EMPTY_MIN, EMPTY_MAX, 0

    def add(self, cls, v):
        self.n_match += 1
        if cls == DEFINED:
            self.n += 1; self.sum += v; self.min = min(self.min, v); self.max = max(self.max, v)

    def tup(self):
        s = self.sum % (1 << 128)
        hi = s >> 64
        return (self.n_match, self.n, self.min, self.max, s & ((1 << 64) - 1), hi - (1 << 64) if hi >= (1 << 63) else hi)


def agg_bytes(recs):
    return np.array([r.tup() for r in recs], bmx.AGG_DTYPE)


def selection(m, base, clauses):
    return np.nonzero(wcm.brute(m, base, clauses))[0]


def brute_agg(m, base, clauses, e, group=None, group_lo=0, ngroups=0, sel=None):
    """-> (records: ndarray of AGG_DTYPE, ngroups + 1 of them (1 when ungrouped), (n_undef, n_range))"""
    recs = [Rec() for _ in range(ngroups + 1 if ngroups else 1)]
    x = [0, 0]
    if group is not None:
        m._f(group)
    for i in (selection(m, base, clauses) if sel is None else sel):
        cls, v = classify(m, e, i)
        if cls != DEFINED:
            x[cls - 1] += 1
        g = 0
        if ngroups:
            gv = int(m.val[group][i])
            g = gv - group_lo if m.st[group][i] == DATA and group_lo <= gv < group_lo + ngroups else ngroups
        recs[g].add(cls, v)
    return agg_bytes(recs), tuple(x)


def brute_group(m, base, clauses, e, group, cap=65536, sel=None):
    """-> (records: ndarray of GROUP_DTYPE sorted by key, or None on overflow; res: ndarray of GROUP_RES_DTYPE (n_groups 0 on overflow: the call gives a lower
    bound there); (n_undef, n_range))"""
    m._f(group)
    by_key, absent, total, x = {}, Rec(), Rec(), [0, 0]
    for i in (selection(m, base, clauses) if sel is None else sel):
        cls, v = classify(m, e, i)
        if cls != DEFINED:
            x[cls - 1] += 1
        total.add(cls, v)
        if m.st[group][i] == DATA:
            by_key.setdefault(int(m.val[group][i]), Rec()).add(cls, v)
        else:
            absent.add(cls, v)
    over = len(by_key) > cap
    res = np.zeros(1, bmx.GROUP_RES_DTYPE)
    res["n_groups"] = 0 if over else len(by_key); res["flags"] = bmx.GROUP_OVERFLOW if over else 0
    res["absent"] = agg_bytes([absent])[0]; res["total"] = agg_bytes([total])[0]
    if over:
        return None, res, tuple(x)
    recs = np.zeros(len(by_key), bmx.GROUP_DTYPE)
    for j, k in enumerate(sorted(by_key)):
        recs[j]["key"] = k; recs[j]["agg"] = agg_bytes([by_key[k]])[0]
    return recs, res, tuple(x)


def brute_quant(m, base, clauses, e, qs, sel=None):
    """-> (records: ndarray of QUANT_REC_DTYPE in the order of qs, res: ndarray of QUANT_RES_DTYPE, (n_undef, n_range))"""
    sample, n_match, x = [], 0, [0, 0]
    for i in (selection(m, base, clauses) if sel is None else sel):
        n_match += 1
        cls, v = classify(m, e, i)
        if cls == DEFINED:
            sample.append(v)
        else:
            x[cls - 1] += 1
    sample.sort()
    n = len(sample)
    recs = np.zeros(len(qs), bmx.QUANT_REC_DTYPE)
    for j, (num, den) in enumerate(qs):
        if n:
            r = (num * (n - 1)) // den
            v = sample[r]
            recs[j] = (v, r, sum(1 for s in sample if s < v), sum(1 for s in sample if s == v))
    res = np.zeros(1, bmx.QUANT_RES_DTYPE)
    res[0] = (n_match, n, sample[0] if n else EMPTY_MIN, sample[-1] if n else EMPTY_MAX)
    return recs, res, tuple(x)


# ---- the numpy model ----
def measure(m, e):
    """-> (cls: uint8 per node, val: int64 per node, 0 where the node is not DEFINED)"""
    a, op, b = e
    m._f(a); m._f(b)
    both = (m.st[a] == DATA) & (m.st[b] == DATA)
    x, y = m.val[a].astype(object), m.val[b].astype(object)          # Python ints: the product of two 54-bit numbers has 107 bits
    r = apply_op(op, x, y)
    inr = np.array([-VAL_MAX <= int(v) <= VAL_MAX for v in r], bool) if m.N else np.zeros(0, bool)
    cls = np.where(~both, UNDEF, np.where(inr, DEFINED, RANGE)).astype(np.uint8)
    val = np.array([int(v) if c == DEFINED else 0 for v, c in zip(r, cls)], np.int64) if m.N else np.zeros(0, np.int64)
    return cls, val


def _model_rec(sel, cls, val):
    """the record of the nodes in the mask sel"""
    r = Rec()
    d = sel & (cls == DEFINED)
    r.n_match, r.n = int(sel.sum()), int(d.sum())
    if r.n:
        r.sum = int(val[d].astype(object).sum()); r.min = int(val[d].min()); r.max = int(val[d].max())
    return r


def _model_x(sel, cls):
    return int((sel & (cls == UNDEF)).sum()), int((sel & (cls == RANGE)).sum())


def model_agg(m, base, clauses, e, group=None, group_lo=0, ngroups=0):
    sel = m.mask(base, clauses)
    cls, val = measure(m, e)
    if not ngroups:
        return agg_bytes([_model_rec(sel, cls, val)]), _model_x(sel, cls)
    m._f(group)
    gv = m.val[group]
    inw = (m.st[group] == DATA) & (gv >= group_lo) & (gv < group_lo + ngroups)       # (group_lo + ngroups stays far inside int64 in every test)
    recs = [_model_rec(sel & inw & (gv == group_lo + g), cls, val) for g in range(ngroups)] + [_model_rec(sel & ~inw, cls, val)]
    return agg_bytes(recs), _model_x(sel, cls)


def model_group(m, base, clauses, e, group, cap=65536):
    sel = m.mask(base, clauses)
    cls, val = measure(m, e)
    m._f(group)
    has = m.st[group] == DATA
    keys = np.unique(m.val[group][sel & has])
    over = len(keys) > cap
    res = np.zeros(1, bmx.GROUP_RES_DTYPE)
    res["n_groups"] = 0 if over else len(keys); res["flags"] = bmx.GROUP_OVERFLOW if over else 0
    res["absent"] = agg_bytes([_model_rec(sel & ~has, cls, val)])[0]; res["total"] = agg_bytes([_model_rec(sel, cls, val)])[0]
    if over:
        return None, res, _model_x(sel, cls)
    recs = np.zeros(len(keys), bmx.GROUP_DTYPE)
    for j, k in enumerate(keys):
        recs[j]["key"] = k; recs[j]["agg"] = agg_bytes([_model_rec(sel & has & (m.val[group] == k), cls, val)])[0]
    return recs, res, _model_x(sel, cls)


def model_quant(m, base, clauses, e, qs):
    sel = m.mask(base, clauses)
    cls, val = measure(m, e)
    s = np.sort(val[sel & (cls == DEFINED)])
    n = len(s)
    recs = np.zeros(len(qs), bmx.QUANT_REC_DTYPE)
    for j, (num, den) in enumerate(qs):
        if n:
            r = bmx.quant_rank(num, den, n)
            recs[j] = (s[r], r, int((s < s[r]).sum()), int((s == s[r]).sum()))
    res = np.zeros(1, bmx.QUANT_RES_DTYPE)
    res[0] = (int(sel.sum()), n, s[0] if n else EMPTY_MIN, s[-1] if n else EMPTY_MAX)
    return recs, res, _model_x(sel, cls)


def shadow(m, s, e):
    """field s := the expression's value on exactly the nodes where it is DEFINED, absent elsewhere: the plain form on s measures what the expression form
    measures on (a, op, b)"""
    cls, val = measure(m, e)
    idx = np.nonzero(cls == DEFINED)[0]
    m.val.pop(s, None); m.st.pop(s, None); m.ts.pop(s, None); m._f(s)
    m.set(s, idx, val[idx], ts=3)


# ---- the stand-in ----
def _probe(m, f, i):
    """agg_probe: a tombstoned row IS found, with VAL_DELETED in it"""
    m._f(f)
    st = m.st[f][i]
    return (st != ABSENT), (int(m.val[f][i]) if st == DATA else VAL_DELETED)


def fetch(m, base, e, i, group=None, defect=None, tags=None, probes=None):
    """expr_fetch + expr_value for the SELECTED node i -> (cls, value or None, have_g, gval)"""
    fa, op, fb = e
    x = int(m.val[base][i])
    a = b = gval = x
    have_a, have_b, have_g = fa == base, fb == base, group == base
    same = fb == fa and fb != base
    srcs = [(fa, not have_a), (fb, not have_b and not same), (group, group is not None and group != base)]
    for k, (f, probed) in enumerate(srcs):          # ONE loop, three rounds: a, b, the group field
        if not probed:
            continue
        if probes is not None:
            probes.append(f)
        found, y = _probe(m, f, i)
        if found and (y != VAL_DELETED or (defect == "tomb_as_value" and k < 2)):
            if k == 0:
                a, have_a = y, True
            elif k == 1:
                b, have_b = y, True
            else:
                gval, have_g = y, True
        elif tags is not None and k < 2:
            tags.add("undef_tomb" if found else ("undef_a" if k == 0 else "undef_b"))
            if found and same:
                tags.add("undef_tomb")
    if same:
        b, have_b = a, have_a
    if tags is not None:
        tags.add("both_column" if fa == base and fb == base else "a_column" if fa == base else "b_column" if fb == base else "same_field_one_probe" if same else "two_probes")
    have = have_a and have_b
    if defect == "sub_swapped" and op == "-":
        a, b = b, a
    exact = apply_op(op, a, b)
    fits64 = I64MIN <= exact <= I64MAX
    p = _wrap(exact)
    if op == "*":
        inr = fits64 or defect == "mul_wrapped_64"   # __builtin_mul_overflow; the defect looks at the low 64 bits alone
    else:
        inr = True                                   # (|a|, |b| <= 2^53 - 1: the sum fits 64 bits)
    inr = inr and (-VAL_MAX <= p <= VAL_MAX or defect == "no_range_check")
    if tags is not None and have and not (-VAL_MAX <= exact <= VAL_MAX):
        tags.add("range_add" if op != "*" else "range_mul_64" if fits64 else "range_mul_128")
    if not have:
        return (RANGE if defect == "undef_in_range" else UNDEF), None, have_g, gval
    return (DEFINED, p, have_g, gval) if inr else (RANGE, None, have_g, gval)


def standin_agg(m, base, clauses, e, defect=None, tags=None, probes=None, sel=None):
    """the flat aggregate (one record, (n_undef, n_range)) as the lanes' stand-in gives it"""
    r, x = Rec(), [0, 0]
    for i in (selection(m, base, clauses) if sel is None else sel):
        cls, v, _, _ = fetch(m, base, e, i, None, defect, tags, probes)
        if cls != DEFINED:
            x[cls - 1] += 1
        r.add(cls, v)
    if defect == "n_is_match":
        r.n = r.n_match                                # k_agg_finish's shortcut, which holds for no computed measure
    return agg_bytes([r]), tuple(x)


# ---- the layouts of the kernel-edge tests ----
ALL = [[(FB, I64MIN, I64MAX)]]          # every node that holds the base field
P1, P2 = 441650591, 20394401            # P1 * P2 = 2^53 - 1
BIG = 1 << 32


def edge_table(ids, node, wide):
    """-> ClockModel: FB on every node (3, + 2^40 when wide), F1 = 5 and F2 = 7 everywhere: every node DEFINED for every op. node[p]: the node at position p."""
    n = len(ids)
    m = ClockModel(ids)
    m.set(FB, node, np.full(n, 3 + ((1 << 40) if wide else 0)), ts=7)
    m.set(F1, node, np.full(n, 5)); m.set(F2, node, np.full(n, 7))
    return m


def edge_layouts(wide, n=65, width=None):
    """yields (name, mutate(m, node) or None, expr, probed fields per selected node in order). The mutations accumulate on one table (built by edge_table), as
    the GPU test applies them to one engine. The selection is ALL. width: the column's elements per 16-byte unit (4 / 2); default by `wide`."""
    Ew = width or (2 if wide else 4)
    wave = 64 * Ew

    def lone(cls, p):
        """every node of the class's opposite, the node at p alone in `cls`"""
        def mut(m, node, p=p):
            k = len(node)
            others = np.delete(node, p)
            if cls == DEFINED:        # everybody else lacks F1 (tombstoned at even positions, never written at odd ones would need a new table: tombstones do)
                m.tomb(F1, others); m.set(F1, node[[p]], [5])
            elif cls == UNDEF:
                m.set(F1, others, np.full(k - 1, 5)); m.tomb(F1, node[[p]])
            else:
                m.set(F1, others, np.full(k - 1, 5)); m.set(F1, node[[p]], [VAL_MAX])
            m.set(F2, node, np.full(k, 7))
        return mut

    for p in edge_spots(n, Ew):
        yield ("lone defined node at %d" % p, lone(DEFINED, p), (F1, "+", F2), [F1, F2])
        yield ("lone undefined node at %d" % p, lone(UNDEF, p), (F1, "*", F2), [F1, F2])
        yield ("lone out-of-range node at %d" % p, lone(RANGE, p), (F1, "+", F2), [F1, F2])

    def restore(m, node):
        m.set(F1, node, np.full(len(node), 5)); m.set(F2, node, np.full(len(node), 7))
    yield ("everybody defined again", restore, (F2, "-", F1), [F2, F1])

    def wave_out(m, node):          # the first wave's rows (all of them when the column is shorter) all out of range
        k = min(len(node), wave)
        m.set(F1, node[:k], np.full(k, 1 << 27)); m.set(F2, node[:k], np.full(k, 1 << 26))
    yield ("a wave all out of range", wave_out, (F1, "*", F2), [F1, F2])

    def products(m, node):          # the products at the edge of the range, one after the other by position
        k = len(node)
        pa = np.array([P1, 1 << 26, 94906265, 94906266, VAL_MAX, BIG, 0, -1, 1, -VAL_MAX, -P1], np.int64)
        pb = np.array([P2, 1 << 27, 94906265, 94906267, VAL_MAX, BIG + 1, VAL_MAX, VAL_MAX, -VAL_MAX, -VAL_MAX, P2], np.int64)
        j = np.arange(k) % len(pa)
        m.set(F1, node, pa[j]); m.set(F2, node, pb[j])
    yield ("products at the edge", products, (F1, "*", F2), [F1, F2])
    yield ("sums at the edge", None, (F1, "+", F2), [F1, F2])
    yield ("differences, a - b", None, (F1, "-", F2), [F1, F2])
    yield ("differences, b - a", None, (F2, "-", F1), [F2, F1])
    yield ("squares: one probe", None, (F1, "*", F1), [F1])
    yield ("base * probed", None, (FB, "*", F1), [F1])
    yield ("probed - base", None, (F2, "-", FB), [F2])
    yield ("base * base: no probe", None, (FB, "*", FB), [])

    def states(m, node):            # a tombstone is no value, on either side; an absent row neither (fx: a field some nodes never held)
        m.set(F1, node, np.full(len(node), 2)); m.set(F2, node, np.full(len(node), 3))
        m.tomb(F1, node[::3]); m.tomb(F2, node[1::4])
    yield ("tombstones on either side", states, (F1, "*", F2), [F1, F2])
    yield ("tombstones, doubled", None, (F1, "+", F1), [F1])


# ---- the seeded generator ----
PLANT = 77                      # the base values PLANT .. PLANT + 4 belong to the planted nodes; the random ones stay below
SIGNS = [(1, 1, 1, 1), (1, -1, 1, -1), (-1, 1, -1, 1), (1, 1, -1, -1)]      # the planted out-of-range nodes' F1..F4, times VAL_MAX


def seeded_table(n, seed=20250501, salt=0, wide=False):
    """-> ClockModel: FB on 90 % of the nodes (5 % absent, 5 % tombstoned), F1..F4 each data / absent / tombstoned on 60 / 25 / 15 %, small values -3..5 with a
    few at +-VAL_MAX, +-2^27 and +-94906266, so that every op has nodes on both sides of the range. The last 5 nodes are planted: one that holds the base field
    alone (undefined for every expression with a probed operand) and four with F1..F4 at +-VAL_MAX in the sign patterns SIGNS (out of range for + and * in the
    first, for every difference of two distinct operands in one of the others)."""
    rng = np.random.default_rng(seed)
    m = ClockModel(node_ids(n + 5, 90_000 + salt))
    off = (1 << 40) if wide else 0
    for f, (p_data, p_tomb) in [(FB, (0.90, 0.05))] + [(f, (0.60, 0.15)) for f in PROBED]:
        u = rng.random(n)
        held = np.nonzero(u < p_data + p_tomb)[0]
        v = rng.integers(-3, 6, len(held)).astype(np.int64)
        far = rng.random(len(held)) < 0.06
        v[far] = rng.choice(np.array([VAL_MAX, -VAL_MAX, 1 << 27, -(1 << 27), 94906266, -94906266, 1 << 26], np.int64), int(far.sum()))
        if f == FB:
            v = np.where(far, v, v + off)
        m.set(f, held, v)
        m.tomb(f, np.nonzero((u >= p_data) & (u < p_data + p_tomb))[0])
    planted = np.arange(n, n + 5)
    m.set(FB, planted, PLANT + np.arange(5) + off)
    for j, sg in enumerate(SIGNS):
        for f, s1 in zip(PROBED, sg):
            m.set(f, planted[[1 + j]], [s1 * VAL_MAX])
    return m


def plant_clause(wide=False):
    off = (1 << 40) if wide else 0
    return [(FB, PLANT + off, PLANT + 4 + off)]


def seeded_programs(count=60, seed=20250502, wide=False):
    """count (clauses, (a, b)) pairs: wcm's seeded programs of plain, pair and clock literals with the planted nodes' clause behind them, and two operands of
    which at least one is probed. A pair goes with all three ops; a == b is left to + and * (a - a is 0 wherever it is defined): ops_of()."""
    rng = np.random.default_rng(seed)
    fields = [FB] + PROBED
    out = []
    for prog in wcm.seeded_programs(count, seed + 1):
        while True:
            a, b = (fields[int(j)] for j in rng.integers(0, len(fields), 2))
            if (a, b) != (FB, FB):
                break
        while sum(wcm.entries(c) for c in prog) >= wcm.MAX_LITS:     # room for the planted nodes' literal
            prog = prog[:-1]
        out.append((prog + [plant_clause(wide)], (a, b)))
    return out


def ops_of(a, b):
    return ("+", "*") if a == b else OPS


# ---- the calls as the library wrote them, into buffers that held a pattern (x: an Engine or a Comm) ----
FILL = 0xA5


def _xres(xr):
    assert (xr[16:] == FILL).all(), "bytes behind the bmx_expr_res were written"
    v = xr[:16].view(bmx.EXPR_RES_DTYPE)[0]
    return int(v["n_undef"]), int(v["n_range"])


def _call(x, name, args):
    import ctypes as C  # noqa: F401
    one = isinstance(x, bmx.Engine)
    fn = getattr(x.L, ("bmx_" if one else "bmx_comm_") + name)
    x._chk(fn(x.h, *args, bmx.MEM_HOST) if one else fn(x.h, *args))


def _eptr(e):
    import ctypes as C
    ex = E(e)
    return ex, C.cast(C.byref(ex), C.c_void_p)


def raw_agg(x, base, clauses, e, group=None, group_lo=0, ngroups=0):
    """-> (records, (n_undef, n_range)) as brute_agg gives them"""
    nrec = ngroups + 1 if ngroups else 1
    out = np.full(48 * (nrec + 1), FILL, np.uint8).view(bmx.AGG_DTYPE)
    xr = np.full(32, FILL, np.uint8)
    ex, p = _eptr(e)
    _call(x, "where_aggregate_expr", (*bmx._where_args(base, clauses), p, bmx.AGG_NO_FIELD if group is None else int(group), int(group_lo), int(ngroups), bmx._ptr(out), bmx._ptr(xr)))
    assert (out[nrec:].view(np.uint8) == FILL).all(), "bytes behind the records were written"
    return out[:nrec].copy(), _xres(xr)


def raw_group(x, base, clauses, e, group, cap=65536):
    """-> (records or None on overflow, res, (n_undef, n_range)) as brute_group gives them; on overflow n_groups (a lower bound above cap) is checked here and
    zeroed, and no record may have been written"""
    out = np.full(56 * (cap + 1), FILL, np.uint8).view(bmx.GROUP_DTYPE)
    res = np.full(112 + 16, FILL, np.uint8)
    xr = np.full(32, FILL, np.uint8)
    ex, p = _eptr(e)
    _call(x, "where_group_expr", (*bmx._where_args(base, clauses), p, int(group), bmx._ptr(out), int(cap), bmx._ptr(res), bmx._ptr(xr)))
    assert (res[112:] == FILL).all(), "bytes behind the result record were written"
    r = res[:112].view(bmx.GROUP_RES_DTYPE).copy()
    if int(r[0]["flags"]) & bmx.GROUP_OVERFLOW:
        assert int(r[0]["n_groups"]) > cap and (out.view(np.uint8) == FILL).all()
        r["n_groups"] = 0
        return None, r, _xres(xr)
    n = int(r[0]["n_groups"])
    assert n <= cap and (out[n:].view(np.uint8) == FILL).all(), "bytes behind the records were written"
    return out[:n].copy(), r, _xres(xr)


def raw_quant(x, base, clauses, e, qs):
    """-> (records, res, (n_undef, n_range)) as brute_quant gives them"""
    out = np.full(32 * (len(qs) + 1), FILL, np.uint8).view(bmx.QUANT_REC_DTYPE)
    res = np.full(32 + 16, FILL, np.uint8)
    xr = np.full(32, FILL, np.uint8)
    ex, p = _eptr(e)
    _call(x, "where_quantiles_expr", (*bmx._where_args(base, clauses), p, *bmx._quant_tail(0, qs)[1:], bmx._ptr(out), bmx._ptr(res), bmx._ptr(xr)))
    assert (out[len(qs):].view(np.uint8) == FILL).all() and (res[32:] == FILL).all(), "bytes behind the answer were written"
    return out[:len(qs)].copy(), res[:32].view(bmx.QUANT_RES_DTYPE).copy(), _xres(xr)


def same(a, b):
    """two answers (tuples of arrays, None and tuples of ints), byte for byte"""
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b
