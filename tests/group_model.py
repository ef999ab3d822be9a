"""A numpy model of the group-by over discovered values (include/bmx_group.h, csrc/group_kernels.h), shared by test_group_model.py (CPU) and the GPU tests
(helper, not a test). The table and the selection are where_agg_model's (a state per field and node: absent, data, tombstone).

Two halves:

answer(m, base, clauses, group, measure, cap) : the brute-force answer — numpy.unique over the selected nodes' group values, the records of where_agg_model
    (integer reductions, the 128-bit sum through Python ints) -> (records sorted by key, result record), or on overflow (no records, flags, absent, total).

The kernel's geometry, restated: mix() / home() (the global table's hash and home slot), cache_set() (the LDS cache: SETS sets of WAYS ways per workgroup),
slots_for(cap), and where a row of the base column runs: place(pos, n, E, cus) -> (workgroup, wave, lane, step). walk() inserts keys into a table in a given
order and reports each key's path: ('home',), ('walk', n), ('wrap', n) when the walk passed the last slot, ('noroom',). Device(...) is a sequential stand-in
engine built from these pieces: rows in position order, per workgroup a cache whose ways go to the keys that come first, bypass rows straight to the table,
one flush per workgroup, then k_group_finish's rule. It tags every row 'hit' or 'bypass' and every table access with walk()'s tags.

What does not depend on the order in which lanes arrive, and is therefore what the GPU tests assert from the model: the answer; the number of keys of one
workgroup and set that bypass (distinct keys - WAYS, if positive); the set of occupied slots; and, for keys that all share one home slot, the multiset of walk
lengths (0, 1, 2, ...). Which key gets which way or which slot depends on who comes first."""
import numpy as np

import where_agg_model as wam
from where_agg_model import DATA, Model  # noqa: F401

AGG_DTYPE = wam.AGG_DTYPE
GROUP_DTYPE = np.dtype([("key", "<i8"), ("agg", AGG_DTYPE)])
GROUP_RES_DTYPE = np.dtype([("n_groups", "<u8"), ("flags", "<u4"), ("reserved", "<u4"), ("absent", AGG_DTYPE), ("total", AGG_DTYPE)])
OVERFLOW, MAX_CAP = 1, 1 << 20
WAYS, SETS = 4, 256
CACHE = WAYS * SETS
THREADS, U = 512, 4                      # top_sweep: 512 lanes, 4 loads of 16 bytes in flight per lane
M64 = (1 << 64) - 1
FILL = 0x5A


# ---- the kernel's arithmetic ----
def mix(key):
    """MurmurHash3's 64-bit finalizer over the key's two's complement"""
    x = int(key) & M64
    x ^= x >> 33; x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33; x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def mix_np(keys):
    x = np.asarray(keys, np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xff51afd7ed558ccd)
        x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xc4ceb9fe1a85ec53)
        x = x ^ (x >> np.uint64(33))
    return x


def slots_for(cap):
    s = 64
    while s < 2 * cap:
        s <<= 1
    return s


def home(key, slots):
    return mix(key) & (slots - 1)


def cache_set(key):
    k = int(key) & M64
    return ((((k & 0xFFFFFFFF) ^ (k >> 32)) * 0x9E3779B1) & 0xFFFFFFFF) >> 24


def cache_set_np(keys):
    k = np.asarray(keys, np.int64).astype(np.uint64)
    w = ((k & np.uint64(0xFFFFFFFF)) ^ (k >> np.uint64(32))).astype(np.uint64)
    return (((w * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)).astype(np.int64)


def grid(n, E, cus=256):
    per_wg = 4 * THREADS * U * E
    return max(1, min((n + per_wg - 1) // per_wg, 2 * cus))


def place(pos, n, E, cus=256):
    """where the row at position pos of an n-row column runs -> (workgroup, wave, lane, step); step numbers the wave's calls of the row code in order"""
    pos = np.asarray(pos, np.int64)
    unit, e = pos // E, pos % E
    rnd, within = unit // (THREADS * U), unit % (THREADS * U)
    u, tid = within // THREADS, within % THREADS
    g = grid(n, E, cus)
    return rnd % g, tid // 64, tid % 64, ((rnd // g) * U + u) * E + e


def walk(keys, slots, table=None):
    """insert `keys` (distinct) in this order into a table of `slots` slots -> ({key: tag}, table); tag: ('home',) / ('walk', n) / ('wrap', n) / ('noroom',)"""
    table = {} if table is None else table          # slot -> key
    tags = {}
    for k in keys:
        h = home(k, slots)
        for p in range(slots):
            s = (h + p) & (slots - 1)
            if s not in table or table[s] == k:
                table[s] = k
                tags[k] = ("home",) if p == 0 else (("wrap", p) if h + p >= slots else ("walk", p))
                break
        else:
            tags[k] = ("noroom",)
    return tags, table


def keys_with_home(slot, slots, count, start=1, step=1, avoid=()):
    """the first `count` keys start, start + step, ... whose home slot is `slot`"""
    out, k = [], start
    while len(out) < count:
        if home(k, slots) == slot and k not in avoid:
            out.append(k)
        k += step
    return out


def keys_with_set(cset, count, start=1, step=1, avoid=()):
    out, k = [], start
    while len(out) < count:
        if cache_set(k) == cset and k not in avoid:
            out.append(k)
        k += step
    return out


# ---- the brute-force answer ----
def answer(m, base, clauses, group, measure=None, cap=65536):
    sel = m.mask(base, clauses)
    m._f(group)
    if measure is not None:
        m._f(measure)
    have_m = (m.st[measure] == DATA) if measure is not None else None

    def rec(rows):
        return wam.record(int(rows.sum()), None if measure is None else m.val[measure][rows & have_m])

    have_g = sel & (m.st[group] == DATA)
    res = np.zeros((), GROUP_RES_DTYPE)
    res["absent"] = rec(sel & ~have_g); res["total"] = rec(sel)
    keys = np.unique(m.val[group][have_g])
    res["n_groups"] = len(keys)
    if len(keys) > cap:
        res["flags"] = OVERFLOW
        return np.zeros(0, GROUP_DTYPE), res
    out = np.zeros(len(keys), GROUP_DTYPE)
    gv = m.val[group]
    for i, k in enumerate(keys):
        out[i]["key"] = k; out[i]["agg"] = rec(have_g & (gv == k))
    return out, res


def sum_of(r):
    return (int(r["sum_hi"]) << 64) + int(r["sum_lo"])


def invariant(recs, res):
    """sum of the groups + absent == total, for n_match, n and the sum"""
    t, a = res["total"], res["absent"]
    return (int(recs["agg"]["n_match"].sum()) + int(a["n_match"]) == int(t["n_match"]) and int(recs["agg"]["n"].sum()) + int(a["n"]) == int(t["n"])
            and sum(sum_of(x["agg"]) for x in recs) + sum_of(a) == sum_of(t))


def check(got_recs, got_res, want_recs, want_res, cap, host=True):
    """every comparison the GPU tests make -> None or what differs. got_recs: the caller's whole buffer of cap + 1 records, pattern-filled before the call."""
    got_recs = np.asarray(got_recs, GROUP_DTYPE)
    if bytes(np.asarray(got_res["absent"]).tobytes()) != bytes(np.asarray(want_res["absent"]).tobytes()):
        return ("absent", got_res["absent"], want_res["absent"])
    if bytes(np.asarray(got_res["total"]).tobytes()) != bytes(np.asarray(want_res["total"]).tobytes()):
        return ("total", got_res["total"], want_res["total"])
    if int(got_res["reserved"]) != 0:
        return ("reserved", int(got_res["reserved"]))
    if int(want_res["flags"]) & OVERFLOW:
        if int(got_res["flags"]) != OVERFLOW or not (cap < int(got_res["n_groups"]) <= int(want_res["n_groups"])):
            return ("overflow", int(got_res["flags"]), int(got_res["n_groups"]))
        return None if (got_recs.view(np.uint8) == FILL).all() else ("out written on overflow",)
    if int(got_res["flags"]) != 0 or int(got_res["n_groups"]) != len(want_recs):
        return ("n_groups / flags", int(got_res["flags"]), int(got_res["n_groups"]), len(want_recs))
    d = len(want_recs)
    if not (got_recs[d:].view(np.uint8) == FILL).all():
        return ("written at or beyond out[D]",)
    g = got_recs[:d]
    if host and not np.array_equal(g["key"], np.sort(g["key"])):
        return ("host records not sorted by key",)
    g = g[np.argsort(g["key"], kind="stable")]
    if g.tobytes() != np.asarray(want_recs, GROUP_DTYPE).tobytes():
        bad = [i for i in range(d) if g[i].tobytes() != want_recs[i].tobytes()]
        return ("record", bad[0], g[bad[0]], want_recs[bad[0]])
    if not invariant(g, got_res):
        return ("invariant",)
    return None


# ---- the sequential stand-in engine ----
class _Acc:
    __slots__ = ("nm", "vals")

    def __init__(self):
        self.nm = 0; self.vals = []

    def add(self, nm, val):
        self.nm += nm
        if val is not None:
            self.vals.append(val)

    def merge(self, o):
        self.nm += o.nm; self.vals += o.vals

    def record(self, measured):
        return wam.record(self.nm, np.array(self.vals, np.int64) if measured else None)


class Device:
    """One query over a column laid out by position. rows: per position (selected, group value or None, measure value or None). defect: None, or one of
    'drop_bypass' (a row that bypasses the cache is lost), 'lose_wrap' (a walk stops at the last slot instead of wrapping), 'absent_in_group' (a row without a
    group value is added to key 0), 'unsorted' (the host answer is left in table order)."""

    def __init__(self, n, E, cap, measured, cus=256, defect=None):
        self.n, self.E, self.cap, self.measured, self.cus, self.defect = n, E, cap, measured, cus, defect
        self.slots = slots_for(cap)
        self.table, self.acc, self.claims, self.overflow = {}, {}, 0, False
        self.tags = set(); self.row_tags = {}
        self.absent, self.total = _Acc(), _Acc()

    def _slot(self, key):
        h = home(key, self.slots)
        for p in range(self.slots):
            if self.defect == "lose_wrap" and h + p >= self.slots:
                break
            s = (h + p) & (self.slots - 1)
            if s not in self.table:
                self.table[s] = key; self.acc[s] = _Acc(); self.claims += 1
            if self.table[s] == key:
                self.tags.add("home" if p == 0 else ("wrap" if h + p >= self.slots else "walk"))
                if p:
                    self.tags.add(("len", p))
                return s
            if (p & 63) == 63 and self.claims > self.cap:
                break
        self.overflow = True; self.tags.add("noroom")
        return None

    def run(self, sel, gkey, mval):
        """sel[pos]: bool; gkey[pos]: int or None; mval[pos]: int or None"""
        pos = np.arange(self.n)
        wg, wave, lane, step = place(pos, self.n, self.E, self.cus)
        for g in range(grid(self.n, self.E, self.cus)):
            cache = {}                                     # set -> {key: _Acc}
            for p in pos[wg == g]:
                if not sel[p]:
                    continue
                self.total.add(1, mval[p])
                k = gkey[p]
                if k is None:
                    self.absent.add(1, mval[p])
                    if self.defect != "absent_in_group":
                        continue
                    k = 0
                ways = cache.setdefault(cache_set(k), {})
                if k in ways or len(ways) < WAYS:
                    ways.setdefault(k, _Acc()).add(1, mval[p]); self.row_tags[int(p)] = "hit"; self.tags.add("hit")
                    continue
                self.row_tags[int(p)] = "bypass"; self.tags.add("bypass")
                if self.defect == "drop_bypass":
                    continue
                s = self._slot(k)
                if s is not None:
                    self.acc[s].add(1, mval[p])
            for ways in cache.values():                    # the flush
                for k, a in ways.items():
                    s = self._slot(k)
                    if s is not None:
                        self.acc[s].merge(a)
        return self.finish()

    def finish(self):
        res = np.zeros((), GROUP_RES_DTYPE)
        res["absent"] = self.absent.record(self.measured); res["total"] = self.total.record(self.measured)
        res["n_groups"] = self.claims
        out = np.full(56 * (self.cap + 1), FILL, np.uint8).view(GROUP_DTYPE)
        if self.claims > self.cap or self.overflow:
            res["flags"] = OVERFLOW
            return out, res
        order = sorted(self.table) if self.defect == "unsorted" else sorted(self.table, key=lambda s: self.table[s])
        for i, s in enumerate(order):
            out[i]["key"] = self.table[s]; out[i]["agg"] = self.acc[s].record(self.measured)
        return out, res


def rows_of(m, base, clauses, group, measure, pos_nodes):
    """the model's table in position order -> (sel, gkey, mval) for Device.run; pos_nodes: node numbers of the base index's positions"""
    sel = m.mask(base, clauses)[pos_nodes]
    m._f(group)
    gk = [int(v) if s == DATA else None for v, s in zip(m.val[group][pos_nodes], m.st[group][pos_nodes])]
    if measure is None:
        mv = [None] * len(pos_nodes)
    else:
        m._f(measure)
        mv = [int(v) if s == DATA else None for v, s in zip(m.val[measure][pos_nodes], m.st[measure][pos_nodes])]
    return sel, gk, mv


# ---- helpers of the GPU tests ----
def raw_group(x, base, clauses, group, measure=None, cap=64, room=None):
    """bmx_where_group (Engine) / bmx_comm_where_group (Comm), host memory, into pattern-filled buffers -> (the whole buffer of cap + 1 records, result record)"""
    import ctypes as C

    import bmx
    out = np.full(56 * ((cap if room is None else room) + 1), FILL, np.uint8).view(GROUP_DTYPE)
    res = np.full(112, FILL, np.uint8).view(GROUP_RES_DTYPE)
    args = (*bmx._where_args(base, clauses), *bmx._group_tail(measure, group), bmx._ptr(out), int(cap), bmx._ptr(res))
    x._chk(x.L.bmx_where_group(x.h, *args, bmx.MEM_HOST) if isinstance(x, bmx.Engine) else x.L.bmx_comm_where_group(x.h, *args))
    return out, res[0]


def ask(x, m, base, clauses, group, measure=None, cap=64):
    """one query checked against the brute-force answer -> (records, result record)"""
    out, res = raw_group(x, base, clauses, group, measure, cap)
    want = answer(m, base, clauses, group, measure, cap)
    bad = check(out, res, *want, cap)
    assert bad is None, (clauses, group, measure, cap, bad)
    return out[:0 if int(res["flags"]) else int(res["n_groups"])].copy(), res


# ---- the seeded suite (the CPU test asserts what it relies on; the GPU test runs it) ----
def _names():
    from oracle import streams
    f = {k: streams.fnv1a32("group." + k) for k in ("base", "one", "two", "three", "four", "five", "measure", "key", "nobody", "select")}
    f["more"] = [streams.fnv1a32("group.extra%d" % k) for k in range(3)]
    return f


BIG = 2**53 - 1
WIDE = 2**40
N_SEED, SEED_TABLE, SEED_PROGS, N_PROGS = 5000, 60606, 20250924, 60   # (the program seed: the first from 20250919 on that meets test_group_model.py's conditions)


def seeded_model(wide=False):
    """5000 nodes: a base field 0..11, five probed fields and three more 0..5 in all three states, a measure field of both signs, and a key field nobody's
    program names: 300 sparse values over +-(2^53 - 1), among them 0, +-1 and +-(2^53 - 1). wide: one more node whose base value forces the int64 column."""
    F = _names()
    rng = np.random.default_rng(SEED_TABLE)
    n = N_SEED + (1 if wide else 0)
    m = Model(wam.node_ids(n, 8800))
    m.set(F["base"], np.arange(N_SEED), rng.integers(0, 12, N_SEED))
    tombs = {}
    for f, pr in zip([F[k] for k in ("one", "two", "three", "four", "five")] + F["more"], (0.9, 0.7, 0.5, 0.3, 0.6, 0.33, 0.33, 0.33)):
        idx = np.nonzero(rng.random(N_SEED) < pr)[0]
        m.set(f, idx, rng.integers(0, 6, len(idx)))
        tombs[f] = idx[rng.random(len(idx)) < 0.1]
    pool = np.concatenate([[0, 1, -1, BIG, -BIG], rng.integers(-BIG, BIG, 295)])
    idx = np.nonzero(rng.random(N_SEED) < 0.7)[0]
    m.set(F["key"], idx, pool[rng.integers(0, len(pool), len(idx))]); tombs[F["key"]] = idx[rng.random(len(idx)) < 0.1]
    idx = np.nonzero(rng.random(N_SEED) < 0.8)[0]
    m.set(F["measure"], idx, rng.integers(-WIDE, WIDE, len(idx))); tombs[F["measure"]] = idx[rng.random(len(idx)) < 0.1]
    tombs[F["base"]] = np.arange(17, N_SEED, 97)
    if wide:
        m.set(F["base"], [N_SEED], [WIDE]); m.set(F["key"], [N_SEED], [5]); m.set(F["one"], [N_SEED], [3])
    return m, tombs


def seeded_queries():
    """-> [(clauses, group field, measure field or None)]: the programs crossed with group = base field / a field of the program / the key field nobody names,
    measure = none / base / probed"""
    F = _names()
    probed = [F[k] for k in ("one", "two", "three", "four", "five")]
    out = []
    for k, p in enumerate(wam.random_programs(N_PROGS, SEED_PROGS, F["base"], probed, F["more"])):
        named = [t[0] for c in p for t in c if t[0] != F["base"]]
        group = [F["base"], named[0] if named else F["one"], F["key"], named[-1] if named else F["two"]][k % 4]
        measure = [None, F["base"], F["measure"]][(k // 4) % 3]
        out.append((p, group, measure))
    return out


def apply_tombs(m, tombs):
    for f, idx in tombs.items():
        m.tomb(f, idx)


# ---- the edge suite: columns laid out by position (both the CPU stand-in and the GPU run them) ----
def edge_layouts(wide):
    """-> [dict(name, n, cap, keys (int64 by position), present (bool by position), sel (bool by position), tags (what Device must reach), base (the keys may
    also be the base column itself))]"""
    E = 2 if wide else 4
    rnd = THREADS * U * E                                     # rows of one round of a workgroup: 8192 / 4096
    start = WIDE if wide else 1
    L = []

    def add(name, n, cap, keys, tags, sel=None, present=None, base=False):
        keys = np.asarray(keys, np.int64)
        L.append(dict(name=name, n=n, cap=cap, keys=keys, present=np.ones(n, bool) if present is None else present, sel=np.ones(n, bool) if sel is None else sel,
                      tags=set(tags), base=base))

    pos = np.arange(300)
    for k in (2, 3, 5):
        ks = keys_with_home(17, 64, k, start)
        add("same_home_%d" % k, 300, 8, np.array(ks)[pos % k], {"hit", "home", "walk", ("len", k - 1)}, base=True)
    ks = keys_with_home(63, 64, 2, start)
    add("wrap", 300, 8, np.array(ks)[pos % 2], {"home", "wrap", ("len", 1)}, base=True)
    ks = keys_with_home(40, 64, 65, start)
    pos = np.arange(700)
    add("walk_slots_less_one", 700, 8, np.array(ks[:64])[pos % 64], {"home", "walk", "wrap", ("len", 63)})
    add("no_room", 700, 8, np.array(ks)[pos % 65], {"noroom", ("len", 63)})
    ks = keys_with_set(9, 6, start)
    pos = np.arange(300)
    add("two_keys_one_set", 300, 8, np.array(ks[:2])[pos % 2], {"hit"}, base=True)
    add("set_overflows", 300, 8, np.array(ks)[pos % 6], {"hit", "bypass"}, base=True)
    n = 64 * E * 3
    lane = place(np.arange(n), n, E)[2]
    add("wave_on_one_key", n, 8, np.full(n, start + 6), {"hit", "home"})
    add("lanes_on_64_keys", n, 64, start + lane * 3, {"hit"})
    add("lane_0_alone", n, 8, start + (np.arange(n) % 5), {"hit"}, sel=lane == 0)
    add("lane_63_alone", n, 8, start + (np.arange(n) % 5), {"hit"}, sel=lane == 63)
    for n in (1, E - 1, E, E + 1, 64 * E - 1, 64 * E, 64 * E + 1, rnd - 1, rnd, rnd + 1, 4 * rnd + 1):
        # (4 rounds + 1 row: two workgroups; the same keys in both and on both sides of every chunk border, so the flushes add into one slot)
        present = np.arange(n) % 11 != 3
        add("size_%d" % n, n, 8, start + (np.arange(n) % 7) * 1000003, {"hit", "home"} if n > 3 else set(), present=present)
    return L
