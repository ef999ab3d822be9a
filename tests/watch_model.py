"""A numpy model of the standing queries (include/bmx_watch.h), shared by test_watch_model.py (CPU: the model's own invariants) and the GPU tests (helper, not a
test). The table is a state per field and node (absent, data, tombstone) as in test_gpu_where.py; mask(base, clauses) is bmx_scan_where's truth. A watch's
committed set is a mask keyed by NODE, not by index position, so the model knows nothing of how the device lays its index out: the expected lists are the
caller's position order (index_ids(base) as node numbers) filtered by `now & ~committed` and by `committed & ~now`, and on RESET all of `now` and nothing.

The seeded run: N0 = 3 * 8192 + 37 nodes with a base field and two probed fields, then rounds of one merge batch (value updates, new nodes) and one batch of
tombstones each. Rounds 10..14 are QUIET: base values move inside their decade only (every program below cuts the base field at decades), the probed fields are left
alone, an unrelated field is written and the new nodes come without the base field — so each program has a poll that reports nothing."""
import numpy as np

from oracle import streams

ABSENT, DATA, TOMB = 0, 1, 2
BLOCK = 8192
FB, F1, F2, F3 = (streams.fnv1a32(s) for s in ("watch.base", "watch.one", "watch.two", "watch.other"))
VAL_DELETED = -(1 << 63)

PROGRAMS = [
    [[(FB, 10, 19)]],                                                        # a plain range, 10 % of the base values
    [[(FB, 0, 49), (F1, 2, 5)], [(F2, 7, 9), (F1, 0, 1, True)]],             # a two-clause OR with a NOT
    [[(F1, 3, 6, True), (FB, 20, 29, True)]],                                # negations only
]
POLL_EVERY = [1, 3, 5]          # watch k is polled behind every POLL_EVERY[k]-th round: the longer gaps see net changes
QUIET = range(10, 15)
N0, NEW_PER_ROUND, ROUNDS, SEED = 3 * BLOCK + 37, 20, 40, 20250117


def node_ids(n, salt=0):
    return streams.splitmix64_np(np.arange(1 + salt, n + 1 + salt, dtype=np.uint64))


class Model:
    """the table: val[f][i], st[f][i] (ABSENT / DATA / TOMB) of node i"""

    def __init__(self, ids):
        self.ids = np.asarray(ids, np.uint64); self.N = len(self.ids); self.val = {}; self.st = {}
        self.order = np.argsort(self.ids); self.sorted_ids = self.ids[self.order]

    def _f(self, f):
        if f not in self.val:
            self.val[f] = np.zeros(self.N, np.int64); self.st[f] = np.zeros(self.N, np.uint8)

    def set(self, f, idx, vals):
        self._f(f); self.val[f][idx] = vals; self.st[f][idx] = DATA

    def tomb(self, f, idx):
        self._f(f); self.st[f][idx] = TOMB

    def rows(self, f, ts):
        i = np.nonzero(self.st[f] == DATA)[0]
        return self.ids[i], np.full(len(i), f, np.uint32), np.full(len(i), ts, np.int64), self.val[f][i]

    def lit(self, t):
        f, lo, hi = t[0], int(t[1]), int(t[2])
        self._f(f)
        pos = (self.st[f] == DATA) & (self.val[f] >= lo) & (self.val[f] <= hi) if lo <= hi else np.zeros(self.N, bool)
        return ~pos if len(t) > 3 and t[3] else pos

    def mask(self, base, clauses):
        self._f(base)
        any_clause = np.zeros(self.N, bool)
        for c in clauses:
            all_lits = np.ones(self.N, bool)
            for t in c:
                all_lits &= self.lit(t)
            any_clause |= all_lits
        return any_clause & (self.st[base] == DATA)

    def index_of(self, ids):
        """node numbers of ids (all of them nodes of the model)"""
        k = np.searchsorted(self.sorted_ids, ids)
        assert (self.sorted_ids[k] == ids).all()
        return self.order[k]

    def apply(self, batch):
        """one batch of a seeded run (node, field, value) -> the table; VAL_DELETED leaves a tombstone"""
        node, field, val = batch
        for f in np.unique(field):
            k = field == f
            dead = val[k] == VAL_DELETED
            self.set(int(f), node[k][~dead], val[k][~dead]); self.tomb(int(f), node[k][dead])

    def columns(self, batch, ts):
        node, field, val = batch
        return self.ids[node], field.astype(np.uint32), np.full(len(node), ts, np.int64), val.astype(np.int64)


class Expected:
    def __init__(self, entered, left, n_match, reset, overflow):
        self.entered, self.left, self.n_entered, self.n_left, self.n_match, self.reset, self.overflow = entered, left, len(entered), len(left), n_match, reset, overflow


class Watches:
    """the committed sets, one mask over the model's nodes per watch key"""

    def __init__(self, model):
        self.m = model; self.committed = {}; self.fresh = set()

    def create(self, key, base, clauses):
        self.committed[key] = (base, clauses, np.zeros(self.m.N, bool)); self.fresh.add(key)

    def reset(self, key=None):
        """the base index was laid out anew: the device empties the committed set"""
        for k in ([key] if key is not None else list(self.committed)):
            self.committed[k][2][:] = False; self.fresh.add(k)

    def poll(self, key, pos_nodes, cap_entered=None, cap_left=None):
        """pos_nodes: the node numbers of the base index's positions, in position order. Commits as the device does: only if both lists fit."""
        base, clauses, c = self.committed[key]
        now = self.m.mask(base, clauses)
        ent, lft = pos_nodes[(now & ~c)[pos_nodes]], pos_nodes[(c & ~now)[pos_nodes]]
        assert len(ent) == int((now & ~c).sum()) and len(lft) == int((c & ~now).sum()), "a committed or matching node is missing from the index"
        fits = (cap_entered is None or len(ent) <= cap_entered) and (cap_left is None or len(lft) <= cap_left)
        x = Expected(self.m.ids[ent], self.m.ids[lft], int(now.sum()), key in self.fresh, not fits)
        if fits:
            c[:] = now; self.fresh.discard(key)
        return x


def seeded_model(rounds=ROUNDS, salt=0):
    """-> (model with every node the run will ever create, the initial batch)"""
    rng = np.random.default_rng(SEED)
    m = Model(node_ids(N0 + NEW_PER_ROUND * rounds, 31000 + salt))
    old = np.arange(N0)
    parts = [(old, np.full(N0, FB), rng.integers(0, 100, N0))]
    for f, pr in ((F1, 0.8), (F2, 0.5)):
        idx = old[rng.random(N0) < pr]
        parts.append((idx, np.full(len(idx), f), rng.integers(0, 10, len(idx))))
    return m, tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def seeded_rounds(m, rounds=ROUNDS):
    """yields (round, merge batch, tombstone batch); each batch is (node, field, value) with distinct (node, field) keys. Reads the model's CURRENT state (apply
    both batches before asking for the next round)."""
    rng = np.random.default_rng(SEED + 1)
    for r in range(rounds):
        new = np.arange(N0 + NEW_PER_ROUND * r, N0 + NEW_PER_ROUND * (r + 1))
        live = np.nonzero(m.st[FB] != ABSENT)[0]
        parts, tombs = [], []
        if r in QUIET:
            idx = rng.choice(np.nonzero(m.st[FB] == DATA)[0], 200, replace=False)
            parts.append((idx, FB, (m.val[FB][idx] // 10) * 10 + rng.integers(0, 10, len(idx))))           # inside the decade: no program's truth changes
            idx = rng.choice(live, 300, replace=False)
            parts.append((idx, F3, rng.integers(0, 10, len(idx))))
            parts.append((new, F1, rng.integers(0, 10, len(new))))                                         # nodes without the base field: outside every universe
        else:
            for f, top, k in ((FB, 100, 250), (F1, 10, 250), (F2, 10, 150)):
                idx = rng.choice(live, k, replace=False)                                                    # rows of every state: absent -> data, tombstone -> data, data -> data
                parts.append((idx, f, rng.integers(0, top, k)))
            parts.append((new, FB, rng.integers(0, 100, len(new))))
            parts.append((new[::2], F1, rng.integers(0, 10, len(new[::2]))))
            for f, k in ((FB, 40), (F1, 60), (F2, 30)):
                tombs.append((rng.choice(np.nonzero(m.st[f] == DATA)[0], k, replace=False), f))
        merge = (np.concatenate([p[0] for p in parts]), np.concatenate([np.full(len(p[0]), p[1]) for p in parts]), np.concatenate([p[2] for p in parts]).astype(np.int64))
        if tombs:       # a key the merge batch of this round writes is not tombstoned in the same round: one writer per key and round
            written = set(zip(merge[0].tolist(), merge[1].tolist()))
            tn = np.concatenate([t[0] for t in tombs]); tf = np.concatenate([np.full(len(t[0]), t[1]) for t in tombs])
            keep = np.array([(a, b) not in written for a, b in zip(tn.tolist(), tf.tolist())], bool)
            tomb = (tn[keep], tf[keep], np.full(int(keep.sum()), VAL_DELETED, np.int64))
        else:
            tomb = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
        yield r, merge, tomb


def polled(r, k):
    return (r + 1) % POLL_EVERY[k] == 0
