"""GPU: the kernels of replica reconciliation (csrc/sync_kernels.h: k_digest_buckets in its LDS and its global form, PredSlotSync, EmitRecs; csrc/select.h:
k_sel_count, k_sel_write over the table, which also serve bmx_dump_rows and the index build) at the edges of the digest's wave stack, its 256-slot chunk,
the export's 512-slot tile and the end of the table — small tables laid out slot by slot instead of large random ones.

The probe sequence of slot.h (ProbeSeq<4>) is restated below and INVERTED: node_hash is a bijection on 64 bits, so Table.ids_for builds, for any slot, a
node id whose home is that slot. With at most one key per slot no key ever leaves its home, so a test says which slots hold a row, a tombstone or nothing,
and the table is exactly that (asserted once per table, Table.premise: dump_rows, index_ids and export_rows in ascending slot order against the model).

Every check is exact equality with numpy over the model. Which branches a layout reaches is computed from the model (_digest_tags: a replay of the digest's
per-wave `fill`; _export_tags: sel_geom<2>), asserted per test, and the last test asserts that the layouts together reach the whole list."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from bmx import synth
from oracle.oracle import rows_digest

DEL = bmx.VAL_DELETED
FA, FB = synth.fnv1a32("age"), synth.fnv1a32("score")
M64 = (1 << 64) - 1
EMPTY_ID = M64
TS_MAX = VAL_MAX = (1 << 53) - 1
CHUNK, ROUND, DIG_WAVES, DIG_LDS_LOG2 = 256, 64, 8, 10       # sync_kernels.h: 64 x DIG_U slots, one load round, waves per workgroup, the LDS form's largest L
TILE, SEL_MAX_BLOCKS = 512, 1024                              # select.h: SEL_THREADS x E (E = 2), SEL_MAX_BLOCKS
LS = (0, 1, 4, 5, 6, 10, 11, 16)                              # digests asked of every table
LS_BITS = (0, 5, 6, 10, 16)                                   # bucket-bit vectors asked of every table
GUARD = 8
FILL = 0x5A5A5A5A5A5A5A5A                                     # what a device vector holds before a digest writes into it
REC_ID, REC_AUX = 0xABABABABABABABAB, 0xCDCDCDCD              # what a record holds before an export writes into it
DEVICE = "cuda"

MIX1, MIX2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
INV1, INV2 = pow(MIX1, -1, 1 << 64), pow(MIX2, -1, 1 << 64)
NH_MUL, NH_ADD = 0x9FB21C651E98DF25, 0x632BE59BD9B4E019
NH_INV = pow(NH_MUL, -1, 1 << 64)

DIGEST_TAGS = ["drain at exactly 64", "stack at 127", "left-over 0", "left-over 1", "left-over 63", "ragged chunk", "wave without a chunk",
               "carry into a second chunk", "global form"]
EXPORT_TAGS = ["ragged last tile", "tile beyond the table", "tiles_per_block > 1", "match in the last live thread", "matches on both sides of a block border",
               "matches only in block 0", "matches only in the last block"]


# ---- slot.h, restated ----

def mix64(x):
    x ^= x >> 33; x = x * MIX1 & M64; x ^= x >> 33; x = x * MIX2 & M64; x ^= x >> 33
    return x


def unmix64(x):
    """x ^= x >> 33 is its own inverse (the shift is more than half the word); the multipliers are odd"""
    x ^= x >> 33; x = x * INV2 & M64; x ^= x >> 33; x = x * INV1 & M64; x ^= x >> 33
    return x


def node_hash(id):
    return mix64((id * NH_MUL + NH_ADD) & M64)


def field_c(field):
    return ((int(field) * 0x9E3779B9) & 0xFFFFFFFF) >> 30


def home_slot(id, field, nslots):
    """where ProbeSeq<4> starts the key (id, field) in a table of nslots slots; Python ints"""
    h = node_hash(int(id))
    return ((h * (nslots // 4)) >> 64) * 4 + ((field_c(field) + (h & 0xFFFFFFFF)) & 3)


def home_slots(ids, fields, nslots):
    """the same for arrays (numpy; nslots < 2^32, so the high product fits 64 bits in two halves)"""
    u = np.uint64
    x = np.asarray(ids, u)
    with np.errstate(over="ignore"):
        x = x * u(NH_MUL) + u(NH_ADD)
        x = x ^ (x >> u(33)); x = x * u(MIX1); x = x ^ (x >> u(33)); x = x * u(MIX2); x = x ^ (x >> u(33))
        nl = u(nslots // 4)
        hi, lo = x >> u(32), x & u(0xFFFFFFFF)
        line = (hi * nl + ((lo * nl) >> u(32))) >> u(32)
        fc = ((np.asarray(fields, np.uint32).astype(u) * u(0x9E3779B9)) & u(0xFFFFFFFF)) >> u(30)
    return (line * u(4) + ((fc + lo) & u(3))).astype(np.int64)


def slots_for(capacity_rows, load_pct):
    """bmx_merge.inc slots_for"""
    return (max(4096, (capacity_rows * 100 + load_pct - 1) // load_pct) + 3) & ~3


def capacity_for(nslots, load_pct=90):
    """a capacity_rows whose table has exactly nslots slots"""
    c = max(1, (nslots - 4) * load_pct // 100)
    while slots_for(c, load_pct) < nslots:
        c += 1
    assert slots_for(c, load_pct) == nslots, (nslots, c)
    return c


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the row digest, restated and tied to the oracle's ----

def _np_digest(id, field, ts, val, L):
    """numpy group-by: (sums, counts) per bucket of a row set"""
    sm = synth.splitmix64_np
    h = sm(np.asarray(val, np.int64).astype(np.uint64))
    h = sm(h ^ np.asarray(ts, np.int64).astype(np.uint64))
    h = sm(h ^ np.asarray(field, np.uint32).astype(np.uint64))
    d = sm(h ^ np.asarray(id, np.uint64))
    assert int(d.sum(dtype=np.uint64)) == rows_digest(id, field, ts, val)
    b = bmx.key_bucket(id, field, L).astype(np.int64)
    sums = np.zeros(1 << L, np.uint64); counts = np.zeros(1 << L, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(sums, b, d)
    np.add.at(counts, b, np.uint64(1))
    return sums, counts


def _same(got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def _same_recs(got, want, what):
    assert got.dtype == bmx.DELTA_REC_DTYPE
    for col in ("id", "field", "ts", "val", "aux"):
        _same(got[col], want[col], (what, col))


# ---- which branches a table reaches (numpy over the model only) ----

def _digest_grid(nslots, cus):
    chunks = (nslots + CHUNK - 1) // CHUNK
    return chunks, max(1, min((chunks + DIG_WAVES - 1) // DIG_WAVES, 2 * cus))


def _digest_tags(sel, nslots, cus):
    """replay of k_digest_buckets' per-wave `fill`; sel: one bool per slot, the rows the flag lets in"""
    tags = set()
    chunks, blocks = _digest_grid(nslots, cus)
    bit = np.zeros(chunks * CHUNK, bool); bit[:nslots] = sel
    per_round = bit.reshape(chunks, CHUNK // ROUND, ROUND).sum(2)
    busy = np.flatnonzero(per_round.sum(1))
    W = blocks * DIG_WAVES
    if W > chunks:
        tags.add("wave without a chunk")
    for w in sorted({int(c) % W for c in busy}):                # (a wave without a row ends as it began: fill 0, nothing on the stack)
        fill = 0
        for i, c in enumerate(range(w, chunks, W)):
            if i and fill:
                tags.add("carry into a second chunk")
            if (c + 1) * CHUNK > nslots and per_round[c].sum():
                tags.add("ragged chunk")
            for k in per_round[c].tolist():
                fill += k
                assert fill <= 127
                if fill == 127:
                    tags.add("stack at 127")
                if fill >= ROUND:
                    if fill == ROUND:
                        tags.add("drain at exactly 64")
                    fill -= ROUND
        if fill in (0, 1, 63):
            tags.add("left-over %d" % fill)
    if max(LS) > DIG_LDS_LOG2:
        tags.add("global form")
    return tags


def sel_geom(n):
    """select.h sel_geom<2>: (tiles, blocks, tiles_per_block)"""
    tiles = max(1, (n + TILE - 1) // TILE)
    blocks = min(tiles, SEL_MAX_BLOCKS)
    tpb = (tiles + blocks - 1) // blocks
    return tiles, (tiles + tpb - 1) // tpb, tpb


def _export_tags(match, nslots):
    """match: the slots an export selects, ascending"""
    tags = set()
    tiles, blocks, tpb = sel_geom(nslots)
    if not len(match):
        return tags
    match = np.asarray(match, np.int64)
    if nslots % TILE and match[-1] >= (nslots // TILE) * TILE:
        tags.add("ragged last tile")
    if match[-1] >= ((nslots - 1) // 2) * 2:
        tags.add("match in the last live thread")
    if tpb > 1:
        tags.add("tiles_per_block > 1")
    if blocks * tpb > tiles:
        tags.add("tile beyond the table")
    blk = match // (tpb * TILE)
    border = np.flatnonzero((np.diff(match) == 1) & (np.diff(blk) == 1))
    if len(border):
        tags.add("matches on both sides of a block border")
    if blocks > 1 and blk[-1] == 0:
        tags.add("matches only in block 0")
    if blocks > 1 and blk[0] == blocks - 1:
        tags.add("matches only in the last block")
    return tags


def _expect(seen, tags, what):
    missing = sorted(set(tags) - seen)
    assert not missing, (what, "the layout was meant to reach", missing, "and reached", sorted(seen))


# ---- a layout: which slots hold a row, which of them a tombstone ----

class Spec:
    def __init__(self, name, slots, tomb=(), marked_only=False, bucket=None, hot=(), clocks=None, expect=()):
        self.name = name
        self.slots = np.unique(np.asarray(slots, np.int64))
        self.tomb = np.isin(self.slots, np.asarray(tomb, np.int64))
        self.marked_only = marked_only        # no row comes from load_rows: every stored clock carries an epoch mark
        self.bucket = bucket                  # (L, b): every key falls into bucket b of 2^L
        self.hot = np.isin(self.slots, np.asarray(hot, np.int64))     # these rows hold the largest clock, 2^53 - 1, and no other row does
        self.clocks = clocks
        self.expect = set(expect)


CLOCKS = [0, 7, 7, 1000, TS_MAX, 12345, 7]                       # 7 is held by several rows: `since` = 7 and 8 cut between rows that exist
VALUES = [0, VAL_MAX, -VAL_MAX, 5, -1]
LOAD, REF, DELTA = 0, 1, 2


class Table:
    """One engine whose table is laid out by slot. The model, in ascending slot order: slot, id, field, ts (the clock without any mark), val (DEL: a tombstone)."""

    def __init__(self, e, nslots):
        self.e, self.nslots = e, nslots
        z = np.zeros(0, np.int64)
        self.slot, self.id, self.field, self.ts, self.val = z, z.astype(np.uint64), z.astype(np.uint32), z, z

    def ids_for(self, slots, field, salt=0):
        """a node id for every slot whose key (id, field) starts its probe sequence there; another salt gives another id"""
        slots = np.asarray(slots, np.int64)
        fields = np.broadcast_to(np.asarray(field, np.uint32), slots.shape)
        nl = self.nslots // 4
        out = np.zeros(len(slots), np.uint64)
        for k, (s, f) in enumerate(zip(slots.tolist(), fields.tolist())):
            line, c = divmod(s, 4)
            h = ((line << 64) + nl - 1) // nl                  # the smallest h with (h * nl) >> 64 == line
            h = (h & ~3) + 4 * (1 + salt) + ((c - field_c(f)) & 3)
            out[k] = ((unmix64(h) - NH_ADD) * NH_INV) & M64
        assert (home_slots(out, fields, self.nslots) == slots).all() and (out != np.uint64(EMPTY_ID)).all()
        return out

    def ids_in_bucket(self, slots, fields, L, bucket):
        """the same, searching the salt until the key falls into `bucket` of 2^L (about 2^L tries per key)"""
        ids = np.zeros(len(slots), np.uint64)
        todo = np.arange(len(slots))
        salt = 0
        while len(todo):
            cand = self.ids_for(slots[todo], fields[todo], salt)
            ok = bmx.key_bucket(cand, fields[todo], L) == bucket
            ids[todo[ok]] = cand[ok]
            todo = todo[~ok]
            salt += 1
            assert salt < 64 << L
        return ids

    def lay(self, spec):
        """write the layout into the (empty) table: load_rows, a merge of absent keys under each insert rule, then put_rows of the tombstones over loaded rows"""
        assert len(self.slot) == 0
        slots = spec.slots
        n = len(slots)
        i = np.arange(n)
        fields = np.where(i % 2 == 0, FA, FB).astype(np.uint32)
        ids = self.ids_in_bucket(slots, fields, *spec.bucket) if spec.bucket else self.ids_for(slots, fields, salt=3)
        kind = (i % 2 + 1) if spec.marked_only else i % 3
        kind = np.where(spec.tomb, LOAD, kind)
        kind = np.where(spec.hot & (kind == REF), DELTA, kind)
        clocks = np.asarray(spec.clocks if spec.clocks is not None else CLOCKS, np.int64)
        ts = np.where(spec.hot, TS_MAX, clocks[i % len(clocks)])
        val = np.asarray(VALUES, np.int64)[i % len(VALUES)]
        e = self.e
        if e is not None:
            for k, write in ((LOAD, e.load_rows), (REF, lambda *a: e.merge_batch(*a, insert_mode=bmx.INSERT_REFERENCE)), (DELTA, lambda *a: e.merge_batch(*a, insert_mode=bmx.INSERT_DELTA))):
                m = kind == k
                if m.any():
                    r = write(ids[m], fields[m], ts[m], val[m])
                    assert k == LOAD or len(r[0]) == int(m.sum()), "every delta of an absent key wins"
        ts = np.where(kind == REF, 2, ts)                       # the reference's rule: a row created by a merge starts at clock 2
        if spec.tomb.any():
            m = spec.tomb
            ts = np.where(m, np.asarray([1000, 7, TS_MAX - 1], np.int64)[i % 3], ts)
            val = np.where(m, DEL, val)
            if e is not None:
                e.put_rows(ids[m], fields[m], ts[m], val[m])
        self.slot, self.id, self.field, self.ts, self.val = slots, ids, fields, ts.astype(np.int64), val.astype(np.int64)
        self.kind = kind
        return self

    @property
    def data(self):
        return self.val != DEL

    def recs(self, idx):
        r = np.zeros(len(self.slot[idx]), bmx.DELTA_REC_DTYPE)
        r["id"], r["field"], r["ts"], r["val"] = self.id[idx], self.field[idx], self.ts[idx], self.val[idx]
        return r

    def premise(self, capacity_rows):
        """nothing below means anything unless the table is the model: same size, and every row where the layout put it"""
        e, d = self.e, self.data
        assert len(self.slot) <= capacity_rows
        assert e.info().n_slots == self.nslots, "the table did not grow"
        got = e.dump_rows()
        for g, w, col in zip(got, (self.id[d], self.field[d], self.ts[d], self.val[d]), ("id", "field", "ts", "val")):
            _same(g, w, ("dump_rows in slot order", col))
        for f in (FA, FB):
            e.index_build(f)
            _same(e.index_ids(f), self.id[self.field == f], ("index_ids in slot order, tombstones included", f))
        recs, n = e.export_rows()
        assert n == int(d.sum())
        _same_recs(recs, self.recs(d), "export_rows in slot order")

    def sel(self, tombstones):
        """one bool per slot: the rows a digest with this flag takes"""
        bit = np.zeros(self.nslots, bool)
        bit[self.slot[self.data | bool(tombstones)]] = True
        return bit

    # ---- the queries of one table: (arguments of export_rows, the model's rows they select) ----
    def queries(self):
        d = self.data
        n = len(self.slot)
        clk = np.unique(self.ts)
        if len(clk):
            exact = int(clk[len(clk) // 2])
            sinces = sorted({0, int(clk[0]), exact, exact + 1, int(clk[-1]), int(clk[-1]) + 1})
        else:
            sinces = [0, 1]
        out = []
        for only in (False, True):
            for since in sinces:
                out.append((dict(since=since, only_tombstones=only), (d != only) & (self.ts >= since)))
        for L in LS_BITS:
            bk = bmx.key_bucket(self.id, self.field, L)
            words = max(1, (1 << L) // 64)
            picks = [("nothing", np.zeros(words, np.uint64), np.zeros(n, bool)), ("everything", np.full(words, M64, np.uint64), np.ones(n, bool))]
            dd = np.flatnonzero(d)
            for name, j in (("one bucket", dd[len(dd) // 2] if len(dd) else None), ("the first row's bucket", dd[0] if len(dd) else None), ("the last row's bucket", dd[-1] if len(dd) else None)):
                b = int(bk[j]) if j is not None else (1 << L) - 1
                picks.append((name, bmx.bucket_bits_of([b], L), bk == b))
            for name, bits, m in picks:
                out.append((dict(log2_buckets=L, bucket_bits=bits), d & m))
        if len(clk):
            b = int(bmx.key_bucket(self.id[-1:], self.field[-1:], 6)[0])
            out.append((dict(since=exact, log2_buckets=6, bucket_bits=bmx.bucket_bits_of([b], 6)), d & (self.ts >= exact) & (bmx.key_bucket(self.id, self.field, 6) == b)))
        return out

    def tags(self, cus):
        t = _digest_tags(self.sel(False), self.nslots, cus) | _digest_tags(self.sel(True), self.nslots, cus)
        for _, m in self.queries():
            t |= _export_tags(self.slot[m], self.nslots)
        return t


# ---- the checks ----

def _torch():
    import torch
    return torch


def _dev_sync():
    if DEVICE == "cuda":
        _torch().cuda.synchronize()


def check_digest(t, Ls=LS):
    """digest(L, flag) into host memory and into device vectors full of garbage, against a numpy group-by of the model's rows"""
    torch = _torch()
    e = t.e
    for flag in (False, True):
        m = t.data | flag
        for L in Ls:
            B = 1 << L
            want = _np_digest(t.id[m], t.field[m], t.ts[m], t.val[m], L)
            sums, counts = e.digest(L, tombstones=flag)
            _same(sums, want[0], ("digest sums", L, flag)); _same(counts, want[1], ("digest counts", L, flag))
            ds = torch.full((B + GUARD,), FILL, dtype=torch.int64, device=DEVICE); dc = torch.full((B + GUARD,), FILL, dtype=torch.int64, device=DEVICE)
            _dev_sync()
            e.digest_dev(L, ds, dc, tombstones=flag); e.sync()
            hs, hc = ds.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint64)
            _same(hs[:B], want[0], ("digest sums, device", L, flag)); _same(hc[:B], want[1], ("digest counts, device", L, flag))
            assert (hs[B:] == np.uint64(FILL)).all() and (hc[B:] == np.uint64(FILL)).all(), ("nothing behind 2^L is written", L, flag)


def _guarded(k):
    g = np.zeros(k, bmx.DELTA_REC_DTYPE)
    g["id"] = REC_ID; g["aux"] = REC_AUX; g["ts"] = -1; g["val"] = -1
    return g


def _untouched(g, what):
    assert (g["id"] == REC_ID).all() and (g["aux"] == REC_AUX).all() and (g["ts"] == -1).all() and (g["val"] == -1).all(), (what, "nothing behind min(n, cap) is written")


def check_export(t):
    """every query of the table, record for record in slot order; then the caps, into pageable memory, page-locked memory and device memory"""
    torch = _torch()
    e = t.e
    for kw, m in t.queries():
        recs, n = e.export_rows(**kw)
        assert n == int(m.sum()), (kw, n, int(m.sum()))
        _same_recs(recs, t.recs(m), kw)
    d_n = torch.zeros(1, dtype=torch.int64, device=DEVICE)
    for L in LS_BITS:                                           # device bucket bits: nothing, and the last row's bucket
        qs = [q for q in t.queries() if q[0].get("log2_buckets") == L and "since" not in q[0]]
        for kw, m in (qs[0], qs[-1]):
            k = int(m.sum())
            d_bits = torch.from_numpy(kw["bucket_bits"].view(np.int64).copy()).to(DEVICE)
            d_out = torch.full((4 * (k + GUARD),), -1, dtype=torch.int64, device=DEVICE)
            d_n.fill_(-1); _dev_sync()
            e.export_rows_dev(d_out, k, d_n, log2_buckets=L, bucket_bits=d_bits); e.sync()
            h = d_out.cpu().numpy()
            assert int(d_n.item()) == k, (L, "device bits")
            _same_recs(h[:4 * k].view(bmx.DELTA_REC_DTYPE), t.recs(m), (L, "device bits"))
            assert (h[4 * k:] == -1).all()
    for kw, m in ((dict(), t.data), (dict(only_tombstones=True, since=7), ~t.data & (t.ts >= 7))):
        n = int(m.sum())
        want = t.recs(m)
        for cap in sorted({0, 1, n - 1, n, n + 1, t.nslots + 7} - {-1}):
            k = min(n, cap)
            g = _guarded(cap + GUARD)                           # pageable memory: through the staging buffer, which the ascending caps make grow
            recs, nn = e.export_rows(out=g[:cap], **kw)
            assert nn == n and len(recs) == k, (kw, cap, "the count is the full one")
            _same_recs(g[:k], want[:k], (kw, cap, "pageable")); _untouched(g[k:], (kw, cap, "pageable"))
            hb = bmx.HostBuffer(32 * (cap + GUARD))             # page-locked memory: the kernel writes the records where the caller wants them
            a = hb.array(bmx.DELTA_REC_DTYPE, cap + GUARD)
            a[:] = _guarded(cap + GUARD)
            recs, nn = e.export_rows(out=a[:cap], **kw)
            assert nn == n and len(recs) == k
            _same_recs(a[:k], want[:k], (kw, cap, "page-locked")); _untouched(a[k:], (kw, cap, "page-locked"))
            del a, recs; hb.close()
            d_out = torch.from_numpy(_guarded(cap + GUARD).view(np.int64)).to(DEVICE)
            d_n.fill_(-1); _dev_sync()
            e.export_rows_dev(d_out, cap, d_n, **kw); e.sync()
            h = d_out.cpu().numpy().view(bmx.DELTA_REC_DTYPE)
            assert int(d_n.item()) == n, (kw, cap, "device count")
            _same_recs(h[:k], want[:k], (kw, cap, "device")); _untouched(h[k:], (kw, cap, "device"))


# ---- small tables ----

SMALL = (4096, 4100, 4352)       # 16 chunks, 2 workgroups, 8 tiles; a 17th chunk and a 9th tile of 4 slots; 17 whole chunks, 8.5 tiles


def _chunk(c, offs):
    return c * CHUNK + np.asarray(offs, np.int64)


def small_specs(nslots):
    chunks = (nslots + CHUNK - 1) // CHUNK
    last = np.arange((chunks - 1) * CHUNK, nslots)
    ragged = nslots % CHUNK != 0
    idle = {"wave without a chunk"} if chunks % DIG_WAVES else set()
    tail = {"match in the last live thread"} | ({"ragged chunk"} if ragged else set()) | ({"ragged last tile"} if nslots % TILE else set())
    full = np.arange(CHUNK)
    S = [
        Spec("an empty table", [], expect=idle),
        Spec("one row in slot 0", [0], expect={"left-over 1"} | idle),
        Spec("one row in the last slot", [nslots - 1], expect={"left-over 1"} | tail),
        Spec("rows only in the last chunk", last[-67:], tomb=last[-3:-1], expect=tail),
        Spec("a fully occupied chunk", _chunk(3, full), expect={"drain at exactly 64", "left-over 0"}),
        Spec("63 rows, a full round, one row", _chunk(2, np.r_[0:63, 64:128, 128]), expect={"stack at 127", "drain at exactly 64", "left-over 0"}),
        Spec("chunks that leave 1 and 63", np.r_[_chunk(4, np.arange(65)), _chunk(5, np.r_[0:21, 64:85, 192:213])], expect={"drain at exactly 64", "left-over 1", "left-over 63"}),
        Spec("a chunk with every other slot occupied", _chunk(6, full[::2]), expect={"drain at exactly 64", "left-over 0"}),
        Spec("a dense chunk, every second row a tombstone", _chunk(7, full), tomb=_chunk(7, full[1::2]), expect={"drain at exactly 64", "left-over 0"}),
        Spec("a dense chunk of rows created by merges only", _chunk(8, full), marked_only=True, expect={"drain at exactly 64", "left-over 0"}),
        Spec("a dense chunk in one bucket of sixteen", _chunk(9, full), bucket=(4, 11), expect={"drain at exactly 64", "left-over 0"}),
        Spec("runs across the export's block borders", np.r_[500:524, 2040:2056], tomb=[505, 2050], expect={"matches on both sides of a block border"}),
    ]
    return S


NAMES = [s.name for s in small_specs(4096)]


def _engine(nslots):
    cap = capacity_for(nslots)
    return bmx.Engine(cap, flags=bmx.CTX_FIXED_CAPACITY, load_pct=90), cap


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("nslots", SMALL)
def test_small_table_layouts(nslots, name):
    """one layout in one table of 4096, 4100 or 4352 slots: the premise, every digest, every export"""
    spec = small_specs(nslots)[NAMES.index(name)]
    e, cap = _engine(nslots)
    with e:
        t = Table(e, nslots).lay(spec)
        t.premise(cap)
        if spec.bucket:
            L, b = spec.bucket
            assert (bmx.key_bucket(t.id, t.field, L) == b).all()
        if spec.name == "a dense chunk, every second row a tombstone":
            assert (t.sel(True)[7 * CHUNK:8 * CHUNK]).all() and (t.sel(False)[7 * CHUNK:8 * CHUNK] == (np.arange(CHUNK) % 2 == 0)).all()
        if spec.marked_only:
            assert (t.kind != LOAD).all()
        _expect(t.tags(_cus()), spec.expect, (nslots, name))
        check_digest(t)
        check_export(t)


# ---- one large table: every wave of the digest walks two chunks ----

def large_nslots(cus):
    G = 2 * cus * DIG_WAVES
    return (2 * G + 1) * CHUNK + 4, G


def large_spec(cus):
    """wave 5: 63 left over from its first chunk meet a full round in its second. Wave 9: 1 left over meets an empty second chunk. Wave 12: rows in its
    second chunk only. Wave 0: a third chunk, the table's last whole one. Wave 1: tombstones among rows in its first chunk — the only tombstones, all in the
    export's block 0 — and the ragged chunk of 4 slots. The rows of the last two chunks hold the largest clock: `since` = 2^53 - 1 matches in the export's
    last block only."""
    nslots, G = large_nslots(cus)
    hot = np.r_[_chunk(2 * G, [0, 255]), _chunk(2 * G + 1, [0, 1, 2, 3])]
    slots = np.r_[_chunk(5, np.arange(63)), _chunk(5 + G, np.arange(64)), _chunk(9, [100]), _chunk(12 + G, np.arange(64, 128)), _chunk(1, np.arange(40, 81)), hot]
    tiles, blocks, tpb = sel_geom(nslots)
    assert _chunk(1, 81) <= tpb * TILE and hot[0] >= (blocks - 1) * tpb * TILE
    expect = {"carry into a second chunk", "stack at 127", "left-over 63", "left-over 1", "left-over 0", "drain at exactly 64", "ragged chunk", "global form",
              "ragged last tile", "match in the last live thread", "matches only in block 0", "matches only in the last block"}
    if tiles > SEL_MAX_BLOCKS:
        assert blocks * tpb > tiles, "the last block has tiles beyond the table"
        expect |= {"tiles_per_block > 1", "tile beyond the table"}
    return nslots, Spec("the large table", slots, tomb=_chunk(1, np.arange(41, 81, 2)), hot=hot, clocks=[0, 7, 7, 1000, 12345], expect=expect)


class Large:
    def __init__(self):
        self.cus = _cus()
        self.nslots, self.spec = large_spec(self.cus)
        self.e, self.cap = _engine(self.nslots)
        self.t = Table(self.e, self.nslots).lay(self.spec)
        self.t.premise(self.cap)
        chunks, blocks = _digest_grid(self.nslots, self.cus)
        assert blocks == 2 * self.cus and chunks == 2 * blocks * DIG_WAVES + 2, "every wave walks two chunks, waves 0 and 1 a third"
        _expect(self.t.tags(self.cus), self.spec.expect, "the large table")


@pytest.fixture(scope="module")
def large():
    L = Large()
    yield L
    L.e.close()


def test_large_table_digests(large):
    """(2G + 1) x 256 + 4 slots, G = the waves of the digest's grid: left-overs carried from a wave's first chunk into its second, in both accumulation forms"""
    check_digest(large.t)


def test_large_table_exports(large):
    """tiles_per_block = 5 at 256 CUs, the last block with tiles beyond the table; matches only in block 0, only in the last block, in the last tile"""
    check_export(large.t)


# ---- the layouts together reach every branch on the list ----

def test_the_layouts_reach_every_branch():
    cus = _cus()
    seen = set()
    for nslots in SMALL:
        for spec in small_specs(nslots):
            seen |= Table(None, nslots).lay(spec).tags(cus)
    nslots, spec = large_spec(cus)
    seen |= Table(None, nslots).lay(spec).tags(cus)
    _expect(seen, DIGEST_TAGS + EXPORT_TAGS, "all layouts")
