"""GPU: the kernels of the vector-clock table's reconciliation (csrc/vc_sync_kernels.h: k_vc_digest in its LDS and its global form, k_vc_frontier,
PredVSlotSync, EmitVRecs, k_vc_unpack; csrc/select.h: k_sel_count, k_sel_write over the table) at the edges of the digest's wave stack, its 16-slot round and
128-slot chunk, the export's 512-slot tile, the unpack's 256-record workgroup and the end of the table — small tables laid out slot by slot instead of large
random ones. The method of test_gpu_sync_kernel_edges.py, restated for this table.

The probe sequence of slot.h (ProbeSeq<2>: two slots per line, the field's start bit is hash >> 31) is restated below and INVERTED: node_hash is a bijection
on 64 bits, so Table.ids_for builds, for any slot, a node id whose home is that slot. With at most one key per slot no key ever leaves its home, so a test
says which slots hold a row and the table is exactly that (asserted once per table, Table.premise: the table did not grow, and the export of everything
comes back in ascending slot order, record for record).

Every check is exact equality with numpy over the model. Which branches a layout reaches is computed from the model (_digest_tags: a replay of the digest's
per-wave `fill`; _frontier_tags; _export_tags: sel_geom<2>), asserted per test, and the last test asserts that the layouts together reach the whole list."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from bmx import synth
import vc_sync_model as M

FA, FB = synth.fnv1a32("age"), synth.fnv1a32("score")
M64 = (1 << 64) - 1
EMPTY_ID = M64
VAL_MAX = (1 << 53) - 1
ROUND, CHUNK, DIG_WAVES, FR_WAVES, STACK_MAX, DIG_LDS_LOG2 = 16, 128, 8, 4, 79, 10   # vc_sync_kernels.h: slots per load instruction, per wave step; waves per workgroup; 63 + 16
TILE, SEL_MAX_BLOCKS = 512, 1024                                                     # select.h: SEL_THREADS x E (E = 2), SEL_MAX_BLOCKS
UNPACK = 256                                                                         # records per workgroup of k_vc_unpack

MIX1, MIX2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
INV1, INV2 = pow(MIX1, -1, 1 << 64), pow(MIX2, -1, 1 << 64)
NH_MUL, NH_ADD = 0x9FB21C651E98DF25, 0x632BE59BD9B4E019
NH_INV = pow(NH_MUL, -1, 1 << 64)

DIGEST_TAGS = ["drain at exactly 64", "stack at 79", "a full round", "left-over 0", "left-over 1", "left-over 63", "ragged chunk", "ragged round", "wave without a chunk",
               "carry into a second chunk", "global form"]
FRONTIER_TAGS = ["frontier: wave without a chunk", "frontier: several chunks per wave", "frontier: the maximum sits in the ragged round", "frontier: an empty table"]
EXPORT_TAGS = ["ragged last tile", "tile beyond the table", "tiles_per_block > 1", "match in the last live thread", "matches on both sides of a block border",
               "matches only in block 0", "matches only in the last block", "a row without a clock under a frontier"]
UNPACK_TAGS = ["unpack: one record", "unpack: a full workgroup", "unpack: one record past a workgroup", "unpack: a ragged workgroup"]


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
    return ((int(field) * 0x9E3779B9) & 0xFFFFFFFF) >> 31


def home_slot(id, field, nslots):
    """where ProbeSeq<2> starts the key (id, field) in a table of nslots slots; Python ints"""
    h = node_hash(int(id))
    return ((h * (nslots // 2)) >> 64) * 2 + ((field_c(field) + (h & 0xFFFFFFFF)) & 1)


def nslots_for(capacity_rows):
    """bmx_vc_create"""
    return (max(4096, 2 * capacity_rows) + 1) & ~1


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- which branches a table reaches (numpy over the model only) ----

def _grid(nslots, cus, waves):
    chunks = (nslots + CHUNK - 1) // CHUNK
    return chunks, max(1, min((chunks + waves - 1) // waves, 2 * cus))


def _digest_tags(sel, nslots, cus):
    """replay of k_vc_digest's per-wave `fill`; sel: one bool per slot, the rows"""
    tags = set()
    chunks, blocks = _grid(nslots, cus, DIG_WAVES)
    bit = np.zeros(chunks * CHUNK, bool); bit[:nslots] = sel
    per_round = bit.reshape(chunks, CHUNK // ROUND, ROUND).sum(2)
    busy = np.flatnonzero(per_round.sum(1))
    W = blocks * DIG_WAVES
    if W > chunks:
        tags.add("wave without a chunk")
    if nslots % ROUND and bit[(nslots // ROUND) * ROUND:].any():
        tags.add("ragged round")
    for w in sorted({int(c) % W for c in busy}):                # (a wave without a row ends as it began: fill 0, nothing on the stack)
        fill = 0
        for i, c in enumerate(range(w, chunks, W)):
            if i and fill:
                tags.add("carry into a second chunk")
            if (c + 1) * CHUNK > nslots and per_round[c].sum():
                tags.add("ragged chunk")
            for k in per_round[c].tolist():
                if k == ROUND:
                    tags.add("a full round")
                fill += k
                assert fill <= STACK_MAX
                if fill == STACK_MAX:
                    tags.add("stack at 79")
                if fill >= 64:
                    if fill == 64:
                        tags.add("drain at exactly 64")
                    fill -= 64
        if fill in (0, 1, 63):
            tags.add("left-over %d" % fill)
    if max(M.LS) > DIG_LDS_LOG2:
        tags.add("global form")
    return tags


def _frontier_tags(t, cus):
    tags = set()
    chunks, blocks = _grid(t.nslots, cus, FR_WAVES)
    W = blocks * FR_WAVES
    if W > chunks:
        tags.add("frontier: wave without a chunk")
    if chunks > W:
        tags.add("frontier: several chunks per wave")
    if not len(t.slot):
        tags.add("frontier: an empty table")
        return tags
    c = t.recs["clock"]
    ragged = t.slot >= (t.nslots // ROUND) * ROUND
    if t.nslots % ROUND and ragged.any() and (~ragged).any() and (c[ragged].max(0) > c[~ragged].max(0)).any():
        tags.add("frontier: the maximum sits in the ragged round")
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
    if len(np.flatnonzero((np.diff(match) == 1) & (np.diff(blk) == 1))):
        tags.add("matches on both sides of a block border")
    if blocks > 1 and blk[-1] == 0:
        tags.add("matches only in block 0")
    if blocks > 1 and blk[0] == blocks - 1:
        tags.add("matches only in the last block")
    return tags


def _expect(seen, tags, what):
    missing = sorted(set(tags) - seen)
    assert not missing, (what, "the layout was meant to reach", missing, "and reached", sorted(seen))


# ---- a layout: which slots hold a row ----

class Spec:
    def __init__(self, name, slots, sparse=(), bucket=None, hot=(), warm=(), expect=()):
        self.name = name
        self.slots = np.unique(np.asarray(slots, np.int64))
        self.sparse = np.isin(self.slots, np.asarray(sparse, np.int64))   # created by a merge of absent keys: the one-key clock {local: 2}
        self.bucket = bucket                  # (L, b): every key falls into bucket b of 2^L
        self.hot = np.isin(self.slots, np.asarray(hot, np.int64))         # component 0 = 1000 in these rows and in no other
        self.warm = np.isin(self.slots, np.asarray(warm, np.int64))       # component K - 1 = 500 in these rows and in no other
        self.expect = set(expect)


VALUES = [0, VAL_MAX, -VAL_MAX, 5, -1]


class Table:
    """One table laid out by slot. The model: slot (ascending) and the rows as records (recs) in that order."""

    def __init__(self, e, nslots, K, local):
        self.e, self.nslots, self.K, self.local = e, nslots, K, local
        self.slot = np.zeros(0, np.int64); self.recs = np.zeros(0, bmx.VC_REC_DTYPE)

    def ids_for(self, slots, field, salt=0):
        """a node id for every slot whose key (id, field) starts its probe sequence there; another salt gives another id"""
        slots = np.asarray(slots, np.int64)
        fields = np.broadcast_to(np.asarray(field, np.uint32), slots.shape)
        nl = self.nslots // 2
        out = np.zeros(len(slots), np.uint64)
        for k, (s, f) in enumerate(zip(slots.tolist(), fields.tolist())):
            line, c = divmod(s, 2)
            h = ((line << 64) + nl - 1) // nl                  # the smallest h with (h * nl) >> 64 == line
            h = (h & ~1) + 2 * (1 + salt) + ((c - field_c(f)) & 1)
            out[k] = ((unmix64(h) - NH_ADD) * NH_INV) & M64
            assert home_slot(out[k], f, self.nslots) == s and int(out[k]) != EMPTY_ID
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
        """write the layout into the (empty) table: ONE load_rows call for the dense rows, then one merge of absent keys for the sparse ones"""
        assert len(self.slot) == 0
        K, slots = self.K, spec.slots
        n = len(slots)
        assert n <= self.nslots // 2 - 1
        i = np.arange(n)
        fields = np.where(i % 2 == 0, FA, FB).astype(np.uint32)
        ids = self.ids_in_bucket(slots, fields, *spec.bucket) if spec.bucket else self.ids_for(slots, fields, salt=3)
        clocks = np.zeros((n, K), np.uint32); ks = np.zeros(n, np.uint32)
        for j in range(n):                                       # row j names j % (K + 1) writers, starting at writer j, components 1..9: none at all every (K + 1)-th row
            keys = [(j + k) % K for k in range(j % (K + 1))]
            for k in keys:
                clocks[j, k] = 1 + (7 * j + 3 * k) % 9
            if spec.hot[j]:
                keys = keys if 0 in keys else keys + [0]
                clocks[j, 0] = 1000
            if spec.warm[j]:
                keys = keys if K - 1 in keys else keys + [K - 1]
                clocks[j, K - 1] = 500
            ks[j] = bmx.keyset(keys)
        val = np.asarray(VALUES, np.int64)[i % len(VALUES)]
        state = np.where(spec.sparse, bmx.VC_SPARSE, bmx.VC_DENSE)
        d, s = ~spec.sparse, spec.sparse
        if self.e is not None:
            if d.any():
                self.e.load_rows(ids[d], fields[d], clocks[d], val[d], keysets=ks[d])
            if s.any():
                f, u = self.e.merge_batch(ids[s], fields[s], clocks[s], val[s], keysets=ks[s])
                assert len(u) == int(s.sum()) and (f == bmx.FLAG_INCOMING).all(), "every delta of an absent key is a first write"
        clocks[s] = 0; clocks[s, self.local] = 2; ks[s] = bmx.keyset([self.local])     # the reference's rule (src/bullet-crt.js:172-185)
        self.slot = slots
        self.recs = M.recs_of(ids, fields, clocks, val, ks, state)
        return self

    def premise(self, capacity_rows):
        """nothing below means anything unless the table is the model: same size, and every row where the layout put it"""
        i = self.e.info()
        assert i.n_slots == self.nslots == nslots_for(capacity_rows), "the table did not grow"
        assert len(self.slot) <= self.nslots // 2 - 1 and i.n_rows == len(self.slot)
        got, n = self.e.export_rows()
        assert n == len(self.slot)
        M.same_recs(got, self.recs, "the export of everything in ascending slot order")

    def sel(self):
        bit = np.zeros(self.nslots, bool)
        bit[self.slot] = True
        return bit

    def queries(self):
        """M.queries plus the first and the last row's buckets (the ends of the table)"""
        qs = M.queries(self.recs, self.K, M.np_frontier(self.recs))
        if len(self.slot):
            for L in (4, 10):
                bk = bmx.key_bucket(self.recs["id"], self.recs["field"], L)
                for j in (0, -1):
                    qs.append((dict(log2_buckets=L, bucket_bits=bmx.bucket_bits_of([int(bk[j])], L)), bk == bk[j]))
        return qs

    def tags(self, cus):
        t = _digest_tags(self.sel(), self.nslots, cus) | _frontier_tags(self, cus)
        for kw, m in self.queries():
            t |= _export_tags(self.slot[m], self.nslots)
            if "frontier" in kw and len(self.slot) and (self.recs["clock"].sum(1) == 0).any():
                assert not m[self.recs["clock"].sum(1) == 0].any()
                t.add("a row without a clock under a frontier")
        return t


def check_all(t):
    e = t.e
    M.check_digest(e, t.recs)
    M.check_frontier(e, t.recs)
    for kw, m in t.queries():
        got, n = e.export_rows(**kw)
        assert n == int(m.sum()), (kw, n, int(m.sum()))
        M.same_recs(got, t.recs[m], kw)
    M.check_export(e, t.recs, t.K, M.np_frontier(t.recs), ordered=True, caps=True)


# ---- small tables ----

SMALL = {4096: (3, 1), 4100: (8, 5), 4352: (1, 0)}       # slots: (K, local). 32 chunks and 8 tiles; a 33rd chunk, a 257th round and a 9th tile of 4 slots; 34 whole chunks, 8.5 tiles


def _chunk(c, offs):
    return c * CHUNK + np.asarray(offs, np.int64)


def small_specs(nslots):
    chunks = (nslots + CHUNK - 1) // CHUNK
    last = np.arange((chunks - 1) * CHUNK, nslots)
    idle = {"wave without a chunk"} if chunks % DIG_WAVES else set()
    tail = {"match in the last live thread"} | ({"ragged chunk"} if nslots % CHUNK else set()) | ({"ragged round"} if nslots % ROUND else set()) | ({"ragged last tile"} if nslots % TILE else set())
    full = np.arange(CHUNK)
    S = [
        Spec("an empty table", [], expect=idle | {"frontier: an empty table"}),
        Spec("one row in slot 0", [0], expect={"left-over 1"} | idle),
        Spec("one row in the last slot", [nslots - 1], hot=[nslots - 1], expect={"left-over 1"} | tail),
        Spec("rows only in the last chunk", np.r_[last[-67:] if len(last) >= 67 else last, 5], hot=last[-1:], sparse=last[-3:-1],
             expect=tail | ({"frontier: the maximum sits in the ragged round"} if nslots % ROUND else set())),
        Spec("a fully occupied chunk", _chunk(3, full), expect={"drain at exactly 64", "a full round", "left-over 0"}),
        Spec("63 rows, a full round, one row", _chunk(2, np.r_[0:63, 64:80, 96]), expect={"stack at 79", "a full round"}),
        Spec("chunks that leave 1 and 63", np.r_[_chunk(4, np.arange(65)), _chunk(5, np.r_[0:21, 32:53, 100:121])], expect={"drain at exactly 64", "left-over 1", "left-over 63"}),
        Spec("a chunk with every other slot occupied", _chunk(6, full[::2]), expect={"drain at exactly 64", "left-over 0"}),
        Spec("dense and sparse rows mixed in a full chunk", _chunk(7, full), sparse=_chunk(7, full[1::3]), expect={"drain at exactly 64", "left-over 0"}),
        Spec("a full chunk in one bucket of sixteen", _chunk(9, full), bucket=(4, 11), expect={"drain at exactly 64", "left-over 0"}),
        Spec("runs across the export's block borders", np.r_[500:524, 2040:2056], sparse=[505, 2050], expect={"matches on both sides of a block border"}),
    ]
    return S


NAMES = [s.name for s in small_specs(4096)]


def _engine(nslots, K, local):
    cap = nslots // 2
    assert nslots_for(cap) == nslots
    return bmx.EngineVC(cap, K, local), cap


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("nslots", sorted(SMALL))
def test_small_table_layouts(nslots, name):
    """one layout in one table of 4096, 4100 or 4352 slots: the premise, every digest, the frontier, every export"""
    spec = small_specs(nslots)[NAMES.index(name)]
    K, local = SMALL[nslots]
    e, cap = _engine(nslots, K, local)
    try:
        t = Table(e, nslots, K, local).lay(spec)
        t.premise(cap)
        if spec.bucket:
            L, b = spec.bucket
            assert (bmx.key_bucket(t.recs["id"], t.recs["field"], L) == b).all()
        if spec.sparse.any():
            assert (t.recs["state"][spec.sparse] == bmx.VC_SPARSE).all() and (t.recs["state"] == bmx.VC_DENSE).any()
        _expect(t.tags(_cus()), spec.expect, (nslots, name))
        check_all(t)
    finally:
        e.close()


# ---- the unpack in front of the merge: record counts around its 256-record workgroup ----

UNPACK_NS = {1: "unpack: one record", 255: "unpack: a ragged workgroup", 256: "unpack: a full workgroup", 257: "unpack: one record past a workgroup"}


@pytest.mark.parametrize("n", sorted(UNPACK_NS))
def test_unpack_at_its_workgroup_edges(n):
    """n records through merge_records, host and device, against merge_batch over their columns on a twin table; K = 3 of the record's 8 components travel"""
    import torch
    K, local = 3, 1
    src = Table(None, 4096, K, local).lay(Spec("records", np.arange(0, 2 * n, 2), sparse=np.arange(0, 2 * n, 6)))
    recs = src.recs.copy()
    recs["aux"] = 0xDEADBEEF; recs["state"] = 0x99                     # ignored on merge
    eh, ed, tw = (bmx.EngineVC(2048, K, local) for _ in range(3))
    want = None
    for rnd in range(2):                                                # into the empty table, then onto its rows with larger clocks
        if rnd:
            recs["clock"][:, :K] += np.arange(n, dtype=np.uint32)[:, None] % 3; recs["val"] //= 2
            live = recs["clock"][:, :K] != 0
            recs["keyset"] = [bmx.keyset(np.flatnonzero(l).tolist()) for l in live]
        want = tw.merge_batch(recs["id"], recs["field"], np.ascontiguousarray(recs["clock"][:, :K]), recs["val"], keysets=recs["keyset"])
        got = eh.merge_records(recs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, rnd, "host")
        d = torch.from_numpy(recs.view(np.int64).copy()).to(M.DEVICE)
        d_upd = torch.full((n + 8,), -1, dtype=torch.int32, device=M.DEVICE); d_nu = torch.full((1,), -1, dtype=torch.int64, device=M.DEVICE); d_fl = torch.full((n + 8,), 0x55, dtype=torch.uint8, device=M.DEVICE)
        torch.cuda.synchronize()
        ed.merge_records_dev(n, d, updated=d_upd, n_updated=d_nu, flags=d_fl); ed.sync()
        nu = int(d_nu.item())
        assert nu == len(want[1]) and np.array_equal(d_upd.cpu().numpy()[:nu].view(np.uint32), want[1]) and (d_upd.cpu().numpy()[n:] == -1).all(), (n, rnd, "device")
        assert np.array_equal(d_fl.cpu().numpy()[:n], want[0]) and (d_fl.cpu().numpy()[n:] == 0x55).all()
    assert len(want[1]) > 0 or n == 1
    rows = M.by_key(tw.dump_rows())
    assert len(rows) == n
    for e in (eh, ed):
        M.same_recs(M.by_key(e.dump_rows()), rows, (n, "rows after the merges"))
    for e in (eh, ed, tw):
        e.close()


# ---- one large table: every wave of the digest walks two chunks ----

def large_nslots(cus):
    """(2G + x) whole chunks and a ragged one of 4 slots, G = the waves of the digest's grid; x the smallest count for which the export's last block has a tile
    beyond the table -> (nslots, G, index of the last whole chunk)"""
    G = 2 * cus * DIG_WAVES
    for x in range(1, 33):
        nslots = (2 * G + x) * CHUNK + 4
        tiles, blocks, tpb = sel_geom(nslots)
        if tiles > SEL_MAX_BLOCKS and blocks * tpb > tiles:
            break
    else:
        x = 1
    return (2 * G + x) * CHUNK + 4, G, 2 * G + x - 1


def large_spec(cus):
    """wave 5: 63 left over from its first chunk meet a full round in its second (the stack at 79). Wave 7: 48 meet 16 (a drain at exactly 64, nothing left).
    Wave 9: 1 left over meets an empty second chunk. Wave 12: 63 rows in its second chunk only. The first waves walk a third chunk; the table's last whole one and
    the ragged chunk of 4 slots behind it hold rows. Chunk 1: the only rows with the large last component, all in the export's block 0. The rows of the last two
    chunks alone hold the large component 0: a frontier one below it matches in the export's last block only."""
    nslots, G, lastc = large_nslots(cus)
    tiles, blocks, tpb = sel_geom(nslots)
    ends = np.r_[_chunk(lastc, [0, 127]), _chunk(lastc + 1, [0, 1, 2, 3])]
    hot = ends[ends >= (blocks - 1) * tpb * TILE]                  # (the last block begins at or before the ragged chunk: a live tile of it holds 4 slots at least)
    warm = _chunk(1, np.arange(40, 81))
    slots = np.r_[_chunk(5, np.arange(63)), _chunk(5 + G, np.arange(16)), _chunk(7, np.arange(48)), _chunk(7 + G, np.arange(16)), _chunk(9, [100]),
                  _chunk(12 + G, np.arange(64, 127)), warm, ends]
    assert warm[-1] < tpb * TILE and len(hot) >= 4 and blocks > 1
    expect = {"carry into a second chunk", "stack at 79", "a full round", "left-over 63", "left-over 1", "left-over 0", "drain at exactly 64", "ragged chunk", "ragged round",
              "global form", "ragged last tile", "match in the last live thread", "matches only in block 0", "matches only in the last block",
              "frontier: several chunks per wave", "a row without a clock under a frontier"}
    if (hot >= (nslots // ROUND) * ROUND).all():
        expect.add("frontier: the maximum sits in the ragged round")
    if tiles > SEL_MAX_BLOCKS:
        assert blocks * tpb > tiles, "the last block has tiles beyond the table"
        expect |= {"tiles_per_block > 1", "tile beyond the table"}
    return nslots, Spec("the large table", slots, sparse=_chunk(5, np.arange(1, 63, 5)), hot=hot, warm=warm, expect=expect)


class Large:
    K, local = 3, 2

    def __init__(self):
        self.cus = _cus()
        self.nslots, self.spec = large_spec(self.cus)
        self.e, self.cap = _engine(self.nslots, self.K, self.local)
        self.t = Table(self.e, self.nslots, self.K, self.local).lay(self.spec)
        self.t.premise(self.cap)
        chunks, blocks = _grid(self.nslots, self.cus, DIG_WAVES)
        assert blocks == 2 * self.cus and chunks > 2 * blocks * DIG_WAVES, "every wave walks two chunks, the first ones a third"
        assert self.nslots > SEL_MAX_BLOCKS * TILE
        _expect(self.t.tags(self.cus), self.spec.expect, "the large table")


@pytest.fixture(scope="module")
def large():
    L = Large()
    yield L
    L.e.close()


def test_large_table_digests_and_frontier(large):
    """more than 2G x 128 slots, G = the waves of the digest's grid: left-overs carried from a wave's first chunk into its second, in both accumulation forms"""
    M.check_digest(large.t.e, large.t.recs)
    fr = M.check_frontier(large.t.e, large.t.recs)
    assert fr[0] == 1000 and fr[large.K - 1] == 500


def test_large_table_exports(large):
    """tiles_per_block > 1 and the last block with tiles beyond the table; matches only in block 0, only in the last block, in the last live thread"""
    t = large.t
    fr = M.np_frontier(t.recs)
    f0 = fr.copy(); f0[0] -= 1
    f2 = fr.copy(); f2[large.K - 1] -= 1
    tiles, blocks, tpb = sel_geom(t.nslots)
    for f, where in ((f0, blocks - 1), (f2, 0)):
        m = M.beyond(t.recs, f, large.K)
        assert m.any() and (t.slot[m] // (tpb * TILE) == where).all()
    check_all(t)


# ---- the layouts together reach every branch on the list ----

def test_the_layouts_reach_every_branch():
    cus = _cus()
    seen = set(UNPACK_NS.values())
    for nslots, (K, local) in SMALL.items():
        for spec in small_specs(nslots):
            seen |= Table(None, nslots, K, local).lay(spec).tags(cus)
    nslots, spec = large_spec(cus)
    seen |= Table(None, nslots, Large.K, Large.local).lay(spec).tags(cus)
    _expect(seen, DIGEST_TAGS + FRONTIER_TAGS + EXPORT_TAGS + UNPACK_TAGS, "all layouts")
