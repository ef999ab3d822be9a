"""No GPU: the arithmetic of tests/test_gpu_sync_kernel_edges.py itself — the inverted probe sequence, its layouts, its queries, caps and guard checks and the
branches its replays say the layouts reach — run against a stand-in engine in plain numpy that places every key by the restated probe sequence of slot.h
and answers dump_rows, index_ids, digest, export_rows and info().n_slots from its own table, in slot order. The CU query is patched to 2, so the large table
is a few hundred KB. It proves nothing about a kernel; it proves that every constructed id lands in its slot, that every layout fits its table, that every
expected tag is reached — and, with stand-ins that carry one defect each, that the GPU suite's checks fail on a subtly wrong answer."""
import numpy as np
import pytest

import bmx
import test_gpu_sync_kernel_edges as edges

DEL = edges.DEL
MARK = 53


class Info:
    pass


class Fake:
    """a table of nslots slots: id (EMPTY_ID: empty), field, the stored clock (bits 53..60: the epoch that created the row) and the value"""
    defect = None

    def __init__(self, capacity_rows, device=0, flags=0, load_pct=0):
        assert flags == bmx.CTX_FIXED_CAPACITY and load_pct == 90
        self.cap = capacity_rows
        self.n = edges.slots_for(capacity_rows, load_pct)
        self.id = np.full(self.n, edges.EMPTY_ID, np.uint64); self.field = np.zeros(self.n, np.uint32)
        self.ts = np.zeros(self.n, np.int64); self.val = np.zeros(self.n, np.int64)
        self.epoch = 0
        self.ix = {}

    def __enter__(self): return self
    def __exit__(self, *a): pass
    def close(self): pass
    def sync(self): pass

    def _find(self, id, field):
        """ProbeSeq<4>: the line's four slots cyclically from the start, then the next line"""
        s0 = edges.home_slot(id, field, self.n)
        line, c = divmod(s0, 4)
        nl = self.n // 4
        for _ in range(nl):
            for k in range(4):
                s = line * 4 + ((c + k) & 3)
                if int(self.id[s]) == edges.EMPTY_ID or (int(self.id[s]) == id and int(self.field[s]) == field):
                    return s
            line = 0 if line + 1 == nl else line + 1
        raise AssertionError("table full")

    def _write(self, id, field, ts, val, rule):
        id = np.asarray(id, np.uint64); field = np.asarray(field, np.uint32); ts = np.asarray(ts, np.int64); val = np.asarray(val, np.int64)
        assert len(set(zip(id.tolist(), field.tolist()))) == len(id)
        assert ((ts >= 0) & (ts <= edges.TS_MAX)).all() and ((np.abs(val) <= edges.VAL_MAX) | ((val == DEL) & (rule == "put"))).all()
        self.epoch += 1
        won = []
        for j, (i, f, t, v) in enumerate(zip(id.tolist(), field.tolist(), ts.tolist(), val.tolist())):
            s = self._find(i, f)
            if int(self.id[s]) == edges.EMPTY_ID:
                self.id[s] = i; self.field[s] = f; self.val[s] = v
                self.ts[s] = (2 if rule == "ref" else t) | (self.epoch << MARK)
                won.append(j)
            elif rule == "put" or (t, v) > (int(self.ts[s]) & edges.TS_MAX, int(self.val[s])):
                self.ts[s] = t; self.val[s] = v
                won.append(j)
        assert (self.id != np.uint64(edges.EMPTY_ID)).sum() <= self.cap
        return np.array(won, np.uint32)

    def load_rows(self, id, field, ts, val): self._write(id, field, ts, val, "delta")
    def put_rows(self, id, field, ts, val): self._write(id, field, ts, val, "put")

    def merge_batch(self, id, field, ts, val, insert_mode=bmx.INSERT_REFERENCE, want_flags=True):
        return self._write(id, field, ts, val, "ref" if insert_mode == bmx.INSERT_REFERENCE else "delta"), None, None

    def info(self):
        i = Info(); i.n_slots = self.n
        return i

    def _occ(self): return self.id != np.uint64(edges.EMPTY_ID)
    def _clock(self): return self.ts if self.defect == "the stored clock not masked" else self.ts & edges.TS_MAX
    def row_count(self): return int(self._occ().sum())

    def dump_rows(self):
        m = self._occ() & (self.val != DEL)
        return self.id[m], self.field[m], (self.ts & edges.TS_MAX)[m], self.val[m]

    def index_build(self, f):
        self.ix[int(f)] = self.id[self._occ() & (self.field == f)].copy()

    def index_ids(self, f): return self.ix[int(f)].copy()

    def digest(self, log2_buckets=10, tombstones=False):
        L = int(log2_buckets)
        m = self._occ() & ((self.val != DEL) | bool(tombstones) | (self.defect == "a tombstone counted with tombstones off"))
        if self.defect == "rows left on the stack behind the last chunk dropped":
            chunks, blocks = edges._digest_grid(self.n, edges._cus())
            W = blocks * edges.DIG_WAVES
            for w in range(W):
                mine = np.concatenate([np.flatnonzero(m[c * edges.CHUNK:(c + 1) * edges.CHUNK]) + c * edges.CHUNK for c in range(w, chunks, W)] + [np.zeros(0, np.int64)])
                if len(mine) % 64:
                    m[mine[-(len(mine) % 64):]] = False
        bits = 10 if (L == 11 and self.defect == "L = 11 bucketed with 10 bits") else L
        b = bmx.key_bucket(self.id[m], self.field[m], bits).astype(np.int64)
        sm = edges.synth.splitmix64_np
        h = sm(self.val[m].astype(np.uint64)); h = sm(h ^ self._clock()[m].astype(np.uint64)); h = sm(h ^ self.field[m].astype(np.uint64)); d = sm(h ^ self.id[m])
        sums = np.zeros(1 << L, np.uint64); counts = np.zeros(1 << L, np.uint64)
        with np.errstate(over="ignore"):
            np.add.at(sums, b, d)
        np.add.at(counts, b, np.uint64(1))
        return sums, counts

    def digest_dev(self, log2_buckets, sums, counts, tombstones=False):
        s, c = self.digest(log2_buckets, tombstones)
        sums.numpy()[:len(s)] = s.view(np.int64); counts.numpy()[:len(c)] = c.view(np.int64)

    def _export(self, since, L, bits, only):
        clock = self._clock()
        m = self._occ() & ((self.val == DEL) == bool(only)) & ((clock > since) if self.defect == "since compared with >" else (clock >= since))
        if bits is not None:
            bk = bmx.key_bucket(self.id, self.field, L).astype(np.int64)
            w = np.asarray(bits, np.uint64)
            m &= ((w[bk >> 6] >> (bk & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
        if self.defect == "the last ragged tile dropped" and self.n % edges.TILE:
            m[(self.n // edges.TILE) * edges.TILE:] = False
        r = np.zeros(int(m.sum()), bmx.DELTA_REC_DTYPE)
        r["id"], r["field"], r["ts"], r["val"] = self.id[m], self.field[m], clock[m], self.val[m]
        if self.defect == "records in a non-slot order":
            r = r[::-1].copy()
        return r

    def export_rows(self, since=0, log2_buckets=0, bucket_bits=None, only_tombstones=False, cap=None, out=None):
        r = self._export(since, log2_buckets, bucket_bits, only_tombstones)
        if out is None:
            return (r if cap is None else r[:cap]), len(r)
        k = min(len(r), len(out))
        out[:k] = r[:k]
        return out[:k], len(r)

    def export_rows_dev(self, out, cap, n_out, since=0, log2_buckets=0, bucket_bits=None, only_tombstones=False):
        r = self._export(since, log2_buckets, None if bucket_bits is None else bucket_bits.numpy().view(np.uint64), only_tombstones)
        n_out[0] = len(r)
        k = min(len(r), cap)
        if out is not None and k:
            out.numpy()[:4 * k] = r[:k].view(np.int64)


class FakeHostBuffer:
    def __init__(self, nbytes): self.raw = np.zeros(nbytes, np.uint8)
    def array(self, dtype, count, offset=0): return np.frombuffer(self.raw, dtype=np.dtype(dtype), count=count, offset=offset)
    def close(self): pass


def _defective(what):
    return type("Wrong", (Fake,), {"defect": what})


@pytest.fixture
def standin(monkeypatch):
    monkeypatch.setattr(bmx, "Engine", Fake)
    monkeypatch.setattr(bmx, "HostBuffer", FakeHostBuffer)
    monkeypatch.setattr(edges, "DEVICE", "cpu")
    monkeypatch.setattr(edges, "_cus", lambda: 2)
    return monkeypatch


@pytest.mark.parametrize("nslots", [4096, 4100, 4352, 1_048_836, 2_097_156])
def test_every_constructed_id_maps_back_to_its_slot(nslots):
    """ids_for against the scalar restatement of ProbeSeq<4> (Python ints), which shares no arithmetic with the array form ids_for checks itself with"""
    t = edges.Table(None, nslots)
    rng = np.random.default_rng(nslots)
    slots = np.unique(np.r_[0:300, nslots - 5:nslots, rng.integers(0, nslots, 2000)])
    for salt in (0, 1, 7):
        for f in (edges.FA, edges.FB, 0, 0xFFFFFFFE):
            ids = t.ids_for(slots, f, salt)
            assert len(set(ids.tolist())) == len(ids) and edges.EMPTY_ID not in set(ids.tolist())
            assert [edges.home_slot(i, f, nslots) for i in ids.tolist()] == slots.tolist()
    a, b = t.ids_for(slots, edges.FA, 0), t.ids_for(slots, edges.FA, 1)
    assert (a != b).all()
    assert edges.unmix64(edges.mix64(0x0123456789ABCDEF)) == 0x0123456789ABCDEF and edges.mix64(edges.unmix64(5)) == 5


def test_the_table_sizes_come_out_as_asked():
    for nslots in edges.SMALL + (edges.large_nslots(2)[0], edges.large_nslots(256)[0]):
        c = edges.capacity_for(nslots)
        assert edges.slots_for(c, 90) == nslots and nslots % 4 == 0
    assert edges.large_nslots(256)[0] == 2_097_412 and edges.sel_geom(2_097_412) == (4097, 820, 5)
    assert edges.sel_geom(4096) == (8, 8, 1) and edges.sel_geom(4100) == (9, 9, 1) and edges.sel_geom(4352) == (9, 9, 1) and edges.sel_geom(0) == (1, 1, 1)
    assert edges._digest_grid(4096, 256) == (16, 2) and edges._digest_grid(4100, 256) == (17, 3) and edges._digest_grid(2_097_412, 256) == (8194, 512)


@pytest.mark.parametrize("name", edges.NAMES)
@pytest.mark.parametrize("nslots", edges.SMALL)
def test_small_table_layouts(standin, nslots, name):
    edges.test_small_table_layouts(nslots, name)


def test_the_large_table(standin):
    L = edges.Large()
    assert L.nslots == 65 * 256 + 4 and len(L.t.slot) <= L.cap
    edges.check_digest(L.t)
    edges.check_export(L.t)


def test_every_layout_fits_and_the_layouts_reach_every_branch(monkeypatch):
    """without any engine, at the CU count of an MI355X: the rows of every layout against capacity_rows, and the union of the tags"""
    monkeypatch.setattr(edges, "_cus", lambda: 256)
    for nslots in edges.SMALL:
        for spec in edges.small_specs(nslots):
            assert len(spec.slots) <= edges.capacity_for(nslots) and (len(spec.slots) == 0 or spec.slots[-1] < nslots)
            assert spec.expect <= edges.Table(None, nslots).lay(spec).tags(256), (nslots, spec.name)
    nslots, spec = edges.large_spec(256)
    assert len(spec.slots) <= edges.capacity_for(nslots) and spec.slots[-1] == nslots - 1
    assert {"tiles_per_block > 1", "tile beyond the table"} <= spec.expect <= edges.Table(None, nslots).lay(spec).tags(256)
    edges.test_the_layouts_reach_every_branch()


WRONG = [
    ("since compared with >", 4096, "a fully occupied chunk"),
    ("the last ragged tile dropped", 4100, "one row in the last slot"),
    ("rows left on the stack behind the last chunk dropped", 4096, "one row in slot 0"),
    ("rows left on the stack behind the last chunk dropped", 4352, "chunks that leave 1 and 63"),
    ("the stored clock not masked", 4096, "a dense chunk of rows created by merges only"),
    ("L = 11 bucketed with 10 bits", 4096, "a fully occupied chunk"),
    ("records in a non-slot order", 4096, "a chunk with every other slot occupied"),
    ("a tombstone counted with tombstones off", 4096, "a dense chunk, every second row a tombstone"),
]


@pytest.mark.parametrize("defect,nslots,name", WRONG)
def test_a_wrong_stand_in_is_caught(standin, defect, nslots, name):
    edges.test_small_table_layouts(nslots, name)                # (the right stand-in passes the very same test)
    standin.setattr(bmx, "Engine", _defective(defect))
    with pytest.raises(AssertionError):
        edges.test_small_table_layouts(nslots, name)


@pytest.mark.parametrize("defect", ["since compared with >", "the last ragged tile dropped", "rows left on the stack behind the last chunk dropped", "the stored clock not masked",
                                    "L = 11 bucketed with 10 bits", "records in a non-slot order"])
def test_a_wrong_stand_in_is_caught_on_the_large_table(standin, defect):
    standin.setattr(bmx, "Engine", _defective(defect))
    with pytest.raises(AssertionError):
        L = edges.Large()
        edges.check_digest(L.t)
        edges.check_export(L.t)


def test_the_replays_on_hand_made_cases():
    n = 4100
    bit = np.zeros(n, bool)
    assert edges._digest_tags(bit, n, 256) == {"wave without a chunk", "global form"}
    assert edges._digest_tags(np.zeros(4096, bool), 4096, 256) == {"global form"}
    bit[0:63] = True; bit[64:128] = True
    assert edges._digest_tags(bit, n, 256) >= {"stack at 127", "left-over 63"} and "drain at exactly 64" not in edges._digest_tags(bit, n, 256)
    bit[128] = True
    assert edges._digest_tags(bit, n, 256) >= {"stack at 127", "drain at exactly 64", "left-over 0"}
    bit[:] = False; bit[4099] = True
    assert edges._digest_tags(bit, n, 256) >= {"ragged chunk", "left-over 1"}
    bit = np.zeros(16 * 256 * 3, bool); bit[5] = True                      # one CU: 16 waves, three chunks each
    assert "carry into a second chunk" in edges._digest_tags(bit, len(bit), 1) and "carry into a second chunk" not in edges._digest_tags(bit, len(bit), 256)
    last = {"ragged last tile", "match in the last live thread", "matches only in the last block"}
    assert edges._export_tags([4099], 4100) == last and edges._export_tags([4098], 4100) == last
    assert edges._export_tags([4097], 4100) == last - {"match in the last live thread"} and edges._export_tags([4095], 4100) == set() and edges._export_tags([], 4100) == set()
    assert edges._export_tags([511, 512], 4096) == {"matches on both sides of a block border"} and edges._export_tags([510, 511], 4096) == {"matches only in block 0"}
    assert edges._export_tags([2559, 2560], 2_097_412) == {"matches on both sides of a block border", "tiles_per_block > 1", "tile beyond the table"}
    assert edges._export_tags([2_097_411], 2_097_412) >= {"matches only in the last block", "ragged last tile", "match in the last live thread"}
