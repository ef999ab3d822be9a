"""GPU: the column scan's own kernels (csrc/select.h: k_scan_mask, k_scan_emit<.., 1> and <.., 8>, scan_emit_stream_block; csrc/scan_kernels.h: PredRange32,
PredRange64, PredFilter, EmitIds, EmitPos) and k_agg_sweep (csrc/agg_kernels.h) at their lane, mask-word, stream-step, flush-group, wave, block and workgroup
edges — small, structured, adversarial columns instead of large random ones.

Every check is exact integer equality against numpy. The index's id column (index_ids) says which row sits at every position, so a test lays a column out BY
POSITION: which positions match, which hold a tombstone. With match = the matching positions in ascending order the scan must return match as positions and
col[match] as ids, element for element ("in index-column order", bmx.h), and len(match) as the count — also into a device buffer that starts in either half
of a 16-byte unit, under every cap, with nothing written outside [0, min(count, cap)).

Which branch of the emit pass a layout reaches is computed from the numpy model (_branches: the counts per 8192-row block against the stream threshold, the
matches per 512-row flush group, the parity of the first output slot, a workgroup's total against 8192) and asserted per test, never read off the answer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from oracle import streams
from oracle.oracle import VAL_DELETED

FA, FS, FG = streams.fnv1a32("age"), streams.fnv1a32("score"), streams.fnv1a32("group")
TOMB = VAL_DELETED
I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)
BLOCK = 8192                      # select.h SCAN_BLOCK_ELEMS
STREAM_MIN = 2400                 # select.h SCAN_STREAM_MIN
SUB8_BLOCKS = 2048                # select.h SCAN_SUB8_BLOCKS
NEVER = 0xFFFFFFFF
FILL = 0x5A5A5A5A5A5A5A5A         # what a device buffer holds before a scan writes into it
QLO, QHI = 10, 12                 # the layouts' query: a matching position holds 10, 11 or 12, any other 9 or 13
DEVICE = "cuda"


def _enc(v, wide):
    """the column's value for the small number v: as it is (int32 column), or shifted left by 33 plus 2^32 — no such value fits int32, the order is kept"""
    v = np.asarray(v, np.int64)
    return (v << 33) + (1 << 32) if wide else v


def _same(got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


class Column:
    """One indexed field of one engine, n rows, laid out by position. `key` is the model: the value at every position (TOMB: a tombstone)."""

    def __init__(self, e, f, n, first):
        self.e, self.f, self.n = e, f, n
        ids = streams.splitmix64_np(np.arange(1, n + 1, dtype=np.uint64))
        first = np.broadcast_to(np.asarray(first, np.int64), (n,)).copy()
        e.load_rows(ids, np.full(n, f, np.uint32), np.full(n, 5, np.int64), first)
        e.index_build(f)
        self.col = e.index_ids(f)
        assert len(self.col) == n and np.array_equal(np.sort(self.col), np.sort(ids)) and not (self.col == np.uint64(FILL)).any()
        order = np.argsort(ids, kind="stable")
        self.key = first[order[np.searchsorted(ids[order], self.col)]]
        self.clock = 10

    def set(self, key):
        """the column holds key[p] at position p: one merge of n deltas under a newer clock (every delta wins), then the tombstones"""
        key = np.asarray(key, np.int64)
        assert key.shape == (self.n,)
        dead = key == TOMB
        self.clock += 10
        n = self.n
        won = self.e.merge_batch(self.col, np.full(n, self.f, np.uint32), np.full(n, self.clock, np.int64), np.where(dead, 0, key))[0]
        assert len(won) == n, "every delta of the test wins"
        if dead.any():
            self.clock += 10
            k = int(dead.sum())
            self.e.put_rows(self.col[dead], np.full(k, self.f, np.uint32), np.full(k, self.clock, np.int64), np.full(k, TOMB, np.int64))
        assert np.array_equal(self.e.index_ids(self.f), self.col), "the test's premise: no position of the index is renumbered"
        self.key = key.copy()

    def match(self, lo, hi):
        return np.flatnonzero((self.key != TOMB) & (self.key >= lo) & (self.key <= hi))


def _engine(rows):
    return bmx.Engine(max(1 << 14, 4 * rows))


# ---- which branches of k_scan_emit<EmitIds, ..> a set of matching positions reaches (numpy only) ----

def _branches(match, n, stream_min=STREAM_MIN, sub8_blocks=SUB8_BLOCKS, out_odd=0):
    """tags of the branches the id output takes for these matches. out_odd: the output buffer starts in the upper half of a 16-byte unit"""
    tags = set()
    nb = max(1, (n + BLOCK - 1) // BLOCK)
    bit = np.zeros(nb * BLOCK, bool); bit[match] = True
    cnt = bit.reshape(nb, BLOCK).sum(1)
    before = np.concatenate([[0], np.cumsum(bit)])             # rank in front of every row

    def block(b, pre):
        if cnt[b] >= stream_min:
            tags.add(pre + "stream")
            if (b + 1) * BLOCK > n:
                tags.add(pre + "stream, ragged block")
                if n - b * BLOCK == 1:
                    tags.add(pre + "stream, one-row block")
            groups = bit[b * BLOCK:(b + 1) * BLOCK].reshape(16, 512).sum(1)
            for j, T in enumerate(groups.tolist()):
                head = 1 if T and ((out_odd + int(before[b * BLOCK + j * 512])) & 1) else 0
                rest = T - head
                tags.add(pre + ("T == 0" if T == 0 else "T == 1" if T == 1 else "T == 512" if T == 512 else "T > 1"))
                if head:
                    tags.add(pre + ("head only" if rest == 0 else "head"))
                if rest & 1:
                    tags.add(pre + "odd rest")
                if rest >> 1:
                    tags.add(pre + "pairs")
            if (groups.reshape(4, 4).sum(1) == 0).any():
                tags.add(pre + "stream, a wave without a match")
        else:
            tags.add(pre + ("gather" if cnt[b] else "gather, empty block"))
            if cnt[b] and n - b * BLOCK == 1:
                tags.add(pre + "gather, one-row block")

    if nb > sub8_blocks:
        for wg in range((nb + 7) // 8):
            blocks = range(8 * wg, min(nb, 8 * wg + 8))
            tot = int(cnt[8 * wg:8 * wg + 8].sum())
            if tot <= BLOCK and not tot >= ((8 * stream_min) & 0xFFFFFFFF):
                tags |= {"sub8 fast path", "sub8 fast path, %d matches" % tot} if tot in (0, 1, BLOCK) else {"sub8 fast path"}
                if tot and match[np.searchsorted(match, 8 * wg * BLOCK + 65535, "right") - 1] == 8 * wg * BLOCK + 65535:
                    tags.add("sub8 fast path, local offset 65535")
            else:
                tags |= {"sub8 fall-through", "sub8 fall-through, %d matches" % tot} if tot == BLOCK + 1 else {"sub8 fall-through"}
                kinds = set()
                for b in blocks:
                    block(b, "sub8 ")
                    kinds.add("s" if cnt[b] >= stream_min else "g")
                if kinds == {"s", "g"}:
                    tags.add("sub8 fall-through, blocks stream and gather")
            if len(blocks) < 8:
                tags.add("sub8 workgroup of %d block%s" % (len(blocks), "" if len(blocks) == 1 else "s"))
    else:
        for b in range(nb):
            block(b, "")
    return tags


# ---- the checks ----

def _dense_cap(match):
    """an odd cap that ends the answer in the middle of the longest run of consecutive matches (None: no run of three)"""
    if len(match) < 3:
        return None
    cut = np.flatnonzero(np.diff(match) != 1)
    starts = np.concatenate([[0], cut + 1]); ends = np.concatenate([cut + 1, [len(match)]])
    k = int(np.argmax(ends - starts))
    if ends[k] - starts[k] < 3:
        return None
    return (int(starts[k] + ends[k]) // 2) | 1


class DevOut:
    """a device buffer of ids and a device count word, made once per test"""

    def __init__(self, n):
        import torch
        self.torch = torch
        self.buf = torch.empty(n + 9, dtype=torch.int64, device=DEVICE)
        self.n_out = torch.zeros(1, dtype=torch.int64, device=DEVICE)
        assert self.buf.data_ptr() % 16 == 0

    def sync(self):
        if DEVICE == "cuda":
            self.torch.cuda.synchronize()

    def check(self, c, lo, hi, match, what, seen=None, **form):
        e, f = c.e, c.f
        k = len(match)
        want = c.col[match]
        for off in (0, 1):
            if seen is not None and k:
                seen |= _branches(match, c.n, out_odd=off, **form)
            for cap in sorted({k, k - 1, 1, _dense_cap(match)} - {None, -1}):
                self.buf.fill_(FILL); self.n_out.fill_(-1); self.sync()
                e.scan_range_dev(f, lo, hi, self.buf[off:], cap, self.n_out)
                e.sync()
                got = self.buf.cpu().numpy().view(np.uint64)
                m = min(k, cap)
                assert int(self.n_out.item()) == k, (what, off, cap, "the count is the full one")
                _same(got[off:off + m], want[:m], (what, "device ids", off, cap))
                assert (got[:off] == np.uint64(FILL)).all() and (got[off + m:] == np.uint64(FILL)).all(), (what, off, cap, "nothing outside [0, min(count, cap)) is written")


def _check(c, lo, hi, what, dev=None, seen=None, **form):
    """positions, ids and count of one range against the model; `dev`: the same into a device buffer"""
    e, f = c.e, c.f
    match = c.match(lo, hi)
    _same(e.scan_range_pos(f, lo, hi), match, (what, "positions"))
    _same(e.scan_range(f, lo, hi), c.col[match], (what, "ids"))
    assert e.scan_count(f, lo, hi) == len(match), (what, "count")
    if dev is not None:
        dev.check(c, lo, hi, match, what, seen, **form)
    return match


# ---- layouts: which positions match, which hold a tombstone ----

def _runs(n):
    """[a, b) with a and b even and odd, inside one mask word and across a flush-group, a wave and a block border"""
    out = []
    for border, name in ((40, "inside one word"), (512, "across a flush-group border"), (2048, "across a wave border"), (8192, "across a block border"), (16384, "across the second block border")):
        for da, db in ((6, 6), (5, 7), (6, 7), (5, 6)):
            a, b = border - da, min(border + db, n)
            if a < b and (border < n or border == 40):
                out.append(("run [%d, %d) %s" % (a, b, name), a, b))
    return out


def _layouts(n, rng, reduced=False):
    """(name, match by position, tombstone by position); every layout is followed by its complement"""
    p = np.arange(n)
    none = np.zeros(n, bool)
    out = []

    def add(name, m, dead=none):
        out.append((name, m & ~dead, dead)); out.append(("all but: " + name, ~m & ~dead, dead))

    add("nothing", none)
    for s in sorted({0, 1, 31, 32, 511, 512, 2047, 2048, 8191, 8192, n - 1}):
        if 0 <= s < n:
            add("a single match at %d" % s, p == s)
    for name, a, b in _runs(n):
        add(name, (p >= a) & (p < b))
    for length in (2399, 2400, 2401):              # the default stream threshold from both sides; waves 2 and 3 of the block stay empty
        for b0 in (0, BLOCK):
            a = b0 + 101
            if a + length <= min(n, b0 + 4096):
                add("a run of %d in the block at %d" % (length, b0), (p >= a) & (p < a + length))
    if n % BLOCK == 1 and n > BLOCK:
        add("a dense block followed by a one-row last block", p >= n - 1 - BLOCK)
        add("a dense block followed by a one-row last block without a match", (p >= n - 1 - BLOCK) & (p < n - 1))
    add("a 30 % mix", rng.random(n) < 0.3)
    if reduced:
        return out
    add("every 2nd from 0", p % 2 == 0); add("every 2nd from 1", p % 2 == 1)
    add("every 32nd on bit 0", p % 32 == 0); add("every 32nd on bit 31", p % 32 == 31)
    add("every 128th", p % 128 == 127); add("every 512th", p % 512 == 0)
    for w in range(4):
        if 2048 * (w + 1) <= n:
            add("wave %d full, three empty" % w, (p >= 2048 * w) & (p < 2048 * (w + 1)))
    add("everything, tombstones scattered over it", ~none, (p % 7 == 3) | (p == 0) | (p == n - 1) | (p % 512 == 511))
    add("a 30 % mix, tombstones scattered over matches and others", rng.random(n) < 0.3, rng.random(n) < 0.2)
    for length in (2399, 2400):                    # 2401 / 2402 positions of which two are tombstones: the block's count is what the threshold sees
        if 101 + length + 2 <= min(n, 4096):
            add("a run of %d around two tombstones" % length, (p >= 101) & (p < 101 + length + 2), (p == 200) | (p == 1301))
    return out


def _keys(m, dead, wide):
    """values for a layout: 10, 11, 12 at matching positions, 9 and 13 at the others"""
    p = np.arange(len(m), dtype=np.int64)
    return np.where(dead, TOMB, _enc(np.where(m, QLO + p % 3, np.where(p % 2 == 0, QLO - 1, QHI + 1)), wide))


def _lane_sizes(wide):
    e = 2 if wide else 4
    return {e - 1, e, e + 1}


SIZES = sorted({1, 2, 3, 4, 5} | {s + d for s in (32, 128, 512, 2048, 8192, 16384, 24576) for d in (-1, 0, 1)})


def _run_layouts(c, wide, layouts, dev, seen, **form):
    lo, hi = int(_enc(QLO, wide)), int(_enc(QHI, wide))
    for name, m, dead in layouts:
        c.set(_keys(m, dead, wide))
        match = _check(c, lo, hi, (c.n, wide, name, form), dev, seen, **form)
        _same(match, np.flatnonzero(m), name)                  # (the layout is what it says)


def _expect(seen, tags, what):
    missing = sorted(set(tags) - seen)
    assert not missing, (what, "the layouts were meant to reach", missing, "and reached", sorted(seen))


def _default_tags(n):
    """what the layouts of a size must reach under the default switches, by the model"""
    tags = {"gather"}
    if n > 2502:          # the runs of 2400 and 2401 and the complements of small layouts stream
        tags |= {"stream", "T == 0", "T > 1", "T == 512", "head", "odd rest", "pairs", "stream, a wave without a match"}
    if n % BLOCK > 2502:
        tags |= {"stream, ragged block"}
    if n > BLOCK and n % BLOCK == 1:
        tags |= {"gather, one-row block"}
    if n > BLOCK:
        tags |= {"gather, empty block"}
    return tags


# ---- A. every layout at every size, default switches ----

@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_every_layout_under_the_default_switches(wide, n):
    """k_scan_mask (PredRange32: four rows per lane, eight lanes per mask word; PredRange64: two and sixteen) and k_scan_emit<.., 1>: the gather below 2400 matches
    per block, the streamed output from there on. Sizes: 1..5, and one less, exactly and one more than a mask word, a stream step, a flush group, a wave, one,
    two and three blocks."""
    f = FS if wide else FA
    assert _lane_sizes(wide) <= set(SIZES)
    rng = np.random.default_rng(100 + n)
    seen = set()
    with _engine(n) as e:
        c = Column(e, f, n, _enc(0, wide))
        _run_layouts(c, wide, _layouts(n, rng), DevOut(n), seen)
    _expect(seen, _default_tags(n), (n, wide))


# ---- B. a reduced set under each switch of the id output ----

SIZES_B = [1, 5, 33, 129, 511, 513, 2047, 2049, 8191, 8192, 8193, 16385, 24577]
FORMS = {
    "every block streams": ({"BMX_SCAN_STREAM_MIN": "1"}, {"stream_min": 1}),
    "no block streams": ({"BMX_SCAN_STREAM_MIN": "0xFFFFFFFF"}, {"stream_min": NEVER}),
    "sixteen loads deep": ({"BMX_SCAN_NT": "4"}, {}),
    "every block streams, sixteen loads deep": ({"BMX_SCAN_STREAM_MIN": "1", "BMX_SCAN_NT": "4"}, {"stream_min": 1}),
}


def _form_tags(form, n):
    if form == "no block streams":
        return {"gather"}
    if form == "sixteen loads deep":
        return _default_tags(n)
    tags = {"stream", "T == 0", "T == 1", "head only"}          # a single match: one flush group with one id, fifteen with none; at an odd slot it is all head
    if n >= 513:
        tags |= {"T > 1", "head", "odd rest", "pairs"}
    if n >= 2049:
        tags |= {"T == 512", "stream, a wave without a match"}
    if n % BLOCK:
        tags |= {"stream, ragged block"}
    if n % BLOCK == 1:
        tags |= {"stream, one-row block"}
    return tags


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", SIZES_B)
def test_reduced_layouts_under_each_switch(monkeypatch, wide, form, n):
    """BMX_SCAN_STREAM_MIN=1: every block with a match streams — flush groups without a match (T == 0), with one, an answer that is all head, an odd rest, a
    ragged and a one-row streamed block. 0xFFFFFFFF: the gather for every density. BMX_SCAN_NT=4: scan_emit_stream_block<16>. The switches are read per scan."""
    f = FS if wide else FA
    env, model = FORMS[form]
    rng = np.random.default_rng(200 + n)
    seen = set()
    with _engine(n) as e:
        c = Column(e, f, n, _enc(0, wide))
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _run_layouts(c, wide, _layouts(n, rng, reduced=True), DevOut(n), seen, **model)
    if form == "no block streams":
        assert not any("stream" in t or t.startswith("T ") for t in seen), seen
    _expect(seen, _form_tags(form, n), (n, wide, form))


# ---- C. eight blocks per workgroup: BMX_SCAN_SUB8_BLOCKS=1 ----

SIZES_C = [8193, 65535, 65536, 65537, 131075]
GROUP = 8 * BLOCK


def _layouts_sub8(n, rng):
    p = np.arange(n)
    none = np.zeros(n, bool)
    out = []

    def add(name, m):
        out.append((name, m, none))

    first = p < GROUP
    spread = p % 8 == 0                                  # 1024 matches in every whole block: 8192 in a whole group
    if n >= GROUP:
        add("8192 matches spread over the first workgroup's blocks", first & spread)
        add("8193 matches spread over the first workgroup's blocks", first & (spread | (p == 4099)))
        add("a single match on the last row of the first workgroup", p == GROUP - 1)
        add("all but a single match on the last row of the first workgroup", p != GROUP - 1)
    else:
        add("8192 matches: the first block", p < BLOCK)
        add("8192 matches in the workgroup's first two blocks", (p >= 1) & (p < BLOCK + 1))
    if n >= 2 * GROUP:
        add("8192 matches in the first workgroup, 8193 in the second", spread & (p < 2 * GROUP) | (p == GROUP + 4099))
        add("8193 matches in the first workgroup, 8192 in the second, one in the third", spread & (p < 2 * GROUP) | (p == 4099) | (p == n - 1))
        add("a single match on the last row of the second workgroup", p == 2 * GROUP - 1)
    add("everything", ~none)
    add("the last row only", p == n - 1)
    add("all but the last row", p != n - 1)
    a, b = BLOCK + 100, min(n, 4 * BLOCK + 1000)
    add("a dense run [%d, %d): blocks that stream beside blocks that gather" % (a, b), (p >= a) & (p < b))
    add("a run of 2400 and 5000 spread matches: one block streams, the workgroup falls through", ((p >= 101) & (p < 2501)) | ((p >= BLOCK) & (p % 8 == 1) & (p < 6 * BLOCK)))
    add("a 30 % mix", rng.random(n) < 0.3)
    add("a 10 % mix", rng.random(n) < 0.1)
    for s in sorted({0, 8191, 8192, n - 1}):
        add("a single match at %d" % s, p == s)
    for name, a, b in _runs(n):
        if "block border" in name:
            add(name, (p >= a) & (p < b))
    return out


def _sub8_tags(n):
    tags = {"sub8 fast path", "sub8 fast path, 1 matches", "sub8 fall-through", "sub8 stream", "sub8 gather", "sub8 fall-through, blocks stream and gather", "sub8 T == 512", "sub8 head", "sub8 odd rest"}
    tags |= {"sub8 fast path, %d matches" % BLOCK}
    if n >= GROUP:
        tags |= {"sub8 fall-through, %d matches" % (BLOCK + 1), "sub8 fast path, local offset 65535"}
    last = (n % GROUP + BLOCK - 1) // BLOCK                   # blocks of a last workgroup that has fewer than eight
    if 0 < last < 8:
        tags |= {"sub8 workgroup of %d block%s" % (last, "" if last == 1 else "s")}
    if n == BLOCK + 1:                                         # (a last workgroup of nothing but a one-row block never leaves the fast path)
        tags |= {"sub8 gather, one-row block"}
    return tags


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES_C)
def test_eight_blocks_per_workgroup(monkeypatch, wide, n):
    """k_scan_emit<.., 8> on columns of 2 to 17 blocks: its one-scan fast path up to 8192 matches per workgroup (the largest 16-bit local offset, 65535,
    among them) and its block-by-block fall-through from 8193 on, both kinds of workgroup in one scan, blocks that stream beside blocks that gather, a last
    workgroup of one one-row block (65,537 rows) and of one three-row block (131,075)."""
    f = FS if wide else FA
    rng = np.random.default_rng(300 + n)
    seen = set()
    with _engine(n) as e:
        c = Column(e, f, n, _enc(0, wide))
        monkeypatch.setenv("BMX_SCAN_SUB8_BLOCKS", "1")
        _run_layouts(c, wide, _layouts_sub8(n, rng), DevOut(n), seen, sub8_blocks=1)
    _expect(seen, _sub8_tags(n), (n, wide))


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("stream_min", [1, NEVER])
@pytest.mark.parametrize("n", [BLOCK + 1, GROUP + 1])
def test_eight_blocks_per_workgroup_with_the_stream_forced_and_off(monkeypatch, wide, stream_min, n):
    """the same kernel where every block with a match streams (the fast path is left from eight matches on; at 8193 rows the workgroup's second block is one
    streamed row) and where none does"""
    f = FS if wide else FA
    rng = np.random.default_rng(400 + n)
    seen = set()
    with _engine(n) as e:
        c = Column(e, f, n, _enc(0, wide))
        monkeypatch.setenv("BMX_SCAN_SUB8_BLOCKS", "1")
        monkeypatch.setenv("BMX_SCAN_STREAM_MIN", "%d" % stream_min)
        p = np.arange(n)
        few = [0, 31, 4000, 8191, 8192, 30000, 65534, 65535]
        more = [("up to seven matches in the first workgroup", np.isin(p, few[:3] + few[4:]), np.zeros(n, bool)), ("up to eight matches", np.isin(p, few), np.zeros(n, bool))]
        _run_layouts(c, wide, _layouts_sub8(n, rng) + more, DevOut(n), seen, sub8_blocks=1, stream_min=stream_min)
    if stream_min == 1:
        _expect(seen, {"sub8 fast path", "sub8 fall-through", "sub8 stream", "sub8 T == 0", "sub8 T == 1", "sub8 head only", "sub8 gather, empty block"}
                | ({"sub8 stream, one-row block"} if n == BLOCK + 1 else set()), (n, wide))
    else:
        _expect(seen, {"sub8 fast path", "sub8 fall-through", "sub8 gather"} | ({"sub8 gather, one-row block"} if n == BLOCK + 1 else set()), (n, wide))
        assert not any("stream" in t for t in seen), seen


# ---- D. extreme values in the ragged last lane group, and the query bounds ----

BOUNDS = [(-(1 << 62), 1 << 62), (I32_MIN, I32_MAX), (I32_MAX, I32_MAX), (I32_MIN + 1, I32_MIN + 1), (I32_MIN, I32_MIN), (1 << 31, 1 << 40), (-(1 << 40), -(1 << 31) - 1),
          (5, 4), (1 << 62, -(1 << 62)), (I32_MIN + 1, 0), (0, I32_MAX), (-3, 3)]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 33, 8191, 8193, 8195])
def test_extreme_values_in_the_last_lane_group_and_the_query_bounds(wide, n):
    """INT32_MAX and INT32_MIN + 1 as real values of the int32 column in its last, ragged lane group (read element by element), tombstones beside them (INT32_MIN
    in that column); the same rows with one real -(2^31), which makes the index scan its int64 column. Bounds: everything, all of int32, single extreme values,
    ranges beyond int32 on either side (empty on the int32 column), lo > hi."""
    f = FA
    rng = np.random.default_rng(500 + n)
    key = rng.integers(-4, 5, n).astype(np.int64)
    tail = np.arange(n - n % 4 if n % 4 else n - 1, n) if not wide else np.arange(n - n % 2 if n % 2 else n - 1, n)
    key[tail] = np.resize(np.array([I32_MAX, I32_MIN + 1, I32_MAX], np.int64), len(tail))
    key[0] = I32_MIN + 1 if n > 4 else key[0]
    if n >= 6:
        key[[n // 2, n - 5]] = TOMB
    if wide:
        key[n // 3 if n > 2 else 0] = I32_MIN                  # a real -(2^31)
    with _engine(n) as e:
        c = Column(e, f, n, 0)
        c.set(key)
        dev = DevOut(n)
        total = 0
        for lo, hi in BOUNDS:
            total += len(_check(c, lo, hi, (n, wide, lo, hi), dev))
        assert len(c.match(I32_MIN, I32_MIN)) == (1 if wide else 0) and (len(c.match(I32_MAX, I32_MAX)) >= 1 or (wide and n == 1)) and total > 0
        assert len(c.match(1 << 31, 1 << 40)) == 0 and len(c.match(-(1 << 40), -(1 << 31) - 1)) == 0


# ---- E. the declarative filter: PredFilter, two rows per lane, always on the int64 column ----

@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 31, 33, 513, 2049, 8193, 16385])
def test_filter_of_two_terms_in_column_order(monkeypatch, wide, n):
    """scan_filter([(f, lo, hi), (g, glo, ghi)]): the second field absent on every third node, then true for every node, then true at every other position;
    ids in column order against the model, under the default switches and with every block streaming"""
    f = FS if wide else FA
    rng = np.random.default_rng(600 + n)
    lo, hi = int(_enc(QLO, wide)), int(_enc(QHI, wide))
    p = np.arange(n)
    seen = set()
    with _engine(2 * n) as e:
        c = Column(e, f, n, _enc(0, wide))
        clock = 7

        def set_g(rows, vals):
            nonlocal clock
            clock += 10
            k = int(rows.sum())
            if k:
                assert len(e.merge_batch(c.col[rows], np.full(k, FG, np.uint32), np.full(k, clock, np.int64), np.broadcast_to(np.asarray(vals, np.int64), (n,))[rows])[0]) == k

        steps = [("absent on every third node", lambda: set_g(p % 3 != 0, 100), p % 3 != 0),
                 ("true for every node", lambda: set_g(p % 3 == 0, 100), np.ones(n, bool)),
                 ("true at every other position", lambda: set_g(p >= 0, np.where(p % 2 == 0, 100, 201)), p % 2 == 0)]
        for gname, write, gtrue in steps:
            write()
            for name, m, dead in _layouts(n, rng, reduced=True):
                c.set(_keys(m, dead, wide))
                want = np.flatnonzero(m & gtrue)
                for env in ({}, {"BMX_SCAN_STREAM_MIN": "1"}):
                    for k, v in env.items():
                        monkeypatch.setenv(k, v)
                    _same(e.scan_filter([(f, lo, hi), (FG, 100, 200)]), c.col[want], (n, wide, gname, name, env, "filter"))
                    _same(e.scan_filter([(f, lo, hi), (FG, 100, 200)], cap=len(want) // 2 + 1), c.col[want[:len(want) // 2 + 1]], (n, wide, gname, name, env, "filter, cap"))
                    if len(want):
                        seen |= _branches(want, n, stream_min=1 if env else STREAM_MIN)
                    for k in env:
                        monkeypatch.delenv(k)
                _same(e.scan_filter([(f, lo, hi), (FG, 300, 400)]), [], (n, wide, gname, name, "second term false everywhere"))
    _expect(seen, {"stream", "T == 0", "T == 1", "gather"}, (n, wide))


# ---- F. k_agg_sweep: the ragged tail is block 0's; a round is 8192 int32 / 4096 int64 elements ----

def _agg_want(vals, group_lo, ngroups):
    """Python-int arithmetic: vals = the matching rows' values"""
    recs = [[0, 0, None, None] for _ in range(ngroups + 1 if ngroups else 1)]
    for v in vals:
        g = v - group_lo if ngroups and 0 <= v - group_lo < ngroups else ngroups
        r = recs[g]
        r[0] += 1; r[1] += v
        r[2] = v if r[2] is None else min(r[2], v); r[3] = v if r[3] is None else max(r[3], v)
    return recs


def _agg_check(e, f, lo, hi, vals, group_lo, what):
    vals = [int(v) for v in vals]
    got = e.scan_aggregate([(f, lo, hi)], measure=f)
    (cnt, s, mn, mx), = _agg_want(vals, 0, 0)
    assert (got.n_match, got.n, got.sum, got.min, got.max) == (cnt, cnt, s, mn, mx), (what, got)
    for ngroups in (1, 100, 1025):
        got = e.scan_aggregate([(f, lo, hi)], measure=f, group=f, group_lo=group_lo, ngroups=ngroups)
        want = _agg_want(vals, group_lo, ngroups)
        assert len(got) == ngroups + 1
        for g, (r, (cnt, s, mn, mx)) in enumerate(zip(got, want)):
            assert (r.n_match, r.n, r.sum, r.min, r.max) == (cnt, cnt, s, mn, mx), (what, ngroups, g, r)
    assert e.scan_count(f, lo, hi) == len(vals), what


@pytest.mark.parametrize("kind", ["int32", "int64 shifted", "int64 by one -2^31"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 4095, 4096, 4097, 4099, 8191, 8192, 8193, 8197])
def test_aggregates_of_short_columns_and_at_the_sweeps_round(kind, n):
    """scan_aggregate([(f, lo, hi)], measure=f), alone and grouped by f into 1, 100 and 1025 groups (the LDS form and the form of global atomics): every row,
    none, the ragged tail only, tombstones in the tail"""
    wide = kind != "int32"
    shifted = kind == "int64 shifted"
    f = FS if shifted else FA
    p = np.arange(n, dtype=np.int64)
    E = 2 if wide else 4
    tail = p >= n - n % E if n % E else p >= n - 1
    val = _enc((p * 7) % 1500, shifted)                        # 0 .. 1499: inside and outside the windows of 1, 100 and 1025 groups
    out = _enc(np.where((p % 2 == 0) & (kind != "int64 by one -2^31"), -1 - p % 3, 2001 + p % 5), shifted)      # (the third kind's query reaches down to -2^31)
    lo, hi = int(_enc(0, shifted)), int(_enc(2000, shifted))
    none = np.zeros(n, bool)
    layouts = [("every row", ~none, none), ("none", none, none), ("the tail only", tail, none), ("every row, tombstones in the tail", ~none, tail & (p % 2 == 1) | (p == n - 1)),
               ("every row, tombstones scattered", ~none, p % 5 == 2), ("all but the tail", ~tail, none)]
    with _engine(n) as e:
        c = Column(e, f, n, _enc(0, shifted))
        for name, m, dead in layouts:
            key = np.where(dead, TOMB, np.where(m, val, out))
            qlo = lo
            if kind == "int64 by one -2^31" and not dead[n - 1]:
                key[n - 1] = I32_MIN                            # the row that makes the column wide sits in the tail; the query reaches down to it where the tail matches
                qlo = I32_MIN if m[n - 1] else lo
            c.set(key)
            match = c.match(qlo, hi)
            _agg_check(e, f, qlo, hi, c.key[match], lo, (kind, n, name))
            _same(e.scan_range_pos(f, qlo, hi), match, (kind, n, name, "positions"))
