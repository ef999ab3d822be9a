"""A numpy / Python-int restatement of the ordered top-k select (csrc/top_kernels.h, csrc/bmx_top.inc), shared by test_top_kernel_edges_model.py (CPU: the
model's own invariants) and tests/test_gpu_top_kernel_edges.py (helper, not a test).

want(vals, ids, k, desc, after)  : the expected answer — lexsort over (id, +-val) of the eligible rows, the cursor applied, sliced to k (the model of
                                   test_gpu_top.py). This is what the device is compared with.
trace(vals, ids, k, desc)        : the set of tags the select reaches for these ELIGIBLE rows: it follows k_top_init, k_top_digit, k_top_find and k_top_compact
                                   round by round (select() returns the whole record: tags, the boundary, the rows the compaction admits).

The tags are computed from the rows alone, never read off an answer. Every constant is restated here (Geom); a test may scale them down."""
import numpy as np

EMPTY_ID = 2**64 - 1              # bmx.h: the id no node may have
VAL_MAX = 2**53 - 1               # bmx.h VAL_MAX: |value| of a stored number


class Geom:
    """the select's constants"""

    def __init__(self, digit_bits=11, cand=4096, id_bits=64, find_bins=8, value_bits=64):
        self.digit_bits = digit_bits                  # top_kernels.h TOP_DIGIT_BITS
        self.bins = 1 << digit_bits                   # top_kernels.h TOP_BINS
        self.cand = cand                              # top_kernels.h TOP_CAND (== bmx_top.h BMX_TOP_MAX_K)
        self.id_bits = id_bits                        # the node id is one 64-bit word (k_top_find: nsh = 64u at the switch; k_top_init: sh = 64u)
        self.find_bins = find_bins                    # top_kernels.h k_top_find: "eight bins per thread"
        self.value_bits = value_bits                  # bmx_top.inc top_launch: sizeof(T) * 8 bits of key - kmin, 32 in the 4-byte column, 64 in the 8-byte one
        # bmx_top.inc top_launch: `passes` — the digit rounds one query enqueues (3 + 6 on the int32 column, 6 + 6 on the int64 column)
        self.passes = -(-value_bits // digit_bits) + -(-id_bits // digit_bits)


GEOM64, GEOM32 = Geom(value_bits=64), Geom(value_bits=32)

ALL, SELECT, EMPTY = "every eligible row is a candidate (all)", "the select runs", "no eligible row"
SHORT_V, FULL_V, SHORT_I, FULL_I = "short last value digit", "full last value digit", "short last id digit", "full last id digit"
SWITCH, ONE_VALUE = "value digits used up, id digits follow", "one value, id digits from the start"
DONE_V, DONE_I = "done on the whole value word", "done on the whole id"
BIN_0, BIN_TOP = "rank in bin 0", "rank in the last bin (2047)"
FIND_LAST, FIND_FIRST = "rank in a k_top_find thread's last bin", "rank in a k_top_find thread's first bin (not bin 0)"
ROW_FIRST, ROW_LAST, ROW_LAST_OF_THREAD = "rank is the first row of its bin", "rank is the last row of its bin", "rank is the last row of its k_top_find thread (r == off + s)"
ONE_BIN = "one bin holds every row"
ELIG_CAND, ELIG_CAND1 = "exactly 4096 eligible (all)", "4097 eligible (the select)"
DONE_CAND, NOT_DONE_CAND1 = "done with exactly 4096 rows at or below", "not done with 4097 rows at or below"
OUT_OF_PASSES = "more digit rounds than top_launch enqueues"


def value_passes(n): return "value passes: %d" % n
def id_passes(n): return "id passes: %d" % n


# every tag the GPU file's layouts must reach between them (the issue's list); INT32_CANNOT: the 4-byte column's key word has at most 32 bits = 3 digits
TAGS = ({value_passes(n) for n in range(6)} | {id_passes(n) for n in range(7)}
        | {SHORT_V, FULL_V, SHORT_I, SWITCH, ONE_VALUE, DONE_V, DONE_I, BIN_0, BIN_TOP, FIND_LAST, FIND_FIRST, ROW_FIRST, ROW_LAST, ROW_LAST_OF_THREAD, ONE_BIN,
           ELIG_CAND, ELIG_CAND1, DONE_CAND, NOT_DONE_CAND1})
INT32_CANNOT = {value_passes(4), value_passes(5)}


def keys(vals, desc):
    """top_kernels.h top_key: u = (uint64)v ^ 2^63, ~u with BMX_TOP_DESC"""
    u = np.asarray(vals, np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    return ~u if desc else u


def eligible(vals, ids, desc, after):
    """top_kernels.h top_after: strictly behind the cursor (id, val) in (key, id) order; the cursor's value may be any int64"""
    vals = np.asarray(vals, np.int64); ids = np.asarray(ids, np.uint64)
    if after is None:
        return np.ones(len(vals), bool)
    u = keys(vals, desc)
    au = keys(np.array([int(after[1])], np.int64), desc)[0]
    return (u > au) | ((u == au) & (ids > np.uint64(int(after[0]))))


def want(vals, ids, k, desc=False, after=None):
    """-> (ids, vals of the first k eligible rows in order, n_eligible)"""
    vals = np.asarray(vals, np.int64); ids = np.asarray(ids, np.uint64)
    assert len(vals) == len(ids) and (np.abs(vals) <= VAL_MAX).all() and not (ids == np.uint64(EMPTY_ID)).any()
    keep = eligible(vals, ids, desc, after)
    ids, v = ids[keep], vals[keep]
    key = -v if desc else v                              # |v| <= 2^53 - 1: exact
    o = np.lexsort((ids, key))[:k]
    return ids[o], v[o], len(ids)


def _shr(a, s):
    """a >> s for a uint64 array and 0 <= s <= 64"""
    return np.zeros_like(a) if s >= 64 else a >> np.uint64(s)


class Select:
    """what one query's chain of kernels leaves behind"""
    tags = None; admitted = None; n_admitted = 0; kk = 0; all = False; phase = 0; sh = 0; pre = 0; vfix = 0; below = 0; in_bin = 0; rounds = 0
    first_digit = None        # the digit every row takes in the first round (None: no round runs)


def select(vals, ids, k, desc=False, geom=GEOM64):
    vals = np.asarray(vals, np.int64); ids = np.asarray(ids, np.uint64)
    G, S, tags = geom, Select(), set()
    n = len(vals)
    S.tags = tags; S.kk = kk = min(k, n)
    if n == 0:
        tags |= {EMPTY, value_passes(0), id_passes(0)}; S.admitted = np.zeros(0, bool)
        return S
    u = keys(vals, desc)
    kmin, kmax = int(u.min()), int(u.max())              # k_top_sweep0
    word_v = u - np.uint64(kmin)
    if n == G.cand: tags.add(ELIG_CAND)
    if n == G.cand + 1: tags.add(ELIG_CAND1)
    if n <= G.cand:                                      # k_top_init: done at once
        tags |= {ALL, value_passes(0), id_passes(0)}
        S.all = True; S.admitted = np.ones(n, bool); S.n_admitted = n
        return S
    tags.add(SELECT)
    d = kmax - kmin
    assert d < (1 << G.value_bits), "the key word of this column is wider than its values allow"
    if d: phase, sh = 0, d.bit_length()
    else: phase, sh = 1, G.id_bits; tags.add(ONE_VALUE)
    pre = vfix = below = 0
    done, vp, ip, in_bin = False, 0, 0, 0
    while not done:
        if vp + ip == G.passes:                          # bmx_top.inc top_launch enqueues no more
            tags.add(OUT_OF_PASSES)
            break
        w = min(sh, G.digit_bits); nsh = sh - w          # k_top_digit
        if phase == 0:
            word = word_v; share = _shr(word, sh) == np.uint64(pre)
        else:
            word = ids; share = (word_v == np.uint64(vfix)) & (_shr(word, sh) == np.uint64(pre))
        digit = (_shr(word, nsh) & np.uint64((1 << w) - 1)).astype(np.int64)
        if S.first_digit is None: S.first_digit = digit
        hist = np.bincount(digit[share], minlength=G.bins)
        vp, ip = vp + (phase == 0), ip + (phase == 1)
        r = kk - below                                   # k_top_find
        assert 1 <= r <= int(hist.sum()), "the rank lies among the rows that share the prefix"
        cum = np.cumsum(hist)
        b = int(np.searchsorted(cum, r, "left")); in_bin = int(hist[b]); c = int(cum[b]) - in_bin
        t0 = b - b % G.find_bins
        off, s = int(cum[t0]) - int(hist[t0]), int(hist[t0:t0 + G.find_bins].sum())
        assert off < r <= off + s
        if nsh == 0:
            tags.add((FULL_V if w == G.digit_bits else SHORT_V) if phase == 0 else (FULL_I if w == G.digit_bits else SHORT_I))
        if b == 0: tags.add(BIN_0)
        if b == G.bins - 1: tags.add(BIN_TOP)
        if b % G.find_bins == G.find_bins - 1: tags.add(FIND_LAST)
        if b % G.find_bins == 0 and b > 0: tags.add(FIND_FIRST)
        if r == c + 1: tags.add(ROW_FIRST)
        if r == c + in_bin: tags.add(ROW_LAST)
        if r == off + s: tags.add(ROW_LAST_OF_THREAD)
        if in_bin == int(hist.sum()): tags.add(ONE_BIN)
        below += c; pre = (pre << w) | b
        done = below + in_bin <= G.cand
        if below + in_bin == G.cand: tags.add(DONE_CAND)
        if below + in_bin == G.cand + 1: tags.add(NOT_DONE_CAND1)
        if done and nsh == 0: tags.add(DONE_V if phase == 0 else DONE_I)
        if not done and nsh == 0:
            assert phase == 0, "the composite key is unique: the bin of a whole key holds one row"
            phase, vfix, pre, nsh = 1, pre, 0, G.id_bits; tags.add(SWITCH)
        sh = nsh
    tags |= {value_passes(vp), id_passes(ip)}
    # k_top_compact: every row at or below the boundary
    if phase == 0: adm = _shr(word_v, sh) <= np.uint64(pre)
    else: adm = (word_v < np.uint64(vfix)) | ((word_v == np.uint64(vfix)) & (_shr(ids, sh) <= np.uint64(pre)))
    S.admitted = adm; S.n_admitted = int(adm.sum())
    S.phase, S.sh, S.pre, S.vfix, S.below, S.in_bin, S.rounds = phase, sh, pre, vfix, below, in_bin, vp + ip
    return S


def trace(vals, ids, k, desc=False, geom=GEOM64):
    return select(vals, ids, k, desc, geom).tags
