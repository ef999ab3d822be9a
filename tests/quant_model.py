"""A numpy model of the exact quantiles over boolean filters (include/bmx_quant.h), shared by test_quant_model.py (CPU: the stand-in against brute force) and
the GPU tests (helper, not a test). The table and the selection are where_agg_model.Model's.

quantiles(m, base, clauses, measure, qs) : the records and the result record of bmx_where_quantiles, every byte: numpy.sort of the sample, bmx.quant_rank for the
                                           rank, searchsorted for n_below and n_equal.
select(vals, bits, qs, geom)             : a sequential stand-in of k_quant_init / k_quant_digit / k_quant_find (csrc/quant_kernels.h) over values and mask bits
                                           laid out BY INDEX POSITION. It gives the same records and, beside them, a Trace of the paths the kernels took: the
                                           number of digit passes, the distinct live prefixes (NP) of each pass, the bin every rank landed in, what the waves of
                                           the digit sweep saw (all of a wave's rows in one bin, in 64 bins, lane 0 or lane 63 alone), and how many histogram
                                           bins two workgroups both flushed. The GPU edge tests assert these tags on the stand-in before they ask the device, so a
                                           test that no longer reaches its path fails instead of passing for nothing.
The geometry (Geom) is the kernels': DIGIT_BITS = 11, 512 threads, 4 loads in flight, waves of 64, E = 4 or 2 values per load, eight bins per thread of
k_quant_find; test_quant_model.py scales it down."""
import numpy as np

import bmx
from where_agg_model import DATA

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
BIAS = 1 << 63
FILL = 0x5A


def records(sample, qs):
    """sample: the measure values (any order) -> (records, min, max) by sorting"""
    v = np.sort(np.asarray(sample, np.int64))
    out = np.zeros(len(qs), bmx.QUANT_REC_DTYPE)
    if len(v):
        for i, (num, den) in enumerate(qs):
            r = bmx.quant_rank(num, den, len(v))
            lo, hi = np.searchsorted(v, v[r], "left"), np.searchsorted(v, v[r], "right")
            out[i] = (int(v[r]), r, int(lo), int(hi - lo))
    return out, (int(v[0]) if len(v) else I64MAX), (int(v[-1]) if len(v) else I64MIN)


def quantiles(m, base, clauses, measure, qs):
    """-> (records: QUANT_REC_DTYPE[len(qs)], res: a 0-d QUANT_RES_DTYPE)"""
    sel = m.mask(base, clauses)
    m._f(measure)
    have = sel & (m.st[measure] == DATA)
    out, mn, mx = records(m.val[measure][have], qs)
    res = np.zeros((), bmx.QUANT_RES_DTYPE)
    res["n_match"] = int(sel.sum()); res["n"] = int(have.sum()); res["min"] = mn; res["max"] = mx
    return out, res


class Geom:
    """the shape of the digit sweep and of the bin search"""

    def __init__(self, E, digit_bits=11, threads=512, inflight=4, wave=64, find_threads=256, max_groups=512, rounds_per_group=4):
        self.E, self.digit_bits, self.threads, self.inflight, self.wave, self.find_threads = E, digit_bits, threads, inflight, wave, find_threads
        self.max_groups, self.rounds_per_group = max_groups, rounds_per_group
        self.bins = 1 << digit_bits
        assert self.bins % find_threads == 0 and threads % wave == 0
        self.share = self.bins // find_threads              # bins per thread of the bin search

    def round_units(self):
        return self.threads * self.inflight                 # units one workgroup loads per round

    def groups(self, n):
        """bmx_query.inc sweep_grid: no workgroup with fewer than rounds_per_group rounds, max_groups (two per CU) at most, one at least"""
        per = self.rounds_per_group * self.round_units() * self.E
        return int(max(1, min((n + per - 1) // per, self.max_groups)))


class Trace:
    def __init__(self):
        self.passes = 0            # digit passes that ran
        self.np = []               # distinct live prefixes of each pass
        self.widths = []           # digit width of each pass
        self.bins = []             # per pass: the bin of every rank
        self.one_bin_waves = 0     # waves (one element slot of one load) with >= 2 rows counted, all in one (histogram, bin): they add once
        self.max_bins_in_wave = 0  # the most distinct (histogram, bin) one wave hit
        self.lane0_alone = 0       # waves whose only counted row sits in lane 0 / in the last lane
        self.last_lane_alone = 0
        self.shared_bins = 0       # (pass, histogram, bin) that two or more workgroups flushed
        self.groups = 1


def _bits(d):
    return int(d).bit_length()


def select(vals, bits, qs, geom):
    """vals: int64 per index position, bits: bool per position (selected and measured) -> (records, Trace)"""
    vals = np.asarray(vals, np.int64); bits = np.asarray(bits, bool)
    g = geom
    t = Trace()
    n_pos = len(vals)
    t.groups = g.groups(n_pos)
    pos = np.nonzero(bits)[0]
    u = vals[pos].astype(np.uint64) ^ np.uint64(BIAS)
    n = len(pos)
    out = np.zeros(len(qs), bmx.QUANT_REC_DTYPE)
    if not n:
        return out, t
    kmin, kmax = int(u.min()), int(u.max())
    word = (u - np.uint64(kmin)).astype(np.uint64)
    # where a position sits in the sweep (csrc/top_kernels.h top_sweep): unit -> round, workgroup, load slot, thread; the element slot is pos % E
    unit = pos // g.E
    per_round = t.groups * g.round_units()
    rem = unit % per_round
    group = rem // g.round_units()
    slot = (rem % g.round_units()) // g.threads
    tid = rem % g.threads
    lane = tid % g.wave
    wave_key = ((((unit // per_round) * t.groups + group) * g.inflight + slot) * (g.threads // g.wave) + tid // g.wave) * g.E + pos % g.E
    # k_quant_init
    nq = len(qs)
    rank = [bmx.quant_rank(a, b, n) for a, b in qs]
    prefix, below, n_equal = [0] * nq, [0] * nq, [n] * nq
    live, slot_of = [0], [0] * nq
    sh = _bits(kmax - kmin)
    while sh:
        w = min(sh, g.digit_bits); nsh = sh - w
        t.np.append(len(live))                               # what the pass starts with: 1 for the first, what the find before it left for the others
        # k_quant_digit
        pre = word >> np.uint64(sh) if sh < 64 else np.zeros(n, np.uint64)
        j = np.full(n, -1, np.int64)
        for k, p in enumerate(live):
            j[pre == np.uint64(p)] = k
        ok = j >= 0
        d = j * g.bins + ((word >> np.uint64(nsh)) & np.uint64((1 << w) - 1)).astype(np.int64)
        hist = np.bincount(d[ok], minlength=len(live) * g.bins).reshape(len(live), g.bins)
        # what the waves saw
        wk, dk, ln = wave_key[ok], d[ok], lane[ok]
        if len(wk):
            order = np.lexsort((dk, wk)); wk, dk, ln = wk[order], dk[order], ln[order]
            new_wave = np.ones(len(wk), bool); new_wave[1:] = wk[1:] != wk[:-1]
            new_bin = new_wave.copy(); new_bin[1:] |= dk[1:] != dk[:-1]
            wid = np.cumsum(new_wave) - 1
            rows_in_wave = np.bincount(wid); bins_in_wave = np.bincount(wid, new_bin)
            t.one_bin_waves += int(((rows_in_wave >= 2) & (bins_in_wave == 1)).sum())
            t.max_bins_in_wave = max(t.max_bins_in_wave, int(bins_in_wave.max()))
            alone = rows_in_wave[wid] == 1
            t.lane0_alone += int((alone & (ln == 0)).sum()); t.last_lane_alone += int((alone & (ln == g.wave - 1)).sum())
            gb = np.unique(np.stack([d[ok], group[ok]]), axis=1)               # distinct (bin, workgroup)
            t.shared_bins += int((np.bincount(gb[0]) >= 2).sum())
        # k_quant_find
        bins = []
        for i in range(nq):
            h = hist[slot_of[i]]
            c = np.cumsum(h)
            target = rank[i] - below[i]
            b = int(np.searchsorted(c, target, "right"))
            assert b < g.bins, "a rank fell out of its histogram"
            prefix[i] = (prefix[i] << w) | b; below[i] += int(c[b] - h[b]); n_equal[i] = int(h[b])
            bins.append(b)
        live = []
        for i in range(nq):
            if prefix[i] not in live:
                live.append(prefix[i])
            slot_of[i] = live.index(prefix[i])
        t.passes += 1; t.widths.append(w); t.bins.append(bins)
        sh = nsh
    for i in range(nq):
        v = ((kmin + prefix[i]) ^ BIAS)
        out[i] = (v - (1 << 64) if v >= BIAS else v, rank[i], below[i], n_equal[i])
    return out, t


# ---- helpers of the GPU tests ----
def raw(x, base, clauses, measure, qs, with_res=True):
    """the records and the result record of bmx_where_quantiles (Engine) / bmx_comm_where_quantiles (Comm) as the library wrote them, into buffers that held a
    pattern; nothing is written behind the last record"""
    out = np.full(32 * (len(qs) + 1), FILL, np.uint8).view(bmx.QUANT_REC_DTYPE)
    res = np.full(32, FILL, np.uint8).view(bmx.QUANT_RES_DTYPE)
    args = (*bmx._where_args(base, clauses), *bmx._quant_tail(measure, qs), bmx._ptr(out), bmx._ptr(res) if with_res else None)
    x._chk(x.L.bmx_where_quantiles(x.h, *args, bmx.MEM_HOST) if isinstance(x, bmx.Engine) else x.L.bmx_comm_where_quantiles(x.h, *args))
    assert (out[len(qs):].view(np.uint8) == FILL).all(), "nothing is written behind the last record"
    if not with_res:
        assert (res.view(np.uint8) == FILL).all()
    return out[:len(qs)].copy(), res[0].copy()


def same(got, want):
    """every byte of the records and of the result record; -> None or what differs"""
    if got[0].tobytes() != want[0].tobytes():
        return ("records", got[0], want[0])
    if got[1].tobytes() != want[1].tobytes():
        return ("res", got[1], want[1])
    return None


# ---- the cases of the GPU kernel-edge tests: values and mask bits BY INDEX POSITION, the quantiles, and the tags the stand-in's Trace must show ----
def _q(r, n):
    """the quantile whose rank in a sample of n is exactly r (n - 1 <= QUANT_MAX_DEN)"""
    assert 0 <= r < n and n - 1 <= bmx.QUANT_MAX_DEN
    return (r, n - 1) if n > 1 else (0, 1)


def _must(pred):
    def check(t):
        assert pred(t), vars(t)
    return check


def edge_cases(E, max_bits, geom=None):
    """-> a list of (name, vals, bits, qs, check): vals int64 and bits bool per position, check(trace) asserts the path. E = values per 16-byte load (4: the
    4-byte column, 2: the 8-byte column or the value scratch); max_bits: 32 for the 4-byte column (its values stay inside int32), 54 otherwise."""
    g = geom or Geom(E)
    rng = np.random.default_rng(1000 + E + max_bits)
    DB, B = g.digit_bits, g.bins
    rnd = g.round_units() * E                                # rows of one workgroup's round
    cases = []

    def add(name, vals, bits, qs, check):
        vals = np.asarray(vals, np.int64); bits = np.asarray(bits, bool)
        assert len(vals) == len(bits) and len(vals) <= 200000 and 1 <= len(qs) <= bmx.QUANT_MAX
        cases.append((name, vals, bits, qs, check))

    # 1. value spans: every digit count, a short and a full last digit
    for span in [s for s in (0, 1, DB, DB + 1, 2 * DB, 2 * DB + 1, 32, 3 * DB, 4 * DB, 4 * DB + 1, 54) if s <= max_bits]:
        n = 3000 + span
        lo = -(1 << (span - 1)) + 1 if span else -5          # straddles zero
        top = (1 << span) - 1 if span < 54 else (1 << 54) - 2          # the whole domain: -(2^53 - 1) .. 2^53 - 1
        lo = lo if span < 54 else -((1 << 53) - 1)
        if span == 32:
            lo, top = -(1 << 31) + 1, (1 << 32) - 2          # INT32_MIN + 1 .. INT32_MAX
        v = lo + (rng.integers(0, top + 1, n, dtype=np.uint64).astype(np.int64) if top else np.zeros(n, np.int64))
        bits = rng.random(n) < 0.7
        on = np.nonzero(bits)[0]
        v[on[0]] = lo; v[on[-1]] = lo + top                  # both ends are in the sample
        want_bits = _bits(top)
        passes, last = (want_bits + DB - 1) // DB, (want_bits - 1) % DB + 1 if want_bits else 0

        def check(t, passes=passes, last=last):
            assert t.passes == passes and (not passes or t.widths[-1] == last), (t.passes, t.widths, passes, last)
        add("span %d" % span, v, bits, [(0, 1), (1, 2), (1, 1), (1, 4), (99, 100)], check)

    # 2. the rank in bin 0, in the last bin, and on either side of a bin-search thread's share
    n = B + 500
    v = np.zeros(n, np.int64); bits = np.zeros(n, bool)
    at = rng.permutation(n)[:B]
    v[at] = np.arange(B); bits[at] = True; v[~bits] = rng.integers(0, B, n - B)          # one of each value in the sample: rank r lands in bin r
    sh = g.share
    want = [0, B - 1, sh - 1, sh, 2 * sh - 1, 2 * sh, B - sh - 1, B - sh]
    add("bin edges", v, bits, [_q(r, B) for r in want], _must(lambda t, want=want: t.bins == [want]))

    # 3. eight ranks in one bin through the last pass; eight ranks in eight bins after the first digit; two ranks that part only in the last digit
    n = 9000
    span = 2 * DB + 1
    v = rng.integers(0, 1 << span, n); bits = np.ones(n, bool)
    tie = (1 << (span - 1)) + 5
    v[2000:7000] = tie                                        # 5000 of one value: ranks 2000 .. 6999 or so
    v[0] = 0; v[1] = (1 << span) - 1
    srt = np.sort(v); first = int(np.searchsorted(srt, tie)); cnt = int((v == tie).sum())
    add("one bin throughout", v, bits, [_q(first + k * (cnt // 8), n) for k in range(8)],
        _must(lambda t: t.np == [1, 1, 1] and t.one_bin_waves > 0))
    add("eight bins", v, bits, [_q(int(np.searchsorted(srt, (k << (span - 3)) + 1)) if k else 0, n) for k in (0, 7, 3, 1, 6, 2, 5, 4)],
        _must(lambda t: t.np == [1, 8, 8] and len(set(t.bins[0])) == 8))
    v2 = v.copy(); v2[2000:4500] = tie - 1                    # tie - 1 and tie differ in the last bit only (tie is odd)
    assert tie % 2 == 1
    srt2 = np.sort(v2); f2 = int(np.searchsorted(srt2, tie - 1))
    add("parting in the last digit", v2, bits, [_q(f2 + 10, n), _q(f2 + 2500 + 10, n)],
        _must(lambda t: t.np == [1, 1, 1] and t.bins[-1][0] != t.bins[-1][1] and t.bins[0][0] == t.bins[0][1]))
    # ranks on both sides of a tie group's edges
    add("tie edges", v, bits, [_q(r, n) for r in (first - 1, first, first + cnt - 1, first + cnt)], _must(lambda t: t.passes == 3))

    # 4. a wave in one bin (all equal but two), in 64 bins, lane 0 or the last lane alone
    n = 64 * E * 40
    pos = np.arange(n)
    v = np.full(n, 7, np.int64); v[0] = 0; v[n - 1] = B - 1
    add("a wave in one bin", v, np.ones(n, bool), [(1, 2), (0, 1), (1, 1)], _must(lambda t: t.one_bin_waves >= 30))
    v = (pos // E) % B
    add("a wave in 64 bins", v, np.ones(n, bool), [(1, 2), (1, 3)], _must(lambda t: t.max_bins_in_wave == g.wave))
    bits = (pos % (g.wave * E) == 0) | (pos % (g.wave * E) == g.wave * E - 1)
    v = rng.integers(-500, 500, n)
    add("lane 0 or the last lane alone", v, bits, [(1, 2), (0, 1), (1, 1)],
        _must(lambda t: t.lane0_alone >= 40 and t.last_lane_alone >= 40))

    # 5. index sizes around the unit, the wave, a workgroup's round, the step to a second workgroup and the grid's first stride; a ragged last unit whose last
    #    row is the maximum
    for n in sorted({1, E - 1, E, E + 1, 31, 32, 33, 64 * E - 1, 64 * E, 64 * E + 1, rnd - 1, rnd, rnd + 1, 4 * rnd - 1, 4 * rnd, 4 * rnd + 1, 4 * rnd + 2 * rnd + E + 1} - {0}):
        v = (np.arange(n) * 7) % 1000 - 300
        v[n - 1] = 5000                                       # the last row, in a ragged unit when n % E != 0, holds the maximum
        bits = np.ones(n, bool) if n < 40 else (np.arange(n) % 3 != 1)
        bits[n - 1] = True
        groups = g.groups(n)

        def check(t, groups=groups, n=n):
            assert t.groups == groups and (groups == 1 or t.shared_bins > 0), (n, t.groups, groups, t.shared_bins)
        add("size %d" % n, v, bits, [(1, 1), (1, 2), (0, 1)], check)
    return cases
