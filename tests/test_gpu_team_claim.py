"""GPU: the probe kernel's two claim modes (csrc/merge_kernels.h: team_claim, decide_and_claim, resolve_one; BMX_CLAIM_MODE=store|team) at the edges of the team
geometry — a wave claims in four rounds of sixteen deltas, the team of delta 16p + i being lanes 4i, 4i+1, 4i+2 of round p's swap instruction.

Built on the harness of tests/test_gpu_merge_kernel_edges.py (Laid.merge: winners, n_applied, n_rows and the n_conflicts bounds of that module's docstring — they
hold in either mode: a claimer is never below the pre-batch row) and tests/test_gpu_lookup_edges.py: 4096-slot tables, batches built delta by delta, expectations
from oracle.oracle.Oracle, everything exact. Every case runs in both claim modes (the environment is set before the Engine is made), over the entry variants
host, dev and recs, both insert rules and BMX_K1_WAVES 8 and 5.

  geometry      n deltas on n resident keys, n around the round, wave and block borders: all winning; every second one losing (teams with masked-off neighbours,
                whole quads off); every third one equal to its row (head claimed, row untouched)
  one resident  one resident key with 2..6 deltas in one round, on both sides of a round border, of a wave border and in different 256-blocks; ascending,
                descending, the maximum in the middle, all equal (the smallest index wins), all below the row, exactly one above it
  one absent    the same positions on an absent key: the creator's path is the store path, followers claim the head only, the creating delta is not the winner
  back to back  two batches on the same 64 resident keys enqueued without a host read in between: the second batch's deltas lie between the pre-batch values and
                the first batch's winners and must lose — the swapped values reached memory and no stale line was read behind the kernel boundary
  index         the single-key cases under a maintained index on the field: a scan afterwards names the oracle's rows (the change log through slot_of)
  fuzz          three batches of 20,000 deltas over 2,000 keys, half of them resident, on a 16,384-row engine"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
from bmx import synth
from oracle.oracle import Oracle, rows_digest
import test_gpu_sync_kernel_edges as edges
import test_gpu_merge_kernel_edges as mk

REF, DELTA = mk.REF, mk.DELTA
F0, NSLOTS = mk.F0, mk.NSLOTS
CLAIMS = ("team", "store")
SIZES = (1, 3, 15, 16, 17, 63, 64, 65, 129)
MEMBERS = (2, 3, 4, 5, 6)


def combos():
    for claim in CLAIMS:
        for variant in mk.VARIANTS:
            for rule in (REF, DELTA):
                for waves in (8, 5):
                    yield pytest.param(claim, variant, rule, waves, id="%s-%s-%s-w%d" % (claim, variant, "delta" if rule else "ref", waves))


def engine(monkeypatch, claim, waves=8, capacity=None, **kw):
    """an Engine in claim mode `claim` (None: the default) on the smallest table"""
    if claim is None:
        monkeypatch.delenv("BMX_CLAIM_MODE", raising=False)
    else:
        monkeypatch.setenv("BMX_CLAIM_MODE", claim)
    e = bmx.Engine(capacity or edges.capacity_for(NSLOTS), load_pct=90, **({"flags": bmx.CTX_FIXED_CAPACITY} if capacity is None else {}), **kw)
    assert e.claim_mode() == (claim or "team")
    e.set_probe_waves(waves)
    return e


def keys(a, n):
    return synth.splitmix64_np(np.arange(a, a + n, dtype=np.uint64))


def load(t, id, ts, val):
    n = len(id)
    rows = (id, np.full(n, F0, np.uint32), np.asarray(ts, np.int64), np.asarray(val, np.int64))
    t.e.load_rows(*rows); t.o.load_rows(*rows)


# ---- team geometry ----

@pytest.mark.parametrize("claim,variant,rule,waves", list(combos()))
def test_team_geometry_on_resident_keys(monkeypatch, claim, variant, rule, waves):
    with engine(monkeypatch, claim, waves) as e:
        t = mk.Laid(e, [])
        id = keys(1, max(SIZES))
        load(t, id, np.full(len(id), 10), np.arange(len(id)) % 7 - 3)
        bno = 0
        for pattern in ("all win", "every second loses", "every third equals its row"):
            for n in SIZES:
                bno += 1
                j = np.arange(n)
                ts = np.full(n, 10 + 10 * bno, np.int64); val = (j * 5 + bno) % 11 - 5
                if pattern == "every second loses":
                    ts[1::2] = 0
                elif pattern == "every third equals its row":
                    cur = [t.o.get_row(int(k), F0) for k in id[:n][2::3]]
                    ts[2::3] = [c[0] for c in cur]; val[2::3] = [c[1] for c in cur]
                a = t.merge((id[:n], np.full(n, F0, np.uint32), ts, val.astype(np.int64)), variant, rule, 0, (pattern, n))
                want = {"all win": n, "every second loses": (n + 1) // 2, "every third equals its row": n - n // 3}[pattern]
                assert len(a) == want, (pattern, n, len(a))
                t.check_state((pattern, n))
        assert e.info().n_slots == NSLOTS


# ---- one key, several deltas ----

def positions(k):
    """name -> (indices of the k members, batch size)"""
    return {"one round": ([1, 3, 4, 7, 9, 14][:k], 65), "rounds 0 and 1": (sorted([15, 16, 14, 17, 13, 18][:k]), 65),
            "lanes 63 and 64": (sorted([63, 64, 62, 65, 61, 66][:k]), 130), "256-blocks": ([b * 256 + (b * 37 + 5) % 256 for b in range(k)], 256 * k + 1)}


def resident_orders(k):
    """(name, the members' (ts, val) in index order) against a row that holds (60, 0)"""
    mid = k // 2
    low = [(1, 50 + j) for j in range(k)]
    return [("ascending", [(100 + j, j) for j in range(k)]), ("descending", [(100 + k - j, j) for j in range(k)]),
            ("the maximum in the middle", [(100 + (k - abs(j - mid)), j) for j in range(k)]), ("all equal", [(100, 7)] * k),
            ("all below the row", low), ("exactly one above the row", low[:mid] + [(100, 7)] + low[mid + 1:])]


def absent_orders(k):
    return [(s, v) for s, start, v, _ in mk.scenarios(k) if start is None]


def single_key_batches(t, variant, rule, orders, start, tag, ready=None, after=None):
    """every (members, positions, order) as one batch on a key of its own among unique filler deltas; the rows are all loaded first, then ready() runs"""
    n_fill = 256 * max(MEMBERS) + 1
    fill = keys(1, n_fill)
    load(t, fill, np.full(n_fill, 10), np.zeros(n_fill))
    cases = [(k, pname, pos, n, oname, values) for k in MEMBERS for pname, (pos, n) in positions(k).items() for oname, values in orders(k)]
    own = keys(1_000_000, len(cases))
    if start:
        load(t, own, np.full(len(own), start[0]), np.full(len(own), start[1]))
    if ready:
        ready()
    for bno, (k, pname, pos, n, oname, values) in enumerate(cases, 1):
        what = (tag, k, pname, oname)
        key = int(own[bno - 1])
        a = t.merge(mk.list_batch(pos, n, fill, bno, key, values), variant, rule, 0, what)
        won = np.isin(np.asarray(pos, np.uint32), a & np.uint32(bmx.APPLIED_INDEX))
        if start and max(values) <= start:
            assert not won.any(), (what, "applied names a key nobody won")
        else:
            assert won.sum() == 1, (what, "one member wins")
            assert won[0] or oname != "all equal", (what, "the smallest index wins")
        assert t.e.get_row(key, F0) == t.o.get_row(key, F0), what
        if after:
            after(what)
    assert rows_digest(*t.e.dump_rows()) == t.o.digest()


@pytest.mark.parametrize("claim,variant,rule,waves", list(combos()))
def test_one_resident_key_with_several_deltas(monkeypatch, claim, variant, rule, waves):
    with engine(monkeypatch, claim, waves) as e:
        single_key_batches(mk.Laid(e, []), variant, rule, resident_orders, (60, 0), "resident")
        assert e.info().n_slots == NSLOTS


@pytest.mark.parametrize("claim,variant,rule,waves", list(combos()))
def test_one_absent_key_with_several_deltas(monkeypatch, claim, variant, rule, waves):
    assert any("beats the creating delta" in s for s, _ in absent_orders(3))
    with engine(monkeypatch, claim, waves) as e:
        single_key_batches(mk.Laid(e, []), variant, rule, absent_orders, None, "absent")
        assert e.info().n_slots == NSLOTS


# ---- two batches back to back ----

@pytest.mark.parametrize("claim", CLAIMS)
@pytest.mark.parametrize("rule", [REF, DELTA])
@pytest.mark.parametrize("waves", [8, 5])
def test_second_batch_sees_what_the_first_one_swapped(monkeypatch, claim, rule, waves):
    import torch
    dev = torch.device(mk.DEVICE)
    id = keys(1, 64)
    j = np.arange(64, dtype=np.int64)
    # batch 1: every key twice — a winner (100, j) and, a wave later, a second claimer (90, j) that beat the row as well; batch 2: (50, j), above the pre-batch (10, 0)
    b1 = (np.concatenate([id, id]), np.full(128, F0, np.uint32), np.concatenate([np.full(64, 100), np.full(64, 90)]).astype(np.int64), np.concatenate([j, j]))
    b2 = (id, np.full(64, F0, np.uint32), np.full(64, 50, np.int64), j)
    with engine(monkeypatch, claim, waves) as e:
        t = mk.Laid(e, [])
        load(t, id, np.full(64, 10), np.zeros(64))
        outs = []
        for b in (b1, b2):
            n = len(b[0])
            d = (torch.from_numpy(b[0].view(np.int64)).to(dev), torch.from_numpy(b[1].view(np.int32)).to(dev), torch.from_numpy(b[2]).to(dev), torch.from_numpy(b[3]).to(dev))
            applied = torch.zeros(n, dtype=torch.int32, device=dev); n_applied = torch.zeros(1, dtype=torch.int64, device=dev); stats = torch.zeros(4, dtype=torch.int64, device=dev)
            e.merge_batch_dev(n, *d, rule, applied=applied, n_applied=n_applied, stats=stats)         # enqueued only: nothing is read before both batches are in
            outs.append((d, applied, n_applied, stats))
        e.sync()
        for b, (_, applied, n_applied, stats) in zip((b1, b2), outs):
            _, want = t.o.merge_batch(*b, rule)
            na = int(n_applied.cpu()[0])
            mk._same(applied.cpu().numpy().view(np.uint32)[:na], want, "applied_idx")
            assert int(stats.cpu()[0]) == len(want)
        assert len(want) == 0, "the second batch loses against what the first one swapped"
        t.check_state("after both batches", list(zip(id.tolist(), [F0] * 64)))


# ---- a maintained index on the field ----

@pytest.mark.parametrize("claim", CLAIMS)
@pytest.mark.parametrize("start", [(60, 0), None], ids=["resident", "absent"])
def test_single_key_cases_under_a_maintained_index(monkeypatch, claim, start):
    lo, hi = -(1 << 40), 1 << 40
    with engine(monkeypatch, claim) as e:
        t = mk.Laid(e, [])
        full = []

        def scan(what):
            mk._same(np.sort(e.scan_range(F0, lo, hi)), np.sort(t.o.scan_range(F0, lo, hi)), (what, "scan_range"))
            mk._same(np.sort(e.scan_range(F0, 0, 7)), np.sort(t.o.scan_range(F0, 0, 7)), (what, "scan_range 0..7"))

        def build():
            e.index_build(F0); scan("fresh"); full.append(e.index_refresh_counts()[0])
        single_key_batches(t, "host", REF, resident_orders if start else absent_orders, start, "indexed", ready=build, after=scan)
        assert e.index_refresh_counts()[0] == full[0], "the index followed the change log: it was not built from the table again"


# ---- fuzz ----

@pytest.mark.parametrize("claim", CLAIMS)
@pytest.mark.parametrize("rule", [REF, DELTA])
def test_seeded_fuzz(monkeypatch, claim, rule):
    rng = np.random.default_rng(606)
    pool = keys(9_000_000, 2000)
    with engine(monkeypatch, claim, capacity=16384) as e:
        t = mk.Laid(e, [])
        load(t, pool[:1000], rng.integers(1, 20, 1000), rng.integers(-9, 10, 1000))
        for bno in range(3):
            n = 20000
            b = (pool[rng.integers(0, 2000, n)], np.full(n, F0, np.uint32), rng.integers(0, 12 + 6 * bno, n).astype(np.int64), rng.integers(-9, 10, n).astype(np.int64))
            _, want = t.o.merge_batch(*b, rule)
            a, _, st = e.merge_batch(*b, rule)
            mk._same(a, want, ("fuzz", bno, "applied_idx"))
            assert (st.n_applied, st.n_rows) == (len(want), len(t.o)), ("fuzz", bno)
            t.check_state(("fuzz", bno))


# ---- the self-check and the mode switch ----

def test_selfcheck_claim_sees_no_torn_pair_and_its_control_does():
    reads, torn, control = bmx.selfcheck_claim(0)
    assert reads > 10**7 and torn == 0 and control > 0, (reads, torn, control)


def test_claim_mode_default_and_override(monkeypatch):
    with engine(monkeypatch, None) as e:
        assert e.claim_mode() == "team"
    with engine(monkeypatch, "store") as e:
        assert e.claim_mode() == "store"
    with engine(monkeypatch, "team") as e:
        assert e.claim_mode() == "team"
