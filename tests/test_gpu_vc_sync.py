"""GPU: replica reconciliation of the vector-clock table (include/bmx_vc_sync.h) against the CPU model — OracleVC fed the same loads and merges, its rows read
back with dump_rows + get_rows. Every comparison is exact equality: the per-bucket digests with a numpy group-by, the version vector, the filtered exports
record for record, the record merge with the oracle's merge_batch over the records' columns and with merge_batch on a twin engine, and the pull / reconcile
drivers of bmx/replica.py with the model pulled the same way."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
from bmx import replica, synth
from oracle.oracle import OracleVC
import vc_sync_model as M

TABLES = ["K1", "K3", "K8", "grown", "empty"]


def _batch(rng, n, nkeys, K, cmax, full):
    ids = M.key_ids(rng.integers(0, nkeys, n))
    fields = np.array([synth.field_hash(int(x)) for x in rng.integers(0, 2, n)], np.uint32)
    clocks = rng.integers(0, cmax + 1, (n, K)).astype(np.uint32)
    val = rng.integers(-1000, 1001, n).astype(np.int64)
    return ids, fields, clocks, val, M.rand_keysets(rng, clocks, K, full=full)


def _build(K, local, capacity, seed, rows=2400):
    """about 5000 rows: a keyed load_rows, then two merges with key sets that also create rows (sparse first writes)"""
    rng = np.random.default_rng(seed)
    e = bmx.EngineVC(capacity, K, local); o = OracleVC(K, local)
    b = _batch(rng, 3 * rows // 2, rows, K, 5, 0.5)                  # (ids x 2 fields: ~2400 x 2 keys, most of them hit)
    e.load_rows(b[0], b[1], b[2], b[3], keysets=b[4]); o.load_rows(b[0], b[1], b[2], b[3], keysets=b[4])
    for r in range(2):
        b = _batch(rng, 3000, rows + 600 * (r + 1), K, 6 + r, 0.3)
        f1, u1 = e.merge_batch(b[0], b[1], b[2], b[3], keysets=b[4]); f2, u2 = o.merge_batch(b[0], b[1], b[2], b[3], keysets=b[4])
        assert np.array_equal(f1, f2) and np.array_equal(u1, u2)
    return e, o


class T:
    def __init__(self, name):
        self.name = name
        if name == "empty":
            self.K, self.local = 3, 1
            self.e, self.o = bmx.EngineVC(4096, 3, 1), OracleVC(3, 1)
        elif name == "grown":
            self.K, self.local = 3, 2
            self.e, self.o = _build(3, 2, 1024, 77)
            assert self.e.info().n_slots > 4096, "the load grew the table"
        else:
            self.K = int(name[1:]); self.local = self.K - 1
            self.e, self.o = _build(self.K, self.local, 20000, 40 + self.K)
        self.rows = M.model_rows(self.o)                              # sorted by (id, field); never changed
        if name not in ("empty",):
            assert 3500 <= len(self.rows) <= 6500 and (self.rows["state"] == bmx.VC_SPARSE).any() and (self.rows["state"] == bmx.VC_DENSE).any()


@pytest.fixture(scope="module")
def tables():
    made = {}

    def get(name):
        if name not in made:
            made[name] = T(name)
        return made[name]
    yield get
    for t in made.values():
        t.e.close()


@pytest.mark.parametrize("name", TABLES)
def test_info_digest_and_frontier(tables, name):
    t = tables(name)
    i = t.e.info()
    assert (i.n_rows, i.k_writers, i.local_writer, i.table_bytes, i.device, i.reserved) == (len(t.rows), t.K, t.local, 64 * i.n_slots, 0, 0)
    assert i.n_slots % 2 == 0 and i.n_slots >= 2 * i.n_rows + 2 and (name != "grown" or i.capacity_rows == i.n_slots // 2)
    assert i.n_rows == t.e.row_count() == len(t.o)
    M.check_digest(t.e, t.rows)
    fr = M.check_frontier(t.e, t.rows)
    assert (fr[t.K:] == 0).all()
    if name == "empty":
        assert not fr.any()


@pytest.mark.parametrize("name", TABLES)
def test_exports(tables, name):
    """everything, bucket bits (host and device resident), frontiers, both; the caps into pageable, page-locked and device memory"""
    t = tables(name)
    dump = t.e.dump_rows()
    assert (dump["aux"] == 0).all()
    M.same_recs(M.by_key(dump), t.rows, "export of everything == the model's rows")
    M.check_export(t.e, t.rows, t.K, M.np_frontier(t.rows), ordered=False, caps=True)


def test_equal_rows_in_tables_of_different_width_give_equal_digests():
    rng = np.random.default_rng(5)
    b = _batch(rng, 3000, 2500, 3, 7, 0.4)
    e3, e8 = bmx.EngineVC(8000, 3, 1), bmx.EngineVC(8000, 8, 1)
    c8 = np.zeros((len(b[0]), 8), np.uint32); c8[:, :3] = b[2]
    e3.load_rows(b[0], b[1], b[2], b[3], keysets=b[4]); e8.load_rows(b[0], b[1], c8, b[3], keysets=b[4])
    m = _batch(rng, 1000, 3000, 3, 9, 0.4)                         # a merge on top: sparse rows of the same local writer in both
    m8 = np.zeros((len(m[0]), 8), np.uint32); m8[:, :3] = m[2]
    f3, _ = e3.merge_batch(m[0], m[1], m[2], m[3], keysets=m[4]); f8, _ = e8.merge_batch(m[0], m[1], m8, m[3], keysets=m[4])
    assert np.array_equal(f3, f8)
    for L in (0, 10, 16):
        a, b_ = e3.digest(L), e8.digest(L)
        assert np.array_equal(a[0], b_[0]) and np.array_equal(a[1], b_[1]) and a[1].sum() == e3.row_count() > 2000
    assert np.array_equal(e3.frontier(), e8.frontier())
    M.same_recs(M.by_key(e3.dump_rows()), M.by_key(e8.dump_rows()), "the same records")
    e3.close(); e8.close()


def _second(K, local, seed):
    """a second table with content of its own that overlaps the first's keys"""
    rng = np.random.default_rng(seed)
    b = _batch(rng, 2500, 3000, K, 6, 0.5)
    out = []
    for _ in range(3):
        e = bmx.EngineVC(4096, K, local)
        e.load_rows(b[0], b[1], b[2], b[3], keysets=b[4])
        out.append(e)
    o = OracleVC(K, local); o.load_rows(b[0], b[1], b[2], b[3], keysets=b[4])
    return out, o


@pytest.mark.parametrize("name", ["K1", "K3", "K8"])
def test_merge_records_equals_merge_batch(tables, name):
    t = tables(name)
    K = t.K
    recs = t.e.dump_rows()                                           # slot order: the order the records travel in
    (e_host, e_dev, e_twin), o = _second(K, 0, 900 + K)
    want_f, want_u = M.merge_recs(o, recs)
    f, u = e_host.merge_records(recs)
    assert np.array_equal(f, want_f) and np.array_equal(u, want_u), "host records == the oracle's merge_batch"
    tf, tu = e_twin.merge_batch(recs["id"], recs["field"], np.ascontiguousarray(recs["clock"][:, :K]), recs["val"], keysets=recs["keyset"])
    assert np.array_equal(f, tf) and np.array_equal(u, tu), "== merge_batch on a twin engine"
    # device to device: the records exported into device memory, merged from there
    n = len(recs)
    d_recs = torch.empty(8 * n, dtype=torch.int64, device=M.DEVICE); d_n = torch.zeros(1, dtype=torch.int64, device=M.DEVICE)
    d_upd = torch.full((n + 8,), -1, dtype=torch.int32, device=M.DEVICE); d_nu = torch.full((1,), -1, dtype=torch.int64, device=M.DEVICE); d_fl = torch.full((n + 8,), 0x55, dtype=torch.uint8, device=M.DEVICE)
    torch.cuda.synchronize()
    t.e.export_rows_dev(d_recs, n, d_n); t.e.sync()
    assert int(d_n.item()) == n
    e_dev.merge_records_dev(n, d_recs, updated=d_upd, n_updated=d_nu, flags=d_fl); e_dev.sync()
    nu = int(d_nu.item())
    assert nu == len(want_u) and np.array_equal(d_upd.cpu().numpy()[:nu].view(np.uint32), want_u) and (d_upd.cpu().numpy()[n:] == -1).all()
    assert np.array_equal(d_fl.cpu().numpy()[:n], want_f) and (d_fl.cpu().numpy()[n:] == 0x55).all()
    want_rows = M.model_rows(o)
    for e in (e_host, e_dev, e_twin):
        assert e.row_count() == len(o)
        M.same_recs(M.by_key(e.dump_rows()), want_rows, "rows after the merge == the model's")
    # a table's own export changes nothing in it
    for e in (e_host, e_dev):
        own = e.dump_rows()
        f, u = e.merge_records(own)
        assert len(u) == 0 and not (f & (bmx.FLAG_INCOMING | bmx.FLAG_CONCURRENT)).any()
        M.same_recs(M.by_key(e.dump_rows()), want_rows, "unchanged by its own export")
    assert e_host.merge_records(recs[:0])[1].tolist() == []
    d_nu.fill_(-1); torch.cuda.synchronize()
    e_dev.merge_records_dev(0, None, n_updated=d_nu); e_dev.sync()
    assert int(d_nu.item()) == 0
    for e in (e_host, e_dev, e_twin):
        e.close()


def test_a_record_with_a_component_beyond_k_is_refused():
    e = bmx.EngineVC(4096, 3, 0)
    r = M.recs_of(M.key_ids([1, 2, 3]), [synth.field_hash(0)] * 3, np.array([[1, 0, 2], [0, 1, 0], [3, 3, 3]], np.uint32), [5, 6, 7], [bmx.keyset([0, 2]), bmx.keyset([1]), bmx.keyset([0, 1, 2])], [1, 1, 1])
    f, u = e.merge_records(r)
    assert u.tolist() == [0, 1, 2] and e.row_count() == 3
    bad = r.copy(); bad["clock"][1, 3] = 1
    with pytest.raises(bmx.BmxError) as ei:
        e.merge_records(bad)
    assert ei.value.code == bmx.ERR_RANGE
    d = torch.from_numpy(bad.view(np.int64).copy()).to(M.DEVICE)
    torch.cuda.synchronize()
    e.merge_records_dev(3, d)                                       # device mode: the error is sticky
    with pytest.raises(bmx.BmxError) as ei:
        e.sync()
    assert ei.value.code == bmx.ERR_RANGE
    e.close()


# ---- the drivers ----

def _pull_model(dst, src):
    M.merge_recs(dst, M.model_rows(src))


def _equal_to_model(e, o, what):
    M.same_recs(M.by_key(e.dump_rows()), M.model_rows(o), what)


@pytest.mark.parametrize("seed", [3, 17])
def test_pull_and_reconcile(seed):
    """the generator of test_vc_sync_cabi.py's convergence premise: after every pull the device rows equal the model's, the loop ends within 3 rounds"""
    ea, eb = bmx.EngineVC(4096, 3, 0), bmx.EngineVC(4096, 3, 1)
    oa, ob = OracleVC(3, 0), OracleVC(3, 1)
    for e, o, who in ((ea, oa, 0), (eb, ob, 1)):
        for id, field, clocks, val, ks in M.replica_merges(seed, who):
            f1, u1 = e.merge_batch(id, field, clocks, val, keysets=ks); f2, u2 = o.merge_batch(id, field, clocks, val, keysets=ks)
            assert np.array_equal(f1, f2) and np.array_equal(u1, u2)
    _equal_to_model(ea, oa, "a before"); _equal_to_model(eb, ob, "b before")
    # pulls under a frontier first, into a third table that holds what a holds: a's own frontier (it dominates every clock of these inputs: nothing is
    # shipped), and that frontier lowered by one in b's component
    L = 6
    src, mine = M.model_rows(ob), M.model_rows(oa)
    da, db = M.np_digest(mine, L), M.np_digest(src, L)
    differing = np.flatnonzero((da[0] != db[0]) | (da[1] != db[1]))
    in_diff = np.isin(bmx.key_bucket(src["id"], src["field"], L), differing)
    fr = ea.frontier()
    M.same(fr, M.np_frontier(mine), "a's frontier")
    low = fr.copy(); low[1] -= 1
    for f, some in ((fr, False), (low, True)):
        ahead = M.beyond(src, f, 3)
        assert (in_diff & ~ahead).any(), "some rows of the differing buckets are dominated by the frontier"
        assert (in_diff & ahead).any() == some
        ef = bmx.EngineVC(4096, 3, 0)
        for id, field, clocks, val, ks in M.replica_merges(seed, 0):
            ef.merge_batch(id, field, clocks, val, keysets=ks)
        r = replica.pull_vc(ef, eb, L=L, frontier=f)
        assert r["buckets_differing"] == len(differing) > 0 and r["rows_shipped"] == int((in_diff & ahead).sum()), "no row the frontier dominates is shipped"
        ef.close()
    # the reconcile loop, step by step against the model
    log = []
    for rnd in range(3):
        r1 = replica.pull_vc(ea, eb, L=L); _pull_model(oa, ob)
        _equal_to_model(ea, oa, ("a after pull", rnd))
        r2 = replica.pull_vc(eb, ea, L=L); _pull_model(ob, oa)
        _equal_to_model(eb, ob, ("b after pull", rnd))
        log.append((r1, r2))
        if r1["buckets_differing"] == 0 and r2["buckets_differing"] == 0:
            break
    assert log[-1][0]["buckets_differing"] == 0 and log[-1][1]["buckets_differing"] == 0, ("ends within 3 rounds", log)
    assert log[0][0]["rows_shipped"] > 0 and log[0][0]["rows_updated"] > 0
    for Lq in (0, 10):
        da, db = ea.digest(Lq), eb.digest(Lq)
        assert np.array_equal(da[0], db[0]) and np.array_equal(da[1], db[1])
    M.same_recs(M.by_key(ea.dump_rows()), M.by_key(eb.dump_rows()), "equal tables")
    # between equal tables nothing is shipped, and reconcile_vc says so in one round
    assert replica.pull_vc(ea, eb) == {"buckets_differing": 0, "rows_shipped": 0, "rows_updated": 0}
    rr = replica.reconcile_vc(ea, eb, L=L)
    assert len(rr) == 1 and rr[0][0]["buckets_differing"] == 0 and rr[0][1]["buckets_differing"] == 0
    ea.close(); eb.close()


def test_reconcile_vc_runs_the_loop_itself():
    ea, eb = bmx.EngineVC(4096, 3, 0), bmx.EngineVC(4096, 3, 1)
    for e, who in ((ea, 0), (eb, 1)):
        for id, field, clocks, val, ks in M.replica_merges(29, who):
            e.merge_batch(id, field, clocks, val, keysets=ks)
    rr = replica.reconcile_vc(ea, eb, L=10, rounds=3)
    assert 2 <= len(rr) <= 3 and rr[-1][0]["buckets_differing"] == 0 and rr[-1][1]["buckets_differing"] == 0 and rr[0][0]["buckets_differing"] > 0
    M.same_recs(M.by_key(ea.dump_rows()), M.by_key(eb.dump_rows()), "equal tables")
    ea.close(); eb.close()
