"""GPU: replica reconciliation (include/bmx.h "replica reconciliation"): per-bucket digests, the filtered export as delta records and
bmx.replica on top of them. Expected values come from the oracle or from numpy over inputs the tests make themselves (the bucket function is
bmx.key_bucket, the header's formula in numpy; the row digest is restated below and tied to oracle.rows_digest)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bmx
from bmx import replica, synth
from oracle.oracle import Oracle, INSERT_REFERENCE, rows_digest

DEL = bmx.VAL_DELETED


def _row_digests(id, field, ts, val):
    """per-row form of oracle.rows_digest (four chained splitmix64 over val, ts, field, id)"""
    sm = synth.splitmix64_np
    h = sm(np.asarray(val, np.int64).astype(np.uint64))
    h = sm(h ^ np.asarray(ts, np.int64).astype(np.uint64))
    h = sm(h ^ np.asarray(field, np.uint32).astype(np.uint64))
    return sm(h ^ np.asarray(id, np.uint64))


def _np_digest(id, field, ts, val, L):
    """numpy group-by: (sums, counts) per bucket of a row set"""
    d = _row_digests(id, field, ts, val)
    assert int(d.sum(dtype=np.uint64)) == rows_digest(id, field, ts, val)
    b = bmx.key_bucket(id, field, L).astype(np.int64)
    sums = np.zeros(1 << L, np.uint64); counts = np.zeros(1 << L, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(sums, b, d)
    np.add.at(counts, b, np.uint64(1))
    return sums, counts


def _total(sums):
    return int(np.asarray(sums, np.uint64).sum(dtype=np.uint64))


def _same(dig, want):
    return np.array_equal(dig[0], want[0]) and np.array_equal(dig[1], want[1])


def _tuples(id, field, ts, val):
    """a row set as a sorted structured array (comparison as a set of 4-tuples)"""
    a = np.zeros(len(id), bmx.DELTA_REC_DTYPE)
    a["id"], a["field"], a["ts"], a["val"] = id, field, ts, val
    return np.sort(a, order=["id", "field", "ts", "val"])


def _rec_tuples(recs):
    assert not recs["aux"].any()
    return _tuples(recs["id"], recs["field"], recs["ts"], recs["val"])


def _merged_state(R=200_000, D=50_000, seed=31):
    res = synth.big_resident(R, seed=seed)
    bs = [synth.big_deltas(D, R, seed=seed + 1, insert_pct=10, hot_pct=20, hot_keys=50, unique=False, batch=b, drift=40_000) for b in range(3)]
    o = Oracle(); o.load_rows(*res)
    for b in bs:
        o.merge_batch(*b)
    return res, bs, o


def _fill(e, res, bs):
    e.load_rows(*res)
    for b in bs:
        if isinstance(e, bmx.Engine):
            e.merge_batch(*b, want_flags=False)
        else:
            e.merge(*b)


def test_digest_equals_oracle_and_numpy_group_by():
    res, bs, o = _merged_state()
    with bmx.Engine(600_000) as e:
        _fill(e, res, bs)
        dump = e.dump_rows()
        assert rows_digest(*dump) == o.digest()
        for L in (0, 4, 10, 13):                       # 10: the LDS form, 13: the global form
            sums, counts = e.digest(L)
            assert len(sums) == len(counts) == 1 << L
            assert _total(sums) == o.digest() == rows_digest(*dump), L
            assert int(counts.sum()) == len(o) == len(dump[0])
            assert _same((sums, counts), _np_digest(*dump, L)), L
        # a device-memory call gives the same vectors, zeroed by the call itself
        dev = torch.device("cuda", 0)
        ds = torch.full((1024,), 77, dtype=torch.int64, device=dev); dc = torch.full((1024,), 77, dtype=torch.int64, device=dev)
        e.digest_dev(10, ds, dc); e.sync()
        assert _same((ds.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint64)), e.digest(10))
        # bad arguments on a live context
        z = np.zeros(1 << 16, np.uint64)
        assert e.L.bmx_digest(e.h, 17, 0, C.c_void_p(z.ctypes.data), C.c_void_p(z.ctypes.data), bmx.MEM_HOST) == bmx.ERR_INVALID
        assert e.L.bmx_digest(e.h, 10, 0, C.c_void_p(z.ctypes.data), C.c_void_p(z.ctypes.data), 5) == bmx.ERR_INVALID
        assert e.L.bmx_export_rows(e.h, 0, 17, None, 0, None, 0, None, bmx.MEM_HOST) == bmx.ERR_INVALID
        assert e.L.bmx_export_rows(e.h, 0, 10, None, 0, None, 0, None, 5) == bmx.ERR_INVALID
    o.close()


def test_digest_does_not_depend_on_the_table_shape():
    res, bs, o = _merged_state(seed=41)
    want = {}
    with bmx.Engine(600_000, load_pct=35) as e:
        _fill(e, res, bs)
        for L in (4, 10, 13):
            want[L] = e.digest(L)
            assert _total(want[L][0]) == o.digest()
        n = e.row_count()
        e.reserve(4 * n)
        for L in (4, 10, 13):
            assert _same(e.digest(L), want[L]), ("after reserve", L)
    with bmx.Engine(600_000, load_pct=70) as e:
        _fill(e, res, bs)
        for L in (4, 10, 13):
            assert _same(e.digest(L), want[L]), ("load 70", L)
        e.reserve(4 * e.row_count())
        assert _same(e.digest(10), want[10])
    for N in (1, 2, 4, 8):
        with bmx.Comm([0] * N, 600_000 // N + 100_000) as c:
            _fill(c, res, bs)
            for L in (4, 10, 13):
                assert _same(c.digest(L), want[L]), (N, L)
            recs, n = c.export_rows()
            assert n == len(o) and np.array_equal(_rec_tuples(recs), _tuples(*c.dump_rows()))
    o.close()


def test_tombstones_leave_their_buckets_or_change_them():
    res, bs, o = _merged_state(seed=51)
    k = 300
    with bmx.Engine(600_000) as e:
        _fill(e, res, bs)
        id, f, ts, val = e.dump_rows()
        before = {L: e.digest(L) for L in (4, 10, 13)}
        pick = np.random.default_rng(3).choice(len(id), k, replace=False)
        tts = ts[pick] + 5
        e.put_rows(id[pick], f[pick], tts, np.full(k, DEL, np.int64))
        keep = np.ones(len(id), bool); keep[pick] = False
        ts2 = ts.copy(); ts2[pick] = tts
        val2 = val.copy(); val2[pick] = DEL
        for L in (4, 10, 13):
            plain = e.digest(L)
            assert _same(plain, _np_digest(id[keep], f[keep], ts[keep], val[keep], L)), L
            gone = _np_digest(id[pick], f[pick], ts[pick], val[pick], L)          # exactly those rows left: counts - 1, sums - their old digest
            with np.errstate(over="ignore"):
                assert np.array_equal(before[L][0] - gone[0], plain[0]) and np.array_equal(before[L][1] - gone[1], plain[1])
            flagged = e.digest(L, tombstones=True)
            assert not _same(flagged, before[L]) and not _same(flagged, plain)
            assert _same(flagged, _np_digest(id, f, ts2, val2, L)), L
            assert int(flagged[1].sum()) == len(id) and int(plain[1].sum()) == len(id) - k
    o.close()


def test_export_filters_and_capacity():
    res, bs, o = _merged_state(seed=61)
    k = 200
    with bmx.Engine(600_000) as e:
        _fill(e, res, bs)
        id, f, ts, val = e.dump_rows()
        pick = np.random.default_rng(4).choice(len(id), k, replace=False)
        tid, f_t, tts = id[pick], f[pick], ts[pick] + 9
        e.put_rows(tid, f[pick], tts, np.full(k, DEL, np.int64))
        id, f, ts, val = e.dump_rows()
        assert len(id) == len(o) - k
        # everything
        recs, n = e.export_rows()
        assert n == len(id) == len(recs) and np.array_equal(_rec_tuples(recs), _tuples(id, f, ts, val))
        # "in table order" (bmx.h): record for record the order of dump_rows, which walks the same slots
        assert np.array_equal(recs["id"], id) and np.array_equal(recs["field"], f) and np.array_equal(recs["ts"], ts) and np.array_equal(recs["val"], val)
        # since = median clock
        since = int(np.median(ts))
        m = ts >= since
        r2, n2 = e.export_rows(since=since)
        assert n2 == int(m.sum()) and 0 < n2 < n and np.array_equal(_rec_tuples(r2), _tuples(id[m], f[m], ts[m], val[m]))
        # three buckets of 1024
        want_b = [5, 64, 1023]
        bits = bmx.bucket_bits_of(want_b, 10)
        m = np.isin(bmx.key_bucket(id, f, 10), want_b)
        r3, n3 = e.export_rows(log2_buckets=10, bucket_bits=bits)
        assert n3 == int(m.sum()) and n3 > 0 and np.array_equal(_rec_tuples(r3), _tuples(id[m], f[m], ts[m], val[m]))
        # both filters, global-form bucket count
        b13 = bmx.key_bucket(id, f, 13)
        want13 = np.unique(b13)[:40]
        m = np.isin(b13, want13) & (ts >= since)
        r4, n4 = e.export_rows(since=since, log2_buckets=13, bucket_bits=bmx.bucket_bits_of(want13, 13))
        assert n4 == int(m.sum()) and np.array_equal(_rec_tuples(r4), _tuples(id[m], f[m], ts[m], val[m]))
        # tombstones only: the k keys with their clocks
        rt, nt = e.export_rows(only_tombstones=True)
        assert nt == k and (rt["val"] == DEL).all()
        gts, gval, found = e.get_rows(rt["id"], rt["field"])
        assert found.all() and (gval == DEL).all() and np.array_equal(gts, rt["ts"])
        srt = np.argsort(tid)
        assert np.array_equal(_rec_tuples(rt), _tuples(tid[srt], f_t[srt], tts[srt], np.full(k, DEL, np.int64)))
        # cap = half the matches: full count, the same first records, nothing behind out[cap]
        cap = n // 2
        guard = np.zeros(cap + 64, bmx.DELTA_REC_DTYPE)
        guard["id"] = 0xABABABABABABABAB; guard["aux"] = 0xCDCDCDCD
        mm = C.c_uint64()
        e._chk(e.L.bmx_export_rows(e.h, 0, 0, None, 0, C.c_void_p(guard.ctypes.data), cap, C.cast(C.byref(mm), C.c_void_p), bmx.MEM_HOST))
        assert mm.value == n
        assert np.array_equal(guard[:cap], recs[:cap])
        assert (guard["id"][cap:] == 0xABABABABABABABAB).all() and (guard["aux"][cap:] == 0xCDCDCDCD).all()
        # two calls give the same order
        again, _ = e.export_rows()
        assert np.array_equal(again, recs)
        # page-locked memory is written by the kernel itself: same records
        hb = bmx.HostBuffer(32 * n)
        pinned, np_ = e.export_rows(out=hb.array(bmx.DELTA_REC_DTYPE, n))
        assert np_ == n and np.array_equal(pinned, recs)
        del pinned; hb.close()
        # device memory: same records, same count, guard behind cap untouched
        dev = torch.device("cuda", 0)
        d_out = torch.full((4 * (cap + 16),), -1, dtype=torch.int64, device=dev)
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        e.export_rows_dev(d_out, cap, d_n); e.sync()
        h = d_out.cpu().numpy()
        assert int(d_n.item()) == n and np.array_equal(h[:4 * cap].view(bmx.DELTA_REC_DTYPE), recs[:cap]) and (h[4 * cap:] == -1).all()
        d_bits = torch.from_numpy(bits.view(np.int64)).to(dev)
        d_all = torch.zeros(4 * n3, dtype=torch.int64, device=dev)
        e.export_rows_dev(d_all, n3, d_n, log2_buckets=10, bucket_bits=d_bits); e.sync()
        assert int(d_n.item()) == n3 and np.array_equal(d_all.cpu().numpy().view(bmx.DELTA_REC_DTYPE), r3)
        e.export_rows_dev(None, 0, d_n, since=since); e.sync()
        assert int(d_n.item()) == n2
    o.close()


def test_epoch_mark_does_not_leak():
    """a row created by an INSERT_REFERENCE merge stores the clock 2 with the running epoch in bits 53-60 until the next sweep"""
    R, D = 50_000, 30_000
    res = synth.big_resident(R, seed=71)
    d = synth.big_deltas(D, R, seed=72, insert_pct=50, unique=True)
    o = Oracle(); o.load_rows(*res)
    o.merge_batch(*d)
    created = ~np.isin(d[0], res[0])
    assert created.sum() > D // 3
    with bmx.Engine(300_000) as e:
        e.load_rows(*res)
        e.merge_batch(*d, insert_mode=INSERT_REFERENCE, want_flags=False)
        recs, n = e.export_rows()
        assert n == len(o)
        assert (recs["ts"] >= 0).all() and (recs["ts"] < (1 << 53)).all()
        assert (recs["ts"][np.isin(recs["id"], d[0][created])] == 2).all()
        assert np.array_equal(_rec_tuples(recs), _tuples(*o.dump_rows()))
        for L in (10, 13):
            sums, counts = e.digest(L)
            assert _total(sums) == o.digest()
            assert _same((sums, counts), _np_digest(*o.dump_rows(), L))
    o.close()


def test_digest_orders_behind_deferred_compactions():
    dev = torch.device("cuda", 0)
    R, D, NB = 400_000, 131_072, 8
    res = synth.big_resident(R, seed=81)
    hb = [synth.big_deltas(D, R, seed=82, insert_pct=10, hot_pct=20, hot_keys=97, unique=False, batch=b, drift=40_000) for b in range(NB)]
    o = Oracle(); o.load_rows(*res)
    for b in hb:
        o.merge_batch(*b)
    db = [(torch.from_numpy(np.ascontiguousarray(i).view(np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(f).view(np.int32)).to(dev),
           torch.from_numpy(np.ascontiguousarray(t)).to(dev), torch.from_numpy(np.ascontiguousarray(v)).to(dev)) for i, f, t, v in hb]
    applied = torch.zeros((NB, D), dtype=torch.int32, device=dev)
    n_applied = torch.zeros(NB, dtype=torch.int64, device=dev)
    with bmx.Engine(2 * (R + NB * D)) as e:
        e.load_rows(*res)
        torch.cuda.synchronize(dev)
        for b in range(NB):
            e.merge_batch_dev(D, *db[b], INSERT_REFERENCE, applied=applied[b], n_applied=n_applied[b:b + 1])
        sums, counts = e.digest(10)                      # no sync() in between
        assert e.deferred_counts()[0] == NB
        assert _total(sums) == o.digest() and int(counts.sum()) == len(o)
        recs, n = e.export_rows()
        assert n == len(o) and np.array_equal(_rec_tuples(recs), _tuples(*o.dump_rows()))
    o.close()


# ---- bmx.replica ----
def _join(*states):
    """numpy state join: per key the lexicographic max of (ts, val), a tombstone (INT64_MIN) being the smallest value"""
    id = np.concatenate([s[0] for s in states]); f = np.concatenate([s[1] for s in states])
    ts = np.concatenate([s[2] for s in states]); val = np.concatenate([s[3] for s in states])
    order = np.lexsort((val, ts, f, id))
    id, f, ts, val = id[order], f[order], ts[order], val[order]
    last = np.ones(len(id), bool)
    last[:-1] = (id[1:] != id[:-1]) | (f[1:] != f[:-1])
    return id[last], f[last], ts[last], val[last]


def _with_tombstones(state, tid, tf, tts):
    """a state after put_rows of tombstones on keys it holds"""
    id, f, ts, val = (x.copy() for x in state)
    key = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(id.tolist(), f.tolist()))}
    for a, b, t in zip(tid.tolist(), tf.tolist(), tts.tolist()):
        i = key[(a, b)]
        ts[i] = t; val[i] = DEL
    return id, f, ts, val


def _check_state(e, want):
    """the engine holds exactly `want` (data rows through dump_rows, tombstones through get_rows)"""
    id, f, ts, val = want
    data = val != DEL
    assert np.array_equal(_tuples(*e.dump_rows()), _tuples(id[data], f[data], ts[data], val[data]))
    assert e.row_count() == len(id)
    if (~data).any():
        gts, gval, found = e.get_rows(id[~data], f[~data])
        assert found.all() and (gval == DEL).all() and np.array_equal(gts, ts[~data])


def _np_differing(sa, sb, L):
    da, db = _np_digest(*sa, L), _np_digest(*sb, L)
    return np.nonzero((da[0] != db[0]) | (da[1] != db[1]))[0]


def _data_rows_in(state, buckets, L):
    id, f, ts, val = state
    return int((np.isin(bmx.key_bucket(id, f, L), buckets) & (val != DEL)).sum())


def test_reconcile_two_engines():
    R, D, L = 200_000, 40_000, 10
    res = synth.big_resident(R, seed=91)
    X = synth.big_deltas(D, R, seed=92, insert_pct=10, unique=True, batch=0)
    Y0 = synth.big_deltas(D, R, seed=93, insert_pct=10, hot_pct=10, hot_keys=40, unique=False, batch=1)
    # Y overlaps X: half of X's keys again, a quarter of them with X's own clock and another value (ties on ts)
    h = D // 2
    yts = X[2][:h].copy(); yts[h // 2:] += 17
    Y = (np.concatenate([X[0][:h], Y0[0]]), np.concatenate([X[1][:h], Y0[1]]), np.concatenate([yts, Y0[2]]), np.concatenate([X[3][:h] ^ 5, Y0[3]]))
    oa = Oracle(); oa.load_rows(*res); oa.merge_batch(*X)
    ob = Oracle(); ob.load_rows(*res); ob.merge_batch(*Y)
    pre_a = oa.dump_rows()
    bid, bf, bts, _ = ob.dump_rows()
    pick = np.random.default_rng(9).choice(len(bid), 500, replace=False)
    tts = bts[pick] + np.where(np.arange(500) % 2 == 0, 1_000_000_000, 0)     # half of them above anything A holds, half at B's own clock
    pre_b = _with_tombstones(ob.dump_rows(), bid[pick], bf[pick], tts)
    want = _join(pre_a, pre_b)
    with bmx.Engine(600_000) as a, bmx.Engine(600_000, load_pct=35) as b:
        a.load_rows(*res); a.merge_batch(*X, want_flags=False)
        b.load_rows(*res); b.merge_batch(*Y, want_flags=False)
        b.put_rows(bid[pick], bf[pick], tts, np.full(500, DEL, np.int64))
        _check_state(a, pre_a); _check_state(b, pre_b)
        diff_ab = _np_differing(pre_a, pre_b, L)
        ra = replica.pull(a, b, L)
        assert ra["buckets_differing"] == len(diff_ab) > 0
        assert ra["rows_shipped"] == _data_rows_in(pre_b, diff_ab, L)
        assert ra["tombstones_shipped"] == 500 and 0 < ra["tombstones_applied"] <= 500
        _check_state(a, want)                              # a <- b made a the join already
        diff_ba = _np_differing(want, pre_b, L)
        rb = replica.pull(b, a, L)
        assert rb["buckets_differing"] == len(diff_ba) and rb["rows_shipped"] == _data_rows_in(want, diff_ba, L)
        _check_state(b, want)
        assert _same(a.digest(L, tombstones=True), b.digest(L, tombstones=True))
        assert _same(a.digest(13, tombstones=True), _np_digest(*want, 13))
        r2 = replica.reconcile(a, b, L)
        for r in r2:
            assert r == {"buckets_differing": 0, "rows_shipped": 0, "tombstones_shipped": 0, "tombstones_applied": 0}
    oa.close(); ob.close()


def test_reconcile_touches_only_the_buckets_that_differ():
    R, L = 200_000, 10
    res = synth.big_resident(R, seed=95)
    bk = bmx.key_bucket(res[0], res[1], L)
    m = np.isin(bk, [17, 900])
    assert m.sum() > 200
    delta = (res[0][m], res[1][m], res[2][m] + 50, res[3][m] + 1)
    oa = Oracle(); oa.load_rows(*res); oa.merge_batch(*delta)
    with bmx.Engine(500_000) as a, bmx.Comm([0, 0], 300_000) as b:
        a.load_rows(*res); a.merge_batch(*delta, want_flags=False)
        b.load_rows(*res)
        r = replica.pull(b, a, L)                          # a Comm as the receiving end: records through host memory
        assert r["buckets_differing"] == 2 and r["rows_shipped"] == int(m.sum()) and r["tombstones_shipped"] == 0
        assert rows_digest(*b.dump_rows()) == oa.digest()
        assert _same(a.digest(L, tombstones=True), b.digest(L, tombstones=True))
        assert replica.pull(a, b, L)["buckets_differing"] == 0
    oa.close()


def test_full_size_digest_equals_oracle():
    """the bench's config-2 table: 10M rows, 3 x 1M deltas (the oracle side is the one test_gpu_fullsize computes, once per session)"""
    from test_gpu_fullsize import _oracle_side
    res, bs, _, n_rows, digest = _oracle_side("config2")
    with bmx.Engine(22_000_000) as e:
        e.load_rows(*res)
        for b in bs:
            e.merge_batch(*b, want_flags=False)
        for L in (10, 13):
            sums, counts = e.digest(L)
            assert _total(sums) == digest and int(counts.sum()) == n_rows, L
        _, n = e.export_rows(cap=0)
        assert n == n_rows
