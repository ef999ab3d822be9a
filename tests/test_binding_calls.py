"""What the Python binding sends to libbmx.so, checked without a GPU and without the library: a stub stands in for the ctypes library object and records
every call; the record must equal tests/binding_calls.json, which was written by this file's own recorder (python tests/test_binding_calls.py OUT.json) run
against the binding as it stood before its split into modules. A difference is a bug in the binding, never a reason to record again."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "binding_calls.json")
HANDLE = C.c_void_p(0xB0B0)              # the handle every instance holds
DEV = 0x10000                            # "device pointers" are plain ints from here on, 0x100 apart: the record tells them apart


class Stub:
    """in place of the ctypes library: every bmx_* attribute records (name, normalised args) and returns 0; outputs stay as the binding zeroed them"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("bmx_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append([name, [norm(a) for a in args]])
            return 0
        return fn


def norm(a):
    if a is None:
        return None
    if a is HANDLE:
        return "h"
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    if isinstance(a, C.c_void_p):        # numpy-backed and cast pointers: only that they are there; the fake device pointers: which one
        return None if not a.value else ("ptr:%#x" % a.value if a.value < (1 << 24) else "ptr")
    if isinstance(a, (C.Array, C.Structure)):
        return "bytes:" + bytes(a).hex()
    if hasattr(a, "_obj"):               # byref(x): what it points at
        return ["ref", norm(a._obj)]
    if hasattr(a, "value"):              # a ctypes scalar
        return a.value
    raise TypeError("unexpected argument %r" % (a,))


def dev(i):
    return DEV + 0x100 * i


def record(bmx):
    """-> {"Class.method[/variant]": [[function, args], ...]} for every scan / where / watch method of Engine, Comm and EngineVC in all its forms, and for the
    other methods that hand a by-reference result to the library"""
    L = Stub()

    def make(cls, **attrs):
        o = cls.__new__(cls)
        o.L, o.h = L, HANDLE
        for k, v in attrs.items():
            setattr(o, k, v)
        return o

    e = make(bmx.Engine, device=0, _watch_base={7: 3})
    c = make(bmx.Comm, N=2)
    v = make(bmx.EngineVC, K=2, device=0)
    out = {}

    def run(key, fn, *a, **kw):
        L.calls = []
        fn(*a, **kw)
        assert L.calls, key
        assert key not in out, key
        out[key] = L.calls

    FULL = (2, [[(3, 1, 9), (4, -5, 5, True)], [((3, 4), 0, 2), (bmx.Clock(5, tombs=True), 10, 20, True)]])    # a program with every kind of literal: scan_where, watch_create
    P = (2, [[(3, 1, 9)]])                                                                                  # the program of the other calls (it keeps the record small)
    Q = (6, [[(6, 0, 100)]])                                                                                # an inner / seed program
    T = [(1, 0, 10), (2, -3, 3)]                                                                            # terms
    X = bmx.Expr(3, "*", 4)
    QS = [(1, 2), (9, 10)]
    KEYS = [3, (4, -10, 5)]
    VALS = np.array([5, 6, 7], np.int64)
    NODES = np.array([11, 12, 13], np.uint64)

    # ---- host forms that Engine and Comm share ----
    for tag, q in (("Engine", e), ("Comm", c)):
        run(tag + ".scan_aggregate", q.scan_aggregate, T, measure=3, group=4, group_lo=-2, ngroups=3)
        run(tag + ".scan_aggregate/plain", q.scan_aggregate, T)
        run(tag + ".scan_top", q.scan_top, T, 5, desc=True, after=(9, -4))
        run(tag + ".scan_top/start", q.scan_top, T, 5)
        run(tag + ".scan_where", q.scan_where, *FULL)
        run(tag + ".scan_where/count", q.scan_where, *P, count_only=True)
        run(tag + ".where_aggregate", q.where_aggregate, *P, measure=3, group=4, group_lo=-2, ngroups=3)
        run(tag + ".where_aggregate/plain", q.where_aggregate, *P)
        run(tag + ".where_top", q.where_top, *P, 5, desc=True, after={"id": 9, "val": -4})
        run(tag + ".where_group", q.where_group, *P, 4, measure=3, cap=7)
        run(tag + ".where_group/count", q.where_group, *P, 4)
        run(tag + ".where_quantiles", q.where_quantiles, *P, 3, QS)
        run(tag + ".where_aggregate_expr", q.where_aggregate_expr, *P, X, group=4, group_lo=-2, ngroups=3)
        run(tag + ".where_group_expr", q.where_group_expr, *P, 4, X, cap=7)
        run(tag + ".where_quantiles_expr", q.where_quantiles_expr, *P, X, QS)
        run(tag + ".where_rows", q.where_rows, *P, [3, 4], cap=5, with_ts=True, start=(4 if q is e else (1, 4)))
        run(tag + ".where_rows/all", q.where_rows, *P, [3, 4])
        run(tag + ".where_group_first", q.where_group_first, *P, 4, 3, fields=[5, 6], desc=True, with_ts=True, cap=7)
        run(tag + ".where_group_first/plain", q.where_group_first, *P, 4, 3)
        run(tag + ".where_group_top", q.where_group_top, *P, 4, 3, 2, fields=[5, 6], desc=True, with_ts=True, cap=7)
        run(tag + ".where_group_top/refused", q.where_group_top, *P, 4, 3, 99, cap=7)
        run(tag + ".where_group_multi", q.where_group_multi, *P, KEYS, measure=3, cap=7)
        run(tag + ".where_update", q.where_update, *P, 5, bmx.UPD_ADD, operand=2, src=6, ts=1234, force=True, cap=5, start=(4 if q is e else (1, 4)), want_ids=True)
        run(tag + ".where_update/all", q.where_update, *P, 5, bmx.UPD_SET, operand=2, ts=1234)
        run(tag + ".where_semijoin", q.where_semijoin, *P, 3, *Q, 6, anti=True, cap=5, set_cap=9)
        run(tag + ".where_semijoin/all", q.where_semijoin, *P, 3, *Q, 6)
        run(tag + ".where_semijoin/count", q.where_semijoin, *P, 3, *Q, 6, count_only=True)
        run(tag + ".where_in", q.where_in, *P, 3, VALS, anti=True, cap=5)
        run(tag + ".where_in/all", q.where_in, *P, 3, VALS)
        run(tag + ".where_in/count", q.where_in, *P, 3, VALS, count_only=True)
        run(tag + ".where_reach", q.where_reach, *P, 3, 4, *Q, 6, max_depth=4, set_cap=9, cap=5)
        run(tag + ".where_reach/all", q.where_reach, *P, 3, 4, *Q, 6)
        run(tag + ".where_reach/count", q.where_reach, *P, 3, 4, *Q, 6, count_only=True)
        run(tag + ".where_reach_from", q.where_reach_from, *P, 3, 4, VALS, max_depth=4, set_cap=9, cap=5)
        run(tag + ".where_reach_from/all", q.where_reach_from, *P, 3, 4, VALS)
        run(tag + ".where_reach_from/count", q.where_reach_from, *P, 3, 4, VALS, count_only=True)
        run(tag + ".where_join_group", q.where_join_group, *P, 3, *Q, 6, 7, measure=4, cap=7, map_cap=9)
        run(tag + ".where_join_group/plain", q.where_join_group, *P, 3, *Q, 6, 7)
        run(tag + ".where_map_group", q.where_map_group, *P, 3, VALS, VALS + 1, measure=4, cap=7)
        run(tag + ".where_join_rows", q.where_join_rows, *P, 3, [4, 5], *Q, 6, [7], cap=5, with_ts=True, inner=True, start=(4 if q is e else (1, 4)), map_cap=9)
        run(tag + ".where_join_rows/all", q.where_join_rows, *P, 3, [4, 5], *Q, 6, [7])
        run(tag + ".where_map_rows", q.where_map_rows, *P, 3, [4, 5], VALS, NODES, [7], cap=5, with_ts=True, inner=True, start=(4 if q is e else (1, 4)))
        run(tag + ".where_map_rows/all", q.where_map_rows, *P, 3, [4, 5], VALS, NODES, [7])
        run(tag + ".watch_create", q.watch_create, *FULL)
        run(tag + ".watch_poll", q.watch_poll, 7, cap_entered=4, cap_left=3)
        run(tag + ".watch_poll/all", q.watch_poll, 7)
        run(tag + ".watch_destroy", q.watch_destroy, 7)
        run(tag + ".scan_range", q.scan_range, 3, -1, 8)
        run(tag + ".scan_equals", q.scan_equals, 3, 8)
        run(tag + ".scan_count", q.scan_count, 3, -1, 8)
        run(tag + ".scan_filter", q.scan_filter, T)
        run(tag + ".dump_rows", q.dump_rows)
        run(tag + ".digest", q.digest, 2, tombstones=True)
        run(tag + ".export_rows", q.export_rows, since=5, log2_buckets=6, bucket_bits=np.ones(1, np.uint64), only_tombstones=True)
    run("Engine.scan_where/cap", e.scan_where, *P, cap=5)
    run("Engine.scan_range/cap", e.scan_range, 3, -1, 8, cap=5)
    run("Engine.scan_range/out", e.scan_range, 3, -1, 8, out=np.zeros(4, np.uint64))
    run("Engine.scan_range_pos", e.scan_range_pos, 3, -1, 8, cap=5)
    run("Engine.scan_filter/cap", e.scan_filter, T, cap=5)
    run("Engine.where_update_all", e.where_update_all, *P, 5, bmx.UPD_COPY, src=6, ts=1234, page=8)
    run("Engine.export_rows/cap", e.export_rows, cap=5)
    run("Engine.export_rows/out", e.export_rows, out=np.zeros(4, bmx.DELTA_REC_DTYPE))
    run("Engine.merge_batch", e.merge_batch, [1, 2], [3, 3], [5, 6], [7, 8], insert_mode=bmx.INSERT_DELTA)
    run("Engine.merge_collect", e.merge_collect, (9, 2, True))
    run("Comm.merge", c.merge, [1, 2], [3, 3], [5, 6], [7, 8])

    # ---- device forms: Engine only; the pointers are plain ints ----
    run("Engine.scan_range_dev", e.scan_range_dev, 3, -1, 8, dev(1), 5, dev(2))
    run("Engine.scan_range_pos_dev", e.scan_range_pos_dev, 3, -1, 8, dev(1), 5, dev(2))
    run("Engine.scan_aggregate_dev", e.scan_aggregate_dev, T, dev(1), measure=3, group=4, group_lo=-2, ngroups=3)
    run("Engine.scan_top_dev", e.scan_top_dev, T, 5, dev(1), n_out=dev(2), n_eligible=dev(3), desc=True, after=(9, -4))
    run("Engine.scan_where_dev", e.scan_where_dev, *FULL, dev(1), 5, dev(2))
    run("Engine.where_aggregate_dev", e.where_aggregate_dev, *P, dev(1), measure=3, group=4, group_lo=-2, ngroups=3)
    run("Engine.where_top_dev", e.where_top_dev, *P, 5, dev(1), n_out=dev(2), n_eligible=dev(3), desc=True, after=(9, -4))
    run("Engine.where_group_dev", e.where_group_dev, *P, 4, dev(1), dev(2), measure=3, cap=7)
    run("Engine.where_quantiles_dev", e.where_quantiles_dev, *P, 3, QS, dev(1), res=dev(2))
    run("Engine.where_aggregate_expr_dev", e.where_aggregate_expr_dev, *P, X, dev(1), xres=dev(2), group=4, group_lo=-2, ngroups=3)
    run("Engine.where_group_expr_dev", e.where_group_expr_dev, *P, 4, X, dev(1), dev(2), xres=dev(3), cap=7)
    run("Engine.where_quantiles_expr_dev", e.where_quantiles_expr_dev, *P, X, QS, dev(1), res=dev(2), xres=dev(3))
    run("Engine.where_rows_dev", e.where_rows_dev, *P, [3, 4], 5, dev(1), dev(2), dev(3), dev(4), start=4)
    run("Engine.where_rows_dev/no_ts", e.where_rows_dev, *P, [3, 4], 5, dev(1), dev(2), None, dev(4))
    run("Engine.where_group_first_dev", e.where_group_first_dev, *P, 4, 3, dev(1), dev(2), dev(3), dev(4), fields=[5, 6], desc=True, cap=7)
    run("Engine.where_group_top_dev", e.where_group_top_dev, *P, 4, 3, 2, dev(1), dev(2), dev(3), None, dev(5), fields=[5, 6], cap=7)
    run("Engine.where_group_multi_dev", e.where_group_multi_dev, *P, KEYS, dev(1), dev(2), measure=3, cap=7)
    run("Engine.where_update_dev", e.where_update_dev, *P, 5, bmx.UPD_ADD, 5, dev(1), dev(2), operand=2, src=6, ts=1234, force=True, start=4)
    run("Engine.where_semijoin_dev", e.where_semijoin_dev, *P, 3, *Q, 6, dev(1), 5, dev(2), anti=True, set_cap=9)
    run("Engine.where_in_dev", e.where_in_dev, *P, 3, dev(1), 3, dev(2), 5, dev(3), anti=True)
    run("Engine.where_reach_dev", e.where_reach_dev, *P, 3, 4, *Q, 6, dev(1), dev(2), 5, dev(3), max_depth=4, set_cap=9)
    run("Engine.where_reach_from_dev", e.where_reach_from_dev, *P, 3, 4, dev(1), 3, dev(2), dev(3), 5, dev(4), max_depth=4, set_cap=9)
    run("Engine.where_join_group_dev", e.where_join_group_dev, *P, 3, *Q, 6, 7, dev(1), dev(2), measure=4, cap=7, map_cap=9)
    run("Engine.where_map_group_dev", e.where_map_group_dev, *P, 3, dev(1), dev(2), 3, dev(3), dev(4), measure=4, cap=7)
    run("Engine.where_join_rows_dev", e.where_join_rows_dev, *P, 3, [4, 5], *Q, 6, [7], 5, dev(1), dev(2), dev(3), dev(4), dev(5), dev(6), dev(7), inner=True, start=4, map_cap=9)
    run("Engine.where_join_rows_dev/no_ts", e.where_join_rows_dev, *P, 3, [4, 5], *Q, 6, [7], 5, dev(1), dev(2), None, dev(4), dev(5), None, dev(7))
    run("Engine.where_map_rows_dev", e.where_map_rows_dev, *P, 3, [4, 5], dev(8), dev(9), 3, [7], 5, dev(1), dev(2), dev(3), dev(4), dev(5), dev(6), dev(7), inner=True, start=4)
    run("Engine.watch_poll_dev", e.watch_poll_dev, 7, dev(1), 4, dev(2), 3, dev(3))
    run("Engine.digest_dev", e.digest_dev, 2, dev(1), dev(2))
    run("Engine.export_rows_dev", e.export_rows_dev, dev(1), 5, dev(2), since=5, log2_buckets=6, bucket_bits=dev(3))

    # ---- the vector-clock table ----
    run("EngineVC.scan_range", v.scan_range, 3, -1, 8)
    run("EngineVC.scan_range/count", v.scan_range, 3, -1, 8, count_only=True)
    run("EngineVC.digest", v.digest, 2)
    run("EngineVC.digest_dev", v.digest_dev, 2, dev(1), dev(2))
    run("EngineVC.frontier", v.frontier)
    run("EngineVC.export_rows", v.export_rows, frontier=[1, 2], log2_buckets=6, bucket_bits=np.ones(1, np.uint64))
    run("EngineVC.export_rows/cap", v.export_rows, cap=5)
    run("EngineVC.export_rows_dev", v.export_rows_dev, dev(1), 5, dev(2), frontier=[1, 2])
    run("EngineVC.merge_batch", v.merge_batch, [1, 2], [3, 3], [[1, 0], [0, 2]], [7, 8], keysets=[bmx.keyset([0, 1])] * 2)
    run("EngineVC.merge_records", v.merge_records, np.zeros(2, bmx.VC_REC_DTYPE))
    run("EngineVC.merge_records_dev", v.merge_records_dev, 2, dev(1), updated=dev(2), n_updated=dev(3), flags=dev(4))
    return out


def test_every_query_method_sends_what_it_always_sent():
    import bmx
    with open(TABLE) as f:
        want = json.load(f)
    got = json.loads(json.dumps(record(bmx)))          # (through JSON: tuples and lists compare alike)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_the_record_covers_every_scan_where_and_watch_method():
    import bmx
    with open(TABLE) as f:
        have = {k.split("/")[0] for k in json.load(f)}
    for cls in (bmx.Engine, bmx.Comm, bmx.EngineVC):
        for name in dir(cls):
            if name.startswith(("scan_", "where_", "watch_")):
                assert "%s.%s" % (cls.__name__, name) in have, name


if __name__ == "__main__":                              # python tests/test_binding_calls.py OUT.json: record the binding that is on sys.path
    import bmx
    with open(sys.argv[1], "w") as f:                   # one line per method and variant
        rec = record(bmx)
        f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(rec[k], separators=(",", ":"))) for k in sorted(rec)) + "\n}\n")
