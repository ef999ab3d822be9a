"""CPU-only checks of the surface of include/bmx_join_rows.h: the four symbols exist and are listed in bmx.EXPORTS_JOIN_ROWS while bmx.EXPORTS keeps its 108 names
and the older lists stay as they were, the header declares exactly these four and compiles as C99, the record has the size and offsets the header draws, and
every bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with its own text (which names the
outer or the inner program) in the handle kind's own error word, leaving the other words and pattern-filled outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_join_rows", "bmx_where_map_rows", "bmx_comm_where_join_rows", "bmx_comm_where_map_rows"]
FILL = 0xA5
BASE, INNER, LINK, KEY = 7, 8, 9, 10


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_JOIN_ROWS == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP
                            + bmx.EXPORTS_ROWS + bmx.EXPORTS_SEMI + bmx.EXPORTS_JOIN + bmx.EXPORTS_QUANT), "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_ROWS == ["bmx_where_rows", "bmx_comm_where_rows"]
    assert bmx.EXPORTS_JOIN == ["bmx_where_join_group", "bmx_where_map_group", "bmx_comm_where_join_group", "bmx_comm_where_map_group"]
    assert bmx.EXPORTS_SEMI == ["bmx_where_semijoin", "bmx_where_in", "bmx_comm_where_semijoin", "bmx_comm_where_in"]


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_join_rows.h")).read()
    assert re.search(r'#include\s+"bmx_rows.h"', hdr) and re.search(r'#include\s+"bmx.h"', hdr) and re.search(r'#include\s+"bmx_join.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in ("bmx.h", "bmx_where.h", "bmx_top.h", "bmx_watch.h", "bmx_where_agg.h", "bmx_vc_sync.h", "bmx_group.h", "bmx_rows.h", "bmx_semi.h", "bmx_quant.h", "bmx_join.h"):
        text = open(os.path.join(ROOT, "include", older)).read()
        assert "jrows" not in text and "join_rows" not in text and "map_rows" not in text, older
    assert int(re.search(r"#define\s+BMX_JROWS_INNER\s+(\d+)u", code).group(1)) == bmx.JROWS_INNER == 2
    assert int(re.search(r"#define\s+BMX_JROWS_NO_NODE\s+(0x[0-9A-Fa-f]+)ull", code).group(1), 16) == bmx.JROWS_NO_NODE == 2**64 - 1
    assert bmx.JROWS_INNER & bmx.ROWS_TS == 0


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "join_rows_header.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    assert C.sizeof(bmx.JoinRowsRes) == 72 == bmx.JROWS_RES_DTYPE.itemsize
    want = [("n_match", 0), ("n_out", 8), ("next_pos", 16), ("layout", 24), ("n_joined", 32), ("map_size", 40), ("n_inner", 48), ("n_keyed", 56), ("flags", 64), ("next_shard", 68)]
    assert [(f[0], getattr(bmx.JoinRowsRes, f[0]).offset) for f in bmx.JoinRowsRes._fields_] == want
    assert [(k, bmx.JROWS_RES_DTYPE.fields[k][1]) for k in bmx.JROWS_RES_DTYPE.names] == want
    assert [(k, bmx.JROWS_RES_DTYPE.fields[k][1]) for k in bmx.JROWS_RES_DTYPE.names[:4]] == [(k, bmx.ROWS_RES_DTYPE.fields[k][1]) for k in bmx.ROWS_RES_DTYPE.names[:4]]


def _lens(*a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def _programs(base):
    lits = (bmx.Lit * 40)(*[bmx.Lit(base, 0, 0, 10) for _ in range(40)])                       # every literal on the base field: no field limit in the way
    nine = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 9), 0, 0, 10) for k in range(40)])              # nine distinct fields besides the base
    flag2 = (bmx.Lit * 40)(*[bmx.Lit(base, 2 if k == 3 else 0, 0, 10) for k in range(40)])
    flagh = (bmx.Lit * 40)(*[bmx.Lit(base, (bmx.LIT_NOT | 0x80000000) if k == 0 else 0, 0, 10) for k in range(40)])
    eight = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 8), bmx.LIT_NOT if k % 3 == 0 else 0, -(1 << 63), (1 << 63) - 1) for k in range(40)])
    bad = [                                          # the list of test_where_cabi.py
        (0, _lens(1), lits, b"1..8 clauses"),
        (9, _lens(*[1] * 9), lits, b"1..8 clauses"),
        (1, _lens(0), lits, b"1..8 literals"),
        (3, _lens(2, 0, 2), lits, b"1..8 literals"),
        (1, _lens(9), lits, b"1..8 literals"),
        (5, _lens(8, 8, 8, 8, 1), lits, b"32 literals"),
        (8, _lens(*[8] * 8), lits, b"32 literals"),
        (2, _lens(8, 1), nine, b"8 fields"),
        (1, _lens(4), flag2, b"flag bits"),
        (1, _lens(1), flagh, b"flag bits"),
        (1, None, lits, b"null clause_len or lits"),
        (1, _lens(1), None, b"null clause_len or lits"),
    ]
    good = [(1, _lens(1), lits), (8, _lens(*[4] * 8), eight), (4, _lens(8, 8, 8, 8), eight), (8, _lens(*[1] * 8), nine)]     # each limit reached, none passed
    return bad, good


def test_bad_arguments_are_refused(lib):
    bad_o, good_o = _programs(BASE)
    bad_i, good_i = _programs(INNER)
    bufs = [np.full(8 * 8 * 8, FILL, np.uint8) for _ in range(6)]                              # ids, vals, ts, in_ids, in_vals, in_ts: room for 8 rows of 8 fields
    res = np.full(72, FILL, np.uint8)
    keys = np.arange(8, dtype=np.int64)
    nodes = np.arange(8, dtype=np.uint64) + 100
    P = [C.c_void_p(b.ctypes.data) for b in bufs]
    rp, kp, np_ = C.c_void_p(res.ctypes.data), C.c_void_p(keys.ctypes.data), C.c_void_p(nodes.ctypes.data)
    f8 = (C.c_uint32 * 9)(*range(20, 29))
    NOF = bmx.AGG_NO_FIELD

    def refused(call, comm_call, text):
        """both mem modes with a NULL context, and a NULL communicator: the text lands in the handle kind's own word and leaves the other words alone"""
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_comm_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None) == bmx.ERR_INVALID      # a known text in the communicator's word
            before_comm, before_vc = lib.bmx_comm_last_error(None), lib.bmx_vc_last_error(None)
            assert call(mem) == bmx.ERR_INVALID, text
            for t in text:
                assert t in lib.bmx_last_error(None), (t, lib.bmx_last_error(None))
            assert lib.bmx_comm_last_error(None) == before_comm and lib.bmx_vc_last_error(None) == before_vc
        assert lib.bmx_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None, 0) == bmx.ERR_INVALID              # ... and one in the context's word
        before_ctx, before_vc = lib.bmx_last_error(None), lib.bmx_vc_last_error(None)
        assert comm_call() == bmx.ERR_INVALID, text
        for t in (b"null communicator",) if text == (b"null context",) else text:
            assert t in lib.bmx_comm_last_error(None), (t, lib.bmx_comm_last_error(None))
        assert lib.bmx_last_error(None) == before_ctx and lib.bmx_vc_last_error(None) == before_vc

    def outs(o):
        return tuple(None if k in o else P[j] for j, k in enumerate(("ids", "val", "ts", "in_ids", "in_val", "in_ts")))

    def join_rows(outer, inner, link=LINK, nf=2, fields=f8, key=KEY, nif=2, in_fields=f8, map_cap=64, flags=bmx.ROWS_TS, cap=8, null=(), r=rp, text=()):
        head = (BASE, *outer, link, nf, fields, INNER, *inner, key, nif, in_fields, map_cap, flags)
        tail = (cap, *outs(null), r)
        refused(lambda mem: lib.bmx_where_join_rows(None, *head, 0, *tail, mem), lambda: lib.bmx_comm_where_join_rows(None, *head, 0, 0, *tail), text)

    def map_rows(outer, link=LINK, nf=2, fields=f8, k=kp, v=np_, npairs=8, nif=2, in_fields=f8, flags=bmx.ROWS_TS, cap=8, null=(), r=rp, text=()):
        head = (BASE, *outer, link, nf, fields, k, v, npairs, nif, in_fields, flags)
        tail = (cap, *outs(null), r)
        refused(lambda mem: lib.bmx_where_map_rows(None, *head, 0, *tail, mem), lambda: lib.bmx_comm_where_map_rows(None, *head, 0, 0, *tail), text)

    def both(po, pi, **kw):
        join_rows(po, pi, **kw); map_rows(po, **kw)

    # every refusal of either program, with everything else fine; the text says which program
    for nc, lens, ls, text in bad_o:
        join_rows((nc, lens, ls), good_i[0], text=(text, b"outer program", b"where_join_rows: "))
        map_rows((nc, lens, ls), text=(text, b"outer program", b"where_map_rows: "))
    for nc, lens, ls, text in bad_i:
        join_rows(good_o[0], (nc, lens, ls), text=(text, b"inner program"))
    # the calls' own refusals, with programs that are fine
    for po, pi in zip(good_o, good_i):
        both(po, pi, r=None, text=(b"null result record",))
        both(po, pi, nf=9, text=(b"more than BMX_ROWS_MAX_FIELDS fields",))
        both(po, pi, nif=9, text=(b"more than BMX_ROWS_MAX_FIELDS inner fields",))
        both(po, pi, fields=None, text=(b"null fields",))
        both(po, pi, in_fields=None, text=(b"null in_fields",))
        for flags in (4, 8, 0x80000000, bmx.ROWS_TS | bmx.JROWS_INNER | 16):
            both(po, pi, flags=flags, text=(b"unknown flag bits",))
        both(po, pi, null=("ids",), text=(b"null out_ids",))
        both(po, pi, null=("val",), text=(b"null out_val",))
        both(po, pi, null=("ts",), text=(b"null out_ts",))
        both(po, pi, null=("in_ids",), text=(b"null out_in_ids",))
        both(po, pi, null=("in_ids",), nif=0, text=(b"null out_in_ids",))
        both(po, pi, null=("in_val",), text=(b"null out_in_val",))
        both(po, pi, null=("in_ts",), text=(b"null out_in_ts",))
        for mc in (0, bmx.JOIN_MAX_MAP + 1, 1 << 40):
            join_rows(po, pi, map_cap=mc, text=(b"map_cap outside 1..BMX_JOIN_MAX_MAP",))
            map_rows(po, npairs=mc, text=(b"npairs outside 1..BMX_JOIN_MAX_MAP",))
        map_rows(po, k=None, text=(b"null keys",))
        map_rows(po, v=None, text=(b"null node_ids",))
        both(po, pi, link=NOF, text=(b"no link field",))
        join_rows(po, pi, key=NOF, text=(b"no key field",))
        for mem in (7, -1):
            a = (0, 8, *P, rp, mem)
            assert lib.bmx_where_join_rows(None, BASE, *po, LINK, 2, f8, INNER, *pi, KEY, 2, f8, 64, 0, *a) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
            assert lib.bmx_where_map_rows(None, BASE, *po, LINK, 2, f8, kp, np_, 8, 2, f8, 0, *a) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
        # nothing wrong but the handle: the limits reached, and the pointers that are not needed missing
        both(po, pi, nf=8, nif=8, flags=bmx.ROWS_TS | bmx.JROWS_INNER, text=(b"null context",))
        both(po, pi, nf=0, nif=0, fields=None, in_fields=None, null=("val", "ts", "in_val", "in_ts"), text=(b"null context",))
        both(po, pi, flags=bmx.JROWS_INNER, null=("ts", "in_ts"), text=(b"null context",))
        both(po, pi, cap=0, null=("ids", "val", "ts", "in_ids", "in_val", "in_ts"), text=(b"null context",))
        join_rows(po, pi, map_cap=1, link=BASE, key=INNER, text=(b"null context",))
        join_rows(po, pi, map_cap=bmx.JOIN_MAX_MAP, text=(b"null context",))
        map_rows(po, npairs=1, text=(b"null context",))
    assert all((b == FILL).all() for b in bufs) and (res == FILL).all() and (keys == np.arange(8)).all() and (nodes == np.arange(8) + 100).all(), "a refused call writes nothing"
