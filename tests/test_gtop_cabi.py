"""CPU-only checks of the surface of include/bmx_group_top.h: the two symbols exist and are listed in bmx.EXPORTS_GROUP_TOP while bmx.EXPORTS keeps its 108 names
and the older lists stay as they were, the header declares exactly these two, compiles as C99 and keeps clear of the names the older headers' tests look for, the
three records have the size and offsets the header draws, the constants agree, and every bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with its own text in the
handle kind's own error word, leaving the other words and pattern-filled outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_group_top", "bmx_comm_where_group_top"]
FORBIDDEN = ["group_first", "bmx_first", "BMX_FIRST", "bmx_join", "join_group", "map_group", "jrows", "join_rows", "map_rows", "group_multi", "bmx_semi", "bmx_where_in",
             "semijoin", "where_update", "bmx_upd", "BMX_UPD", "where_reach", "bmx_reach", "BMX_REACH"]
FILL = 0xA5
BASE, GROUP, ORDER = 7, 8, 9


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_GROUP_TOP == NEW
    older = (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP + bmx.EXPORTS_ROWS
             + bmx.EXPORTS_SEMI + bmx.EXPORTS_JOIN + bmx.EXPORTS_JOIN_ROWS + bmx.EXPORTS_QUANT + bmx.EXPORTS_CLAIM + bmx.EXPORTS_UPDATE + bmx.EXPORTS_GROUP_MULTI
             + bmx.EXPORTS_REACH + bmx.EXPORTS_FIRST)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in older, "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_GROUP == ["bmx_where_group", "bmx_comm_where_group"] and bmx.EXPORTS_ROWS == ["bmx_where_rows", "bmx_comm_where_rows"]
    assert bmx.EXPORTS_FIRST == ["bmx_where_group_first", "bmx_comm_where_group_first"]
    assert bmx.EXPORTS_REACH == ["bmx_where_reach", "bmx_where_reach_from", "bmx_comm_where_reach", "bmx_comm_where_reach_from"]
    for name in ("where_group_top", "where_group_top_dev"):
        assert callable(getattr(bmx.Engine, name)), name
    assert callable(bmx.Comm.where_group_top) and callable(bmx.gtop_merge)
    assert bmx.GroupTopResult.__slots__[:5] == ("groups", "rows", "vals", "ts", "top")


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_group_top.h")).read()
    assert re.search(r'#include\s+"bmx.h"', hdr) and re.search(r'#include\s+"bmx_where.h"', hdr) and re.search(r'#include\s+"bmx_rows.h"', hdr)
    assert "bmx_first.h" not in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for word in FORBIDDEN:                                  # the older headers' tests scan every header but their own for these, comments included
        assert word not in hdr, word
    assert "mgroup" not in hdr.lower()
    for older in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if older != "bmx_group_top.h":
            text = open(os.path.join(ROOT, "include", older)).read()
            assert "group_top" not in text and "bmx_gtop" not in text and "BMX_GTOP" not in text, older
    assert int(re.search(r"#define\s+BMX_GTOP_DESC\s+(\d+)u", code).group(1)) == bmx.GTOP_DESC == 2 == bmx.FIRST_DESC
    assert int(re.search(r"#define\s+BMX_GTOP_OVERFLOW\s+(\d+)u", code).group(1)) == bmx.GTOP_OVERFLOW == 1
    assert int(re.search(r"#define\s+BMX_GTOP_NO_NODE\s+(0x[0-9A-Fa-f]+)ull", code).group(1), 16) == bmx.GTOP_NO_NODE == 2**64 - 1 == bmx.FIRST_NO_NODE
    assert re.search(r"#define\s+BMX_GTOP_MAX_CAP\s+\(1u << 20\)", code) and bmx.GTOP_MAX_CAP == 1 << 20
    assert int(re.search(r"#define\s+BMX_GTOP_MAX_PER\s+(\d+)u", code).group(1)) == bmx.GTOP_MAX_PER == 16
    assert re.search(r"#define\s+BMX_GTOP_MAX_ROWS\s+\(1u << 22\)", code) and bmx.GTOP_MAX_ROWS == 1 << 22
    assert bmx.GTOP_DESC & bmx.ROWS_TS == 0
    # what the header has to say in words
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    for words in ("the id is STILL ascending", "UNSIGNED 64-bit", "CONTENDERS", "n_rows = min(per, n)", "brings ITS shard's cells", "block g of every array belongs to out[g]",
                  "sum of out[g].n == n_ordered", "n_rows = sum of out[g].n_rows", "res->n_rows is 0", "{BMX_GTOP_NO_NODE, BMX_VAL_DELETED}"):
        assert words in flat, words


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "gtop_header.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layouts():
    for S, D, size, want in ((bmx.GtopGrp, bmx.GTOP_GRP_DTYPE, 32, [("key", 0), ("n_match", 8), ("n", 16), ("n_rows", 24)]),
                             (bmx.GtopRow, bmx.GTOP_ROW_DTYPE, 16, [("id", 0), ("val", 8)]),
                             (bmx.GtopRes, bmx.GTOP_RES_DTYPE, 48, [("n_groups", 0), ("flags", 8), ("per", 12), ("total", 16), ("absent", 24), ("n_ordered", 32), ("n_rows", 40)])):
        assert C.sizeof(S) == size == D.itemsize
        assert [(f[0], getattr(S, f[0]).offset) for f in S._fields_] == want
        assert [(k, D.fields[k][1]) for k in D.names] == want
    assert bmx.GTOP_ROW_DTYPE["id"] == np.dtype("<u8") and bmx.GTOP_GRP_DTYPE["key"] == np.dtype("<i8") and bmx.GTOP_RES_DTYPE["per"] == np.dtype("<u4")


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
    bad, good = _programs(BASE)
    bufs = [np.full(8 * 8 * 8 * 16, FILL, np.uint8) for _ in range(4)]                         # groups, rows, vals, ts: room for 8 groups of 16 rows of 8 fields
    res = np.full(48, FILL, np.uint8)
    P = [C.c_void_p(b.ctypes.data) for b in bufs]
    rp = C.c_void_p(res.ctypes.data)
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

    def top(prog, group=GROUP, order=ORDER, per=4, nf=2, fields=f8, flags=bmx.ROWS_TS, cap=8, null=(), r=rp, text=()):
        outs = tuple(None if k in null else P[j] for j, k in enumerate(("out", "rows", "val", "ts")))
        args = (BASE, *prog, group, order, per, nf, fields, flags, cap, *outs, r)
        refused(lambda mem: lib.bmx_where_group_top(None, *args, mem), lambda: lib.bmx_comm_where_group_top(None, *args), text)

    # every refusal of the program, with everything else fine
    for nc, lens, ls, text in bad:
        top((nc, lens, ls), text=(text,))
    # the call's own refusals, each with its own text, with programs that are fine
    for p in good:
        top(p, r=None, text=(b"where_group_top: null result record",))
        for cap in (0, bmx.GTOP_MAX_CAP + 1, 1 << 40):
            top(p, cap=cap, text=(b"cap outside 1..BMX_GTOP_MAX_CAP",))
        for per in (0, bmx.GTOP_MAX_PER + 1, 1 << 31):
            top(p, per=per, text=(b"per outside 1..BMX_GTOP_MAX_PER",))
        for cap, per in ((bmx.GTOP_MAX_CAP, 5), ((1 << 18) + 1, 16), ((1 << 19) + 1, 8)):
            top(p, cap=cap, per=per, text=(b"cap * per above BMX_GTOP_MAX_ROWS",))
        top(p, null=("out",), text=(b"where_group_top: null output",))
        top(p, null=("rows",), text=(b"where_group_top: null out_rows",))
        top(p, nf=9, text=(b"more than BMX_ROWS_MAX_FIELDS fields",))
        top(p, fields=None, text=(b"null fields",))
        top(p, null=("val",), text=(b"null out_val",))
        top(p, null=("ts",), text=(b"null out_ts",))
        for flags in (4, 8, 0x80000000, bmx.ROWS_TS | bmx.GTOP_DESC | 16):
            top(p, flags=flags, text=(b"unknown flag bits",))
        top(p, group=NOF, text=(b"no group field",))
        top(p, order=NOF, text=(b"no order field",))
        for mem in (7, -1):
            assert lib.bmx_where_group_top(None, BASE, *p, GROUP, ORDER, 4, 2, f8, 0, 8, *P, rp, mem) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
        # nothing wrong but the handle: the limits reached, and the pointers that are not needed missing
        top(p, nf=8, flags=bmx.ROWS_TS | bmx.GTOP_DESC, cap=bmx.GTOP_MAX_CAP, per=4, text=(b"null context",))
        top(p, cap=1 << 18, per=bmx.GTOP_MAX_PER, text=(b"null context",))
        top(p, cap=1, per=1, text=(b"null context",))
        top(p, nf=0, fields=None, null=("val", "ts"), text=(b"null context",))
        top(p, flags=bmx.GTOP_DESC, null=("ts",), text=(b"null context",))
        top(p, group=BASE, order=BASE, cap=1, text=(b"null context",))
        top(p, group=ORDER, order=ORDER, flags=0, null=("ts",), text=(b"null context",))
    assert all((b == FILL).all() for b in bufs) and (res == FILL).all(), "a refused call writes nothing"
