"""CPU-only checks of the surface of include/bmx_first.h: the two symbols exist and are listed in bmx.EXPORTS_FIRST while bmx.EXPORTS keeps its 108 names and the
older lists stay as they were, the header declares exactly these two and compiles as C99, both records have the size and offsets the header draws, the constants
agree, and every bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with its own text in the
handle kind's own error word, leaving the other words and pattern-filled outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_group_first", "bmx_comm_where_group_first"]
FILL = 0xA5
BASE, GROUP, ORDER = 7, 8, 9


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_FIRST == NEW
    older = (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP + bmx.EXPORTS_ROWS
             + bmx.EXPORTS_SEMI + bmx.EXPORTS_JOIN + bmx.EXPORTS_JOIN_ROWS + bmx.EXPORTS_QUANT + bmx.EXPORTS_CLAIM + bmx.EXPORTS_UPDATE + bmx.EXPORTS_GROUP_MULTI
             + bmx.EXPORTS_REACH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in older, "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_GROUP == ["bmx_where_group", "bmx_comm_where_group"] and bmx.EXPORTS_ROWS == ["bmx_where_rows", "bmx_comm_where_rows"]
    assert bmx.EXPORTS_REACH == ["bmx_where_reach", "bmx_where_reach_from", "bmx_comm_where_reach", "bmx_comm_where_reach_from"]
    for name in ("where_group_first", "where_group_first_dev"):
        assert callable(getattr(bmx.Engine, name)), name
    assert callable(bmx.Comm.where_group_first) and callable(bmx.first_merge)
    assert bmx.FirstResult.__slots__[:3] == ("records", "vals", "ts")


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_first.h")).read()
    assert re.search(r'#include\s+"bmx.h"', hdr) and re.search(r'#include\s+"bmx_where.h"', hdr) and re.search(r'#include\s+"bmx_rows.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if older != "bmx_first.h":
            text = open(os.path.join(ROOT, "include", older)).read()
            assert "group_first" not in text and "bmx_first" not in text and "BMX_FIRST" not in text, older
    assert int(re.search(r"#define\s+BMX_FIRST_DESC\s+(\d+)u", code).group(1)) == bmx.FIRST_DESC == 2
    assert int(re.search(r"#define\s+BMX_FIRST_OVERFLOW\s+(\d+)u", code).group(1)) == bmx.FIRST_OVERFLOW == 1
    assert int(re.search(r"#define\s+BMX_FIRST_NO_NODE\s+(0x[0-9A-Fa-f]+)ull", code).group(1), 16) == bmx.FIRST_NO_NODE == 2**64 - 1 == bmx.JROWS_NO_NODE
    assert re.search(r"#define\s+BMX_FIRST_MAX_CAP\s+\(1u << 20\)", code) and bmx.FIRST_MAX_CAP == 1 << 20
    assert bmx.FIRST_DESC & bmx.ROWS_TS == 0
    # what the header has to say in words
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    for words in ("the id is STILL ascending", "UNSIGNED 64-bit", "CONTENDERS", "one representative per group", "brings ITS shard's cells",
                  "row r of every column belongs to out[r]", "sum of out[i].n == n_ordered"):
        assert words in flat, words


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "first_header.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layouts():
    assert C.sizeof(bmx.FirstRec) == 40 == bmx.FIRST_DTYPE.itemsize
    want = [("key", 0), ("id", 8), ("val", 16), ("n_match", 24), ("n", 32)]
    assert [(f[0], getattr(bmx.FirstRec, f[0]).offset) for f in bmx.FirstRec._fields_] == want
    assert [(k, bmx.FIRST_DTYPE.fields[k][1]) for k in bmx.FIRST_DTYPE.names] == want
    assert C.sizeof(bmx.FirstRes) == 40 == bmx.FIRST_RES_DTYPE.itemsize
    want = [("n_groups", 0), ("flags", 8), ("reserved", 12), ("total", 16), ("absent", 24), ("n_ordered", 32)]
    assert [(f[0], getattr(bmx.FirstRes, f[0]).offset) for f in bmx.FirstRes._fields_] == want
    assert [(k, bmx.FIRST_RES_DTYPE.fields[k][1]) for k in bmx.FIRST_RES_DTYPE.names] == want
    assert bmx.FIRST_DTYPE["id"] == np.dtype("<u8") and bmx.FIRST_DTYPE["key"] == np.dtype("<i8")


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
    bufs = [np.full(8 * 8 * 8, FILL, np.uint8) for _ in range(3)]                              # records, vals, ts: room for 8 rows of 8 fields
    res = np.full(40, FILL, np.uint8)
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

    def first(prog, group=GROUP, order=ORDER, nf=2, fields=f8, flags=bmx.ROWS_TS, cap=8, null=(), r=rp, text=()):
        outs = tuple(None if k in null else P[j] for j, k in enumerate(("out", "val", "ts")))
        args = (BASE, *prog, group, order, nf, fields, flags, cap, *outs, r)
        refused(lambda mem: lib.bmx_where_group_first(None, *args, mem), lambda: lib.bmx_comm_where_group_first(None, *args), text)

    # every refusal of the program, with everything else fine
    for nc, lens, ls, text in bad:
        first((nc, lens, ls), text=(text,))
    # the call's own refusals, each with its own text, with programs that are fine
    for p in good:
        first(p, r=None, text=(b"where_group_first: null result record",))
        for cap in (0, bmx.FIRST_MAX_CAP + 1, 1 << 40):
            first(p, cap=cap, text=(b"cap outside 1..BMX_FIRST_MAX_CAP",))
        first(p, null=("out",), text=(b"where_group_first: null output",))
        first(p, nf=9, text=(b"more than BMX_ROWS_MAX_FIELDS fields",))
        first(p, fields=None, text=(b"null fields",))
        first(p, null=("val",), text=(b"null out_val",))
        first(p, null=("ts",), text=(b"null out_ts",))
        for flags in (4, 8, 0x80000000, bmx.ROWS_TS | bmx.FIRST_DESC | 16):
            first(p, flags=flags, text=(b"unknown flag bits",))
        first(p, group=NOF, text=(b"no group field",))
        first(p, order=NOF, text=(b"no order field",))
        for mem in (7, -1):
            assert lib.bmx_where_group_first(None, BASE, *p, GROUP, ORDER, 2, f8, 0, 8, *P, rp, mem) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
        # nothing wrong but the handle: the limits reached, and the pointers that are not needed missing
        first(p, nf=8, flags=bmx.ROWS_TS | bmx.FIRST_DESC, cap=bmx.FIRST_MAX_CAP, text=(b"null context",))
        first(p, nf=0, fields=None, null=("val", "ts"), text=(b"null context",))
        first(p, flags=bmx.FIRST_DESC, null=("ts",), text=(b"null context",))
        first(p, group=BASE, order=BASE, cap=1, text=(b"null context",))
        first(p, group=ORDER, order=ORDER, flags=0, null=("ts",), text=(b"null context",))
    assert all((b == FILL).all() for b in bufs) and (res == FILL).all(), "a refused call writes nothing"
