"""CPU-only checks of the surface of include/bmx_group.h: the two symbols exist and are listed in bmx.EXPORTS_GROUP while bmx.EXPORTS keeps its 108 names and the
older lists stay as they were, the header declares exactly these two and compiles as C99, the records have the sizes and offsets the header draws, and every
bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with its own text in the handle kind's own
error word, leaving the other words and pattern-filled outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_group", "bmx_comm_where_group"]
FILL = 0xA5
BASE = 7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_GROUP == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG, "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_TOP == ["bmx_scan_top", "bmx_comm_scan_top"] and bmx.EXPORTS_WHERE == ["bmx_scan_where", "bmx_comm_scan_where"]
    assert bmx.EXPORTS_WATCH == ["bmx_watch_create", "bmx_watch_poll", "bmx_watch_destroy", "bmx_comm_watch_create", "bmx_comm_watch_poll", "bmx_comm_watch_destroy"]
    assert bmx.EXPORTS_VC_SYNC == ["bmx_vc_rec_digest", "bmx_vc_info", "bmx_vc_digest", "bmx_vc_frontier", "bmx_vc_export_rows", "bmx_vc_merge_records"]
    assert bmx.EXPORTS_WHERE_AGG == ["bmx_where_aggregate", "bmx_where_top", "bmx_comm_where_aggregate", "bmx_comm_where_top"]


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_group.h")).read()
    assert re.search(r'#include\s+"bmx_where.h"', hdr) and re.search(r'#include\s+"bmx.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in ("bmx.h", "bmx_where.h", "bmx_top.h", "bmx_watch.h", "bmx_where_agg.h", "bmx_vc_sync.h"):
        assert "bmx_group" not in open(os.path.join(ROOT, "include", older)).read() and "bmx_where_group" not in open(os.path.join(ROOT, "include", older)).read(), older
    assert int(re.search(r"#define\s+BMX_GROUP_OVERFLOW\s+(\d+)u", code).group(1)) == bmx.GROUP_OVERFLOW == 1
    assert re.search(r"#define\s+BMX_GROUP_MAX_CAP\s+\(1u << 20\)", code) and bmx.GROUP_MAX_CAP == 1 << 20


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "group_header.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    assert bmx.GROUP_DTYPE.itemsize == 56 and bmx.GROUP_DTYPE.fields["key"][1] == 0 and bmx.GROUP_DTYPE.fields["agg"][1] == 8
    assert C.sizeof(bmx.GroupRes) == 112 == bmx.GROUP_RES_DTYPE.itemsize
    want = [("n_groups", 0), ("flags", 8), ("reserved", 12), ("absent", 16), ("total", 64)]
    assert [(f[0], getattr(bmx.GroupRes, f[0]).offset) for f in bmx.GroupRes._fields_] == want
    assert [(k, bmx.GROUP_RES_DTYPE.fields[k][1]) for k in bmx.GROUP_RES_DTYPE.names] == want
    assert C.sizeof(bmx.Agg) == 48 == bmx.AGG_DTYPE.itemsize


def _lens(*a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def _programs():
    lits = (bmx.Lit * 40)(*[bmx.Lit(BASE, 0, 0, 10) for _ in range(40)])                       # every literal on the base field: no field limit in the way
    nine = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 9), 0, 0, 10) for k in range(40)])              # nine distinct fields besides the base
    flag2 = (bmx.Lit * 40)(*[bmx.Lit(BASE, 2 if k == 3 else 0, 0, 10) for k in range(40)])
    flagh = (bmx.Lit * 40)(*[bmx.Lit(BASE, (bmx.LIT_NOT | 0x80000000) if k == 0 else 0, 0, 10) for k in range(40)])
    eight = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 8), bmx.LIT_NOT if k % 3 == 0 else 0, -(1 << 63), (1 << 63) - 1) for k in range(40)])
    bad = [                                          # the list of test_where_cabi.py
        (0, _lens(1), lits, b"1..8 clauses"),        # no clause
        (9, _lens(*[1] * 9), lits, b"1..8 clauses"),
        (1, _lens(0), lits, b"1..8 literals"),       # an empty clause
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
    bad, good = _programs()
    recs = np.full(56 * 8, FILL, np.uint8)
    res = np.full(112, FILL, np.uint8)
    op, rp = C.c_void_p(recs.ctypes.data), C.c_void_p(res.ctypes.data)
    NOF = bmx.AGG_NO_FIELD
    ok_tails = [(NOF, 9, op, 8, rp), (BASE, BASE, op, 1, rp), (9, 11, op, bmx.GROUP_MAX_CAP, rp)]

    def refused(prog, tail, text):
        """both mem modes with a NULL context, and a NULL communicator: the text lands in the handle kind's own word and leaves the other words alone"""
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_comm_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None) == bmx.ERR_INVALID      # a known text in the communicator's word
            before_comm, before_vc = lib.bmx_comm_last_error(None), lib.bmx_vc_last_error(None)
            assert lib.bmx_where_group(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID, text
            assert text in lib.bmx_last_error(None), (text, lib.bmx_last_error(None))
            assert lib.bmx_comm_last_error(None) == before_comm and lib.bmx_vc_last_error(None) == before_vc
        assert lib.bmx_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None, 0) == bmx.ERR_INVALID              # ... and one in the context's word
        before_ctx, before_vc = lib.bmx_last_error(None), lib.bmx_vc_last_error(None)
        assert lib.bmx_comm_where_group(None, BASE, *prog, *tail) == bmx.ERR_INVALID, text
        want = b"null communicator" if text == b"null context" else text
        assert want in lib.bmx_comm_last_error(None), (want, lib.bmx_comm_last_error(None))
        assert lib.bmx_last_error(None) == before_ctx and lib.bmx_vc_last_error(None) == before_vc

    # every refusal of the program, with arguments behind it that are fine
    for nc, lens, ls, text in bad:
        refused((nc, lens, ls), ok_tails[0], text)
    # the call's own refusals, with a program that is fine
    for prog in good:
        refused(prog, (BASE, 9, op, 8, None), b"null result record")
        refused(prog, (BASE, 9, None, 8, rp), b"null output")
        refused(prog, (BASE, 9, None, 1, rp), b"null output")
        refused(prog, (BASE, 9, op, 0, rp), b"cap outside")
        refused(prog, (BASE, 9, None, 0, rp), b"cap outside")
        refused(prog, (BASE, 9, op, bmx.GROUP_MAX_CAP + 1, rp), b"cap outside")
        refused(prog, (BASE, 9, op, 1 << 40, rp), b"cap outside")
        refused(prog, (BASE, NOF, op, 8, rp), b"no group field")
        refused(prog, (NOF, NOF, op, 8, rp), b"no group field")
        for tail in ok_tails:
            for mem in (7, -1):
                assert lib.bmx_where_group(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID
                assert b"bad mem kind" in lib.bmx_last_error(None)
            refused(prog, tail, b"null context")
    assert (recs == FILL).all() and (res == FILL).all(), "a refused call writes nothing"


def test_the_result_object():
    res = np.zeros((), bmx.GROUP_RES_DTYPE)
    res["n_groups"] = 2; res["total"]["n_match"] = 9; res["total"]["n"] = 9; res["absent"]["n_match"] = 1; res["absent"]["n"] = 1
    recs = np.zeros(4, bmx.GROUP_DTYPE); recs["key"] = [-3, 8, 0, 0]; recs["agg"]["n_match"] = [5, 3, 0, 0]; recs["agg"]["n"] = [5, 3, 0, 0]
    g = bmx.GroupResult(res, recs)
    assert (g.n_groups, g.overflow, list(g.groups), g.groups[8].n_match, g.total.n_match, g.absent.n_match) == (2, False, [-3, 8], 3, 9, 1)
    res["flags"] = bmx.GROUP_OVERFLOW; res["n_groups"] = 70
    g = bmx.GroupResult(res, recs)
    assert g.overflow and g.n_groups == 70 and not g.groups and len(g.records) == 0 and g.total.n_match == 9
    c = bmx.GroupRes(); c.n_groups = 1; c.total.n_match = 4; c.total.n = 4
    assert bmx.GroupResult(c, recs).total.n_match == 4
