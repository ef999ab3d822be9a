"""CPU-only checks of the surface of include/bmx_semi.h: the four symbols exist and are listed in bmx.EXPORTS_SEMI while bmx.EXPORTS keeps its 108 names and the
older lists stay as they were, the header declares exactly these four and compiles as C99, the record has the size and offsets the header draws, and every
bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with its own text (which names the outer
or the inner program) in the handle kind's own error word, leaving the other words and pattern-filled outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_semijoin", "bmx_where_in", "bmx_comm_where_semijoin", "bmx_comm_where_in"]
FILL = 0xA5
BASE, INNER, LINK, KEY = 7, 8, 9, 10


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_SEMI == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP
                            + bmx.EXPORTS_ROWS), "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_GROUP == ["bmx_where_group", "bmx_comm_where_group"] and bmx.EXPORTS_ROWS == ["bmx_where_rows", "bmx_comm_where_rows"]
    assert bmx.EXPORTS_WHERE == ["bmx_scan_where", "bmx_comm_scan_where"]


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_semi.h")).read()
    assert re.search(r'#include\s+"bmx_where.h"', hdr) and re.search(r'#include\s+"bmx.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in ("bmx.h", "bmx_where.h", "bmx_top.h", "bmx_watch.h", "bmx_where_agg.h", "bmx_vc_sync.h", "bmx_group.h", "bmx_rows.h"):
        text = open(os.path.join(ROOT, "include", older)).read()
        assert "bmx_semi" not in text and "bmx_where_in" not in text and "semijoin" not in text, older
    assert int(re.search(r"#define\s+BMX_SEMI_OVERFLOW\s+(\d+)u", code).group(1)) == bmx.SEMI_OVERFLOW == 1
    assert int(re.search(r"#define\s+BMX_SEMI_ANTI\s+(\d+)u", code).group(1)) == bmx.SEMI_ANTI == 1
    assert re.search(r"#define\s+BMX_SEMI_MAX_SET\s+\(1u << 20\)", code) and bmx.SEMI_MAX_SET == 1 << 20


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "semi_header.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    assert C.sizeof(bmx.SemiRes) == 32 == bmx.SEMI_RES_DTYPE.itemsize
    want = [("n_match", 0), ("set_size", 8), ("n_inner", 16), ("flags", 24), ("reserved", 28)]
    assert [(f[0], getattr(bmx.SemiRes, f[0]).offset) for f in bmx.SemiRes._fields_] == want
    assert [(k, bmx.SEMI_RES_DTYPE.fields[k][1]) for k in bmx.SEMI_RES_DTYPE.names] == want


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
    ids = np.full(8 * 8, FILL, np.uint8)
    res = np.full(32, FILL, np.uint8)
    vals = np.arange(8, dtype=np.int64)
    op, rp, vp = C.c_void_p(ids.ctypes.data), C.c_void_p(res.ctypes.data), C.c_void_p(vals.ctypes.data)
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

    def semijoin(outer, inner, link=LINK, flags=0, key=KEY, set_cap=64, out=op, cap=8, r=rp, text=()):
        a = (BASE, *outer, link, flags, INNER, *inner, key, set_cap, out, cap, r)
        refused(lambda mem: lib.bmx_where_semijoin(None, *a, mem), lambda: lib.bmx_comm_where_semijoin(None, *a), text)

    def where_in(outer, link=LINK, flags=0, values=vp, nvalues=8, out=op, cap=8, r=rp, text=()):
        a = (BASE, *outer, link, flags, values, nvalues, out, cap, r)
        refused(lambda mem: lib.bmx_where_in(None, *a, mem), lambda: lib.bmx_comm_where_in(None, *a), text)

    # every refusal of either program, with everything else fine; the text says which program
    for nc, lens, ls, text in bad_o:
        semijoin((nc, lens, ls), good_i[0], text=(text, b"outer program", b"where_semijoin: "))
        where_in((nc, lens, ls), text=(text, b"outer program", b"where_in: "))
    for nc, lens, ls, text in bad_i:
        semijoin(good_o[0], (nc, lens, ls), text=(text, b"inner program"))
    # the calls' own refusals, with programs that are fine
    for po, pi in zip(good_o, good_i):
        semijoin(po, pi, r=None, text=(b"null result record",))
        where_in(po, r=None, text=(b"null result record",))
        for sc in (0, bmx.SEMI_MAX_SET + 1, 1 << 40):
            semijoin(po, pi, set_cap=sc, text=(b"set_cap outside",))
            where_in(po, nvalues=sc, text=(b"nvalues outside",))
        where_in(po, values=None, text=(b"null values",))
        semijoin(po, pi, out=None, cap=1, text=(b"null out_ids",))
        where_in(po, out=None, cap=8, text=(b"null out_ids",))
        for fl in (2, 0x80000001, 3):
            semijoin(po, pi, flags=fl, text=(b"unknown flag bits",))
            where_in(po, flags=fl, text=(b"unknown flag bits",))
        semijoin(po, pi, link=NOF, text=(b"no link field",))
        where_in(po, link=NOF, text=(b"no link field",))
        semijoin(po, pi, key=NOF, text=(b"no key field",))
        for mem in (7, -1):
            assert lib.bmx_where_semijoin(None, BASE, *po, LINK, 0, INNER, *pi, KEY, 64, op, 8, rp, mem) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
            assert lib.bmx_where_in(None, BASE, *po, LINK, 1, vp, 8, op, 8, rp, mem) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
        # nothing wrong but the handle: the limits reached (set_cap and nvalues at both ends, the anti flag, counting only)
        for sc, fl, out, cap in ((1, 0, op, 8), (bmx.SEMI_MAX_SET, 1, None, 0), (64, 1, op, 0)):
            semijoin(po, pi, flags=fl, set_cap=sc, out=out, cap=cap, text=(b"null context",))
        where_in(po, nvalues=1, flags=1, out=None, cap=0, text=(b"null context",))
        where_in(po, text=(b"null context",))
    assert (ids == FILL).all() and (res == FILL).all() and (vals == np.arange(8)).all(), "a refused call writes nothing"
