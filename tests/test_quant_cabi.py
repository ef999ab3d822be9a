"""CPU-only checks of the surface of include/bmx_quant.h: the two symbols exist and are listed in bmx.EXPORTS_QUANT while bmx.EXPORTS keeps its 108 names and the
older lists stay as they were, the header declares exactly these two and compiles as C99, the records have the sizes and offsets the header draws (8 / 32 / 32),
and every bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with its own text in the handle
kind's own error word, leaving the other words and pattern-filled outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_quantiles", "bmx_comm_where_quantiles"]
FILL = 0xA5
BASE = 7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_QUANT == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP
                            + bmx.EXPORTS_ROWS + bmx.EXPORTS_SEMI + bmx.EXPORTS_CLAIM), "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_SEMI == ["bmx_where_semijoin", "bmx_where_in", "bmx_comm_where_semijoin", "bmx_comm_where_in"]
    assert bmx.EXPORTS_GROUP == ["bmx_where_group", "bmx_comm_where_group"] and bmx.EXPORTS_ROWS == ["bmx_where_rows", "bmx_comm_where_rows"]
    assert bmx.EXPORTS_WHERE_AGG == ["bmx_where_aggregate", "bmx_where_top", "bmx_comm_where_aggregate", "bmx_comm_where_top"]


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_quant.h")).read()
    assert re.search(r'#include\s+"bmx_where.h"', hdr) and re.search(r'#include\s+"bmx.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in ("bmx.h", "bmx_where.h", "bmx_top.h", "bmx_watch.h", "bmx_where_agg.h", "bmx_vc_sync.h", "bmx_group.h", "bmx_rows.h", "bmx_semi.h", "bmx_claim.h"):
        assert "bmx_quant" not in open(os.path.join(ROOT, "include", older)).read() and "quantiles" not in open(os.path.join(ROOT, "include", older)).read(), older
    assert int(re.search(r"#define\s+BMX_QUANT_MAX\s+(\d+)u", code).group(1)) == bmx.QUANT_MAX == 8
    assert re.search(r"#define\s+BMX_QUANT_MAX_DEN\s+\(1u << 20\)", code) and bmx.QUANT_MAX_DEN == 1 << 20


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "quant_header.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    assert C.sizeof(bmx.QuantQ) == 8 and [(f[0], getattr(bmx.QuantQ, f[0]).offset) for f in bmx.QuantQ._fields_] == [("num", 0), ("den", 4)]
    want = [("value", 0), ("rank", 8), ("n_below", 16), ("n_equal", 24)]
    assert C.sizeof(bmx.QuantRec) == 32 == bmx.QUANT_REC_DTYPE.itemsize
    assert [(f[0], getattr(bmx.QuantRec, f[0]).offset) for f in bmx.QuantRec._fields_] == want == [(k, bmx.QUANT_REC_DTYPE.fields[k][1]) for k in bmx.QUANT_REC_DTYPE.names]
    want = [("n_match", 0), ("n", 8), ("min", 16), ("max", 24)]
    assert C.sizeof(bmx.QuantRes) == 32 == bmx.QUANT_RES_DTYPE.itemsize
    assert [(f[0], getattr(bmx.QuantRes, f[0]).offset) for f in bmx.QuantRes._fields_] == want == [(k, bmx.QUANT_RES_DTYPE.fields[k][1]) for k in bmx.QUANT_RES_DTYPE.names]


def _lens(*a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def _qs(*pairs):
    return (bmx.QuantQ * max(len(pairs), 1))(*[bmx.QuantQ(a, b) for a, b in pairs])


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
    recs = np.full(32 * 9, FILL, np.uint8)
    res = np.full(32, FILL, np.uint8)
    op, rp = C.c_void_p(recs.ctypes.data), C.c_void_p(res.ctypes.data)
    NOF = bmx.AGG_NO_FIELD
    q1, q8 = _qs((1, 2)), _qs(*[(k, 8) for k in range(8)])
    top = _qs((0, 1), (bmx.QUANT_MAX_DEN, bmx.QUANT_MAX_DEN))                                   # the largest denominator is fine
    ok_tails = [(BASE, 1, q1, op, rp), (9, 8, q8, op, None), (11, 2, top, op, rp)]             # (res may be NULL)

    def refused(prog, tail, text):
        """both mem modes with a NULL context, and a NULL communicator: the text lands in the handle kind's own word and leaves the other words alone"""
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_comm_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None) == bmx.ERR_INVALID      # a known text in the communicator's word
            before_comm, before_vc = lib.bmx_comm_last_error(None), lib.bmx_vc_last_error(None)
            assert lib.bmx_where_quantiles(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID, text
            assert text in lib.bmx_last_error(None), (text, lib.bmx_last_error(None))
            assert lib.bmx_comm_last_error(None) == before_comm and lib.bmx_vc_last_error(None) == before_vc
        assert lib.bmx_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None, 0) == bmx.ERR_INVALID              # ... and one in the context's word
        before_ctx, before_vc = lib.bmx_last_error(None), lib.bmx_vc_last_error(None)
        assert lib.bmx_comm_where_quantiles(None, BASE, *prog, *tail) == bmx.ERR_INVALID, text
        want = b"null communicator" if text == b"null context" else text
        assert want in lib.bmx_comm_last_error(None), (want, lib.bmx_comm_last_error(None))
        assert lib.bmx_last_error(None) == before_ctx and lib.bmx_vc_last_error(None) == before_vc

    # every refusal of the program, with arguments behind it that are fine
    for nc, lens, ls, text in bad:
        refused((nc, lens, ls), ok_tails[0], text)
    # the call's own refusals, with a program that is fine
    for prog in good:
        refused(prog, (BASE, 0, q1, op, rp), b"nq outside")
        refused(prog, (BASE, 9, q8, op, rp), b"nq outside")
        refused(prog, (BASE, 1 << 31, q8, op, rp), b"nq outside")
        refused(prog, (BASE, 1, None, op, rp), b"null qs")
        refused(prog, (BASE, 1, q1, None, rp), b"null output")
        refused(prog, (BASE, 1, _qs((0, 0)), op, rp), b"a quantile outside")
        refused(prog, (BASE, 1, _qs((1, bmx.QUANT_MAX_DEN + 1)), op, rp), b"a quantile outside")
        refused(prog, (BASE, 1, _qs((3, 2)), op, rp), b"a quantile outside")
        refused(prog, (BASE, 8, _qs(*[(1, 2)] * 7, (0xFFFFFFFF, 0xFFFFFFFF)), op, rp), b"a quantile outside")            # the last of eight
        refused(prog, (BASE, 2, _qs((1, 2), (2, 1)), op, rp), b"a quantile outside")
        for tail in ok_tails:
            for mem in (7, -1):
                assert lib.bmx_where_quantiles(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID
                assert b"bad mem kind" in lib.bmx_last_error(None)
            refused(prog, tail, b"null context")
    assert (recs == FILL).all() and (res == FILL).all(), "a refused call writes nothing"
