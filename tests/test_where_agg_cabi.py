"""CPU-only checks of the surface of include/bmx_where_agg.h: the four symbols exist and are listed in bmx.EXPORTS_WHERE_AGG while bmx.EXPORTS keeps its 108
names and the older lists stay as they were, the header declares exactly these four, and every bad-argument case is refused before any device work — with a
NULL context and a NULL communicator, in both mem modes, leaving pattern-filled outputs untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_aggregate", "bmx_where_top", "bmx_comm_where_aggregate", "bmx_comm_where_top"]
FILL = 0xA5
BASE = 7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_WHERE_AGG == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in bmx.EXPORTS, "bmx.EXPORTS mirrors bmx.h alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_TOP == ["bmx_scan_top", "bmx_comm_scan_top"] and bmx.EXPORTS_WHERE == ["bmx_scan_where", "bmx_comm_scan_where"]
    assert bmx.EXPORTS_WATCH == ["bmx_watch_create", "bmx_watch_poll", "bmx_watch_destroy", "bmx_comm_watch_create", "bmx_comm_watch_poll", "bmx_comm_watch_destroy"]
    assert bmx.EXPORTS_VC_SYNC == ["bmx_vc_rec_digest", "bmx_vc_info", "bmx_vc_digest", "bmx_vc_frontier", "bmx_vc_export_rows", "bmx_vc_merge_records"]


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_where_agg.h")).read()
    assert re.search(r'#include\s+"bmx_where.h"', hdr) and re.search(r'#include\s+"bmx_top.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    assert "#define" not in code.replace("#define BMX_WHERE_AGG_H", ""), "no new constants: the limits are those of bmx.h, bmx_where.h and bmx_top.h"
    for older in ("bmx.h", "bmx_where.h", "bmx_top.h"):
        assert "bmx_where_agg" not in open(os.path.join(ROOT, "include", older)).read()


def _lens(*a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def _programs():
    lits = (bmx.Lit * 40)(*[bmx.Lit(BASE, 0, 0, 10) for _ in range(40)])                       # every literal on the base field: no field limit in the way
    nine = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 9), 0, 0, 10) for k in range(40)])              # nine distinct fields besides the base
    flag2 = (bmx.Lit * 40)(*[bmx.Lit(BASE, 2 if k == 3 else 0, 0, 10) for k in range(40)])
    flagh = (bmx.Lit * 40)(*[bmx.Lit(BASE, (bmx.LIT_NOT | 0x80000000) if k == 0 else 0, 0, 10) for k in range(40)])
    eight = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 8), bmx.LIT_NOT if k % 3 == 0 else 0, -(1 << 63), (1 << 63) - 1) for k in range(40)])
    bad = [                                          # the list of test_where_cabi.py
        (0, _lens(1), lits),                         # no clause
        (9, _lens(*[1] * 9), lits),                  # more than 8
        (1, _lens(0), lits),                         # an empty clause
        (3, _lens(2, 0, 2), lits),
        (1, _lens(9), lits),                         # a clause of more than 8
        (5, _lens(8, 8, 8, 8, 1), lits),             # 33 literals
        (8, _lens(*[8] * 8), lits),                  # 64
        (2, _lens(8, 1), nine),                      # 9 distinct fields besides the base field
        (1, _lens(4), flag2),                        # unknown flag bits
        (1, _lens(1), flagh),
        (1, None, lits),                             # NULL clause_len
        (1, _lens(1), None),                         # NULL lits
    ]
    good = [(1, _lens(1), lits), (8, _lens(*[4] * 8), eight), (4, _lens(8, 8, 8, 8), eight), (8, _lens(*[1] * 8), nine)]     # each limit reached, none passed
    return bad, good


def test_bad_arguments_are_refused(lib):
    bad, good = _programs()
    agg = np.full(48 * 8, FILL, np.uint8)
    top = np.full(16 * 8, FILL, np.uint8)
    cnt = np.full(16, FILL, np.uint8)
    ap, tp = C.c_void_p(agg.ctypes.data), C.c_void_p(top.ctypes.data)
    ctr = (C.c_void_p(cnt.ctypes.data), C.c_void_p(cnt.ctypes.data + 8))
    cur = bmx.TopRec(5, 5)
    cp = C.cast(C.byref(cur), C.c_void_p)
    NOF = bmx.AGG_NO_FIELD
    agg_ok = [(NOF, NOF, 0, 0, ap), (BASE, 9, -3, 5, ap), (9, BASE, 0, bmx.AGG_MAX_GROUPS, ap)]
    top_ok = [(0, None, 1, tp), (bmx.TOP_DESC, cp, 4096, tp), (0, cp, 7, tp)]

    def refused_agg(prog, tail, why):
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_where_aggregate(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID, why
        assert lib.bmx_comm_where_aggregate(None, BASE, *prog, *tail) == bmx.ERR_INVALID, why

    def refused_top(prog, tail, why):
        for counters in (ctr, (None, None)):
            for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
                assert lib.bmx_where_top(None, BASE, *prog, *tail, *counters, mem) == bmx.ERR_INVALID, why
            assert lib.bmx_comm_where_top(None, BASE, *prog, *tail, *counters) == bmx.ERR_INVALID, why

    # every refusal of the program, with arguments behind it that are fine
    for nc, lens, ls in bad:
        why = (nc, list(lens or []))
        refused_agg((nc, lens, ls), agg_ok[1], why)
        refused_top((nc, lens, ls), top_ok[1], why)
    # the aggregate's and the select's own refusals, with a program that is fine
    assert bmx.AGG_MAX_GROUPS == 65536 and bmx.TOP_MAX_K == 4096
    for prog in good:
        refused_agg(prog, (BASE, 9, 0, 65537, ap), "ngroups > 65536")
        refused_agg(prog, (BASE, NOF, 0, 4, ap), "groups without a group field")
        refused_agg(prog, (BASE, 9, 0, 4, None), "NULL out")
        refused_agg(prog, (NOF, NOF, 0, 0, None), "NULL out")
        refused_top(prog, (0, None, 0, tp), "k == 0")
        refused_top(prog, (0, cp, 4097, tp), "k == 4097")
        refused_top(prog, (2, None, 10, tp), "unknown top flag bits")
        refused_top(prog, (bmx.TOP_DESC | 0x80000000, cp, 10, tp), "unknown top flag bits")
        refused_top(prog, (0, None, 10, None), "NULL out")
        # a bad mem kind, and well-formed arguments with no context / no communicator behind them
        for tail in agg_ok:
            assert lib.bmx_where_aggregate(None, BASE, *prog, *tail, 7) == bmx.ERR_INVALID
            refused_agg(prog, tail, "NULL context")
        for tail in top_ok:
            assert lib.bmx_where_top(None, BASE, *prog, *tail, *ctr, 7) == bmx.ERR_INVALID
            refused_top(prog, tail, "NULL context")
    assert (agg == FILL).all() and (top == FILL).all() and (cnt == FILL).all(), "a refused call writes nothing"
    assert (cur.id, cur.val) == (5, 5)
