"""CPU-only checks of the surface of include/bmx_join.h: the four symbols exist and are listed in bmx.EXPORTS_JOIN while bmx.EXPORTS keeps its 108 names and the
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
NEW = ["bmx_where_join_group", "bmx_where_map_group", "bmx_comm_where_join_group", "bmx_comm_where_map_group"]
FILL = 0xA5
BASE, INNER, LINK, KEY, ATTR, MEASURE = 7, 8, 9, 10, 11, 12


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_JOIN == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP
                            + bmx.EXPORTS_ROWS + bmx.EXPORTS_SEMI + bmx.EXPORTS_QUANT), "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_GROUP == ["bmx_where_group", "bmx_comm_where_group"]
    assert bmx.EXPORTS_SEMI == ["bmx_where_semijoin", "bmx_where_in", "bmx_comm_where_semijoin", "bmx_comm_where_in"]


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_join.h")).read()
    assert re.search(r'#include\s+"bmx_where.h"', hdr) and re.search(r'#include\s+"bmx.h"', hdr) and re.search(r'#include\s+"bmx_group.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in ("bmx.h", "bmx_where.h", "bmx_top.h", "bmx_watch.h", "bmx_where_agg.h", "bmx_vc_sync.h", "bmx_group.h", "bmx_rows.h", "bmx_semi.h", "bmx_quant.h"):
        text = open(os.path.join(ROOT, "include", older)).read()
        assert "bmx_join" not in text and "join_group" not in text and "map_group" not in text, older
    assert int(re.search(r"#define\s+BMX_JOIN_MAP_OVERFLOW\s+(\d+)u", code).group(1)) == bmx.JOIN_MAP_OVERFLOW == 1
    assert int(re.search(r"#define\s+BMX_JOIN_GROUP_OVERFLOW\s+(\d+)u", code).group(1)) == bmx.JOIN_GROUP_OVERFLOW == 2
    assert re.search(r"#define\s+BMX_JOIN_MAX_MAP\s+\(1u << 20\)", code) and bmx.JOIN_MAX_MAP == 1 << 20


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "join_header.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    assert C.sizeof(bmx.JoinRes) == 184 == bmx.JOIN_RES_DTYPE.itemsize
    want = [("n_groups", 0), ("map_size", 8), ("n_inner", 16), ("n_keyed", 24), ("flags", 32), ("reserved", 36), ("absent", 40), ("unmatched", 88), ("total", 136)]
    assert [(f[0], getattr(bmx.JoinRes, f[0]).offset) for f in bmx.JoinRes._fields_] == want
    assert [(k, bmx.JOIN_RES_DTYPE.fields[k][1]) for k in bmx.JOIN_RES_DTYPE.names] == want


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
    recs = np.full(8 * 56, FILL, np.uint8)
    res = np.full(184, FILL, np.uint8)
    keys = np.arange(8, dtype=np.int64)
    vals = np.arange(8, dtype=np.int64) + 100
    op, rp, kp, vp = C.c_void_p(recs.ctypes.data), C.c_void_p(res.ctypes.data), C.c_void_p(keys.ctypes.data), C.c_void_p(vals.ctypes.data)
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

    def join_group(outer, inner, link=LINK, measure=MEASURE, key=KEY, attr=ATTR, map_cap=64, out=op, cap=8, r=rp, text=()):
        a = (BASE, *outer, link, measure, INNER, *inner, key, attr, map_cap, out, cap, r)
        refused(lambda mem: lib.bmx_where_join_group(None, *a, mem), lambda: lib.bmx_comm_where_join_group(None, *a), text)

    def map_group(outer, link=LINK, measure=MEASURE, k=kp, v=vp, npairs=8, out=op, cap=8, r=rp, text=()):
        a = (BASE, *outer, link, measure, k, v, npairs, out, cap, r)
        refused(lambda mem: lib.bmx_where_map_group(None, *a, mem), lambda: lib.bmx_comm_where_map_group(None, *a), text)

    # every refusal of either program, with everything else fine; the text says which program
    for nc, lens, ls, text in bad_o:
        join_group((nc, lens, ls), good_i[0], text=(text, b"outer program", b"where_join_group: "))
        map_group((nc, lens, ls), text=(text, b"outer program", b"where_map_group: "))
    for nc, lens, ls, text in bad_i:
        join_group(good_o[0], (nc, lens, ls), text=(text, b"inner program"))
    # the calls' own refusals, with programs that are fine
    for po, pi in zip(good_o, good_i):
        join_group(po, pi, r=None, text=(b"null result record",))
        map_group(po, r=None, text=(b"null result record",))
        join_group(po, pi, out=None, text=(b"null output",))
        map_group(po, out=None, text=(b"null output",))
        for cap in (0, bmx.GROUP_MAX_CAP + 1, 1 << 40):
            join_group(po, pi, cap=cap, text=(b"cap outside 1..BMX_GROUP_MAX_CAP",))
            map_group(po, cap=cap, text=(b"cap outside 1..BMX_GROUP_MAX_CAP",))
        for mc in (0, bmx.JOIN_MAX_MAP + 1, 1 << 40):
            join_group(po, pi, map_cap=mc, text=(b"map_cap outside 1..BMX_JOIN_MAX_MAP",))
            map_group(po, npairs=mc, text=(b"npairs outside 1..BMX_JOIN_MAX_MAP",))
        map_group(po, k=None, text=(b"null keys",))
        map_group(po, v=None, text=(b"null vals",))
        join_group(po, pi, link=NOF, text=(b"no link field",))
        map_group(po, link=NOF, text=(b"no link field",))
        join_group(po, pi, key=NOF, text=(b"no key field",))
        join_group(po, pi, attr=NOF, text=(b"no attribute field",))
        for mem in (7, -1):
            assert lib.bmx_where_join_group(None, BASE, *po, LINK, MEASURE, INNER, *pi, KEY, ATTR, 64, op, 8, rp, mem) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
            assert lib.bmx_where_map_group(None, BASE, *po, LINK, NOF, kp, vp, 8, op, 8, rp, mem) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
        # nothing wrong but the handle: the limits reached (cap, map_cap and npairs at both ends, no measure, one field in several roles)
        for mc, cap, measure in ((1, 1, NOF), (bmx.JOIN_MAX_MAP, bmx.GROUP_MAX_CAP, MEASURE), (64, 8, BASE)):
            join_group(po, pi, map_cap=mc, cap=cap, measure=measure, text=(b"null context",))
        join_group(po, pi, link=BASE, key=INNER, attr=INNER, text=(b"null context",))
        map_group(po, npairs=1, cap=1, measure=NOF, text=(b"null context",))
        map_group(po, text=(b"null context",))
    assert (recs == FILL).all() and (res == FILL).all() and (keys == np.arange(8)).all() and (vals == np.arange(8) + 100).all(), "a refused call writes nothing"
