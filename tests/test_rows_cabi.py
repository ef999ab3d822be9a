"""CPU-only checks of the surface of include/bmx_rows.h: the two symbols exist and are listed in bmx.EXPORTS_ROWS while bmx.EXPORTS keeps its 108 names and the
older lists stay as they were, the header declares exactly these two and compiles as C99, the record has the size and offsets the header draws, and every
bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with its own text in the handle kind's own
error word, leaving the other words and pattern-filled outputs untouched. (start_shard >= nshards needs a communicator: test_gpu_where_rows_comm.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_rows", "bmx_comm_where_rows"]
FILL = 0xA5
BASE = 7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_ROWS == NEW
    older = bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in older, "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_GROUP == ["bmx_where_group", "bmx_comm_where_group"] and bmx.EXPORTS_WHERE == ["bmx_scan_where", "bmx_comm_scan_where"]


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_rows.h")).read()
    assert re.search(r'#include\s+"bmx_where.h"', hdr) and re.search(r'#include\s+"bmx.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in ("bmx.h", "bmx_where.h", "bmx_top.h", "bmx_watch.h", "bmx_where_agg.h", "bmx_vc_sync.h", "bmx_group.h"):
        assert "bmx_rows" not in open(os.path.join(ROOT, "include", older)).read() and "bmx_where_rows" not in open(os.path.join(ROOT, "include", older)).read(), older
    assert int(re.search(r"#define\s+BMX_ROWS_MAX_FIELDS\s+(\d+)u", code).group(1)) == bmx.ROWS_MAX_FIELDS == 8
    assert int(re.search(r"#define\s+BMX_ROWS_TS\s+(\d+)u", code).group(1)) == bmx.ROWS_TS == 1
    assert int(re.search(r"#define\s+BMX_ROWS_NO_CLOCK\s+\((-\d+)\)", code).group(1)) == bmx.ROWS_NO_CLOCK == -1


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "rows_header.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    assert C.sizeof(bmx.RowsRes) == 40 == bmx.ROWS_RES_DTYPE.itemsize
    want = [("n_match", 0), ("n_out", 8), ("next_pos", 16), ("layout", 24), ("next_shard", 32), ("reserved", 36)]
    assert [(f[0], getattr(bmx.RowsRes, f[0]).offset) for f in bmx.RowsRes._fields_] == want
    assert [(k, bmx.ROWS_RES_DTYPE.fields[k][1]) for k in bmx.ROWS_RES_DTYPE.names] == want


def _lens(*a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def _programs():
    lits = (bmx.Lit * 40)(*[bmx.Lit(BASE, 0, 0, 10) for _ in range(40)])                       # every literal on the base field: no field limit in the way
    nine = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 9), 0, 0, 10) for k in range(40)])              # nine distinct fields besides the base
    flag2 = (bmx.Lit * 40)(*[bmx.Lit(BASE, 2 if k == 3 else 0, 0, 10) for k in range(40)])
    flagh = (bmx.Lit * 40)(*[bmx.Lit(BASE, (bmx.LIT_NOT | 0x80000000) if k == 0 else 0, 0, 10) for k in range(40)])
    eight = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 8), bmx.LIT_NOT if k % 3 == 0 else 0, -(1 << 63), (1 << 63) - 1) for k in range(40)])
    bad = [                                          # everything bmx_scan_where refuses (the list of test_where_cabi.py)
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
    bad, good = _programs()
    ids, vals, ts, res = (np.full(n, FILL, np.uint8) for n in (8 * 16, 8 * 8 * 16, 8 * 8 * 16, 40))
    ip, vp, tp, rp = (C.c_void_p(a.ctypes.data) for a in (ids, vals, ts, res))
    f8 = (C.c_uint32 * 9)(*range(200, 209))
    TS = bmx.ROWS_TS
    # (nfields, fields, flags, start_pos, cap, out_ids, out_val, out_ts, res)
    ok_tails = [(0, None, 0, 0, 16, ip, None, None, rp), (8, f8, TS, 3, 16, ip, vp, tp, rp), (2, f8, 0, 1 << 40, 16, ip, vp, None, rp), (8, f8, TS, 0, 0, None, None, None, rp)]

    def comm_tail(tail):
        return tail[:3] + (0,) + tail[3:]            # start_shard in front of start_pos

    def refused(prog, tail, text):
        """both mem modes with a NULL context, and a NULL communicator: the text lands in the handle kind's own word and leaves the other words alone"""
        NOF = bmx.AGG_NO_FIELD
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_comm_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None) == bmx.ERR_INVALID      # a known text in the communicator's word
            before_comm, before_vc = lib.bmx_comm_last_error(None), lib.bmx_vc_last_error(None)
            assert lib.bmx_where_rows(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID, text
            assert text in lib.bmx_last_error(None), (text, lib.bmx_last_error(None))
            assert lib.bmx_comm_last_error(None) == before_comm and lib.bmx_vc_last_error(None) == before_vc
        assert lib.bmx_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None, 0) == bmx.ERR_INVALID              # ... and one in the context's word
        before_ctx, before_vc = lib.bmx_last_error(None), lib.bmx_vc_last_error(None)
        assert lib.bmx_comm_where_rows(None, BASE, *prog, *comm_tail(tail)) == bmx.ERR_INVALID, text
        want = b"null communicator" if text == b"null context" else text
        assert want in lib.bmx_comm_last_error(None), (want, lib.bmx_comm_last_error(None))
        assert lib.bmx_last_error(None) == before_ctx and lib.bmx_vc_last_error(None) == before_vc

    # every refusal of the program, with arguments behind it that are fine
    for nc, lens, ls, text in bad:
        refused((nc, lens, ls), ok_tails[1], text)
    # the call's own refusals, with a program that is fine
    for prog in good:
        refused(prog, (9, f8, 0, 0, 16, ip, vp, tp, rp), b"more than BMX_ROWS_MAX_FIELDS")
        refused(prog, (1 << 31, f8, 0, 0, 0, None, None, None, rp), b"more than BMX_ROWS_MAX_FIELDS")
        refused(prog, (1, None, 0, 0, 16, ip, vp, tp, rp), b"null fields")
        refused(prog, (8, None, TS, 0, 0, None, None, None, rp), b"null fields")
        refused(prog, (2, f8, 2, 0, 16, ip, vp, tp, rp), b"unknown flag bits in flags")
        refused(prog, (0, None, TS | 0x80000000, 0, 0, None, None, None, rp), b"unknown flag bits in flags")
        refused(prog, (2, f8, TS, 0, 16, ip, vp, tp, None), b"null result record")
        refused(prog, (0, None, 0, 0, 0, None, None, None, None), b"null result record")
        refused(prog, (2, f8, TS, 0, 16, None, vp, tp, rp), b"null out_ids")
        refused(prog, (0, None, 0, 0, 1, None, None, None, rp), b"null out_ids")
        refused(prog, (2, f8, TS, 0, 16, ip, None, tp, rp), b"null out_val")
        refused(prog, (1, f8, 0, 0, 1, ip, None, None, rp), b"null out_val")
        refused(prog, (2, f8, TS, 0, 16, ip, vp, None, rp), b"null out_ts")
        for tail in ok_tails:
            for mem in (7, -1):
                assert lib.bmx_where_rows(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID
                assert b"bad mem kind" in lib.bmx_last_error(None)
            refused(prog, tail, b"null context")
    for a in (ids, vals, ts, res):
        assert (a == FILL).all(), "a refused call writes nothing"


def test_the_result_object():
    res = np.zeros((), bmx.ROWS_RES_DTYPE)
    res["n_match"] = 5; res["n_out"] = 2; res["next_pos"] = 17; res["layout"] = 3; res["next_shard"] = 1
    ids = np.arange(4, dtype=np.uint64); vals = np.arange(8, dtype=np.int64).reshape(2, 4); ts = vals + 100
    r = bmx.RowsResult(res, ids, vals, ts)
    assert (r.n_match, r.n_out, r.next_pos, r.layout, r.next_shard) == (5, 2, 17, 3, 1)
    assert r.ids.tolist() == [0, 1] and r.vals.tolist() == [[0, 1], [4, 5]] and r.ts.tolist() == [[100, 101], [104, 105]]
    assert bmx.RowsResult(res, ids, vals, None).ts is None
    c = bmx.RowsRes(); c.n_match = 1; c.n_out = 1; c.next_pos = 9
    assert bmx.RowsResult(c, ids, np.zeros((0, 4), np.int64), None).vals.shape == (0, 1)
    nf, farr, flags = bmx._rows_fields([3, 3, 9], True)
    assert (nf, list(farr), flags) == (3, [3, 3, 9], bmx.ROWS_TS) and bmx._rows_fields([], False)[0::2] == (0, 0)
