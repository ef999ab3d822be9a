"""CPU-only checks of the surface of include/bmx_update.h: the two symbols exist and are listed in bmx.EXPORTS_UPDATE while bmx.EXPORTS keeps its 108 names and
every older list stays as its own cabi test states it, the header declares exactly these two and compiles as C99 next to bmx.h, the record has the size and
offsets the header draws, and every bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with
the code the header names, leaving pattern-filled outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_update", "bmx_comm_where_update"]
FILL = 0xA5
BASE, TARGET, SRC = 7, 8, 9
BIG = 2**53 - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_UPDATE == NEW
    older = (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP + bmx.EXPORTS_ROWS
             + bmx.EXPORTS_SEMI + bmx.EXPORTS_JOIN + bmx.EXPORTS_JOIN_ROWS + bmx.EXPORTS_QUANT + bmx.EXPORTS_CLAIM)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in older, "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    # every older list as its own cabi test states it
    assert bmx.EXPORTS_TOP == ["bmx_scan_top", "bmx_comm_scan_top"]
    assert bmx.EXPORTS_VC_SYNC == ["bmx_vc_rec_digest", "bmx_vc_info", "bmx_vc_digest", "bmx_vc_frontier", "bmx_vc_export_rows", "bmx_vc_merge_records"]
    assert bmx.EXPORTS_WHERE == ["bmx_scan_where", "bmx_comm_scan_where"]
    assert bmx.EXPORTS_WATCH == ["bmx_watch_create", "bmx_watch_poll", "bmx_watch_destroy", "bmx_comm_watch_create", "bmx_comm_watch_poll", "bmx_comm_watch_destroy"]
    assert bmx.EXPORTS_WHERE_AGG == ["bmx_where_aggregate", "bmx_where_top", "bmx_comm_where_aggregate", "bmx_comm_where_top"]
    assert bmx.EXPORTS_GROUP == ["bmx_where_group", "bmx_comm_where_group"]
    assert bmx.EXPORTS_ROWS == ["bmx_where_rows", "bmx_comm_where_rows"]
    assert bmx.EXPORTS_SEMI == ["bmx_where_semijoin", "bmx_where_in", "bmx_comm_where_semijoin", "bmx_comm_where_in"]
    assert bmx.EXPORTS_JOIN == ["bmx_where_join_group", "bmx_where_map_group", "bmx_comm_where_join_group", "bmx_comm_where_map_group"]
    assert bmx.EXPORTS_JOIN_ROWS == ["bmx_where_join_rows", "bmx_where_map_rows", "bmx_comm_where_join_rows", "bmx_comm_where_map_rows"]
    assert bmx.EXPORTS_QUANT == ["bmx_where_quantiles", "bmx_comm_where_quantiles"]
    assert bmx.EXPORTS_CLAIM == ["bmx_selfcheck_claim", "bmx_get_claim_mode"]
    for name in older:
        assert hasattr(lib, name), name


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_update.h")).read()
    assert re.search(r'#include\s+"bmx.h"', hdr) and re.search(r'#include\s+"bmx_where.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if older != "bmx_update.h":
            text = open(os.path.join(ROOT, "include", older)).read()
            assert "where_update" not in text and "bmx_upd" not in text and "BMX_UPD" not in text, older
    for name, want in (("SET", bmx.UPD_SET), ("DELETE", bmx.UPD_DELETE), ("COPY", bmx.UPD_COPY), ("ADD", bmx.UPD_ADD), ("FORCE", bmx.UPD_FORCE)):
        assert int(re.search(r"#define\s+BMX_UPD_%s\s+(\d+)u" % name, code).group(1)) == want
    assert (bmx.UPD_SET, bmx.UPD_DELETE, bmx.UPD_COPY, bmx.UPD_ADD, bmx.UPD_FORCE) == (0, 1, 2, 3, 1)
    assert re.search(r"#define\s+BMX_UPD_MAX_CAP\s+\(1ull << 24\)", code) and bmx.UPD_MAX_CAP == 1 << 24 == bmx.MAX_BATCH


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "update_header.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    assert C.sizeof(bmx.UpdRes) == 72 == bmx.UPD_RES_DTYPE.itemsize
    want = [("n_match", 0), ("n_nosrc", 8), ("n_range", 16), ("n_sent", 24), ("n_applied", 32), ("n_rows", 40), ("next_pos", 48), ("layout", 56), ("next_shard", 64), ("reserved", 68)]
    assert [(f[0], getattr(bmx.UpdRes, f[0]).offset) for f in bmx.UpdRes._fields_] == want
    assert [(k, bmx.UPD_RES_DTYPE.fields[k][1]) for k in bmx.UPD_RES_DTYPE.names] == want


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
    ids = np.full(8 * 8, FILL, np.uint8)
    res = np.full(72, FILL, np.uint8)
    ip, rp = C.c_void_p(ids.ctypes.data), C.c_void_p(res.ctypes.data)
    NOF = bmx.AGG_NO_FIELD

    def refused(prog, code, text, op=bmx.UPD_SET, operand=1, ts=5, flags=0, cap=8, out=ip, r=rp, src=SRC):
        """both mem modes with a NULL context, and a NULL communicator: the code, and the text in the handle kind's own word, which leaves the other words alone"""
        head = (BASE, *prog, TARGET, op, src, operand, ts, flags)
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_comm_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None) == bmx.ERR_INVALID      # a known text in the communicator's word
            before_comm, before_vc = lib.bmx_comm_last_error(None), lib.bmx_vc_last_error(None)
            assert lib.bmx_where_update(None, *head, 0, cap, out, r, mem) == code, text
            assert text in lib.bmx_last_error(None), (text, lib.bmx_last_error(None))
            assert lib.bmx_comm_last_error(None) == before_comm and lib.bmx_vc_last_error(None) == before_vc
        assert lib.bmx_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None, 0) == bmx.ERR_INVALID              # ... and one in the context's word
        before_ctx, before_vc = lib.bmx_last_error(None), lib.bmx_vc_last_error(None)
        assert lib.bmx_comm_where_update(None, *head, 0, 0, cap, out, r) == code, text
        t = b"null communicator" if text == b"null context" else text
        assert t in lib.bmx_comm_last_error(None), (t, lib.bmx_comm_last_error(None))
        assert lib.bmx_last_error(None) == before_ctx and lib.bmx_vc_last_error(None) == before_vc

    for nc, lens, ls, text in bad:                   # every refusal of the program, with everything else fine
        refused((nc, lens, ls), bmx.ERR_INVALID, text)
    for p in good:
        for op in (4, 5, 0x80000000, 0xFFFFFFFF):
            refused(p, bmx.ERR_INVALID, b"unknown op", op=op)
        for flags in (2, 4, 0x80000000, bmx.UPD_FORCE | 8):
            refused(p, bmx.ERR_INVALID, b"unknown flag bits", flags=flags)
        refused(p, bmx.ERR_INVALID, b"BMX_UPD_DELETE needs BMX_UPD_FORCE", op=bmx.UPD_DELETE)
        for cap in (bmx.UPD_MAX_CAP + 1, 1 << 40):
            refused(p, bmx.ERR_INVALID, b"cap above BMX_UPD_MAX_CAP", cap=cap)
        refused(p, bmx.ERR_INVALID, b"null result record", r=None)
        for ts in (-1, BIG + 1, -(1 << 63), (1 << 63) - 1):
            refused(p, bmx.ERR_RANGE, b"ts outside", ts=ts)
        for op in (bmx.UPD_SET, bmx.UPD_ADD):
            for operand in (BIG + 1, -BIG - 1, -(1 << 63), (1 << 63) - 1):
                refused(p, bmx.ERR_RANGE, b"|operand| > 2^53-1", op=op, operand=operand)
        for mem in (7, -1):
            assert lib.bmx_where_update(None, BASE, *p, TARGET, bmx.UPD_SET, SRC, 1, 5, 0, 0, 8, ip, rp, mem) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
        # nothing wrong but the handle: the limits reached, the operand ignored where the op does not read it, the pointer that is not needed missing
        refused(p, bmx.ERR_INVALID, b"null context")
        refused(p, bmx.ERR_INVALID, b"null context", ts=0, operand=BIG)
        refused(p, bmx.ERR_INVALID, b"null context", ts=BIG, operand=-BIG, op=bmx.UPD_ADD, flags=bmx.UPD_FORCE)
        refused(p, bmx.ERR_INVALID, b"null context", op=bmx.UPD_DELETE, flags=bmx.UPD_FORCE, operand=1 << 60)
        refused(p, bmx.ERR_INVALID, b"null context", op=bmx.UPD_COPY, operand=-(1 << 63), src=BASE)
        refused(p, bmx.ERR_INVALID, b"null context", cap=bmx.UPD_MAX_CAP, out=None)
        refused(p, bmx.ERR_INVALID, b"null context", cap=0, out=None)
    assert (ids == FILL).all() and (res == FILL).all(), "a refused call writes nothing"
