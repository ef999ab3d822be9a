"""CPU-only checks of the standing-query surface (include/bmx_watch.h): the six symbols exist and are listed in bmx.EXPORTS_WATCH while bmx.EXPORTS keeps its 108
names, the result record is the 32 bytes the header draws, the header compiles as C, and every bad-argument case is refused before any device work — with a NULL
context and a NULL communicator, in both mem modes, writing nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_watch_create", "bmx_watch_poll", "bmx_watch_destroy", "bmx_comm_watch_create", "bmx_comm_watch_poll", "bmx_comm_watch_destroy"]
FILL = 0xA5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_WATCH == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in bmx.EXPORTS + bmx.EXPORTS_WHERE + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC, "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_WHERE == ["bmx_scan_where", "bmx_comm_scan_where"] and bmx.EXPORTS_TOP == ["bmx_scan_top", "bmx_comm_scan_top"] and len(bmx.EXPORTS_VC_SYNC) == 6


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_watch.h")).read()
    assert re.search(r'#include\s+"bmx_where.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == set(NEW)
    for other in ("bmx.h", "bmx_where.h"):
        assert "bmx_watch" not in open(os.path.join(ROOT, "include", other)).read(), other
    # the constants of the header and of the binding are the same numbers
    for name, want in (("BMX_WATCH_MAX", bmx.WATCH_MAX), ("BMX_WATCH_RESET", bmx.WATCH_RESET), ("BMX_WATCH_OVERFLOW", bmx.WATCH_OVERFLOW)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, code).group(1)) == want, name


def test_record_layout():
    assert C.sizeof(bmx.WatchRes) == 32
    assert [(f[0], getattr(bmx.WatchRes, f[0]).offset) for f in bmx.WatchRes._fields_] == [("n_entered", 0), ("n_left", 8), ("n_match", 16), ("flags", 24), ("reserved", 28)]
    assert (bmx.WATCH_MAX, bmx.WATCH_RESET, bmx.WATCH_OVERFLOW) == (16, 1, 2)


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "watch_header.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lens(*a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def test_bad_programs_are_refused_by_create(lib):
    BASE = 7
    lits = (bmx.Lit * 40)(*[bmx.Lit(BASE, 0, 0, 10) for _ in range(40)])                       # every literal on the base field: no field limit in the way
    nine = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 9), 0, 0, 10) for k in range(40)])              # nine distinct fields besides the base
    flag2 = (bmx.Lit * 40)(*[bmx.Lit(BASE, 2 if k == 3 else 0, 0, 10) for k in range(40)])
    flagh = (bmx.Lit * 40)(*[bmx.Lit(BASE, (bmx.LIT_NOT | 0x80000000) if k == 0 else 0, 0, 10) for k in range(40)])
    wid = np.full(4, FILL, np.uint8).view(np.uint32)
    wp = C.cast(C.c_void_p(wid.ctypes.data), C.POINTER(C.c_uint32))
    bad = [
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
    for nc, lens, ls in bad:
        assert lib.bmx_watch_create(None, BASE, nc, lens, ls, wp) == bmx.ERR_INVALID, (nc, list(lens or []))
        assert lib.bmx_comm_watch_create(None, BASE, nc, lens, ls, wp) == bmx.ERR_INVALID, (nc, list(lens or []))
    # well-formed programs (each limit reached, none passed): a NULL watch_out, and no context / no communicator behind them
    eight = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 8), bmx.LIT_NOT if k % 3 == 0 else 0, -(1 << 63), (1 << 63) - 1) for k in range(40)])
    for nc, lens, ls in ((1, _lens(1), lits), (8, _lens(*[4] * 8), eight), (4, _lens(8, 8, 8, 8), eight), (8, _lens(*[1] * 8), nine)):
        for out in (None, wp):
            assert lib.bmx_watch_create(None, BASE, nc, lens, ls, out) == bmx.ERR_INVALID
            assert lib.bmx_comm_watch_create(None, BASE, nc, lens, ls, out) == bmx.ERR_INVALID
    assert (wid.view(np.uint8) == FILL).all(), "a refused call writes nothing"
    assert b"null" in lib.bmx_last_error(None) and b"null" in lib.bmx_comm_last_error(None)


def test_bad_poll_and_destroy_arguments_are_refused(lib):
    ent = np.full(64, FILL, np.uint8).view(np.uint64)
    lft = np.full(64, FILL, np.uint8).view(np.uint64)
    res = np.full(32, FILL, np.uint8)
    ep, lp, rp = C.c_void_p(ent.ctypes.data), C.c_void_p(lft.ctypes.data), C.c_void_p(res.ctypes.data)
    cases = [
        (ep, 8, lp, 8, None),        # NULL res
        (None, 8, lp, 8, rp),        # a NULL list with a cap
        (ep, 8, None, 1, rp),
        (None, 1, None, 1, rp),
        (ep, 8, lp, 8, rp),          # nothing wrong but the handle
        (None, 0, None, 0, rp),
    ]
    for e, ce, l, cl, r in cases:
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE, 7, -1):
            assert lib.bmx_watch_poll(None, 0, e, ce, l, cl, r, mem) == bmx.ERR_INVALID, (ce, cl, mem)
        assert lib.bmx_comm_watch_poll(None, 0, e, ce, l, cl, r) == bmx.ERR_INVALID, (ce, cl)
    for w in (0, 15, 16, 0xFFFFFFFF):
        assert lib.bmx_watch_destroy(None, w) == bmx.ERR_INVALID and lib.bmx_comm_watch_destroy(None, w) == bmx.ERR_INVALID
        assert lib.bmx_watch_poll(None, w, ep, 8, lp, 8, rp, bmx.MEM_HOST) == bmx.ERR_INVALID
    assert (ent.view(np.uint8) == FILL).all() and (lft.view(np.uint8) == FILL).all() and (res == FILL).all(), "a refused call writes nothing"


def test_the_poll_object():
    r = bmx.WatchRes(5, 2, 40, bmx.WATCH_RESET | bmx.WATCH_OVERFLOW, 0)
    p = bmx.WatchPoll(r, np.arange(3, dtype=np.uint64), np.arange(10, 20, dtype=np.uint64))
    assert (p.n_entered, p.n_left, p.n_match, p.reset, p.overflow) == (5, 2, 40, True, True)
    assert p.entered.tolist() == [0, 1, 2] and p.left.tolist() == [10, 11], "the lists are cut at the counts and at the caps"
    q = bmx.WatchPoll(bmx.WatchRes(0, 0, 7, 0, 0), np.zeros(4, np.uint64), np.zeros(4, np.uint64))
    assert len(q.entered) == 0 and len(q.left) == 0 and not q.reset and not q.overflow
