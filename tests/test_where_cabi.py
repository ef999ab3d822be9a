"""CPU-only checks of the boolean-filter surface (include/bmx_where.h): the two symbols exist and are listed in bmx.EXPORTS_WHERE while bmx.EXPORTS keeps its 108
names, the literal is the 24 bytes the header draws, and every bad-argument case is refused before any device work — with a NULL context and a NULL
communicator, in both mem modes, writing nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_scan_where", "bmx_comm_scan_where"]
FILL = 0xA5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_WHERE == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in bmx.EXPORTS, "bmx.EXPORTS mirrors bmx.h alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_where.h")).read()
    assert re.search(r'#include\s+"bmx.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == set(NEW)
    main = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert "#include \"bmx_where.h\"" not in main
    # the constants of the header and of the binding are the same numbers
    for name, want in (("BMX_LIT_NOT", bmx.LIT_NOT), ("BMX_WHERE_MAX_CLAUSES", bmx.WHERE_MAX_CLAUSES), ("BMX_WHERE_MAX_LITS", bmx.WHERE_MAX_LITS),
                       ("BMX_WHERE_MAX_FIELDS", bmx.WHERE_MAX_FIELDS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, code).group(1)) == want, name


def test_literal_layout():
    assert C.sizeof(bmx.Lit) == 24 == C.sizeof(bmx.Term)
    assert [(f[0], getattr(bmx.Lit, f[0]).offset) for f in bmx.Lit._fields_] == [("field", 0), ("flags", 4), ("lo", 8), ("hi", 16)]
    assert (bmx.LIT_NOT, bmx.WHERE_MAX_CLAUSES, bmx.WHERE_MAX_LITS, bmx.WHERE_MAX_FIELDS) == (1, 8, 32, 8)


def _lens(*a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def test_bad_arguments_are_refused(lib):
    BASE = 7
    lits = (bmx.Lit * 40)(*[bmx.Lit(BASE, 0, 0, 10) for _ in range(40)])                       # every literal on the base field: no field limit in the way
    nine = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 9), 0, 0, 10) for k in range(40)])              # nine distinct fields besides the base
    flag2 = (bmx.Lit * 40)(*[bmx.Lit(BASE, 2 if k == 3 else 0, 0, 10) for k in range(40)])
    flagh = (bmx.Lit * 40)(*[bmx.Lit(BASE, (bmx.LIT_NOT | 0x80000000) if k == 0 else 0, 0, 10) for k in range(40)])
    out = np.full(64, FILL, np.uint8).view(np.uint64)
    cnt = np.full(8, FILL, np.uint8).view(np.uint64)
    op, cp = C.c_void_p(out.ctypes.data), C.c_void_p(cnt.ctypes.data)
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
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_scan_where(None, BASE, nc, lens, ls, op, 8, cp, mem) == bmx.ERR_INVALID, (nc, list(lens or []))
            assert lib.bmx_scan_where(None, BASE, nc, lens, ls, None, 0, None, mem) == bmx.ERR_INVALID, (nc, list(lens or []))
        assert lib.bmx_comm_scan_where(None, BASE, nc, lens, ls, op, 8, cp) == bmx.ERR_INVALID, (nc, list(lens or []))
    # a bad mem kind, and well-formed programs (each limit reached, none passed) with no context / no communicator behind them
    eight = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 8), bmx.LIT_NOT if k % 3 == 0 else 0, -(1 << 63), (1 << 63) - 1) for k in range(40)])
    for nc, lens, ls in ((1, _lens(1), lits), (8, _lens(*[4] * 8), eight), (4, _lens(8, 8, 8, 8), eight), (8, _lens(*[1] * 8), nine)):
        assert lib.bmx_scan_where(None, BASE, nc, lens, ls, op, 8, cp, 7) == bmx.ERR_INVALID
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_scan_where(None, BASE, nc, lens, ls, op, 8, cp, mem) == bmx.ERR_INVALID
        assert lib.bmx_comm_scan_where(None, BASE, nc, lens, ls, op, 8, cp) == bmx.ERR_INVALID
    assert (out.view(np.uint8) == FILL).all() and (cnt.view(np.uint8) == FILL).all(), "a refused call writes nothing"


def test_the_python_program_builder():
    base, nc, lens, lits = bmx._where_args(7, [[(7, 1, 2), (9, 3, 4, True)], [(11, -5, 5, False)]])
    assert (base, nc, list(lens)) == (7, 2, [2, 1])
    assert [(l.field, l.flags, l.lo, l.hi) for l in lits] == [(7, 0, 1, 2), (9, bmx.LIT_NOT, 3, 4), (11, 0, -5, 5)]
