"""CPU-only checks of the field-to-field literals (include/bmx_where.h BMX_LIT_MINUS / BMX_LIT_SUBTRAHEND) at the C ABI: every malformed entry pair is refused
before any device work with a text of its own — on bmx_scan_where, on bmx_comm_scan_where and in either program of bmx_where_semijoin, with a NULL context or
communicator, writing nothing — and well-formed pair programs at each limit get past the program check: their error is the handle's, not a program's. (Without
the feature those are refused with "unknown flag bits".)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
BASE, INNER, LINK, KEY = 7, 70, 8, 71
MINUS, SUB, NOT = 4, 8, 1
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def _prog(*clauses):
    """clauses of raw (field, flags, lo, hi) entries -> (nclauses, clause_len, lits)"""
    flat = [bmx.Lit(*t) for c in clauses for t in c]
    return len(clauses), (C.c_uint32 * len(clauses))(*[len(c) for c in clauses]), (bmx.Lit * len(flat))(*flat)


def _pair(a, b, lo=0, hi=0, flags=0):
    return [(a, MINUS | flags, lo, hi), (b, SUB, 0, 0)]


def _bad(base):
    plain = (base, 0, 0, 10)
    return [
        (_prog([plain, (100, MINUS, 0, 0)]), b"BMX_LIT_MINUS entry ends its clause"),
        (_prog([(100, MINUS, 0, 0)], [(101, SUB, 0, 0)]), b"BMX_LIT_MINUS entry ends its clause"),                 # the next clause does not count
        (_prog([(100, MINUS, 0, 0), plain]), b"followed by no BMX_LIT_SUBTRAHEND"),
        (_prog([(100, MINUS, 0, 0), (101, MINUS, 0, 0), (102, SUB, 0, 0)]), b"followed by no BMX_LIT_SUBTRAHEND"),
        (_prog([(101, SUB, 0, 0), plain]), b"follows no BMX_LIT_MINUS"),
        (_prog([plain, (101, SUB, 0, 0)]), b"follows no BMX_LIT_MINUS"),
        (_prog(_pair(100, 101) + [(102, SUB, 0, 0)]), b"follows no BMX_LIT_MINUS"),
        (_prog([(100, MINUS, 0, 0), (101, SUB | NOT, 0, 0)]), b"BMX_LIT_SUBTRAHEND goes with no other flag"),
        (_prog([(100, MINUS, 0, 0), (101, SUB | MINUS, 0, 0), (102, SUB, 0, 0)]), b"BMX_LIT_SUBTRAHEND goes with no other flag"),
        (_prog([(100, MINUS, 0, 0), (101, SUB, 1, 0)]), b"lo = hi = 0"),
        (_prog([(100, MINUS, 0, 0), (101, SUB, 0, -1)]), b"lo = hi = 0"),
        (_prog(_pair(100, 100)), b"a field minus itself"),
        (_prog(_pair(base, base, 1, I64MAX)), b"a field minus itself"),
        (_prog(*[_pair(100 + k, 200 + k) * 1 + _pair(300 + k, 400 + k) for k in range(4)], _pair(500, 501)), b"no slot left for a field pair"),
        (_prog(*[[(100 + 2 * k, 0, 0, 1), (101 + 2 * k, 0, 0, 1)] for k in range(4)], _pair(100, 101)), b"no slot left for a field pair"),
        (_prog(*[_pair(100 + k, 200 + k) + _pair(300 + k, 400 + k) for k in range(4)], [(500, 0, 0, 1)]), b"more than 8 fields"),
        # what was refused before stays refused, with the text it had
        (_prog([(100, 2, 0, 0)]), b"unknown flag bits"),
        (_prog([(100, MINUS | 2, 0, 0), (101, SUB, 0, 0)]), b"unknown flag bits"),
        (_prog([(100, MINUS | 0x80000000, 0, 0), (101, SUB, 0, 0)]), b"unknown flag bits"),
        (_prog([(100, MINUS, 0, 0), (101, SUB | 0x80000000, 0, 0)]), b"unknown flag bits"),
        (_prog(_pair(100, 101) * 4 + [plain]), b"1..8 literals"),                                                    # 9 entries in a clause
        (_prog(*[_pair(100, 101) * 4] * 4, [plain]), b"32 literals"),
    ]


def _good(base):
    return [
        _prog(_pair(100, 101, 1, I64MAX)),
        _prog(_pair(100, 101) * 4),                                                                                 # 4 pairs in a clause
        _prog(*[_pair(100, 101, I64MIN, I64MAX, NOT) * 4] * 4),                                                     # 16 in a program: 32 entries
        _prog(*[_pair(100 + k, 200 + k) + _pair(300 + k, 400 + k) for k in range(4)]),                              # 8 pair slots
        _prog(*[_pair(100 + k, 200 + k) + _pair(200 + k, 100 + k) for k in range(4)]),                              # (A, B) and (B, A): 8 slots again
        _prog([(100 + k, 0, 0, 1) for k in range(7)], _pair(100, 101, -5, 5)),                                      # 7 plain fields plus 1 pair
        _prog([(base, 0, 0, 1)] + _pair(base, 100, I64MIN, 5) + _pair(100, base, 0, 0, NOT)),                       # either side the base field
    ]


def test_the_constants_and_the_literal(lib):
    hdr = open(os.path.join(ROOT, "include", "bmx_where.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in (("BMX_LIT_NOT", bmx.LIT_NOT), ("BMX_LIT_MINUS", bmx.LIT_MINUS), ("BMX_LIT_SUBTRAHEND", bmx.LIT_SUBTRAHEND)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, code).group(1)) == want, name
    assert (bmx.LIT_NOT, bmx.LIT_MINUS, bmx.LIT_SUBTRAHEND) == (NOT, MINUS, SUB)
    assert C.sizeof(bmx.Lit) == 24
    for word in ("BMX_LIT_MINUS", "BMX_LIT_SUBTRAHEND", "ninth slot", "probed in each"):
        assert word in hdr[:hdr.index("#ifndef")], "the header's comment describes the literal"


def test_the_python_program_builder():
    base, nc, lens, lits = bmx._where_args(7, [[(7, 1, 2), ((9, 7), 1, I64MAX), (11, 3, 4, True)], [((7, 9), I64MIN, 5, True)], [((9, 11), 0, 0, False)]])
    assert (base, nc, list(lens)) == (7, 3, [4, 2, 2])
    assert [(l.field, l.flags, l.lo, l.hi) for l in lits] == [
        (7, 0, 1, 2), (9, MINUS, 1, I64MAX), (7, SUB, 0, 0), (11, NOT, 3, 4), (7, MINUS | NOT, I64MIN, 5), (9, SUB, 0, 0), (9, MINUS, 0, 0), (11, SUB, 0, 0)]
    # the plain forms come out as they did
    base, nc, lens, lits = bmx._where_args(7, [[(7, 1, 2), (9, 3, 4, True)], [(11, -5, 5, False)]])
    assert (nc, list(lens)) == (2, [2, 1]) and [(l.field, l.flags, l.lo, l.hi) for l in lits] == [(7, 0, 1, 2), (9, NOT, 3, 4), (11, 0, -5, 5)]


def _buffers():
    out = np.full(64, FILL, np.uint8); cnt = np.full(32, FILL, np.uint8)
    return out, cnt, C.c_void_p(out.ctypes.data), C.c_void_p(cnt.ctypes.data)


def test_malformed_pairs_are_refused_each_with_its_text(lib):
    out, cnt, op, cp = _buffers()
    plain_o, plain_i = _prog([(BASE, 0, 0, 10)]), _prog([(INNER, 0, 0, 10)])
    for (p, text), (pi, _) in zip(_bad(BASE), _bad(INNER)):
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_scan_where(None, BASE, *p, op, 8, cp, mem) == bmx.ERR_INVALID, text
            assert text in lib.bmx_last_error(None), (text, lib.bmx_last_error(None))
            assert lib.bmx_where_semijoin(None, BASE, *p, LINK, 0, INNER, *plain_i, KEY, 64, op, 8, cp, mem) == bmx.ERR_INVALID
            assert text in lib.bmx_last_error(None) and b"outer program" in lib.bmx_last_error(None), (text, lib.bmx_last_error(None))
            assert lib.bmx_where_semijoin(None, BASE, *plain_o, LINK, 0, INNER, *pi, KEY, 64, op, 8, cp, mem) == bmx.ERR_INVALID
            assert text in lib.bmx_last_error(None) and b"inner program" in lib.bmx_last_error(None), (text, lib.bmx_last_error(None))
        assert lib.bmx_comm_scan_where(None, BASE, *p, op, 8, cp) == bmx.ERR_INVALID
        assert text in lib.bmx_comm_last_error(None), (text, lib.bmx_comm_last_error(None))
    assert (out == FILL).all() and (cnt == FILL).all(), "a refused call writes nothing"


def test_well_formed_pairs_pass_the_program_check(lib):
    """each limit reached, none passed: what stops the call is the missing handle"""
    out, cnt, op, cp = _buffers()
    for p, pi in zip(_good(BASE), _good(INNER)):
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_scan_where(None, BASE, *p, op, 8, cp, mem) == bmx.ERR_INVALID
            assert lib.bmx_last_error(None).endswith(b"null context"), lib.bmx_last_error(None)
            assert lib.bmx_where_semijoin(None, BASE, *p, LINK, 0, INNER, *pi, KEY, 64, op, 8, cp, mem) == bmx.ERR_INVALID
            assert lib.bmx_last_error(None).endswith(b"null context"), lib.bmx_last_error(None)
        assert lib.bmx_comm_scan_where(None, BASE, *p, op, 8, cp) == bmx.ERR_INVALID
        assert lib.bmx_comm_last_error(None).endswith(b"null communicator"), lib.bmx_comm_last_error(None)
    assert (out == FILL).all() and (cnt == FILL).all()
