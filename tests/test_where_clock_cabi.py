"""CPU-only checks of the clock literals (include/bmx_where.h BMX_LIT_CLOCK / BMX_LIT_CLOCK_TOMB) at the C ABI: a clock bit beside BMX_LIT_MINUS or
BMX_LIT_SUBTRAHEND is refused before any device work with a text of its own — on bmx_scan_where, on bmx_comm_scan_where and in either program of
bmx_where_semijoin, with a NULL context or communicator, writing nothing; unknown flag bits stay unknown beside a clock bit; a clock literal that needs a ninth
slot is refused as a ninth field is; and well-formed programs with each state combination, on the base field and on a probed field, get past the program check:
their error is the handle's, not a program's. (Without the feature those are refused with "unknown flag bits".)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
BASE, INNER, LINK, KEY = 7, 70, 8, 71
NOT, MINUS, SUB, CLOCK, TOMB = 1, 4, 8, 16, 32
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


def _bad(base):
    plain = (base, 0, 0, 10)
    return [
        (_prog([(100, CLOCK | MINUS, 0, 0), (101, SUB, 0, 0)]), b"a clock literal goes with no BMX_LIT_MINUS"),
        (_prog([(100, TOMB | MINUS | NOT, 0, 0), (101, SUB, 0, 0)]), b"a clock literal goes with no BMX_LIT_MINUS"),
        (_prog([(base, CLOCK | TOMB | MINUS, 0, 0), (101, SUB, 0, 0)]), b"a clock literal goes with no BMX_LIT_MINUS"),
        (_prog([plain, (100, CLOCK | MINUS, 0, 0)]), b"a clock literal goes with no BMX_LIT_MINUS"),                  # before the pair's own checks
        (_prog([(100, MINUS, 0, 0), (101, SUB | CLOCK, 0, 0)]), b"a clock literal goes with no BMX_LIT_SUBTRAHEND"),
        (_prog([(100, MINUS, 0, 0), (101, SUB | TOMB, 0, 0)]), b"a clock literal goes with no BMX_LIT_SUBTRAHEND"),
        (_prog([(101, SUB | CLOCK | TOMB, 0, 0)]), b"a clock literal goes with no BMX_LIT_SUBTRAHEND"),
        # what was refused before stays refused, with the text it had
        (_prog([(100, 2, 0, 0)]), b"unknown flag bits"),
        (_prog([(100, 0x80000000, 0, 0)]), b"unknown flag bits"),
        (_prog([(100, CLOCK | 2, 0, 0)]), b"unknown flag bits"),
        (_prog([(100, TOMB | 0x80000000, 0, 0)]), b"unknown flag bits"),
        (_prog([(100, CLOCK | TOMB | NOT | 2, 0, 0)]), b"unknown flag bits"),
        (_prog([(100, CLOCK | MINUS | 2, 0, 0), (101, SUB, 0, 0)]), b"unknown flag bits"),
        (_prog([(100, 64, 0, 0)]), b"unknown flag bits"),
        # a ninth slot: eight probed fields and a clock literal on one more, on the base field, and eight clock slots and a plain field
        (_prog([(100 + k, 0, 0, 1) for k in range(8)], [(200, CLOCK, 0, 1)]), b"more than 8 fields besides the base field"),
        (_prog([(100 + k, 0, 0, 1) for k in range(8)], [(base, CLOCK, 0, 1)]), b"more than 8 fields besides the base field"),
        (_prog([(100 + k, CLOCK | TOMB, 0, 1) for k in range(8)], [(200, 0, 0, 1)]), b"more than 8 fields besides the base field"),
        (_prog([(100 + k, TOMB, 0, 1) for k in range(4)] + [(200 + k, MINUS, 0, 0) if j == 0 else (300 + k, SUB, 0, 0) for k in range(2) for j in range(2)],
               [(400 + k, CLOCK, 0, 1) for k in range(3)]), b"more than 8 fields besides the base field"),
        (_prog([(100, CLOCK, 0, 1)] * 9), b"1..8 literals"),
    ]


def _good(base):
    full = (I64MIN, I64MAX)
    return [
        _prog([(100, CLOCK, 5, I64MAX)]), _prog([(100, TOMB, *full)]), _prog([(100, CLOCK | TOMB, *full)]),                       # a probed field, each state combination
        _prog([(base, CLOCK, 5, I64MAX)]), _prog([(base, TOMB, *full)]), _prog([(base, CLOCK | TOMB, *full)]),                    # the base field
        _prog([(100, CLOCK | NOT, 9, 3)], [(base, CLOCK | TOMB | NOT, 0, 0)]),                                                    # NOT; lo > hi
        _prog([(100 + k, 0, 0, 1) for k in range(8)], [(100 + k, CLOCK, 0, 1) for k in range(8)]),                                # 8 fields: value and clock share a slot
        _prog([(100 + k, CLOCK | TOMB, 0, 1) for k in range(7)] + [(base, CLOCK, 0, 1)], [(base, 0, 0, 1)]),                      # 8 clock slots, one the base field's
        _prog([(100, MINUS, 0, 0), (101, SUB, 0, 0), (100, CLOCK, 0, 1), (101, TOMB, 0, 1), (100, 0, 0, 1)]),                     # a field in a pair, a clock and a value literal
        _prog(*[[(100 + k, CLOCK | (TOMB if k & 1 else 0) | (NOT if k & 2 else 0), k, 10 * k) for k in range(8)]] * 4),           # 32 literals
    ]


def test_the_constants_and_the_header(lib):
    hdr = open(os.path.join(ROOT, "include", "bmx_where.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in (("BMX_LIT_NOT", bmx.LIT_NOT), ("BMX_LIT_MINUS", bmx.LIT_MINUS), ("BMX_LIT_SUBTRAHEND", bmx.LIT_SUBTRAHEND), ("BMX_LIT_CLOCK", bmx.LIT_CLOCK),
                       ("BMX_LIT_CLOCK_TOMB", bmx.LIT_CLOCK_TOMB)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, code).group(1)) == want, name
    assert (bmx.LIT_CLOCK, bmx.LIT_CLOCK_TOMB) == (CLOCK, TOMB)
    assert C.sizeof(bmx.Lit) == 24 and lib.bmx_abi_version() == 4
    for word in ("BMX_LIT_CLOCK", "BMX_LIT_CLOCK_TOMB", "the field is deleted", "a row exists", "not clamped", "ONE slot and ONE"):
        assert word in hdr[:hdr.index("#ifndef")], "the header's comment describes the literal"


def _buffers():
    out = np.full(64, FILL, np.uint8); cnt = np.full(32, FILL, np.uint8)
    return out, cnt, C.c_void_p(out.ctypes.data), C.c_void_p(cnt.ctypes.data)


def test_malformed_clock_literals_are_refused_each_with_its_text(lib):
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


def test_well_formed_clock_literals_pass_the_program_check(lib):
    """each state combination on the base field and on a probed field, each limit reached, none passed: what stops the call is the missing handle"""
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
