"""CPU-only checks of the surface of include/bmx_reach.h: the four symbols exist and are listed in bmx.EXPORTS_REACH while bmx.EXPORTS keeps its 108 names and the
older lists stay as they were, the header declares exactly these four and compiles as C99, the record has the size and offsets the header draws, and every
bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with its own text (which names the edge
or the seed program) in the handle kind's own error word, leaving the other words and pattern-filled outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_reach", "bmx_where_reach_from", "bmx_comm_where_reach", "bmx_comm_where_reach_from"]
FILL = 0xA5
BASE, SEEDB, LINK, KEY, SEEDF = 7, 8, 9, 10, 11


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_REACH == NEW
    older = (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP + bmx.EXPORTS_ROWS
             + bmx.EXPORTS_SEMI + bmx.EXPORTS_JOIN + bmx.EXPORTS_JOIN_ROWS + bmx.EXPORTS_QUANT + bmx.EXPORTS_CLAIM + bmx.EXPORTS_UPDATE + bmx.EXPORTS_GROUP_MULTI)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in older, "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_SEMI == ["bmx_where_semijoin", "bmx_where_in", "bmx_comm_where_semijoin", "bmx_comm_where_in"]
    assert bmx.EXPORTS_JOIN == ["bmx_where_join_group", "bmx_where_map_group", "bmx_comm_where_join_group", "bmx_comm_where_map_group"]
    assert bmx.EXPORTS_GROUP_MULTI == ["bmx_where_group_multi", "bmx_comm_where_group_multi"] and bmx.EXPORTS_UPDATE == ["bmx_where_update", "bmx_comm_where_update"]
    for name in ("where_reach", "where_reach_from", "where_reach_dev", "where_reach_from_dev"):
        assert callable(getattr(bmx.Engine, name)), name
    assert callable(bmx.Comm.where_reach) and callable(bmx.Comm.where_reach_from)
    assert bmx.ReachResult.__slots__[:2] == ("ids", "depth")


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_reach.h")).read()
    assert re.search(r'#include\s+"bmx_where.h"', hdr) and re.search(r'#include\s+"bmx.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if older != "bmx_reach.h":
            text = open(os.path.join(ROOT, "include", older)).read()
            assert "where_reach" not in text and "bmx_reach" not in text and "BMX_REACH" not in text, older
    assert int(re.search(r"#define\s+BMX_REACH_OVERFLOW\s+(\d+)u", code).group(1)) == bmx.REACH_OVERFLOW == 1
    assert int(re.search(r"#define\s+BMX_REACH_MORE\s+(\d+)u", code).group(1)) == bmx.REACH_MORE == 2
    assert int(re.search(r"#define\s+BMX_REACH_MAX_DEPTH\s+(\d+)u", code).group(1)) == bmx.REACH_MAX_DEPTH == 255
    assert re.search(r"#define\s+BMX_REACH_MAX_SET\s+\(1u << 20\)", code) and bmx.REACH_MAX_SET == 1 << 20
    # what the header has to say in words
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    for words in ("Seeds are VALUES, not nodes", "Swapping link_field and key_field", 'says "edge program" or "seed program"', "least fixed point"):
        assert words in flat, words


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "reach_header.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    assert C.sizeof(bmx.ReachRes) == 40 == bmx.REACH_RES_DTYPE.itemsize
    want = [("n_match", 0), ("set_size", 8), ("n_seed", 16), ("n_edges", 24), ("rounds", 32), ("flags", 36)]
    assert [(f[0], getattr(bmx.ReachRes, f[0]).offset) for f in bmx.ReachRes._fields_] == want
    assert [(k, bmx.REACH_RES_DTYPE.fields[k][1]) for k in bmx.REACH_RES_DTYPE.names] == want


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
    bad_e, good_e = _programs(BASE)
    bad_s, good_s = _programs(SEEDB)
    ids = np.full(8 * 8, FILL, np.uint8)
    dep = np.full(8, FILL, np.uint8)
    res = np.full(40, FILL, np.uint8)
    vals = np.arange(8, dtype=np.int64)
    op, dp, rp, vp = (C.c_void_p(a.ctypes.data) for a in (ids, dep, res, vals))
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

    def reach(edge, seed, link=LINK, key=KEY, flags=0, seedf=SEEDF, depth=5, set_cap=64, out=op, outd=dp, cap=8, r=rp, text=()):
        a = (BASE, *edge, link, key, flags, SEEDB, *seed, seedf, depth, set_cap, out, outd, cap, r)
        refused(lambda mem: lib.bmx_where_reach(None, *a, mem), lambda: lib.bmx_comm_where_reach(None, *a), text)

    def reach_from(edge, link=LINK, key=KEY, flags=0, values=vp, nvalues=8, depth=5, set_cap=64, out=op, outd=dp, cap=8, r=rp, text=()):
        a = (BASE, *edge, link, key, flags, values, nvalues, depth, set_cap, out, outd, cap, r)
        refused(lambda mem: lib.bmx_where_reach_from(None, *a, mem), lambda: lib.bmx_comm_where_reach_from(None, *a), text)

    # every refusal of either program, with everything else fine; the text says which program
    for nc, lens, ls, text in bad_e:
        reach((nc, lens, ls), good_s[0], text=(text, b"edge program", b"where_reach: "))
        reach_from((nc, lens, ls), text=(text, b"edge program", b"where_reach_from: "))
    for nc, lens, ls, text in bad_s:
        reach(good_e[0], (nc, lens, ls), text=(text, b"seed program"))
    # the calls' own refusals, with programs that are fine
    for pe, ps in zip(good_e, good_s):
        reach(pe, ps, r=None, text=(b"null result record",))
        reach_from(pe, r=None, text=(b"null result record",))
        for sc in (0, bmx.REACH_MAX_SET + 1, 1 << 40):
            reach(pe, ps, set_cap=sc, text=(b"set_cap outside",))
            reach_from(pe, set_cap=sc, text=(b"set_cap outside",))
            reach_from(pe, nvalues=sc, text=(b"nvalues outside",))
        for d in (0, 256, 0xFFFFFFFF):
            reach(pe, ps, depth=d, text=(b"max_depth outside",))
            reach_from(pe, depth=d, text=(b"max_depth outside",))
        reach_from(pe, values=None, text=(b"null values",))
        reach(pe, ps, out=None, cap=1, text=(b"null out_ids",))
        reach_from(pe, out=None, cap=8, text=(b"null out_ids",))
        reach(pe, ps, outd=None, cap=1, text=(b"null out_depth",))
        reach_from(pe, outd=None, cap=8, text=(b"null out_depth",))
        for fl in (1, 2, 0x80000000):
            reach(pe, ps, flags=fl, text=(b"flags must be 0",))
            reach_from(pe, flags=fl, text=(b"flags must be 0",))
        reach(pe, ps, link=NOF, text=(b"no link field",))
        reach_from(pe, link=NOF, text=(b"no link field",))
        reach(pe, ps, key=NOF, text=(b"no key field",))
        reach_from(pe, key=NOF, text=(b"no key field",))
        reach(pe, ps, seedf=NOF, text=(b"no seed field",))
        for mem in (7, -1):
            assert lib.bmx_where_reach(None, BASE, *pe, LINK, KEY, 0, SEEDB, *ps, SEEDF, 5, 64, op, dp, 8, rp, mem) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
            assert lib.bmx_where_reach_from(None, BASE, *pe, LINK, KEY, 0, vp, 8, 5, 64, op, dp, 8, rp, mem) == bmx.ERR_INVALID and b"bad mem kind" in lib.bmx_last_error(None)
        # nothing wrong but the handle: the limits reached (set_cap, nvalues and max_depth at both ends, counting only, link == key)
        for sc, d, out, outd, cap in ((1, 1, op, dp, 8), (bmx.REACH_MAX_SET, 255, None, None, 0), (64, 255, op, dp, 0)):
            reach(pe, ps, set_cap=sc, depth=d, out=out, outd=outd, cap=cap, text=(b"null context",))
            reach_from(pe, set_cap=sc, depth=d, out=out, outd=outd, cap=cap, text=(b"null context",))
        reach_from(pe, nvalues=1, out=None, outd=None, cap=0, text=(b"null context",))
        reach(pe, ps, link=KEY, text=(b"null context",))
    assert (ids == FILL).all() and (dep == FILL).all() and (res == FILL).all() and (vals == np.arange(8)).all(), "a refused call writes nothing"
