"""CPU-only checks of the surface of include/bmx_group_multi.h: the two symbols exist and are listed in bmx.EXPORTS_GROUP_MULTI while bmx.EXPORTS keeps its 108
names and the older lists stay as they were, the header declares exactly these two and compiles as C99, the records have the sizes and offsets the header draws,
and every bad-argument case is refused before any device work — with a NULL context and a NULL communicator, in both mem modes, with its own text in the handle
kind's own error word, leaving the other words and pattern-filled outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx
from test_group_cabi import _programs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_group_multi", "bmx_comm_where_group_multi"]
FILL = 0xA5
BASE = 7
BIG = 2**53 - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_GROUP_MULTI == NEW
    older = (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP + bmx.EXPORTS_ROWS
             + bmx.EXPORTS_SEMI + bmx.EXPORTS_JOIN + bmx.EXPORTS_JOIN_ROWS + bmx.EXPORTS_QUANT + bmx.EXPORTS_CLAIM + bmx.EXPORTS_UPDATE)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in older, "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_GROUP == ["bmx_where_group", "bmx_comm_where_group"] and bmx.EXPORTS_UPDATE == ["bmx_where_update", "bmx_comm_where_update"]
    assert bmx.EXPORTS_JOIN == ["bmx_where_join_group", "bmx_where_map_group", "bmx_comm_where_join_group", "bmx_comm_where_map_group"]
    assert bmx.EXPORTS_QUANT == ["bmx_where_quantiles", "bmx_comm_where_quantiles"] and bmx.EXPORTS_WHERE == ["bmx_scan_where", "bmx_comm_scan_where"]
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "bmx.EXPORTS_GROUP_MULTI" in src, "build() looks for the new symbols"


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_group_multi.h")).read()
    for inc in ("bmx.h", "bmx_where.h", "bmx_group.h"):
        assert re.search(r'#include\s+"%s"' % re.escape(inc), hdr), inc
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if older != "bmx_group_multi.h":
            text = open(os.path.join(ROOT, "include", older)).read()
            assert "group_multi" not in text and "mgroup" not in text.lower(), older
    assert int(re.search(r"#define\s+BMX_MGROUP_MAX_KEYS\s+(\d+)u", code).group(1)) == bmx.MGROUP_MAX_KEYS == 4
    assert re.search(r"#define\s+BMX_MGROUP_MAX_CAP4\s+\(1u << 14\)", code) and bmx.MGROUP_MAX_CAP4 == 1 << 14


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "mgroup_header.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    assert bmx.MGROUP_DTYPE.itemsize == 80 and bmx.MGROUP_DTYPE.fields["key"][1] == 0 and bmx.MGROUP_DTYPE.fields["agg"][1] == 32
    assert bmx.MGROUP_DTYPE.fields["key"][0].shape == (4,)
    assert C.sizeof(bmx.GroupKey) == 24
    assert [(f[0], getattr(bmx.GroupKey, f[0]).offset) for f in bmx.GroupKey._fields_] == [("field", 0), ("flags", 4), ("origin", 8), ("width", 16)]
    assert C.sizeof(bmx.GroupRes) == 112 == bmx.GROUP_RES_DTYPE.itemsize and C.sizeof(bmx.Agg) == 48 == bmx.AGG_DTYPE.itemsize
    nk, arr = bmx._mgroup_keys([5, (6, -3, 10)])
    assert nk == 2 and (arr[0].field, arr[0].flags, arr[0].origin, arr[0].width) == (5, 0, 0, 1) and (arr[1].field, arr[1].origin, arr[1].width) == (6, -3, 10)


def _keys(*ks):
    return (bmx.GroupKey * max(len(ks), 1))(*[bmx.GroupKey(*k) for k in ks])


def test_bad_arguments_are_refused(lib):
    bad, good = _programs()
    recs = np.full(80 * 8, FILL, np.uint8)
    res = np.full(112, FILL, np.uint8)
    op, rp = C.c_void_p(recs.ctypes.data), C.c_void_p(res.ctypes.data)
    NOF = bmx.AGG_NO_FIELD
    one = _keys((9, 0, 0, 1))
    four = _keys((9, 0, 0, 1), (BASE, 0, -BIG, BIG), (9, 0, BIG, 2), (11, 0, 5, 60))
    ok_tails = [(NOF, 1, one, op, 8, rp), (BASE, 4, four, op, bmx.MGROUP_MAX_CAP4, rp), (9, 3, four, op, bmx.GROUP_MAX_CAP, rp), (9, 2, four, op, 1, rp)]

    def refused(prog, tail, text):
        """both mem modes with a NULL context, and a NULL communicator: the text lands in the handle kind's own word and leaves the other words alone"""
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_comm_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None) == bmx.ERR_INVALID      # a known text in the communicator's word
            before_comm, before_vc = lib.bmx_comm_last_error(None), lib.bmx_vc_last_error(None)
            assert lib.bmx_where_group_multi(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID, text
            assert text in lib.bmx_last_error(None), (text, lib.bmx_last_error(None))
            assert lib.bmx_comm_last_error(None) == before_comm and lib.bmx_vc_last_error(None) == before_vc
        assert lib.bmx_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None, 0) == bmx.ERR_INVALID              # ... and one in the context's word
        before_ctx, before_vc = lib.bmx_last_error(None), lib.bmx_vc_last_error(None)
        assert lib.bmx_comm_where_group_multi(None, BASE, *prog, *tail) == bmx.ERR_INVALID, text
        want = b"null communicator" if text == b"null context" else text
        assert want in lib.bmx_comm_last_error(None), (want, lib.bmx_comm_last_error(None))
        assert lib.bmx_last_error(None) == before_ctx and lib.bmx_vc_last_error(None) == before_vc

    # every refusal of the program, with arguments behind it that are fine
    for nc, lens, ls, text in bad:
        refused((nc, lens, ls), ok_tails[0], text)
    # the call's own refusals, with a program that is fine
    for prog in good:
        refused(prog, (BASE, 1, one, op, 8, None), b"null result record")
        refused(prog, (BASE, 1, one, None, 8, rp), b"null output")
        refused(prog, (BASE, 1, None, op, 8, rp), b"null keys")
        for nk in (0, 5, 1 << 31):
            refused(prog, (BASE, nk, four, op, 8, rp), b"nkeys outside")
        refused(prog, (BASE, 1, _keys((NOF, 0, 0, 1)), op, 8, rp), b"no key field")
        refused(prog, (BASE, 3, _keys((9, 0, 0, 1), (9, 0, 0, 1), (NOF, 0, 0, 1)), op, 8, rp), b"no key field")
        for fl in (1, 0x80000000):
            refused(prog, (BASE, 2, _keys((9, 0, 0, 1), (9, fl, 0, 1)), op, 8, rp), b"key flag bits")
        for w in (0, -1, BIG + 1, -(1 << 63)):
            refused(prog, (BASE, 2, _keys((9, 0, 0, 1), (9, 0, 0, w)), op, 8, rp), b"width outside")
        for o in (BIG + 1, -BIG - 1, (1 << 63) - 1, -(1 << 63)):
            refused(prog, (BASE, 1, _keys((9, 0, o, 1)), op, 8, rp), b"origin outside")
        for cap in (0, bmx.GROUP_MAX_CAP + 1, 1 << 40):
            refused(prog, (BASE, 3, four, op, cap, rp), b"cap outside")
        refused(prog, (BASE, 4, four, op, 0, rp), b"cap outside")
        for cap in (bmx.MGROUP_MAX_CAP4 + 1, bmx.GROUP_MAX_CAP):
            refused(prog, (BASE, 4, four, op, cap, rp), b"cap above BMX_MGROUP_MAX_CAP4")
        for tail in ok_tails:
            for mem in (7, -1):
                assert lib.bmx_where_group_multi(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID
                assert b"bad mem kind" in lib.bmx_last_error(None)
            refused(prog, tail, b"null context")
    assert (recs == FILL).all() and (res == FILL).all(), "a refused call writes nothing"


def test_the_result_object():
    res = np.zeros((), bmx.GROUP_RES_DTYPE)
    res["n_groups"] = 3; res["total"]["n_match"] = 9; res["total"]["n"] = 9; res["absent"]["n_match"] = 1; res["absent"]["n"] = 1
    recs = np.zeros(5, bmx.MGROUP_DTYPE); recs["key"][:3, :2] = [[-3, 9], [-3, 10], [8, -1]]; recs["agg"]["n_match"][:3] = [5, 2, 1]; recs["agg"]["n"][:3] = [5, 2, 1]
    g = bmx.MultiGroupResult(res, recs, 2)
    assert (g.n_groups, g.overflow, list(g.groups), g.groups[(-3, 10)].n_match, g.total.n_match, g.absent.n_match) == (3, False, [(-3, 9), (-3, 10), (8, -1)], 2, 9, 1)
    res["flags"] = bmx.GROUP_OVERFLOW; res["n_groups"] = 70
    g = bmx.MultiGroupResult(res, recs, 2)
    assert g.overflow and g.n_groups == 70 and not g.groups and len(g.records) == 0 and g.total.n_match == 9
    c = bmx.GroupRes(); c.n_groups = 1; c.total.n_match = 4; c.total.n = 4
    assert list(bmx.MultiGroupResult(c, recs, 1).groups) == [(-3,)]
