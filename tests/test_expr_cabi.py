"""CPU-only checks of the surface of include/bmx_expr.h: the six symbols exist and are listed in bmx.EXPORTS_EXPR while the older lists stay as they were, the
header declares exactly these six and compiles as C99, the two records are 16 / 16 bytes, and every bad-argument case is refused before any device work — with
a NULL context and a NULL communicator, in both mem modes, each with its own text in the handle kind's own error word, leaving pattern-filled outputs
untouched. A well-formed call gets past every argument check: the error it ends with is the handle's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_where_aggregate_expr", "bmx_where_group_expr", "bmx_where_quantiles_expr", "bmx_comm_where_aggregate_expr", "bmx_comm_where_group_expr",
       "bmx_comm_where_quantiles_expr"]
FILL = 0xA5
BASE = 7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_EXPR == NEW
    older = (bmx.EXPORTS + bmx.EXPORTS_TOP + bmx.EXPORTS_VC_SYNC + bmx.EXPORTS_WHERE + bmx.EXPORTS_WATCH + bmx.EXPORTS_WHERE_AGG + bmx.EXPORTS_GROUP + bmx.EXPORTS_ROWS
             + bmx.EXPORTS_SEMI + bmx.EXPORTS_JOIN + bmx.EXPORTS_JOIN_ROWS + bmx.EXPORTS_QUANT + bmx.EXPORTS_CLAIM + bmx.EXPORTS_UPDATE + bmx.EXPORTS_GROUP_MULTI
             + bmx.EXPORTS_REACH + bmx.EXPORTS_FIRST + bmx.EXPORTS_GROUP_TOP)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in older, "the older lists mirror the older headers alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_QUANT == ["bmx_where_quantiles", "bmx_comm_where_quantiles"] and bmx.EXPORTS_GROUP == ["bmx_where_group", "bmx_comm_where_group"]
    assert bmx.EXPORTS_WHERE_AGG == ["bmx_where_aggregate", "bmx_where_top", "bmx_comm_where_aggregate", "bmx_comm_where_top"]


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_expr.h")).read()
    for brought in ("bmx.h", "bmx_where.h", "bmx_group.h", "bmx_quant.h"):
        assert re.search(r'#include\s+"%s"' % re.escape(brought), hdr), brought
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == sorted(NEW)
    for older in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if older != "bmx_expr.h":
            assert "bmx_expr" not in open(os.path.join(ROOT, "include", older)).read(), older
    assert [int(re.search(r"#define\s+BMX_EXPR_%s\s+(\d+)u" % k, code).group(1)) for k in ("ADD", "SUB", "MUL")] == [bmx.EXPR_ADD, bmx.EXPR_SUB, bmx.EXPR_MUL] == [1, 2, 3]


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "expr_header.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_record_layout():
    want = [("a", 0), ("b", 4), ("op", 8), ("reserved", 12)]
    assert C.sizeof(bmx.Expr) == 16 and [(f[0], getattr(bmx.Expr, f[0]).offset) for f in bmx.Expr._fields_] == want
    want = [("n_undef", 0), ("n_range", 8)]
    assert C.sizeof(bmx.ExprRes) == 16 == bmx.EXPR_RES_DTYPE.itemsize
    assert [(f[0], getattr(bmx.ExprRes, f[0]).offset) for f in bmx.ExprRes._fields_] == want == [(k, bmx.EXPR_RES_DTYPE.fields[k][1]) for k in bmx.EXPR_RES_DTYPE.names]


def _lens(*a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def _expr(a=11, op=bmx.EXPR_MUL, b=12, reserved=0):
    e = bmx.Expr(a, "*", b)
    e.op, e.reserved = op, reserved
    return e


def _programs():
    lits = (bmx.Lit * 40)(*[bmx.Lit(BASE, 0, 0, 10) for _ in range(40)])                       # every literal on the base field: no field limit in the way
    nine = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 9), 0, 0, 10) for k in range(40)])              # nine distinct fields besides the base
    flag2 = (bmx.Lit * 40)(*[bmx.Lit(BASE, 2 if k == 3 else 0, 0, 10) for k in range(40)])
    eight = (bmx.Lit * 40)(*[bmx.Lit(100 + (k % 8), bmx.LIT_NOT if k % 3 == 0 else 0, -(1 << 63), (1 << 63) - 1) for k in range(40)])
    bad = [                                          # the list of test_where_cabi.py
        (0, _lens(1), lits, b"1..8 clauses"),
        (9, _lens(*[1] * 9), lits, b"1..8 clauses"),
        (1, _lens(0), lits, b"1..8 literals"),
        (1, _lens(9), lits, b"1..8 literals"),
        (5, _lens(8, 8, 8, 8, 1), lits, b"32 literals"),
        (2, _lens(8, 1), nine, b"8 fields"),
        (1, _lens(4), flag2, b"flag bits"),
        (1, None, lits, b"null clause_len or lits"),
        (1, _lens(1), None, b"null clause_len or lits"),
    ]
    good = [(1, _lens(1), lits), (8, _lens(*[4] * 8), eight)]     # (eight probed fields: the operands take no slot of the program)
    return bad, good


def test_bad_arguments_are_refused(lib):
    bad, good = _programs()
    recs = np.full(56 * 16, FILL, np.uint8)
    res = np.full(112, FILL, np.uint8)
    xres = np.full(16, FILL, np.uint8)
    op, rp, xp = C.c_void_p(recs.ctypes.data), C.c_void_p(res.ctypes.data), C.c_void_p(xres.ctypes.data)
    NOF = bmx.AGG_NO_FIELD
    q1 = (bmx.QuantQ * 1)(bmx.QuantQ(1, 2))
    ok = _expr()

    def ptr(e):
        return None if e is None else C.cast(C.byref(e), C.c_void_p)

    # the three forms: (single-context function, sharded function, tail behind the expression, that tail's last argument in front of mem)
    def forms(e, agg_tail=(NOF, 0, 0, op, xp), grp_tail=(9, op, 8, rp, xp), q_tail=(1, q1, op, rp, xp)):
        return [(lib.bmx_where_aggregate_expr, lib.bmx_comm_where_aggregate_expr, (ptr(e),) + agg_tail),
                (lib.bmx_where_group_expr, lib.bmx_comm_where_group_expr, (ptr(e),) + grp_tail),
                (lib.bmx_where_quantiles_expr, lib.bmx_comm_where_quantiles_expr, (ptr(e),) + q_tail)]

    def refused(fn, cfn, prog, tail, text):
        """both mem modes with a NULL context, and a NULL communicator: the text lands in the handle kind's own word and leaves the other words alone"""
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert lib.bmx_comm_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None) == bmx.ERR_INVALID      # a known text in the communicator's word
            before_comm, before_vc = lib.bmx_comm_last_error(None), lib.bmx_vc_last_error(None)
            assert fn(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID, text
            assert text in lib.bmx_last_error(None), (text, lib.bmx_last_error(None))
            assert lib.bmx_comm_last_error(None) == before_comm and lib.bmx_vc_last_error(None) == before_vc
        assert lib.bmx_where_aggregate(None, BASE, 0, None, None, NOF, NOF, 0, 0, None, 0) == bmx.ERR_INVALID              # ... and one in the context's word
        before_ctx, before_vc = lib.bmx_last_error(None), lib.bmx_vc_last_error(None)
        assert cfn(None, BASE, *prog, *tail) == bmx.ERR_INVALID, text
        want = b"null communicator" if text == b"null context" else text
        assert want in lib.bmx_comm_last_error(None), (want, lib.bmx_comm_last_error(None))
        assert lib.bmx_last_error(None) == before_ctx and lib.bmx_vc_last_error(None) == before_vc

    # every refusal of the program, with an expression and arguments behind it that are fine
    for nc, lens, ls, text in bad:
        for fn, cfn, tail in forms(ok):
            refused(fn, cfn, (nc, lens, ls), tail, text)
    for prog in good:
        # the expression's own refusals, each with its text
        for e, text in [(None, b"null measure expression"), (_expr(op=0), b"op outside"), (_expr(op=4), b"op outside"), (_expr(op=0xFFFFFFFF), b"op outside"),
                        (_expr(reserved=1), b"reserved must be 0"), (_expr(a=NOF), b"operand a is no field"), (_expr(b=NOF), b"operand b is no field")]:
            for fn, cfn, tail in forms(e):
                refused(fn, cfn, prog, tail, text)
        texts = {t for t in (b"null measure expression", b"op outside", b"reserved must be 0", b"operand a is no field", b"operand b is no field")}
        assert len(texts) == 5
        # every refusal of the plain forms, with an expression that is fine
        fa, ca, _ = forms(ok)[0]
        refused(fa, ca, prog, (ptr(ok), NOF, 0, 0, None, xp), b"null output")
        refused(fa, ca, prog, (ptr(ok), 9, 0, bmx.AGG_MAX_GROUPS + 1, op, xp), b"more than BMX_AGG_MAX_GROUPS")
        refused(fa, ca, prog, (ptr(ok), NOF, 0, 4, op, xp), b"groups without a group field")
        fg, cg, _ = forms(ok)[1]
        refused(fg, cg, prog, (ptr(ok), 9, op, 8, None, xp), b"null result record")
        refused(fg, cg, prog, (ptr(ok), 9, op, 0, rp, xp), b"cap outside")
        refused(fg, cg, prog, (ptr(ok), 9, op, bmx.GROUP_MAX_CAP + 1, rp, xp), b"cap outside")
        refused(fg, cg, prog, (ptr(ok), 9, None, 8, rp, xp), b"null output")
        refused(fg, cg, prog, (ptr(ok), NOF, op, 8, rp, xp), b"no group field")
        fq, cq, _ = forms(ok)[2]
        refused(fq, cq, prog, (ptr(ok), 0, q1, op, rp, xp), b"nq outside")
        refused(fq, cq, prog, (ptr(ok), 9, q1, op, rp, xp), b"nq outside")
        refused(fq, cq, prog, (ptr(ok), 1, None, op, rp, xp), b"null qs")
        refused(fq, cq, prog, (ptr(ok), 1, q1, None, rp, xp), b"null output")
        refused(fq, cq, prog, (ptr(ok), 1, (bmx.QuantQ * 1)(bmx.QuantQ(3, 2)), op, rp, xp), b"a quantile outside")
        # well-formed calls get past the argument checks: what is left is the mem kind and the handle. Either operand may be the base field, a field of the
        # program or one nobody names; a == b; xres (and the quantiles' res) may be NULL
        for e in (ok, _expr(a=BASE, b=BASE), _expr(a=100, b=BASE, op=bmx.EXPR_SUB), _expr(a=55, b=55, op=bmx.EXPR_ADD)):
            for x in (xp, None):
                for fn, cfn, tail in forms(e, (9, -5, 1025, op, x), (BASE, op, bmx.GROUP_MAX_CAP, rp, x), (1, q1, op, None, x)):
                    for mem in (7, -1):
                        assert fn(None, BASE, *prog, *tail, mem) == bmx.ERR_INVALID
                        assert b"bad mem kind" in lib.bmx_last_error(None)
                    refused(fn, cfn, prog, tail, b"null context")
    assert (recs == FILL).all() and (res == FILL).all() and (xres == FILL).all(), "a refused call writes nothing"
