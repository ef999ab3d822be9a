"""CPU-only checks of the aggregate-query surface (include/bmx.h "aggregate queries"): the two symbols exist and are listed, the record is the 48 bytes the
header draws, and every bad-argument case is refused before any device work — with a NULL context and a NULL communicator, like every other entry point."""
import ctypes as C

import numpy as np
import pytest

import bmx

NEW = ["bmx_scan_aggregate", "bmx_comm_scan_aggregate"]
NOF = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in bmx.EXPORTS, name
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108


def test_record_layout():
    assert C.sizeof(bmx.Agg) == 48
    assert [f[0] for f in bmx.Agg._fields_] == ["n_match", "n", "min", "max", "sum_lo", "sum_hi"]
    assert bmx.AGG_DTYPE.itemsize == 48 and list(bmx.AGG_DTYPE.names) == [f[0] for f in bmx.Agg._fields_]
    for name, _ in bmx.Agg._fields_:
        assert getattr(bmx.Agg, name).offset == bmx.AGG_DTYPE.fields[name][1]
    assert bmx.AGG_NO_FIELD == NOF and bmx.AGG_MAX_GROUPS == 65536


def test_records_become_python_numbers():
    recs = np.zeros(3, bmx.AGG_DTYPE)
    recs[0] = (5, 4, -3, 9, 2**64 - 7, -1)                     # sum = -7
    recs[1] = (2, 0, 2**63 - 1, -(2**63), 0, 0)                # nothing measured
    recs[2] = (4096, 4096, 2**53 - 1, 2**53 - 1, (4096 * (2**53 - 1)) % 2**64, (4096 * (2**53 - 1)) >> 64)
    a, b, c = bmx.agg_results(recs, 2)
    assert (a.n_match, a.n, a.min, a.max, a.sum) == (5, 4, -3, 9, -7)
    assert (b.n_match, b.n, b.min, b.max, b.sum) == (2, 0, None, None, 0)
    assert c.sum == 4096 * (2**53 - 1) and c.sum > 2**63
    # no measure field: n == n_match and min / max keep their empty values -> nothing was measured
    none = np.zeros(1, bmx.AGG_DTYPE); none[0] = (16, 16, 2**63 - 1, -(2**63), 0, 0)
    r = bmx.agg_results(none, 0)
    assert (r.n_match, r.n, r.min, r.max, r.sum) == (16, 16, None, None, 0)
    one = bmx.agg_results(recs, 0)
    assert isinstance(one, bmx.AggResult) and one == a and one != b


def _call(lib, nterms, terms, measure, group, group_lo, ngroups, out, mem):
    return lib.bmx_scan_aggregate(None, nterms, terms, measure, group, group_lo, ngroups, out, mem)


def _ccall(lib, nterms, terms, measure, group, group_lo, ngroups, out):
    return lib.bmx_comm_scan_aggregate(None, nterms, terms, measure, group, group_lo, ngroups, out)


def test_bad_arguments_are_refused(lib):
    terms = (bmx.Term * 9)(*[bmx.Term(7 + k, 0, 0, 10) for k in range(9)])
    out = np.zeros(65537, bmx.AGG_DTYPE)
    op = C.c_void_p(out.ctypes.data)
    bad = [
        (0, terms, NOF, NOF, 0, 0, op),            # no term
        (9, terms, NOF, NOF, 0, 0, op),            # more than 8
        (1, None, NOF, NOF, 0, 0, op),             # NULL terms
        (1, terms, 7, NOF, 0, 0, None),            # NULL out
        (1, terms, 7, 7, 0, 65537, op),            # more than BMX_AGG_MAX_GROUPS groups
        (1, terms, 7, NOF, 0, 1, op),              # groups without a group field
        (2, terms, 7, NOF, 5, 65536, op),
    ]
    for a in bad:
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert _call(lib, *a, mem) == bmx.ERR_INVALID, a
        assert _ccall(lib, *a) == bmx.ERR_INVALID, a
    # a bad mem kind, and well-formed arguments with no context / no communicator behind them
    ok = (2, terms, 8, 7, -5, 100, op)
    assert _call(lib, *ok, 7) == bmx.ERR_INVALID
    assert _call(lib, *ok, bmx.MEM_HOST) == bmx.ERR_INVALID and _call(lib, *ok, bmx.MEM_DEVICE) == bmx.ERR_INVALID
    assert _ccall(lib, *ok) == bmx.ERR_INVALID
    assert not out.view(np.uint8).any(), "a refused call writes nothing"
