"""CPU-only checks of the ordered top-k surface (include/bmx_top.h): the two symbols exist and are listed in bmx.EXPORTS_TOP while bmx.EXPORTS keeps its 108
names, the record is the 16 bytes the header draws, every bad-argument case is refused before any device work — with a NULL context and a NULL communicator,
in both mem modes, writing nothing — and bmx.top_merge, the merge the sharded call documents, equals sorted()."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_scan_top", "bmx_comm_scan_top"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_TOP == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in bmx.EXPORTS, "bmx.EXPORTS mirrors bmx.h alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_top.h")).read()
    assert re.search(r'#include\s+"bmx.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == set(NEW)
    main = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert "#include \"bmx_top.h\"" not in main


def test_record_layout():
    assert C.sizeof(bmx.TopRec) == 16
    assert [f[0] for f in bmx.TopRec._fields_] == ["id", "val"]
    assert bmx.TOP_DTYPE.itemsize == 16 and list(bmx.TOP_DTYPE.names) == ["id", "val"]
    for name, _ in bmx.TopRec._fields_:
        assert getattr(bmx.TopRec, name).offset == bmx.TOP_DTYPE.fields[name][1]
    assert bmx.TOP_DESC == 1 and bmx.TOP_MAX_K == 4096


def _call(lib, nterms, terms, flags, after, k, out, mem, ctr):
    return lib.bmx_scan_top(None, nterms, terms, flags, after, k, out, ctr[0], ctr[1], mem)


def _ccall(lib, nterms, terms, flags, after, k, out, ctr):
    return lib.bmx_comm_scan_top(None, nterms, terms, flags, after, k, out, ctr[0], ctr[1])


def test_bad_arguments_are_refused(lib):
    terms = (bmx.Term * 9)(*[bmx.Term(7 + k, 0, 0, 10) for k in range(9)])
    out = np.zeros(4097, bmx.TOP_DTYPE)
    cnt = np.zeros(2, np.uint64)
    op = C.c_void_p(out.ctypes.data)
    ctr = (C.c_void_p(cnt.ctypes.data), C.c_void_p(cnt.ctypes.data + 8))
    cur = bmx.TopRec(5, 5)
    cp = C.cast(C.byref(cur), C.c_void_p)
    bad = [
        (0, terms, 0, None, 10, op),               # no term
        (9, terms, 0, None, 10, op),               # more than 8
        (1, None, 0, None, 10, op),                # NULL terms
        (1, terms, 0, None, 10, None),             # NULL out
        (1, terms, 0, None, 0, op),                # k == 0
        (1, terms, 0, cp, 4097, op),               # k > BMX_TOP_MAX_K
        (2, terms, 2, None, 10, op),               # unknown flag bits
        (2, terms, bmx.TOP_DESC | 0x80000000, cp, 10, op),
    ]
    for a in bad:
        for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE):
            assert _call(lib, *a, mem, ctr) == bmx.ERR_INVALID, a
            assert _call(lib, *a, mem, (None, None)) == bmx.ERR_INVALID, a
        assert _ccall(lib, *a, ctr) == bmx.ERR_INVALID, a
    # a bad mem kind, and well-formed arguments with no context / no communicator behind them
    for ok in ((2, terms, bmx.TOP_DESC, cp, 4096, op), (1, terms, 0, None, 1, op), (8, terms, 0, cp, 333, op)):
        assert _call(lib, *ok, 7, ctr) == bmx.ERR_INVALID
        assert _call(lib, *ok, bmx.MEM_HOST, ctr) == bmx.ERR_INVALID and _call(lib, *ok, bmx.MEM_DEVICE, ctr) == bmx.ERR_INVALID
        assert _ccall(lib, *ok, ctr) == bmx.ERR_INVALID
    assert not out.view(np.uint8).any() and not cnt.any(), "a refused call writes nothing"


def _key(desc):
    return lambda r: (-r[1] if desc else r[1], r[0])


@pytest.mark.parametrize("desc", [False, True])
def test_top_merge_equals_sorted(desc):
    rng = np.random.default_rng(11 + desc)
    for trial in range(60):
        nlists = int(rng.integers(0, 6))
        lists, union = [], []
        next_id = 0
        for _ in range(nlists):
            n = int(rng.choice([0, 0, 1, 3, 17, 200]))
            # heavy ties: few distinct values, at the ends of the domain too; ids unique over all lists, above 2^63 as well
            vals = rng.choice(np.array([-(2**53 - 1), -3, 0, 0, 1, 1, 1, 2**53 - 1], np.int64), n)
            ids = (np.arange(next_id, next_id + n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) if n else np.zeros(0, np.uint64)
            next_id += n
            recs = sorted(zip([int(x) for x in ids], [int(x) for x in vals]), key=_key(desc))
            union += recs
            a = np.zeros(n, bmx.TOP_DTYPE); a["id"] = [r[0] for r in recs]; a["val"] = [r[1] for r in recs]
            lists.append(a)
        want_all = sorted(union, key=_key(desc))
        for k in (1, 2, max(len(union) - 1, 1), max(len(union), 1), len(union) + 5, 4096):
            got = bmx.top_merge(lists, k, desc)
            assert got.dtype == bmx.TOP_DTYPE
            assert [(int(r["id"]), int(r["val"])) for r in got] == want_all[:k], (trial, k, desc)
    assert len(bmx.top_merge([], 5, desc)) == 0 and len(bmx.top_merge([np.zeros(0, bmx.TOP_DTYPE)], 5, desc)) == 0
