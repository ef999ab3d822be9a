"""CPU-only checks of the vector-clock table's reconciliation surface (include/bmx_vc_sync.h): the six symbols exist and are listed in bmx.EXPORTS_VC_SYNC
while bmx.EXPORTS keeps its 108 names, the record is the 64 bytes the header draws, the row digest of the library equals a restatement in plain Python
integers and the numpy one in the package, every bad-argument case is refused before any device work — with a NULL table, in both mem modes, writing
nothing and touching no other handle's error word — and the premise of the GPU reconcile test holds on the oracle alone: two replicas that pull from
each other hold identical rows within three rounds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bmx
from oracle.oracle import OracleVC
from vc_sync_model import replica_merges, model_rows, merge_recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bmx_vc_rec_digest", "bmx_vc_info", "bmx_vc_digest", "bmx_vc_frontier", "bmx_vc_export_rows", "bmx_vc_merge_records"]
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


def test_new_symbols_are_exported_and_listed(lib):
    assert bmx.EXPORTS_VC_SYNC == NEW
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in bmx.EXPORTS, "bmx.EXPORTS mirrors bmx.h alone"
    assert lib.bmx_abi_version() == 4
    assert len(bmx.EXPORTS) == len(set(bmx.EXPORTS)) == 108
    assert bmx.EXPORTS_TOP == ["bmx_scan_top", "bmx_comm_scan_top"]


def test_the_new_header_declares_exactly_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "bmx_vc_sync.h")).read()
    assert re.search(r'#include\s+"bmx.h"', hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(bmx_[a-z_0-9]+)\s*\(", code)) == set(NEW)
    main = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert "#include \"bmx_vc_sync.h\"" not in main


def test_record_layout():
    assert C.sizeof(bmx.VcRec) == 64 and bmx.VC_REC_DTYPE.itemsize == 64
    assert C.sizeof(bmx.VcTableInfo) == 48
    names = ["id", "field", "aux", "val", "state", "keyset", "clock"]
    assert [f[0] for f in bmx.VcRec._fields_] == names and list(bmx.VC_REC_DTYPE.names) == names
    for name in names:
        assert getattr(bmx.VcRec, name).offset == bmx.VC_REC_DTYPE.fields[name][1], name
    assert [bmx.VC_REC_DTYPE.fields[n][1] for n in names] == [0, 8, 12, 16, 24, 28, 32]
    assert bmx.VC_REC_DTYPE["clock"].shape == (8,)


def test_the_header_compiles_as_c99():
    r = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "vc_sync_header.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the row digest: library == plain Python integers == numpy ----

def _sm(x):
    z = (x + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def _py_digest(r):
    c = [int(x) for x in r["clock"]]
    h = _sm(int(r["val"]) & M64)
    h = _sm(h ^ (int(r["keyset"]) | (int(r["state"]) << 32)))
    for i in range(4):
        h = _sm(h ^ (c[2 * i] | (c[2 * i + 1] << 32)))
    h = _sm(h ^ int(r["field"]))
    return _sm(h ^ int(r["id"]))


def _digest_cases():
    rng = np.random.default_rng(2024)
    n = 1000
    r = np.zeros(n, bmx.VC_REC_DTYPE)
    r["id"] = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    r["field"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    r["val"] = rng.integers(-(2**53 - 1), 2**53, n)
    r["state"] = rng.integers(1, 3, n)
    r["clock"] = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    r["keyset"] = [bmx.keyset(rng.permutation(8)[:int(rng.integers(0, 9))].tolist()) for _ in range(n)]
    r["aux"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)         # no part of the digest
    corners = []
    for val in (2**53 - 1, -(2**53 - 1), 0):
        for comp in (0, 2**32 - 1):
            for ks in (bmx.KEYSET_NONE, bmx.keyset([2]), bmx.keyset([0, 1, 2]), bmx.keyset(range(8)), bmx.keyset([2, 0, 1])):
                for id in (0, 2**64 - 2):
                    for state in (1, 2):
                        corners.append((id, 0xFFFFFFFE if comp else 0, val, state, ks, comp))
    c = np.zeros(len(corners), bmx.VC_REC_DTYPE)
    for k, (id, field, val, state, ks, comp) in enumerate(corners):
        c[k]["id"], c[k]["field"], c[k]["val"], c[k]["state"], c[k]["keyset"] = id, field, val, state, ks
        c[k]["clock"] = comp
    mixed = c.copy(); mixed["clock"][:, 1::2] = 0; mixed["clock"][:, 0] = 1                   # components 0 and 2^32 - 1 side by side
    return np.concatenate([r, c, mixed])


def test_row_digest_library_python_and_numpy_agree(lib):
    recs = _digest_cases()
    want = np.array([_py_digest(r) for r in recs], np.uint64)
    got_np = bmx.vc_rows_digest(recs["id"], recs["field"], recs["clock"], recs["keyset"], recs["state"], recs["val"])
    assert got_np.dtype == np.uint64 and np.array_equal(got_np, want)
    base = recs.ctypes.data
    got_lib = np.array([lib.bmx_vc_rec_digest(C.c_void_p(base + 64 * k)) for k in range(len(recs))], np.uint64)
    assert np.array_equal(got_lib, want)
    assert bmx.vc_rows_digest(recs["id"], recs["field"], recs["clock"], recs["keyset"], recs["state"], recs["val"], summed=True) == sum(int(x) for x in want) & M64
    # narrower clocks are padded with zeros; every word of the row takes part; aux does not
    k3 = recs[:50].copy(); k3["clock"][:, 3:] = 0
    assert np.array_equal(bmx.vc_rows_digest(k3["id"], k3["field"], k3["clock"][:, :3], k3["keyset"], k3["state"], k3["val"]), np.array([_py_digest(r) for r in k3], np.uint64))
    one = recs[:1].copy(); d0 = _py_digest(one[0])
    for col, delta in (("id", 1), ("field", 1), ("val", 1), ("state", 3), ("keyset", 1)):
        x = one.copy(); x[col] ^= delta
        assert _py_digest(x[0]) != d0, col
    for k in range(8):
        x = one.copy(); x["clock"][0, k] ^= 1
        assert _py_digest(x[0]) != d0, k
    x = one.copy(); x["aux"] ^= 0xFFFF
    assert _py_digest(x[0]) == d0 and lib.bmx_vc_rec_digest(C.c_void_p(x.ctypes.data)) == d0


# ---- argument errors ----

def test_bad_arguments_are_refused(lib):
    FILL8 = 0xA5
    s = np.full(1 << 16, FILL8, np.uint8).repeat(8).view(np.uint64)[:1 << 16].copy(); c = s.copy()
    f8 = np.full(8, 0xA5A5A5A5, np.uint32)
    recs = np.zeros(8, bmx.VC_REC_DTYPE); recs_img = recs.tobytes()
    out = np.frombuffer(bytearray([FILL8]) * (64 * 8), bmx.VC_REC_DTYPE).copy()
    cnt = np.full(2, 0xA5A5A5A5A5A5A5A5, np.uint64)
    upd = np.full(8, 0xA5A5A5A5, np.uint32); fl = np.full(8, FILL8, np.uint8)
    bits = np.full(1024, M64, np.uint64)
    p = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    ctx_err, comm_err, vc_before = lib.bmx_last_error(None), lib.bmx_comm_last_error(None), None
    calls = []
    for mem in (bmx.MEM_HOST, bmx.MEM_DEVICE, 7):
        # a NULL table with well-formed other arguments (mem = 7: a bad mem as well)
        calls += [lambda m=mem: lib.bmx_vc_digest(None, 10, 0, p(s), p(c), m),
                  lambda m=mem: lib.bmx_vc_frontier(None, p(f8), m),
                  lambda m=mem: lib.bmx_vc_export_rows(None, p(f8), 10, p(bits), 0, p(out), 8, p(cnt), m),
                  lambda m=mem: lib.bmx_vc_export_rows(None, None, 0, None, 0, None, 0, p(cnt), m),
                  lambda m=mem: lib.bmx_vc_merge_records(None, 8, p(recs), p(upd), p(cnt, 8), p(fl), m),
                  lambda m=mem: lib.bmx_vc_merge_records(None, 0, None, None, p(cnt, 8), None, m),
                  # and each bad argument of its own
                  lambda m=mem: lib.bmx_vc_digest(None, 17, 0, p(s), p(c), m),
                  lambda m=mem: lib.bmx_vc_digest(None, 10, 1, p(s), p(c), m),
                  lambda m=mem: lib.bmx_vc_digest(None, 10, 0x80000000, p(s), p(c), m),
                  lambda m=mem: lib.bmx_vc_digest(None, 10, 0, None, p(c), m),
                  lambda m=mem: lib.bmx_vc_digest(None, 10, 0, p(s), None, m),
                  lambda m=mem: lib.bmx_vc_frontier(None, None, m),
                  lambda m=mem: lib.bmx_vc_export_rows(None, None, 17, None, 0, p(out), 8, p(cnt), m),
                  lambda m=mem: lib.bmx_vc_export_rows(None, None, 10, None, 2, p(out), 8, p(cnt), m),
                  lambda m=mem: lib.bmx_vc_export_rows(None, None, 10, None, 0, None, 8, None, m),
                  lambda m=mem: lib.bmx_vc_merge_records(None, (1 << 24) + 1, p(recs), p(upd), p(cnt, 8), p(fl), m),
                  lambda m=mem: lib.bmx_vc_merge_records(None, 8, None, p(upd), p(cnt, 8), p(fl), m)]
    info = bmx.VcTableInfo()
    calls += [lambda: lib.bmx_vc_info(None, C.byref(info)), lambda: lib.bmx_vc_info(None, None)]
    for k, call in enumerate(calls):
        assert call() == bmx.ERR_INVALID, k
        assert (lib.bmx_vc_last_error(None) or b"") != b"", k
    # nothing was written: the guard fill is everywhere
    assert (s.view(np.uint8) == FILL8).all() and (c.view(np.uint8) == FILL8).all() and (f8 == 0xA5A5A5A5).all()
    assert (out.view(np.uint8) == FILL8).all() and (cnt == 0xA5A5A5A5A5A5A5A5).all() and (upd == 0xA5A5A5A5).all() and (fl == FILL8).all()
    assert recs.tobytes() == recs_img and (bits == M64).all()
    assert bytes(info) == bytes(bmx.VcTableInfo())
    # the text went to the vector-clock error word only
    assert lib.bmx_last_error(None) == ctx_err and lib.bmx_comm_last_error(None) == comm_err
    assert lib.bmx_vc_rec_digest(None) == 0


# ---- the premise of the GPU reconcile test, on the oracle alone ----

def _pull(dst, src):
    """all of src's rows, in (id, field) order, merged into dst with their key sets"""
    merge_recs(dst, model_rows(src))


def _fill(o, seed, who):
    for id, field, clocks, val, ks in replica_merges(seed, who):
        o.merge_batch(id, field, clocks, val, keysets=ks)


@pytest.mark.parametrize("seed", range(40))
def test_two_replicas_converge_within_three_rounds_on_the_oracle(seed):
    """K = 3, local writers 0 and 1, three merges of 400 deltas over 150 ids x 2 fields each. A round is a <- b, then b <- a. (Pins the inputs of
    test_gpu_vc_sync.py's reconcile test; it is a property of the reference's resolve() on these inputs, not of the engine.)"""
    a, b = OracleVC(3, 0), OracleVC(3, 1)
    _fill(a, seed, 0); _fill(b, seed, 1)
    assert not np.array_equal(model_rows(a), model_rows(b))
    rounds = 0
    while rounds < 3 and not np.array_equal(model_rows(a), model_rows(b)):
        _pull(a, b); _pull(b, a)
        rounds += 1
    ra, rb = model_rows(a), model_rows(b)
    assert np.array_equal(ra, rb), (seed, rounds, "rows, key sets and states are identical")
    assert len(ra) > 0 and set(ra["state"].tolist()) <= {bmx.VC_DENSE, bmx.VC_SPARSE}
