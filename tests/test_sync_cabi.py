"""CPU-only checks of the replica-reconciliation surface (include/bmx.h "replica reconciliation"): the symbols exist, bad arguments are refused
before any device work, and the key-bucket function — the one thing two replicas of any shape must agree on — is what the header writes out:
the library, the numpy restatement in the package and the properties a reconciliation relies on (nesting, uniformity)."""
import ctypes as C

import numpy as np
import pytest

import bmx
from bmx import replica, synth

NEW = ["bmx_key_bucket", "bmx_digest", "bmx_export_rows", "bmx_comm_digest", "bmx_comm_export_rows"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return bmx.load_library()


@pytest.fixture(scope="module")
def keys():
    ids = synth.splitmix64_np(np.arange(1, 1_000_001, dtype=np.uint64))
    return ids, [synth.field_hash(i) for i in range(3)]


def test_new_symbols_are_exported_and_listed(lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in bmx.EXPORTS, name
    assert lib.bmx_abi_version() == 4


def test_bad_arguments_are_refused(lib):
    s = np.zeros(1 << 16, np.uint64); c = np.zeros(1 << 16, np.uint64); n = C.c_uint64()
    sp, cp, npn = C.c_void_p(s.ctypes.data), C.c_void_p(c.ctypes.data), C.cast(C.byref(n), C.c_void_p)
    for L, mem in ((10, bmx.MEM_HOST), (17, bmx.MEM_HOST), (10, 7)):
        assert lib.bmx_digest(None, L, 0, sp, cp, mem) == bmx.ERR_INVALID
        assert lib.bmx_export_rows(None, 0, L, None, 0, None, 0, npn, mem) == bmx.ERR_INVALID
    assert lib.bmx_comm_digest(None, 10, 0, sp, cp) == bmx.ERR_INVALID
    assert lib.bmx_comm_export_rows(None, 0, 10, None, 0, None, 0, npn) == bmx.ERR_INVALID
    with pytest.raises(ValueError):
        bmx.key_bucket([1], [2], 17)


@pytest.mark.parametrize("L", [0, 1, 10, 16])
def test_library_and_numpy_agree_on_key_bucket(lib, keys, L):
    ids, fields = keys
    for f in fields:
        want = bmx.key_bucket(ids, np.full(len(ids), f, np.uint32), L)
        assert want.dtype == np.uint32 and int(want.max()) < (1 << L)
        # the library over a spread sample (every 37th key: ctypes calls are slow) and the first 20000
        pick = np.concatenate([np.arange(0, len(ids), 37), np.arange(20000)])
        got = np.array([lib.bmx_key_bucket(int(i), int(f), L) for i in ids[pick]], np.uint32)
        assert np.array_equal(got, want[pick])


def test_library_key_bucket_on_every_key(lib, keys):
    """all 10^6 ids x 3 fields at L = 16 through the library (the other L follow by nesting, checked below on the library too)"""
    ids, fields = keys
    fn = lib.bmx_key_bucket
    for f in fields:
        got = np.fromiter((fn(i, f, 16) for i in ids.tolist()), np.uint32, len(ids))
        want = bmx.key_bucket(ids, np.full(len(ids), f, np.uint32), 16)
        assert np.array_equal(got, want)
        for L in (0, 1, 10):
            assert np.array_equal(bmx.key_bucket(ids, np.full(len(ids), f, np.uint32), L), (want >> (16 - L)) if L else np.zeros_like(want))
    for i, f in ((0, 0), (1, 0), (0xFFFFFFFFFFFFFFFE, 0xFFFFFFFE), (12345, 6789)):
        for L in (0, 1, 10, 16):
            assert fn(i, f, L) == int(bmx.key_bucket([i], [f], L)[0])


def test_buckets_nest(keys):
    ids, fields = keys
    f = np.full(len(ids), fields[1], np.uint32)
    for L in range(0, 16):
        assert np.array_equal(bmx.key_bucket(ids, f, L), bmx.key_bucket(ids, f, L + 1) >> 1)


def test_buckets_are_uniform(keys):
    """10^6 keys over 1024 buckets: mean 977, Poisson sigma ~31; +-25 % is ~8 sigma — a sound mix passes, a truncated one does not"""
    ids, fields = keys
    for f in fields:
        n = np.bincount(bmx.key_bucket(ids, np.full(len(ids), f, np.uint32), 10), minlength=1024)
        mean = len(ids) / 1024.0
        assert n.min() >= 0.75 * mean and n.max() <= 1.25 * mean, (n.min(), n.max())
    # the field takes part: one node's fields spread over the buckets
    b = bmx.key_bucket(np.full(4096, ids[0], np.uint64), np.arange(4096, dtype=np.uint32), 4)
    assert np.bincount(b, minlength=16).min() > 150
    # sequential (unhashed) ids too: nothing relies on the host's id hash
    n = np.bincount(bmx.key_bucket(np.arange(1_000_000, dtype=np.uint64), np.zeros(1_000_000, np.uint32), 10), minlength=1024)
    assert n.min() >= 0.75 * 976.5 and n.max() <= 1.25 * 976.5


def test_key_bucket_does_not_follow_the_owner_hash(keys):
    """the bucket must not be a function of the shard owner: inside one shard of 8 the keys still fill all 8 top-level buckets evenly"""
    ids, fields = keys
    own = synth.owner_of_np(ids, 8)
    b = bmx.key_bucket(ids, np.full(len(ids), fields[0], np.uint32), 3)
    for g in range(8):
        n = np.bincount(b[own == g], minlength=8)
        assert n.min() > 0.9 * n.mean() and n.max() < 1.1 * n.mean()


def test_diff_buckets_on_hand_made_vectors():
    z = np.zeros(1024, np.uint64)
    assert not replica.diff_buckets((z, z), (z, z)).any() and len(replica.diff_buckets((z, z), (z, z))) == 16
    s = z.copy(); s[0] = 5; s[63] = 1; s[64] = 9
    c = z.copy(); c[1023] = 2
    bits = replica.diff_buckets((s, z), (z, c))
    want = np.zeros(16, np.uint64); want[0] = np.uint64(1 | (1 << 63)); want[1] = np.uint64(1); want[15] = np.uint64(1 << 63)
    assert np.array_equal(bits, want) and replica.bucket_count(bits) == 4
    assert np.array_equal(bits, bmx.bucket_bits_of([0, 63, 64, 1023], 10))
    # fewer than 64 buckets still give one whole word
    a = np.array([1, 2], np.uint64); b = np.array([1, 3], np.uint64); n = np.array([1, 1], np.uint64)
    assert replica.diff_buckets((a, n), (b, n)).tolist() == [2]
    o = np.array([7], np.uint64)
    assert replica.diff_buckets((o, o), (o, o)).tolist() == [0]
    # a difference in the counts alone is a difference (two rows whose digests cancel are still two rows)
    assert replica.diff_buckets((a, n), (a, np.array([1, 2], np.uint64))).tolist() == [2]
    with pytest.raises(ValueError):
        replica.diff_buckets((a, n), (z, z))
