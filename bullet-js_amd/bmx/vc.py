"""EngineVC: one bmx_vc, the table whose rows carry a vector clock; and its key-set words and row digest in numpy."""
import ctypes as C

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST, VC_REC_DTYPE, VcTableInfo, _Handle, _np, _ptr, _ref
from .engine import _bucket_words

FLAG_CONCURRENT = 8
VC_ABSENT, VC_DENSE, VC_SPARSE = 0, 1, 2


class EngineVC(_Handle):
    """N4 table (a bmx_vc): rows carry a K-writer vector clock instead of one timestamp. Host arrays only, synchronous.
    clocks are (n, K) uint32, component k = writer k's counter (0 = absent from the reference's clock object)."""
    _destroy, _last_error = "bmx_vc_destroy", "bmx_vc_last_error"

    def __init__(self, capacity_rows, k_writers, local_writer, device=0):
        self._create("bmx_vc_create", int(device), int(capacity_rows), int(k_writers), int(local_writer))
        self.K = int(k_writers)
        self.device = int(device)

    def _cols(self, id, field, clocks, val):
        id = _np(id, np.uint64); field = _np(field, np.uint32); val = _np(val, np.int64)
        clocks = _np(clocks, np.uint32).reshape(len(id), self.K) if len(id) else np.zeros((0, self.K), np.uint32)
        if not (len(id) == len(field) == len(val)):
            raise ValueError("column lengths differ")
        return id, field, clocks, val

    def load_rows(self, id, field, clocks, val, keysets=None):
        """keysets (uint32[n], see keyset()): which writers each clock names and in which order; None = all K, in order."""
        id, field, clocks, val = self._cols(id, field, clocks, val)
        ks = None if keysets is None else _np(keysets, np.uint32)
        self._chk(self.L.bmx_vc_load_rows_ks(self.h, len(id), _ptr(id), _ptr(field), _ptr(clocks), _ptr(ks), _ptr(val)))

    def merge_batch(self, id, field, clocks, val, keysets=None):
        """-> (flags uint8[n], updated uint32[]): per-delta resolve() flags; for each touched row that changed, the index of the
        last delta that updated it, ascending."""
        id, field, clocks, val = self._cols(id, field, clocks, val)
        n = len(id)
        ks = None if keysets is None else _np(keysets, np.uint32)
        if ks is not None and len(ks) != n:
            raise ValueError("column lengths differ")
        flags = np.zeros(n, np.uint8); upd = np.zeros(max(n, 1), np.uint32); nu = C.c_uint64()
        self._chk(self.L.bmx_vc_merge_batch_ks(self.h, n, _ptr(id), _ptr(field), _ptr(clocks), _ptr(ks), _ptr(val), _ptr(upd), C.byref(nu), _ptr(flags)))
        return flags, upd[: nu.value].copy()

    def get_rows(self, id, field, with_keysets=False):
        """-> (clocks (n,K) uint32, val int64[n], state uint8[n]) with state VC_ABSENT / VC_DENSE / VC_SPARSE; with_keysets: + keysets uint32[n]."""
        id = _np(id, np.uint64); field = _np(field, np.uint32)
        n = len(id)
        clocks = np.zeros((n, self.K), np.uint32); val = np.zeros(n, np.int64); st = np.zeros(n, np.uint8)
        if with_keysets:
            ks = np.zeros(n, np.uint32)
            self._chk(self.L.bmx_vc_get_rows_ks(self.h, n, _ptr(id), _ptr(field), _ptr(clocks), _ptr(ks), _ptr(val), _ptr(st)))
            return clocks, val, st, ks
        self._chk(self.L.bmx_vc_get_rows(self.h, n, _ptr(id), _ptr(field), _ptr(clocks), _ptr(val), _ptr(st)))
        return clocks, val, st

    def row_count(self):
        n = C.c_uint64()
        self._chk(self.L.bmx_vc_row_count(self.h, C.byref(n)))
        return n.value

    def scan_range(self, field, lo, hi, count_only=False):
        """node ids of the rows of `field` with lo <= val <= hi (table order), or their number"""
        m = C.c_uint64()
        if count_only:
            self._chk(self.L.bmx_vc_scan_range(self.h, int(field), int(lo), int(hi), None, 0, C.byref(m)))
            return m.value
        cap = max(self.row_count(), 1)
        out = np.zeros(cap, np.uint64)
        self._chk(self.L.bmx_vc_scan_range(self.h, int(field), int(lo), int(hi), _ptr(out), cap, C.byref(m)))
        return out[:min(m.value, cap)].copy()

    # device-pointer form: torch tensors / raw pointers, enqueue-only
    def merge_batch_dev(self, n, id, field, clocks, val, updated=None, n_updated=None, flags=None, keysets=None):
        self._chk(self.L.bmx_vc_merge_batch_ks_dev(self.h, int(n), _ptr(id), _ptr(field), _ptr(clocks), _ptr(keysets), _ptr(val), _ptr(updated), _ptr(n_updated), _ptr(flags)))

    def set_stream(self, stream_ptr):
        self._chk(self.L.bmx_vc_set_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def sync(self):
        self._chk(self.L.bmx_vc_sync(self.h))

    # ---- replica reconciliation (include/bmx_vc_sync.h; bmx/replica.py pull_vc / reconcile_vc drive it) ----
    def info(self):
        out = VcTableInfo()
        self._chk(self.L.bmx_vc_info(self.h, C.byref(out)))
        return out

    def digest(self, log2_buckets=10):
        """-> (sums u64[2^L], counts u64[2^L]): per-bucket sum of the row digests (vc_rows_digest) and number of rows; counts.sum() == row_count()"""
        B = 1 << int(log2_buckets)
        sums = np.zeros(B, np.uint64); counts = np.zeros(B, np.uint64)
        self._chk(self.L.bmx_vc_digest(self.h, int(log2_buckets), 0, _ptr(sums), _ptr(counts), MEM_HOST))
        return sums, counts

    def digest_dev(self, log2_buckets, sums, counts):
        """same into device memory (u64[2^L] each); enqueue-only"""
        self._chk(self.L.bmx_vc_digest(self.h, int(log2_buckets), 0, _ptr(sums), _ptr(counts), MEM_DEVICE))

    def frontier(self):
        """-> u32[8]: the table's version vector, the component-wise maximum of its rows' clocks (zeros behind K and for an empty table)"""
        out = np.zeros(8, np.uint32)
        self._chk(self.L.bmx_vc_frontier(self.h, _ptr(out), MEM_HOST))
        return out

    def frontier_dev(self, out8):
        self._chk(self.L.bmx_vc_frontier(self.h, _ptr(out8), MEM_DEVICE))

    @staticmethod
    def _frontier_words(frontier):
        if frontier is None:
            return None
        f = np.zeros(8, np.uint32)
        v = _np(frontier, np.uint32)
        if len(v) > 8:
            raise ValueError("a frontier has at most 8 components")
        f[:len(v)] = v
        return f

    def export_rows(self, frontier=None, log2_buckets=0, bucket_bits=None, cap=None, out=None):
        """-> (records, n): the rows whose bucket's bit is set (bucket_bits: u64 words, None = every bucket) and, with a frontier (up to 8 u32), whose clock
        exceeds it in some component, as VC_REC_DTYPE records in slot order; n = number of matches, len(records) = min(n, cap). cap=None: everything (one
        counting call first). out: a VC_REC_DTYPE array to fill (e.g. in a HostBuffer) — its length is the cap and the result a view of it."""
        bits = _bucket_words(bucket_bits, log2_buckets)
        fr = self._frontier_words(frontier)
        m = C.c_uint64()
        if out is not None:
            if out.dtype != VC_REC_DTYPE or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a contiguous VC_REC_DTYPE array")
            cap = len(out)
        elif cap is None:
            self._chk(self.L.bmx_vc_export_rows(self.h, _ptr(fr), int(log2_buckets), _ptr(bits), 0, None, 0, _ref(m), MEM_HOST))
            cap = m.value
        recs = out if out is not None else np.zeros(int(cap), VC_REC_DTYPE)
        self._chk(self.L.bmx_vc_export_rows(self.h, _ptr(fr), int(log2_buckets), _ptr(bits), 0, _ptr(recs) if cap else None, int(cap), _ref(m), MEM_HOST))
        return recs[:min(m.value, int(cap))], m.value

    def export_rows_dev(self, out, cap, n_out, frontier=None, log2_buckets=0, bucket_bits=None):
        """same with device memory: out = room for cap 64-byte records (None: count only), n_out = one u64, bucket_bits = device u64 words or None; the frontier
        stays a host vector; enqueue-only"""
        self._chk(self.L.bmx_vc_export_rows(self.h, _ptr(self._frontier_words(frontier)), int(log2_buckets), _ptr(bucket_bits), 0, _ptr(out), int(cap), _ptr(n_out), MEM_DEVICE))

    def dump_rows(self):
        """every row as VC_REC_DTYPE records, in slot order"""
        return self.export_rows()[0]

    def merge_records(self, recs):
        """merge_batch over the records' columns (id, field, clock[:K], keyset, val) -> (flags uint8[n], updated uint32[])"""
        recs = np.ascontiguousarray(recs, VC_REC_DTYPE)
        n = len(recs)
        flags = np.zeros(n, np.uint8); upd = np.zeros(max(n, 1), np.uint32); nu = C.c_uint64()
        self._chk(self.L.bmx_vc_merge_records(self.h, n, _ptr(recs) if n else None, _ptr(upd), _ref(nu), _ptr(flags) if n else None, MEM_HOST))
        return flags, upd[: nu.value].copy()

    def merge_records_dev(self, n, recs, updated=None, n_updated=None, flags=None):
        """device-pointer form: recs = n 64-byte records in device memory; enqueue-only, errors are reported by sync()"""
        self._chk(self.L.bmx_vc_merge_records(self.h, int(n), _ptr(recs), _ptr(updated), _ptr(n_updated), _ptr(flags), MEM_DEVICE))


KEYSET_NONE = 0xFFFFFFFF


def keyset(writers):
    """Key-set word of a clock whose keys are the writers with these indices, in this order (include/bmx.h bmx_vc_keyset)."""
    ks = KEYSET_NONE
    for i, w in enumerate(writers):
        ks = (ks & ~(0xF << (4 * i))) | ((int(w) & 0xF) << (4 * i))
    return ks & 0xFFFFFFFF


def keyset_writers(ks):
    """inverse of keyset(): the writer indices a key-set word names, in order"""
    out = []
    for i in range(8):
        w = (int(ks) >> (4 * i)) & 0xF
        if w == 0xF:
            break
        out.append(w)
    return out


def vc_rows_digest(id, field, clocks8, keysets, state, val, summed=False):
    """The row digest of include/bmx_vc_sync.h, restated in numpy: eight chained splitmix64 over val, keyset | state << 32, the eight clock components in
    pairs, field, id. clocks8: (n, k) u32 with k <= 8 (padded with zeros). -> u64[n], or with summed=True their sum mod 2^64 as a Python int."""
    u = np.uint64
    id = np.asarray(id, u); n = len(id)
    c = np.zeros((n, 8), u)
    if n:
        cl = np.asarray(clocks8, np.uint32).reshape(n, -1)
        c[:, :cl.shape[1]] = cl
    with np.errstate(over="ignore"):
        def sm(x):
            z = x + u(0x9e3779b97f4a7c15)
            z = (z ^ (z >> u(30))) * u(0xbf58476d1ce4e5b9)
            z = (z ^ (z >> u(27))) * u(0x94d049bb133111eb)
            return z ^ (z >> u(31))
        h = sm(np.asarray(val, np.int64).astype(u))
        h = sm(h ^ (np.asarray(keysets, np.uint32).astype(u) | (np.asarray(state, np.uint32).astype(u) << u(32))))
        for i in range(4):
            h = sm(h ^ (c[:, 2 * i] | (c[:, 2 * i + 1] << u(32))))
        h = sm(h ^ np.asarray(field, np.uint32).astype(u))
        d = sm(h ^ id)
        return int(d.sum(dtype=u)) if summed else d
