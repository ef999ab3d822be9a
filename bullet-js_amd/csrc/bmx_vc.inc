// bmx_vc.inc — C ABI of the N4 table (K-writer vector clocks): see include/bmx.h "N4" and vc_kernels.h.
// Included at the end of bmx.hip (one translation unit: the kernels in the shared headers are not inline).
// Host buffers only; every call is synchronous. No CPU path: fails without a GPU.
#include "vc_kernels.h"
#include "../../include/bmx_vc_sync.h"   // (bmx_vc_rec: the handle keeps the staging of bmx_vc_sync.inc)

namespace {

// The per-batch workspace, grown on demand as ONE all-or-nothing group: a batch's staged inputs (host-buffer calls), what link / resolve / compaction pass to
// one another, and the long-list path's buffers (k_vc_resolve_long).
struct VcWorkspace {
  uint64_t cap = 0;
  uint64_t* d_id = nullptr; uint32_t* d_field = nullptr; uint32_t* d_clocks = nullptr; int64_t* d_val = nullptr; uint32_t* d_keysets = nullptr;
  uint32_t* next = nullptr; uint32_t* slot_of = nullptr; uint8_t* wflag = nullptr; uint8_t* flags = nullptr; uint32_t* blk_info = nullptr;
  uint32_t* applied = nullptr; uint8_t* d_state = nullptr;
  VcLongRow* lrows = nullptr; uint32_t* ord = nullptr; uint32_t* bitmap = nullptr; uint32_t bitmap_words = 0;
  int ensure(bmx_vc* t, uint64_t n);         // room for a batch of n deltas; after a failure nothing of it is allocated
  void release() {
    dev_free(d_id); dev_free(d_field); dev_free(d_clocks); dev_free(d_val); dev_free(d_keysets); dev_free(next); dev_free(slot_of); dev_free(wflag); dev_free(flags);
    dev_free(blk_info); dev_free(applied); dev_free(d_state); dev_free(lrows); dev_free(ord); dev_free(bitmap);
    cap = 0; bitmap_words = 0;
  }
};
// Scratch of bmx_vc_scan_range, allocated by the first scan and grown on demand.
struct VcScanScratch {
  uint32_t* sel_counts = nullptr;            // SEL_MAX_BLOCKS
  uint64_t* scan_out = nullptr; uint64_t scan_cap = 0;
  void release() { dev_free(sel_counts); dev_free(scan_out); scan_cap = 0; }
};
// Scratch of the reconciliation sweeps (bmx_vc_sync.inc): what a BMX_MEM_HOST caller's digest vectors, version vector, bucket set and records pass through.
// Allocated by the first call that needs it, grow-only.
struct VcSyncScratch {
  unsigned long long* dig = nullptr;         // 2 x 2^16 words: sums and counts
  unsigned long long* bits = nullptr;        // 2^16 bits
  uint32_t* frontier = nullptr;              // 8 words
  bmx_vc_rec* recs = nullptr; uint64_t recs_cap = 0;
  int cus = 0;                               // compute units of the device (the sweeps' grids), looked up by the first sweep
  void release() { dev_free(dig); dev_free(bits); dev_free(frontier); dev_free(recs); recs_cap = 0; }
};

}  // namespace

struct bmx_vc {
  int device = 0;
  hipStream_t stream = nullptr, own_stream = nullptr;
  VSlot* slots = nullptr;
  uint64_t nslots = 0, capacity_rows = 0;
  uint32_t K = 0, local = 0, epoch = 0;
  // the fixed device words, one group allocated at create
  unsigned long long* row_count = nullptr;   // [1] is a scratch word
  unsigned long long* n_out = nullptr;       // scratch
  uint32_t* status = nullptr;
  unsigned long long* shard_dummy = nullptr; // CTR_SHARDS*CTR_STRIDE zeros (FinishMerge folds them)
  VcLongCtl* lctl = nullptr;                 // the long-list path's control record
  uint64_t rows = 0;                         // exact after every host-buffer call
  uint64_t rows_ub = 0;                      // upper bound while device-pointer batches are in flight
  VcWorkspace ws;
  VcScanScratch scan;
  VcSyncScratch sync;
  std::string err;
  void release() { dev_free(slots); dev_free(row_count); dev_free(n_out); dev_free(status); dev_free(shard_dummy); dev_free(lctl); ws.release(); scan.release(); sync.release(); }
};

namespace {

int VcWorkspace::ensure(bmx_vc* t, uint64_t n) {
  if (n <= cap) return BMX_OK;
  HIPCHK_ON(t, hipStreamSynchronize(t->stream));
  cap = 0;
  const uint64_t c = (std::max<uint64_t>(n, 1u << 14) + 255) & ~255ull;
  const uint64_t bitmap_bytes = (uint64_t)VC_LONG_WGS * (c / 32) * sizeof(uint32_t);
  if (int rc = dev_alloc_all(t, {{d_id, c * 8}, {d_field, c * 4}, {d_clocks, c * t->K * 4}, {d_val, c * 8}, {d_keysets, c * 4}, {next, c * 4}, {slot_of, c * 4}, {wflag, c + 16},
                                 {flags, c}, {blk_info, (c / 256 + 16) * 4}, {applied, c * 4}, {d_state, c}, {lrows, (c / VC_SHORT + 1) * sizeof(VcLongRow)}, {ord, c * 4},
                                 {bitmap, bitmap_bytes}}))
    return rc;
  bitmap_words = (uint32_t)(c / 32);
  HIPCHK_ON(t, hipMemsetAsync(next, 0, c * sizeof(uint32_t), t->stream));
  HIPCHK_ON(t, hipMemsetAsync(bitmap, 0, bitmap_bytes, t->stream));
  cap = c;
  return BMX_OK;
}

// make room for `need_rows` rows at load factor <= 0.5 (keys are unique in the old table, so the rehash needs no compare)
int vc_grow(bmx_vc* t, uint64_t need_rows) {
  uint64_t nslots = t->nslots;
  while (nslots < 2 * need_rows + 2) nslots *= 2;
  if (nslots == t->nslots) return BMX_OK;
  if (nslots > (1ull << 32)) return fail(t, BMX_ERR_INVALID, "vector-clock table would need more than 2^32 slots (slot indices are 32-bit): shard the graph");
  VSlot* fresh = nullptr;
  if (int rc = dev_alloc(t, &fresh, nslots)) return rc;
  hipLaunchKernelGGL(k_vc_init, dim3(2048), dim3(256), 0, t->stream, fresh, nslots);
  hipLaunchKernelGGL(k_vc_rehash, dim3(2048), dim3(256), 0, t->stream, (const VSlot*)t->slots, t->nslots, fresh, nslots, t->status);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if (e != hipSuccess) { dev_free(fresh); return fail(t, BMX_ERR_HIP, std::string("grow: ") + hipGetErrorString(e)); }
  dev_free(t->slots);
  t->slots = fresh; t->nslots = nslots; t->capacity_rows = nslots / 2;
  return BMX_OK;
}

int status_check(bmx_vc* t) {
  uint32_t st = 0;
  HIPCHK_ON(t, hipMemcpyAsync(&st, t->status, sizeof(st), hipMemcpyDeviceToHost, t->stream));
  HIPCHK_ON(t, hipStreamSynchronize(t->stream));
  if (!st) return BMX_OK;
  HIPCHK_ON(t, hipMemsetAsync(t->status, 0, sizeof(uint32_t), t->stream));
  if (st & ST_SPIN) return fail(t, BMX_ERR_INTERNAL, "device protocol fault: bounded spin expired");
  if (st & ST_FULL) return fail(t, BMX_ERR_FULL, "vector-clock table is full");
  return fail(t, BMX_ERR_RANGE, "delta out of domain: reserved key or |val| > 2^53-1");
}

// enqueue link + resolve + compaction for device-resident inputs; outputs stay on the device (applied -> t->ws.applied or the caller's
// buffer, flags likewise). Grows the table first if the batch could push the load factor above 0.5 (rows_ub is a host-side bound).
int enqueue_batch(bmx_vc* t, uint64_t n, const uint64_t* d_id, const uint32_t* d_field, const uint32_t* d_clocks, const uint32_t* d_keysets, const int64_t* d_val, int load,
                  uint32_t* d_applied, unsigned long long* d_n_out, uint8_t* d_flags) {
  int rc;
  if (2 * (t->rows_ub + n) + 2 > t->nslots) {
    unsigned long long r = 0;                      // refresh the bound before paying for a rehash
    HIPCHK_ON(t, hipMemcpyAsync(&r, t->row_count, 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK_ON(t, hipStreamSynchronize(t->stream));
    t->rows_ub = r;
    if (2 * (t->rows_ub + n) + 2 > t->nslots && (rc = vc_grow(t, t->rows_ub + n))) return rc;
  }
  if ((rc = t->ws.ensure(t, n))) return rc;
  if (++t->epoch > EPOCH_MAX) {   // claim tags wrap: forget every link and every head before epoch 1 is reused
    HIPCHK_ON(t, hipMemsetAsync(t->ws.next, 0, t->ws.cap * sizeof(uint32_t), t->stream));
    hipLaunchKernelGGL(k_vc_sweep_heads, dim3(2048), dim3(256), 0, t->stream, t->slots, t->nslots);
    HIPCHK_ON(t, hipGetLastError());
    t->epoch = 1;
  }
  VcArgs A;
  A.slots = t->slots; A.nslots = t->nslots; A.id = d_id; A.field = d_field; A.clocks = d_clocks; A.keysets = d_keysets; A.val = d_val;
  A.n = (uint32_t)n; A.K = t->K; A.local = t->local; A.epoch = t->epoch;
  A.next = t->ws.next; A.slot_of = t->ws.slot_of; A.wflag = t->ws.wflag; A.flags = d_flags; A.blk_info = t->ws.blk_info;
  A.row_count = t->row_count; A.status = t->status; A.load = load;
  A.lctl = t->lctl; A.lrows = t->ws.lrows; A.lrows_cap = (uint32_t)(t->ws.cap / VC_SHORT + 1); A.ord = t->ws.ord; A.bitmap = t->ws.bitmap; A.bitmap_words = t->ws.bitmap_words;
  const uint32_t blocks = (uint32_t)((n + 255) / 256);
  hipLaunchKernelGGL(k_vc_link, dim3(blocks), dim3(256), 0, t->stream, A);
  hipLaunchKernelGGL(k_vc_resolve, dim3(blocks), dim3(256), 0, t->stream, A);
  if (!load) hipLaunchKernelGGL(k_vc_resolve_long, dim3(VC_LONG_WGS), dim3(256), 0, t->stream, A);   // rows with more than VC_SHORT deltas (usually none: the workgroups return at once)
  FinishMerge Fin{d_n_out, nullptr, t->shard_dummy, t->row_count + 1};   // row_count[1] is a scratch word for Fin's "+= 0"
  hipLaunchKernelGGL((k_compact_winners<FinishMerge>), dim3((uint32_t)((n + 4095) / 4096)), dim3(SEL_THREADS), 0, t->stream, t->ws.wflag, t->ws.blk_info, (uint32_t)n,
                     d_applied, Fin, ChgLog{});
  HIPCHK_ON(t, hipGetLastError());
  t->rows_ub += n;
  return BMX_OK;
}

// host buffers: stage inputs, run the batch, fetch outputs (synchronous)
int run_batch(bmx_vc* t, uint64_t n, const uint64_t* id, const uint32_t* field, const uint32_t* clocks, const uint32_t* keysets, const int64_t* val, int load,
              uint32_t* updated_idx, uint64_t* n_updated, uint8_t* flags) {
  if (n > MAX_BATCH) return fail(t, BMX_ERR_INVALID, "batch larger than 2^24 deltas");
  if (n_updated) *n_updated = 0;
  if (n == 0) return BMX_OK;
  if (!id || !field || !clocks || !val) return fail(t, BMX_ERR_INVALID, "null input column");
  int rc;
  if ((rc = t->ws.ensure(t, n))) return rc;
  HIPCHK_ON(t, hipMemcpyAsync(t->ws.d_id, id, n * 8, hipMemcpyHostToDevice, t->stream));
  HIPCHK_ON(t, hipMemcpyAsync(t->ws.d_field, field, n * 4, hipMemcpyHostToDevice, t->stream));
  HIPCHK_ON(t, hipMemcpyAsync(t->ws.d_clocks, clocks, n * t->K * 4, hipMemcpyHostToDevice, t->stream));
  HIPCHK_ON(t, hipMemcpyAsync(t->ws.d_val, val, n * 8, hipMemcpyHostToDevice, t->stream));
  if (keysets) HIPCHK_ON(t, hipMemcpyAsync(t->ws.d_keysets, keysets, n * 4, hipMemcpyHostToDevice, t->stream));
  if ((rc = enqueue_batch(t, n, t->ws.d_id, t->ws.d_field, t->ws.d_clocks, keysets ? t->ws.d_keysets : nullptr, t->ws.d_val, load, t->ws.applied, t->n_out, t->ws.flags))) return rc;
  unsigned long long host[2] = {0, 0};
  HIPCHK_ON(t, hipMemcpyAsync(&host[0], t->n_out, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK_ON(t, hipMemcpyAsync(&host[1], t->row_count, 8, hipMemcpyDeviceToHost, t->stream));
  rc = status_check(t);
  if (rc) return rc;
  t->rows = t->rows_ub = host[1];
  if (updated_idx && host[0]) HIPCHK_ON(t, hipMemcpy(updated_idx, t->ws.applied, host[0] * 4, hipMemcpyDeviceToHost));
  if (flags) HIPCHK_ON(t, hipMemcpy(flags, t->ws.flags, n, hipMemcpyDeviceToHost));
  if (n_updated) *n_updated = host[0];
  return BMX_OK;
}
}  // namespace

extern "C" {

uint32_t bmx_vc_keyset(const uint8_t* w, uint32_t count) {
  uint32_t ks = VC_KS_NONE;
  for (uint32_t i = 0; w && i < count && i < (uint32_t)VC_MAXK; i++) ks = (ks & ~(0xFu << (4 * i))) | ((uint32_t)(w[i] & 0xF) << (4 * i));
  return ks;
}
uint32_t bmx_vc_keyset_dense(uint32_t k_writers) { return vc_ks_dense(k_writers < (uint32_t)VC_MAXK ? k_writers : (uint32_t)VC_MAXK); }

const char* bmx_vc_last_error(const bmx_vc* t) { return t ? t->err.c_str() : g_vc_err.c_str(); }

int bmx_vc_create(int device, uint64_t capacity_rows, uint32_t k_writers, uint32_t local_writer, bmx_vc** out) {
  if (!out || capacity_rows == 0 || k_writers == 0 || k_writers > BMX_VC_MAX_WRITERS || local_writer >= k_writers)
    return fail<bmx_vc>(nullptr, BMX_ERR_INVALID, "bmx_vc_create: bad arguments (1..8 writers, local writer among them)");
  *out = nullptr;
  if (capacity_rows > (1ull << 31) - 2)   // 2 slots per row, 32-bit slot indices in the per-batch workspace
    return fail<bmx_vc>(nullptr, BMX_ERR_INVALID, "bmx_vc_create: table would need more than 2^32 slots (slot indices are 32-bit): shard the graph");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail<bmx_vc>(nullptr, BMX_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  if (device < 0 || device >= ndev) return fail<bmx_vc>(nullptr, BMX_ERR_INVALID, "device index out of range");
  bmx_vc* t = new (std::nothrow) bmx_vc();
  if (!t) return fail<bmx_vc>(nullptr, BMX_ERR_NOMEM, "out of host memory");
  t->device = device; t->K = k_writers; t->local = local_writer; t->capacity_rows = capacity_rows;
  t->nslots = (std::max<uint64_t>(4096, capacity_rows * 2) + 1) & ~1ull;
  auto bail = [&](int rc) { std::string m = t->err; bmx_vc_destroy(t); g_vc_err = m; return rc; };
  HIPCHK_BAIL(t, hipSetDevice(device));
  HIPCHK_BAIL(t, hipStreamCreateWithFlags(&t->own_stream, hipStreamNonBlocking));
  t->stream = t->own_stream;
  if (int rc = dev_alloc_all(t, {{t->slots, t->nslots * sizeof(VSlot)}, {t->row_count, 16}, {t->n_out, 8}, {t->status, 4}, {t->lctl, sizeof(VcLongCtl)},
                                 {t->shard_dummy, CTR_SHARDS * CTR_STRIDE * sizeof(unsigned long long)}}))
    return bail(rc);
  HIPCHK_BAIL(t, hipMemsetAsync(t->row_count, 0, 16, t->stream));
  HIPCHK_BAIL(t, hipMemsetAsync(t->status, 0, 4, t->stream));
  HIPCHK_BAIL(t, hipMemsetAsync(t->lctl, 0, sizeof(VcLongCtl), t->stream));
  HIPCHK_BAIL(t, hipMemsetAsync(t->shard_dummy, 0, CTR_SHARDS * CTR_STRIDE * sizeof(unsigned long long), t->stream));
  hipLaunchKernelGGL(k_vc_init, dim3(2048), dim3(256), 0, t->stream, t->slots, t->nslots);
  HIPCHK_BAIL(t, hipGetLastError());
  HIPCHK_BAIL(t, hipStreamSynchronize(t->stream));
  *out = t;
  return BMX_OK;
}

void bmx_vc_destroy(bmx_vc* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  if (t->stream) (void)hipStreamSynchronize(t->stream);
  t->release();
  if (t->own_stream) (void)hipStreamDestroy(t->own_stream);
  delete t;
}

int bmx_vc_load_rows_ks(bmx_vc* t, uint64_t n, const uint64_t* id, const uint32_t* field, const uint32_t* clocks, const uint32_t* keysets, const int64_t* val) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  HIPCHK_ON(t, hipSetDevice(t->device));
  const uint64_t chunk = 1u << 22;
  for (uint64_t off = 0; off < n; off += chunk) {
    uint64_t m = std::min<uint64_t>(chunk, n - off);
    int rc = run_batch(t, m, id + off, field + off, clocks + off * t->K, keysets ? keysets + off : nullptr, val + off, 1, nullptr, nullptr, nullptr);
    if (rc) return rc;
  }
  return BMX_OK;
}
int bmx_vc_load_rows(bmx_vc* t, uint64_t n, const uint64_t* id, const uint32_t* field, const uint32_t* clocks, const int64_t* val) {
  return bmx_vc_load_rows_ks(t, n, id, field, clocks, nullptr, val);
}

int bmx_vc_merge_batch_ks(bmx_vc* t, uint64_t n, const uint64_t* id, const uint32_t* field, const uint32_t* clocks, const uint32_t* keysets, const int64_t* val,
                          uint32_t* updated_idx, uint64_t* n_updated, uint8_t* flags) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  HIPCHK_ON(t, hipSetDevice(t->device));
  return run_batch(t, n, id, field, clocks, keysets, val, 0, updated_idx, n_updated, flags);
}
int bmx_vc_merge_batch(bmx_vc* t, uint64_t n, const uint64_t* id, const uint32_t* field, const uint32_t* clocks, const int64_t* val,
                       uint32_t* updated_idx, uint64_t* n_updated, uint8_t* flags) {
  return bmx_vc_merge_batch_ks(t, n, id, field, clocks, nullptr, val, updated_idx, n_updated, flags);
}

int bmx_vc_get_rows_ks(bmx_vc* t, uint64_t n, const uint64_t* id, const uint32_t* field, uint32_t* clocks_out, uint32_t* keysets_out, int64_t* val_out, uint8_t* state_out) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  if (n == 0) return BMX_OK;
  if (!id || !field || !clocks_out || !val_out || !state_out || n > MAX_BATCH) return fail(t, BMX_ERR_INVALID, "bad arguments");
  HIPCHK_ON(t, hipSetDevice(t->device));
  int rc = t->ws.ensure(t, n);
  if (rc) return rc;
  HIPCHK_ON(t, hipMemcpyAsync(t->ws.d_id, id, n * 8, hipMemcpyHostToDevice, t->stream));
  HIPCHK_ON(t, hipMemcpyAsync(t->ws.d_field, field, n * 4, hipMemcpyHostToDevice, t->stream));
  hipLaunchKernelGGL(k_vc_get, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, t->stream, t->slots, t->nslots, (uint32_t)n, t->K, t->ws.d_id, t->ws.d_field,
                     t->ws.d_clocks, t->ws.d_val, t->ws.d_state, keysets_out ? t->ws.d_keysets : nullptr);
  HIPCHK_ON(t, hipGetLastError());
  HIPCHK_ON(t, hipMemcpyAsync(clocks_out, t->ws.d_clocks, n * t->K * 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK_ON(t, hipMemcpyAsync(val_out, t->ws.d_val, n * 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK_ON(t, hipMemcpyAsync(state_out, t->ws.d_state, n, hipMemcpyDeviceToHost, t->stream));
  if (keysets_out) HIPCHK_ON(t, hipMemcpyAsync(keysets_out, t->ws.d_keysets, n * 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK_ON(t, hipStreamSynchronize(t->stream));
  return BMX_OK;
}
int bmx_vc_get_rows(bmx_vc* t, uint64_t n, const uint64_t* id, const uint32_t* field, uint32_t* clocks_out, int64_t* val_out, uint8_t* state_out) {
  return bmx_vc_get_rows_ks(t, n, id, field, clocks_out, nullptr, val_out, state_out);
}

int bmx_vc_scan_range(bmx_vc* t, uint32_t field, int64_t lo, int64_t hi, uint64_t* out_ids, uint64_t cap, uint64_t* n_out) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  HIPCHK_ON(t, hipSetDevice(t->device));
  VcScanScratch& S = t->scan;
  if (!S.sel_counts) { if (int rc = dev_alloc(t, &S.sel_counts, SEL_MAX_BLOCKS)) return rc; }
  uint64_t want = out_ids ? std::min<uint64_t>(cap, t->nslots) : 0;
  if (want > S.scan_cap) {
    HIPCHK_ON(t, hipStreamSynchronize(t->stream));
    S.scan_cap = 0;
    if (int rc = dev_alloc(t, &S.scan_out, want + want / 4)) return rc;
    S.scan_cap = want + want / 4;
  }
  PredVSlotRange P{t->slots, field, lo, hi};
  SelGeom g = sel_geom<PredVSlotRange::E>(t->nslots);
  hipLaunchKernelGGL((k_sel_count<PredVSlotRange>), dim3(g.blocks), dim3(SEL_THREADS), 0, t->stream, P, t->nslots, g.tiles_per_block, S.sel_counts);
  HIPCHK_ON(t, hipGetLastError());
  unsigned long long m = 0;
  if (want) {
    EmitVIds Em{t->slots, S.scan_out, want};
    FinishCount Fin{t->n_out};
    hipLaunchKernelGGL((k_sel_write<PredVSlotRange, EmitVIds, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, t->stream, P, Em, Fin, t->nslots, g.tiles_per_block, S.sel_counts);
  } else {
    hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(SEL_THREADS), 0, t->stream, (const uint32_t*)S.sel_counts, g.blocks, t->n_out);
  }
  HIPCHK_ON(t, hipGetLastError());
  HIPCHK_ON(t, hipMemcpyAsync(&m, t->n_out, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK_ON(t, hipStreamSynchronize(t->stream));
  if (want && m) HIPCHK_ON(t, hipMemcpy(out_ids, S.scan_out, std::min<uint64_t>(m, want) * 8, hipMemcpyDeviceToHost));
  if (n_out) *n_out = m;
  return BMX_OK;
}

int bmx_vc_row_count(bmx_vc* t, uint64_t* n_out) {
  if (!t || !n_out) return fail(t, BMX_ERR_INVALID, "bad arguments");
  HIPCHK_ON(t, hipSetDevice(t->device));
  unsigned long long r = 0;
  HIPCHK_ON(t, hipMemcpyAsync(&r, t->row_count, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK_ON(t, hipStreamSynchronize(t->stream));
  t->rows = t->rows_ub = r;
  *n_out = r;
  return BMX_OK;
}

int bmx_vc_merge_batch_ks_dev(bmx_vc* t, uint64_t n, const uint64_t* id, const uint32_t* field, const uint32_t* clocks, const uint32_t* keysets, const int64_t* val,
                              uint32_t* updated_idx, uint64_t* n_updated, uint8_t* flags) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  if (n > MAX_BATCH) return fail(t, BMX_ERR_INVALID, "batch larger than 2^24 deltas");
  HIPCHK_ON(t, hipSetDevice(t->device));
  if (n == 0) {
    if (n_updated) HIPCHK_ON(t, hipMemsetAsync(n_updated, 0, 8, t->stream));
    return BMX_OK;
  }
  if (!id || !field || !clocks || !val) return fail(t, BMX_ERR_INVALID, "null input column");
  int rc = t->ws.ensure(t, n);
  if (rc) return rc;
  return enqueue_batch(t, n, id, field, clocks, keysets, val, 0, updated_idx ? updated_idx : t->ws.applied,
                       reinterpret_cast<unsigned long long*>(n_updated ? n_updated : reinterpret_cast<uint64_t*>(t->n_out)), flags);
}
int bmx_vc_merge_batch_dev(bmx_vc* t, uint64_t n, const uint64_t* id, const uint32_t* field, const uint32_t* clocks, const int64_t* val,
                           uint32_t* updated_idx, uint64_t* n_updated, uint8_t* flags) {
  return bmx_vc_merge_batch_ks_dev(t, n, id, field, clocks, nullptr, val, updated_idx, n_updated, flags);
}

int bmx_vc_set_stream(bmx_vc* t, void* hip_stream) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  HIPCHK_ON(t, hipSetDevice(t->device));
  HIPCHK_ON(t, hipStreamSynchronize(t->stream));
  t->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : t->own_stream;
  return BMX_OK;
}

int bmx_vc_sync(bmx_vc* t) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  HIPCHK_ON(t, hipSetDevice(t->device));
  return status_check(t);
}

}  // extern "C"
