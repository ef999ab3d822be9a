// bmx_vc_sync.inc — replica reconciliation of the vector-clock table (include/bmx_vc_sync.h): the table's description, the per-bucket state digest, the version
// vector, the filtered export as 64-byte records and the record merge. Read-only sweeps of the table (vc_sync_kernels.h) plus one unpack kernel in front of
// bmx_vc.inc's enqueue_batch; included by bmx.hip behind bmx_vc.inc (one translation unit), whose handle keeps the scratch (VcSyncScratch).
#include "vc_sync_kernels.h"

namespace {

constexpr uint32_t VC_SYNC_MAX_LOG2 = 16;

inline bool vc_mem_ok(int mem) { return mem == BMX_MEM_HOST || mem == BMX_MEM_DEVICE; }

// the workgroups of one sweep whose waves take VSYNC_CHUNK slots at a time: two per CU at most, never more than the table has chunks for, one at least
int vc_sweep_grid(bmx_vc* t, uint32_t waves_per_wg, uint32_t* blocks) {
  if (!t->sync.cus) {
    int cus = 0;
    HIPCHK_ON(t, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device));
    t->sync.cus = std::max(cus, 1);
  }
  const uint64_t chunks = (t->nslots + VSYNC_CHUNK - 1) / VSYNC_CHUNK;
  *blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((chunks + waves_per_wg - 1) / waves_per_wg, 2ull * (uint64_t)t->sync.cus));
  return BMX_OK;
}

}  // namespace

extern "C" {

uint64_t bmx_vc_rec_digest(const bmx_vc_rec* r) { return r ? vc_row_digest(r->id, r->field, r->val, r->state, r->keyset, r->clock) : 0; }

int bmx_vc_info(bmx_vc* t, bmx_vc_table_info* out) {
  if (!t || !out) return fail(t, BMX_ERR_INVALID, "bmx_vc_info: bad arguments");
  uint64_t rows = 0;
  if (int rc = bmx_vc_row_count(t, &rows)) return rc;
  out->n_slots = t->nslots; out->n_rows = rows; out->capacity_rows = t->capacity_rows; out->table_bytes = t->nslots * sizeof(VSlot);
  out->k_writers = t->K; out->local_writer = t->local; out->device = (uint32_t)t->device; out->reserved = 0;
  return BMX_OK;
}

int bmx_vc_digest(bmx_vc* t, uint32_t log2_buckets, uint32_t flags, uint64_t* sums, uint64_t* counts, int mem) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  if (log2_buckets > VC_SYNC_MAX_LOG2) return fail(t, BMX_ERR_INVALID, "bmx_vc_digest: log2_buckets > 16");
  if (flags) return fail(t, BMX_ERR_INVALID, "bmx_vc_digest: unknown flag");
  if (!sums || !counts) return fail(t, BMX_ERR_INVALID, "bmx_vc_digest: null output");
  if (!vc_mem_ok(mem)) return fail(t, BMX_ERR_INVALID, "bad mem kind");
  HIPCHK_ON(t, hipSetDevice(t->device));
  const bool host = mem == BMX_MEM_HOST;
  const uint64_t B = 1ull << log2_buckets;
  unsigned long long* d_s = reinterpret_cast<unsigned long long*>(sums);
  unsigned long long* d_c = reinterpret_cast<unsigned long long*>(counts);
  if (host) {
    if (!t->sync.dig) { if (int rc = dev_alloc(t, &t->sync.dig, 2ull << VC_SYNC_MAX_LOG2)) return rc; }
    d_s = t->sync.dig; d_c = t->sync.dig + B;
  }
  uint32_t blocks = 1;
  if (int rc = vc_sweep_grid(t, VDIG_WAVES, &blocks)) return rc;
  HIPCHK_ON(t, hipMemsetAsync(d_s, 0, B * sizeof(unsigned long long), t->stream));
  HIPCHK_ON(t, hipMemsetAsync(d_c, 0, B * sizeof(unsigned long long), t->stream));
  const bool nt = t->nslots * sizeof(VSlot) > SCAN_NT_BYTES;
  const bool lds = log2_buckets <= DIG_LDS_LOG2;
#define BMX_VC_DIGEST_LAUNCH(A, N) hipLaunchKernelGGL((k_vc_digest<A, N>), dim3(blocks), dim3(VDIG_THREADS), 0, t->stream, (const VSlot*)t->slots, t->nslots, log2_buckets, d_s, d_c)
  if (lds) { if (nt) BMX_VC_DIGEST_LAUNCH(true, true); else BMX_VC_DIGEST_LAUNCH(true, false); }
  else { if (nt) BMX_VC_DIGEST_LAUNCH(false, true); else BMX_VC_DIGEST_LAUNCH(false, false); }
#undef BMX_VC_DIGEST_LAUNCH
  HIPCHK_ON(t, hipGetLastError());
  if (host) {
    HIPCHK_ON(t, hipMemcpyAsync(sums, d_s, B * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
    HIPCHK_ON(t, hipMemcpyAsync(counts, d_c, B * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
    HIPCHK_ON(t, hipStreamSynchronize(t->stream));
  }
  return BMX_OK;
}

int bmx_vc_frontier(bmx_vc* t, uint32_t* out8, int mem) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  if (!out8) return fail(t, BMX_ERR_INVALID, "bmx_vc_frontier: null output");
  if (!vc_mem_ok(mem)) return fail(t, BMX_ERR_INVALID, "bad mem kind");
  HIPCHK_ON(t, hipSetDevice(t->device));
  const bool host = mem == BMX_MEM_HOST;
  uint32_t* d_out = out8;
  if (host) {
    if (!t->sync.frontier) { if (int rc = dev_alloc(t, &t->sync.frontier, VC_MAXK)) return rc; }
    d_out = t->sync.frontier;
  }
  uint32_t blocks = 1;
  if (int rc = vc_sweep_grid(t, VFR_WAVES, &blocks)) return rc;
  HIPCHK_ON(t, hipMemsetAsync(d_out, 0, VC_MAXK * sizeof(uint32_t), t->stream));
  if (t->nslots * sizeof(VSlot) > SCAN_NT_BYTES) hipLaunchKernelGGL((k_vc_frontier<true>), dim3(blocks), dim3(VFR_THREADS), 0, t->stream, (const VSlot*)t->slots, t->nslots, d_out);
  else hipLaunchKernelGGL((k_vc_frontier<false>), dim3(blocks), dim3(VFR_THREADS), 0, t->stream, (const VSlot*)t->slots, t->nslots, d_out);
  HIPCHK_ON(t, hipGetLastError());
  if (host) {
    HIPCHK_ON(t, hipMemcpyAsync(out8, d_out, VC_MAXK * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
    HIPCHK_ON(t, hipStreamSynchronize(t->stream));
  }
  return BMX_OK;
}

int bmx_vc_export_rows(bmx_vc* t, const uint32_t* frontier8, uint32_t log2_buckets, const uint64_t* bucket_bits, uint32_t flags, bmx_vc_rec* out, uint64_t cap,
                       uint64_t* n_out, int mem) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  if (log2_buckets > VC_SYNC_MAX_LOG2) return fail(t, BMX_ERR_INVALID, "bmx_vc_export_rows: log2_buckets > 16");
  if (flags) return fail(t, BMX_ERR_INVALID, "bmx_vc_export_rows: unknown flag");
  if (!vc_mem_ok(mem)) return fail(t, BMX_ERR_INVALID, "bad mem kind");
  if (!out && !n_out) return fail(t, BMX_ERR_INVALID, "bmx_vc_export_rows: neither records nor a count asked for");
  HIPCHK_ON(t, hipSetDevice(t->device));
  const bool host = mem == BMX_MEM_HOST;
  if (!out) cap = 0;
  if (!t->scan.sel_counts) { if (int rc = dev_alloc(t, &t->scan.sel_counts, SEL_MAX_BLOCKS)) return rc; }
  const unsigned long long* d_bits = reinterpret_cast<const unsigned long long*>(bucket_bits);
  if (host && bucket_bits) {
    if (!t->sync.bits) { if (int rc = dev_alloc(t, &t->sync.bits, (1ull << VC_SYNC_MAX_LOG2) / 64)) return rc; }
    const uint64_t words = std::max<uint64_t>(1, (1ull << log2_buckets) / 64);
    HIPCHK_ON(t, hipMemcpyAsync(t->sync.bits, bucket_bits, words * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream));
    d_bits = t->sync.bits;
  }
  bmx_vc_rec* d_out = out;
  const uint64_t d_cap = std::min<uint64_t>(cap, t->nslots);       // (no table holds more rows than slots)
  bool staged = false;
  if (host && d_cap) {
    if (void* m = mapped_host(out)) d_out = static_cast<bmx_vc_rec*>(m);   // page-locked memory: the kernel writes the records where the caller wants them
    else {
      if (d_cap > t->sync.recs_cap) {
        HIPCHK_ON(t, hipStreamSynchronize(t->stream));
        t->sync.recs_cap = 0;
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(t->nslots, MAX_BATCH), std::max<uint64_t>(d_cap + d_cap / 4, 1u << 12));
        if (int rc = dev_alloc(t, &t->sync.recs, want)) return rc;
        t->sync.recs_cap = want;
      }
      d_out = t->sync.recs; staged = true;
    }
  }
  unsigned long long* d_n = host ? t->n_out : reinterpret_cast<unsigned long long*>(n_out);
  PredVSlotSync P{t->slots, d_bits, log2_buckets, t->K, frontier8 ? 1u : 0u, {0, 0, 0, 0, 0, 0, 0, 0}};
  if (frontier8) for (int k = 0; k < VC_MAXK; k++) P.fr[k] = frontier8[k];      // (a host pointer in both modes, read now)
  SelGeom g = sel_geom<PredVSlotSync::E>(t->nslots);
  hipLaunchKernelGGL((k_sel_count<PredVSlotSync>), dim3(g.blocks), dim3(SEL_THREADS), 0, t->stream, P, t->nslots, g.tiles_per_block, t->scan.sel_counts);
  if (d_cap) {
    EmitVRecs Em{t->slots, d_cap, d_out};
    FinishCount Fin{d_n};
    hipLaunchKernelGGL((k_sel_write<PredVSlotSync, EmitVRecs, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, t->stream, P, Em, Fin, t->nslots, g.tiles_per_block,
                       t->scan.sel_counts);
  } else if (d_n) {
    hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(SEL_THREADS), 0, t->stream, (const uint32_t*)t->scan.sel_counts, g.blocks, d_n);
  }
  HIPCHK_ON(t, hipGetLastError());
  if (host) {
    unsigned long long m = 0;
    HIPCHK_ON(t, hipMemcpyAsync(&m, d_n, sizeof(m), hipMemcpyDeviceToHost, t->stream));
    HIPCHK_ON(t, hipStreamSynchronize(t->stream));
    const uint64_t k = std::min<uint64_t>(m, d_cap);
    if (staged && k) HIPCHK_ON(t, hipMemcpy(out, d_out, k * sizeof(bmx_vc_rec), hipMemcpyDeviceToHost));
    if (n_out) *n_out = m;
  }
  return BMX_OK;
}

int bmx_vc_merge_records(bmx_vc* t, uint64_t n, const bmx_vc_rec* recs, uint32_t* updated_idx, uint64_t* n_updated, uint8_t* flags, int mem) {
  if (!t) return fail(t, BMX_ERR_INVALID, "null table");
  if (!vc_mem_ok(mem)) return fail(t, BMX_ERR_INVALID, "bad mem kind");
  if (n > MAX_BATCH) return fail(t, BMX_ERR_INVALID, "batch larger than 2^24 deltas");
  if (n && !recs) return fail(t, BMX_ERR_INVALID, "null records");
  HIPCHK_ON(t, hipSetDevice(t->device));
  const bool host = mem == BMX_MEM_HOST;
  if (n == 0) {
    if (host) { if (n_updated) *n_updated = 0; }
    else if (n_updated) HIPCHK_ON(t, hipMemsetAsync(n_updated, 0, 8, t->stream));
    return BMX_OK;
  }
  int rc;
  if ((rc = t->ws.ensure(t, n))) return rc;
  const bmx_vc_rec* d_recs = recs;
  if (host) {
    if (n > t->sync.recs_cap) {
      HIPCHK_ON(t, hipStreamSynchronize(t->stream));
      t->sync.recs_cap = 0;
      const uint64_t want = std::min<uint64_t>(MAX_BATCH, std::max<uint64_t>(n + n / 4, 1u << 12));
      if ((rc = dev_alloc(t, &t->sync.recs, want))) return rc;
      t->sync.recs_cap = want;
    }
    HIPCHK_ON(t, hipMemcpyAsync(t->sync.recs, recs, n * sizeof(bmx_vc_rec), hipMemcpyHostToDevice, t->stream));
    d_recs = t->sync.recs;
  }
  VcWorkspace& W = t->ws;
  hipLaunchKernelGGL(k_vc_unpack, dim3((uint32_t)((n + VUNP_THREADS - 1) / VUNP_THREADS)), dim3(VUNP_THREADS), 0, t->stream, d_recs, (uint32_t)n, t->K, W.d_id, W.d_field, W.d_clocks,
                     W.d_keysets, W.d_val);
  HIPCHK_ON(t, hipGetLastError());
  if (!host)
    return enqueue_batch(t, n, W.d_id, W.d_field, W.d_clocks, W.d_keysets, W.d_val, 0, updated_idx ? updated_idx : W.applied,
                         reinterpret_cast<unsigned long long*>(n_updated ? n_updated : reinterpret_cast<uint64_t*>(t->n_out)), flags);
  // host buffers: the tail of bmx_vc.inc's run_batch
  if (n_updated) *n_updated = 0;
  if ((rc = enqueue_batch(t, n, W.d_id, W.d_field, W.d_clocks, W.d_keysets, W.d_val, 0, W.applied, t->n_out, W.flags))) return rc;
  unsigned long long h[2] = {0, 0};
  HIPCHK_ON(t, hipMemcpyAsync(&h[0], t->n_out, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK_ON(t, hipMemcpyAsync(&h[1], t->row_count, 8, hipMemcpyDeviceToHost, t->stream));
  if ((rc = status_check(t))) return rc;
  t->rows = t->rows_ub = h[1];
  if (updated_idx && h[0]) HIPCHK_ON(t, hipMemcpy(updated_idx, W.applied, h[0] * 4, hipMemcpyDeviceToHost));
  if (flags) HIPCHK_ON(t, hipMemcpy(flags, W.flags, n, hipMemcpyDeviceToHost));
  if (n_updated) *n_updated = h[0];
  return BMX_OK;
}

}  // extern "C"
