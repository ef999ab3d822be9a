// bmx_sync.inc — replica reconciliation (bmx.h "replica reconciliation"): key buckets, the per-bucket state digest and the filtered export as delta
// records. Read-only sweeps of the table (sync_kernels.h); included by bmx.hip (one translation unit), which keeps their scratch (SyncScratch).
namespace {

constexpr uint32_t SYNC_MAX_LOG2 = 16;

// the workgroups of one digest sweep: two per CU, never more than the table has chunks for
uint32_t digest_grid(const bmx_ctx* ctx) {
  const uint64_t chunks = (ctx->nslots + 64ull * DIG_U - 1) / (64ull * DIG_U);
  return sweep_grid(ctx, chunks, DIG_WAVES);
}

}  // namespace

extern "C" {

uint32_t bmx_key_bucket(uint64_t id, uint32_t field, uint32_t log2_buckets) { return key_bucket(id, field, std::min<uint32_t>(log2_buckets, SYNC_MAX_LOG2)); }

int bmx_digest(bmx_ctx* ctx, uint32_t log2_buckets, uint32_t flags, uint64_t* sums, uint64_t* counts, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (log2_buckets > SYNC_MAX_LOG2) return fail(ctx, BMX_ERR_INVALID, "bmx_digest: log2_buckets > 16");
  if (flags & ~BMX_SYNC_TOMBSTONES) return fail(ctx, BMX_ERR_INVALID, "bmx_digest: unknown flag");
  if (!sums || !counts) return fail(ctx, BMX_ERR_INVALID, "bmx_digest: null output");
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (int erc = enter(ctx)) return erc;
  const bool host = mem == BMX_MEM_HOST;
  const uint64_t B = 1ull << log2_buckets;
  unsigned long long* d_s = reinterpret_cast<unsigned long long*>(sums);
  unsigned long long* d_c = reinterpret_cast<unsigned long long*>(counts);
  if (host) {
    if (!ctx->sync.dig) { if (int rc = dev_alloc(ctx, &ctx->sync.dig, 2ull << SYNC_MAX_LOG2)) return rc; }
    d_s = ctx->sync.dig; d_c = ctx->sync.dig + B;
  }
  HIPCHK(hipMemsetAsync(d_s, 0, B * sizeof(unsigned long long), ctx->stream));
  HIPCHK(hipMemsetAsync(d_c, 0, B * sizeof(unsigned long long), ctx->stream));
  const uint32_t blocks = digest_grid(ctx);
  const bool nt = ctx->nslots * sizeof(Slot) > SCAN_NT_BYTES;
  const bool lds = log2_buckets <= DIG_LDS_LOG2;
  const uint32_t tomb = (flags & BMX_SYNC_TOMBSTONES) ? 1u : 0u;
#define BMX_DIGEST_LAUNCH(A, N) hipLaunchKernelGGL((k_digest_buckets<A, N>), dim3(blocks), dim3(DIG_THREADS), 0, ctx->stream, (const Slot*)ctx->slots, ctx->nslots, log2_buckets, tomb, d_s, d_c)
  if (lds) { if (nt) BMX_DIGEST_LAUNCH(true, true); else BMX_DIGEST_LAUNCH(true, false); }
  else { if (nt) BMX_DIGEST_LAUNCH(false, true); else BMX_DIGEST_LAUNCH(false, false); }
#undef BMX_DIGEST_LAUNCH
  LAUNCHCHK("k_digest_buckets");
  if (host) {
    HIPCHK(hipMemcpyAsync(sums, d_s, B * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(counts, d_c, B * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return BMX_OK;
}

int bmx_export_rows(bmx_ctx* ctx, int64_t since_ts, uint32_t log2_buckets, const uint64_t* bucket_bits, uint32_t flags, bmx_delta_rec* out, uint64_t cap,
                    uint64_t* n_out, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (log2_buckets > SYNC_MAX_LOG2) return fail(ctx, BMX_ERR_INVALID, "bmx_export_rows: log2_buckets > 16");
  if (flags & ~BMX_EXPORT_ONLY_TOMBSTONES) return fail(ctx, BMX_ERR_INVALID, "bmx_export_rows: unknown flag");
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (int erc = enter(ctx)) return erc;
  const bool host = mem == BMX_MEM_HOST;
  if (!out) cap = 0;
  const unsigned long long* d_bits = reinterpret_cast<const unsigned long long*>(bucket_bits);
  if (host && bucket_bits) {
    if (!ctx->sync.bits) { if (int rc = dev_alloc(ctx, &ctx->sync.bits, (1ull << SYNC_MAX_LOG2) / 64)) return rc; }
    const uint64_t words = std::max<uint64_t>(1, (1ull << log2_buckets) / 64);
    HIPCHK(hipMemcpyAsync(ctx->sync.bits, bucket_bits, words * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    d_bits = ctx->sync.bits;
  }
  bmx_delta_rec* d_out = out;
  const uint64_t d_cap = std::min<uint64_t>(cap, ctx->nslots);     // (no table holds more rows than slots)
  bool staged = false;
  if (host && d_cap) {
    if (void* m = mapped_host(out)) d_out = static_cast<bmx_delta_rec*>(m);   // page-locked memory: the kernel writes the records where the caller wants them
    else {
      if (d_cap > ctx->sync.recs_cap) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        ctx->sync.recs_cap = 0;
        const uint64_t want = std::min<uint64_t>(ctx->nslots, std::max<uint64_t>(d_cap + d_cap / 4, 1u << 12));
        if (int rc = dev_alloc(ctx, &ctx->sync.recs, want)) return rc;
        ctx->sync.recs_cap = want;
      }
      d_out = ctx->sync.recs; staged = true;
    }
  }
  unsigned long long* d_n = host ? &ctx->ds->n_out : reinterpret_cast<unsigned long long*>(n_out);
  // Plain loads by default: in the select skeleton a lane owns two consecutive slots, so four load instructions of a wave touch every 128-byte line, and
  // a nontemporal line does not wait in L2 for the other three (bench_micro/replica_sync.py times both; BMX_SYNC_EXPORT_NT=1 is its A/B switch).
  const char* nt_env = std::getenv("BMX_SYNC_EXPORT_NT");
  const bool nt = nt_env && nt_env[0] == '1' && ctx->nslots * sizeof(Slot) > SCAN_NT_BYTES;
  PredSlotSync P{ctx->slots, since_ts, d_bits, log2_buckets, (flags & BMX_EXPORT_ONLY_TOMBSTONES) != 0, nt};
  SelGeom g = sel_geom<PredSlotSync::E>(ctx->nslots);
  hipLaunchKernelGGL((k_sel_count<PredSlotSync>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, ctx->nslots, g.tiles_per_block, ctx->scan.block_counts);
  if (d_cap) {
    EmitRecs Em{ctx->slots, d_cap, d_out};
    FinishCount Fin{d_n};
    hipLaunchKernelGGL((k_sel_write<PredSlotSync, EmitRecs, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, Em, Fin, ctx->nslots, g.tiles_per_block,
                       ctx->scan.block_counts);
  } else if (d_n) {
    hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(SEL_THREADS), 0, ctx->stream, (const uint32_t*)ctx->scan.block_counts, g.blocks, d_n);
  }
  LAUNCHCHK("bmx_export_rows");
  if (host) {
    unsigned long long m = 0;
    HIPCHK(hipMemcpyAsync(&m, d_n, sizeof(m), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const uint64_t k = std::min<uint64_t>(m, d_cap);
    if (staged && k) HIPCHK(hipMemcpy(out, d_out, k * sizeof(bmx_delta_rec), hipMemcpyDeviceToHost));
    if (n_out) *n_out = m;
  }
  return BMX_OK;
}

}  // extern "C"
