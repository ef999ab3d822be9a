// bmx_index.inc — the dense index of one field (its columns in slot order): the maintenance state and the full build from the table. The refresh from the change
// log, fresh_index and the bmx_index_* entry points are bmx_index_refresh.inc, behind the view's patch (bmx.hip, the include list). Kernels: scan_kernels.h, select.h.
// Included by bmx.hip (one translation unit), which keeps the state (Index, ChangeLog).
namespace {

Index* find_index(bmx_ctx* ctx, uint32_t field) {
  for (auto& ix : ctx->indexes)
    if (ix.field == field) return &ix;
  return nullptr;
}

constexpr size_t IX_MAINTAINED_MAX = PART_MAX_SHARDS / 2;   // two scratch words of DevScalars::part_totals per maintained index

// slot -> index position map (4 B per slot) and the change log; both exist from the first index build on
int ensure_ix_maintenance(bmx_ctx* ctx) {
  int rc;
  if (ctx->chg.slot_pos_n != ctx->nslots) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dev_free(ctx->chg.slot_pos); ctx->chg.slot_pos_n = 0;
    for (auto& ix : ctx->indexes) ix.has_pos = false;
    ctx->chg.valid = false;
    if (ctx->nslots >= (1ull << 31)) return BMX_OK;      // bit 31 of a log entry is the "created" mark: larger tables are rebuilt, not maintained
    if ((rc = dev_alloc(ctx, &ctx->chg.slot_pos, ctx->nslots))) { g_err.clear(); ctx->err.clear(); return BMX_OK; }   // no memory for it: fall back to rebuilds
    ctx->chg.slot_pos_n = ctx->nslots;
    HIPCHK(hipMemsetAsync(ctx->chg.slot_pos, 0xFF, ctx->nslots * sizeof(uint32_t), ctx->stream));
  }
  // the log is only used while it is shorter than max(nslots/8, 1M) entries (fresh_index): size it for that, not for the largest table
  const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(ctx->nslots / 4, 1u << 20) + (1u << 16), 1u << 26);   // 1M .. 64M entries of 8 B
  if (ctx->chg.cap < want) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->chg.cap = 0; ctx->chg.valid = false;
    if ((rc = dev_alloc(ctx, &ctx->chg.log, want))) { g_err.clear(); ctx->err.clear(); return BMX_OK; }
    ctx->chg.cap = want;
  }
  return BMX_OK;
}

// forget the log: every index is either fresh or about to be rebuilt
int reset_chg_log(bmx_ctx* ctx) {
  HIPCHK(hipMemsetAsync(ctx->ds->chg_n, 0, sizeof(ctx->ds->chg_n), ctx->stream));
  ctx->chg.par = 0; ctx->chg.ub = 0;
  return BMX_OK;
}

// (Re)build the dense columns of `field` from the table, in slot order. Synchronous.
int build_index(bmx_ctx* ctx, Index* ix) {
  int mrc = ensure_ix_maintenance(ctx);
  if (mrc) return mrc;
  PredSlotField P{ctx->slots, ix->field};
  SelGeom g = sel_geom<PredSlotField::E>(ctx->nslots);
  hipLaunchKernelGGL((k_sel_count<PredSlotField>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, ctx->nslots, g.tiles_per_block, ctx->scan.block_counts);
  LAUNCHCHK("k_sel_count(index)");
  hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.block_counts, g.blocks, &ctx->ds->n_out);
  LAUNCHCHK("k_sum_counts");
  unsigned long long n = 0;
  HIPCHK(hipMemcpyAsync(&n, &ctx->ds->n_out, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (n + (n >> 4) + (1u << 16) > ix->cap) {   // too little head room left for appended rows: a new set of columns
    free_columns(*ix);
    uint64_t cap = (n + n / 8 + (1u << 16) + 1023) & ~1023ull;   // head room: rows created later are appended
    if (int rc = dev_alloc_all(ctx, {{ix->ids, cap * sizeof(uint64_t)}, {ix->v64, cap * sizeof(int64_t)}, {ix->v32, (cap + 4) * sizeof(int32_t)}})) return rc;
    ix->cap = cap;
  }
  HIPCHK(hipMemsetAsync(&ctx->ds->wide, 0, sizeof(uint32_t), ctx->stream));
  EmitIndex Em{ctx->slots, ix->ids, ix->v64, ix->v32, &ctx->ds->wide, ctx->chg.slot_pos};
  FinishCount Fin{nullptr};
  hipLaunchKernelGGL((k_sel_write<PredSlotField, EmitIndex, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, Em, Fin, ctx->nslots,
                     g.tiles_per_block, ctx->scan.block_counts);
  LAUNCHCHK("k_sel_write(index)");
  uint32_t wide = 0;
  HIPCHK(hipMemcpyAsync(&wide, &ctx->ds->wide, sizeof(wide), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ix->n = n;
  ix->fits32 = wide == 0;
  ix->content++;             // every position may be another row's now
  ix->layout = ++ctx->layout_seq;
  ix->version = ctx->version;
  ix->has_pos = ctx->chg.slot_pos != nullptr;
  ctx->chg.full_builds++;
  // the log starts (or goes on) only if every index now knows its rows' positions and none is waiting for entries already logged
  if (ctx->chg.slot_pos && ctx->chg.log && !ctx->chg.valid && ctx->indexes.size() <= IX_MAINTAINED_MAX) {
    bool all = true;
    for (auto& o : ctx->indexes) all = all && o.has_pos && o.version == ctx->version;
    if (all) { int rc = reset_chg_log(ctx); if (rc) return rc; ctx->chg.valid = true; }
  }
  return BMX_OK;
}

}  // namespace
