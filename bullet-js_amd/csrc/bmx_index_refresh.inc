// bmx_index_refresh.inc — keeping the indexes current (the rest of the index is bmx_index.inc): the refresh from the merges' change log as a list of named steps,
// fresh_index in front of every query, and the bmx_index_* entry points. It calls the view's patch (bmx_view.inc). Included by bmx.hip (one translation unit).
namespace {

// Bring EVERY maintained index up to date from the change log (they share it), then forget the log. Per index: created rows of its field are
// appended in log order, then every logged row of the field gets its current value. One host sync at the end (appended counts, wide flags).
// An index whose value-ordered view is current goes on being current: the refresh captures the change run and the view is patched with it.
// One refresh as its steps hand it on; index k of ctx->indexes has entry k of both lists.
struct LogRefresh {
  struct Res { unsigned long long added; uint32_t wide; uint32_t changed; unsigned long long run; };     // (wide, changed: the two halves of one result word)
  const unsigned long long* n_dev;   // the log's length, on the device
  uint64_t ub;                       // the host's upper bound of it: what the grids are sized for
  std::vector<Res> res;
  std::vector<char> capture;         // the view of index k takes the change run
};

// Which views can stay current: the view is current now and the run fits a capture buffer. Owns capture[] and the views' capture buffers (ensure_change_run: it may
// synchronise and allocate, which is why it runs in front of the first launch), and marks the mapped run-length words "not written".
int plan_capture(bmx_ctx* ctx, LogRefresh& R) {
  for (size_t k = 0; k < ctx->indexes.size(); k++) ctx->host.hres[HRES_RUN + k] = ~0ull;
  for (size_t k = 0; k < ctx->indexes.size(); k++) {
    const Index& ix = ctx->indexes[k];
    OrderedView& v = ctx->indexes[k].view;
    // the view is current and can stay so: capture the change run (needs room for one entry per log entry)
    if (ctx->view.patching && v.ordered_after && v.s_val && v.ord_content == ix.content && v.ord_fits32 == ix.fits32 && ix.n && ix.n < 0xFFFFFFFFull && R.ub <= VIEW_PATCH_MAX_LOG) {
      if (int crc = ensure_change_run(ctx, v, R.ub)) return crc;
      R.capture[k] = v.cl_cap >= R.ub;
    }
  }
  return BMX_OK;
}

// The launches of index k: created rows appended, every logged row's value written, the change run selected. Owns the index's two scratch words (part_totals[] is free
// between partitions: k < PART_MAX_SHARDS / 2 indexes are maintained), the columns' rows behind ix.n, and the view's cl / cl2 buffers. Reads capture[k]. Enqueue only.
int launch_index_refresh(bmx_ctx* ctx, const LogRefresh& R, size_t k) {
  Index& ix = ctx->indexes[k];
  OrderedView& v = ix.view;
  const uint64_t ub = R.ub;
  unsigned long long* d_added = &ctx->ds->part_totals[2 * k];
  uint32_t* d_wide = reinterpret_cast<uint32_t*>(&ctx->ds->part_totals[2 * k + 1]);
  HIPCHK(hipMemsetAsync(d_added, 0, 2 * sizeof(unsigned long long), ctx->stream));
  PredLogCreated P{ctx->chg.log, R.n_dev, ix.field, ctx->chg.slot_pos};
  SelGeom g = sel_geom<PredLogCreated::E>(ub);
  hipLaunchKernelGGL((k_sel_count<PredLogCreated>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, ub, g.tiles_per_block, ctx->scan.block_counts);
  LAUNCHCHK("k_sel_count(log)");
  EmitAppend Em{ctx->chg.log, ctx->slots, ix.ids, ix.v64, ix.v32, d_wide, ctx->chg.slot_pos, ix.n, ix.cap};
  FinishCount Fin{d_added};
  hipLaunchKernelGGL((k_sel_write<PredLogCreated, EmitAppend, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, Em, Fin, ub, g.tiles_per_block,
                     ctx->scan.block_counts);
  LAUNCHCHK("k_sel_write(log)");
  const uint32_t ublocks = (uint32_t)std::min<uint64_t>((ub + 255) / 256, 4096);
  hipLaunchKernelGGL(k_ix_update, dim3(ublocks), dim3(256), 0, ctx->stream, (const uint2*)ctx->chg.log, R.n_dev, (const Slot*)ctx->slots, ix.field, (const uint32_t*)ctx->chg.slot_pos,
                     ix.v64, ix.v32, d_wide, R.capture[k] ? 2u : (v.ordered_after ? 1u : 0u), v.cl_pos, v.cl_old, (uint64_t)v.cl_cap);
  LAUNCHCHK("k_ix_update");
  if (R.capture[k]) {      // the change run without its holes, in log order (ordered select: no atomics), and its length
    PredChanged PC{v.cl_pos, R.n_dev};
    SelGeom gc = sel_geom<PredChanged::E>(ub);
    hipLaunchKernelGGL((k_sel_count<PredChanged>), dim3(gc.blocks), dim3(SEL_THREADS), 0, ctx->stream, PC, ub, gc.tiles_per_block, ctx->scan.block_counts);
    EmitChanged EC{v.cl_pos, v.cl_old, v.cl2_pos, v.cl2_old};
    FinishCount FC{const_cast<unsigned long long*>(&ctx->host.hres[HRES_RUN + k])};
    hipLaunchKernelGGL((k_sel_write<PredChanged, EmitChanged, FinishCount>), dim3(gc.blocks), dim3(SEL_THREADS), 0, ctx->stream, PC, EC, FC, ub, gc.tiles_per_block, ctx->scan.block_counts);
    LAUNCHCHK("k_sel_write(change run)");
  }
  return BMX_OK;
}

// The refresh's one copy and one synchronisation: the indexes' (added, wide | changed) words go into the mapped result words (the change runs' lengths were
// written there by their selects) and are unpacked. Owns res[].
int read_refresh_results(bmx_ctx* ctx, LogRefresh& R) {
  HIPCHK(hipMemcpyAsync(const_cast<unsigned long long*>(&ctx->host.hres[HRES_TOTALS]), ctx->ds->part_totals, 2 * ctx->indexes.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < ctx->indexes.size(); k++) {
    R.res[k].added = ctx->host.hres[HRES_TOTALS + 2 * k];
    const unsigned long long wc = ctx->host.hres[HRES_TOTALS + 2 * k + 1];
    R.res[k].wide = (uint32_t)wc; R.res[k].changed = (uint32_t)(wc >> 32);
    R.res[k].run = R.capture[k] ? ctx->host.hres[HRES_RUN + k] : 0;
  }
  return BMX_OK;
}

// What the launches did to one index, on the host: owns ix.n, fits32, content and the view's ord_content (through the patch). false = the index is NOT up to date.
bool apply_refresh_result(bmx_ctx* ctx, Index& ix, const LogRefresh::Res& res, bool captured) {
  if (ix.n + res.added > ix.cap) {
    // The appended rows did not fit. The entries it missed are gone with the log, so this index must never be refreshed from a LATER log:
    // without its positions it can only come back through build_index(), and the log stops until every index is fresh again.
    ix.version = ~0ull; ix.has_pos = false; ctx->chg.valid = false;
    return false;
  }
  const uint64_t n0 = ix.n;
  ix.n += res.added; if (res.wide) ix.fits32 = false;
  const bool moved = res.added || res.changed || !ix.view.ordered_after;     // (no view: nobody compared, nobody cares)
  if (moved) ix.content++;
  if (moved && captured && ix.fits32 == ix.view.ord_fits32 && res.run <= ix.view.cl_cap && ix.n < 0xFFFFFFFFull) {
    const int prc = ix.view.ord_fits32 ? patch_view_t<int32_t>(ctx, ix, res.run, n0, res.added) : patch_view_t<int64_t>(ctx, ix, res.run, n0, res.added);
    if (prc == 0) ix.view.ord_content = ix.content;       // the view equals a fresh sort of the columns as they are now
  }
  return true;
}

int refresh_from_log(bmx_ctx* ctx) {
  const auto dbg_t0 = std::chrono::steady_clock::now();
  auto dbg_us = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - dbg_t0).count(); };
  double dbg_sync = 0;
  const size_t nix = ctx->indexes.size();
  LogRefresh R{&ctx->ds->chg_n[ctx->chg.par], ctx->chg.ub, std::vector<LogRefresh::Res>(nix), std::vector<char>(nix, 0)};
  if (nix > IX_MAINTAINED_MAX) return fail(ctx, BMX_ERR_INTERNAL, "index maintenance with more indexes than result words");
  int rc;
  if (R.ub) {
    if (!ensure_hres(ctx)) return fail(ctx, BMX_ERR_NOMEM, "index maintenance: no page-locked memory for the result words");
    if ((rc = plan_capture(ctx, R))) return rc;
    for (size_t k = 0; k < nix; k++)
      if ((rc = launch_index_refresh(ctx, R, k))) return rc;
    if ((rc = read_refresh_results(ctx, R))) return rc;
    dbg_sync = dbg_us();
  }
  if ((rc = reset_chg_log(ctx))) return rc;
  for (size_t k = 0; k < nix; k++)      // (an empty log: nothing moved, every index is up to date as it is)
    if (!R.ub || apply_refresh_result(ctx, ctx->indexes[k], R.res[k], R.capture[k])) ctx->indexes[k].version = ctx->version;
  ctx->chg.incremental++;
  if (ctx->view.debug) std::fprintf(stderr, "bmx: refresh from the log: columns up to date after %.1f us, patches done after %.1f us\n", dbg_sync, dbg_us());
  return BMX_OK;
}

int fresh_index(bmx_ctx* ctx, uint32_t field, Index** out) {
  Index* ix = find_index(ctx, field);
  if (!ix) {  // equals()/range() auto-create a missing index: src/bullet-query.js:194-196, 230-232
    if (ctx->indexes.size() >= IX_MAINTAINED_MAX) ctx->chg.valid = false;   // more indexes than the maintenance pass has result words for: they are rebuilt when stale
    ctx->indexes.emplace_back();
    ix = &ctx->indexes.back();
    ix->field = field;
  }
  if (ix->version != ctx->version) {
    // maintained: every index has its positions recorded, the log is complete, and it is shorter than a quarter of the table
    // (beyond that the rebuild's two sequential passes over the table are cheaper than the log's random accesses)
    bool inc = ctx->chg.valid && ix->has_pos && ctx->chg.ub <= std::max<uint64_t>(ctx->nslots / 8, 1u << 20);
    if (inc) for (auto& o : ctx->indexes) inc = inc && (o.has_pos || &o == ix);
    if (inc) {
      int rc = refresh_from_log(ctx);
      if (rc) return rc;
    }
    if (ix->version != ctx->version) {   // not maintained (or its appended rows did not fit): rebuild from the table
      ctx->chg.valid = false;
      int rc = build_index(ctx, ix);
      if (rc) return rc;
    }
  }
  *out = ix;
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_index_build(bmx_ctx* ctx, uint32_t field) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  return fresh_index(ctx, field, &ix);
}

int bmx_index_drop(bmx_ctx* ctx, uint32_t field) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < ctx->indexes.size(); i++)
    if (ctx->indexes[i].field == field) {
      free_columns(ctx->indexes[i]); ctx->indexes[i].view.release();
      ctx->indexes.erase(ctx->indexes.begin() + (long)i);
      if (ctx->indexes.empty()) ctx->chg.release();   // nothing left to maintain: the merges stop logging and the maintenance memory goes back
      return BMX_OK;
    }
  return fail(ctx, BMX_ERR_NO_INDEX, "no index on that field");
}

int bmx_index_size(bmx_ctx* ctx, uint32_t field, uint64_t* n_out) {
  if (!ctx || !n_out) return fail(ctx, BMX_ERR_INVALID, "bad arguments");
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  int rc = fresh_index(ctx, field, &ix);
  if (rc) return rc;
  *n_out = ix->n;
  return BMX_OK;
}

int bmx_index_refresh_counts(bmx_ctx* ctx, uint64_t* full_builds, uint64_t* incremental_updates) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (full_builds) *full_builds = ctx->chg.full_builds;
  if (incremental_updates) *incremental_updates = ctx->chg.incremental;
  return BMX_OK;
}

int bmx_index_ids(bmx_ctx* ctx, uint32_t field, uint64_t first, uint64_t count, uint64_t* out_ids, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  int rc = fresh_index(ctx, field, &ix);
  if (rc) return rc;
  if (first > ix->n || count > ix->n - first) return fail(ctx, BMX_ERR_INVALID, "bmx_index_ids: range beyond the index (bmx_index_size)");
  if (count == 0) return BMX_OK;
  if (!out_ids) return fail(ctx, BMX_ERR_INVALID, "null output");
  HIPCHK(hipMemcpyAsync(out_ids, ix->ids + first, count * sizeof(uint64_t), host_or_dev(mem), ctx->stream));
  if (mem == BMX_MEM_HOST) HIPCHK(hipStreamSynchronize(ctx->stream));
  return BMX_OK;
}

}  // extern "C"
