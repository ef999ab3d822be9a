// bmx_update.inc — update and delete by query (bmx_update.h): bmx_where_update and its sharded form. The program, the mask pass (select.h's k_scan_mask over the
// predicate behind a cursor and a look at the source, update_kernels.h PredUpd, into the scans' own mask and counts), the entry guards and the cursor steps of the
// sharded form are bmx_where.inc's (where_prepare, where_mask_pass, where_enter, where_comm_guard, where_stamp_only, page_note); the emit pass is
// update_kernels.h's k_upd_emit, in bmx_scan.inc's geometry (emit_dispatch), into the context's staging slab of records (UpdScratch). The write itself is
// merge_core's, called as merge_records_internal calls it for the communicator: this file is one more caller of the merge and changes nothing in it. Included by
// bmx.hip (one translation unit), behind everything that was here before it.
namespace {

// what one call writes, checked and brought into the form the kernels take (UpdSrc)
struct UpdWant { uint32_t target; UpdSrc S; int64_t ts; bool force; };

int upd_prepare(uint32_t base_field, uint32_t target_field, uint32_t op, uint32_t src_field, int64_t operand, int64_t ts, uint32_t flags, uint64_t cap,
                const bmx_upd_res* res, UpdWant* out, std::string* why) {
  if (op > BMX_UPD_ADD) { *why = "bmx_where_update: unknown op"; return BMX_ERR_INVALID; }
  if (flags & ~BMX_UPD_FORCE) { *why = "bmx_where_update: unknown flag bits in flags"; return BMX_ERR_INVALID; }
  if (op == BMX_UPD_DELETE && !(flags & BMX_UPD_FORCE)) { *why = "bmx_where_update: BMX_UPD_DELETE needs BMX_UPD_FORCE (the merge has no tombstone path)"; return BMX_ERR_INVALID; }
  if (cap > BMX_UPD_MAX_CAP) { *why = "bmx_where_update: cap above BMX_UPD_MAX_CAP (the merge's batch limit): page with the cursor"; return BMX_ERR_INVALID; }
  if (!res) { *why = "bmx_where_update: null result record"; return BMX_ERR_INVALID; }
  if (ts < 0 || ts > TS_MAX) { *why = "bmx_where_update: ts outside [0, 2^53-1]"; return BMX_ERR_RANGE; }
  if ((op == BMX_UPD_SET || op == BMX_UPD_ADD) && (operand < -VAL_MAX || operand > VAL_MAX)) { *why = "bmx_where_update: |operand| > 2^53-1"; return BMX_ERR_RANGE; }
  UpdWant w{};
  w.target = target_field; w.ts = ts; w.force = (flags & BMX_UPD_FORCE) != 0;
  if (op == BMX_UPD_SET) w.S = UpdSrc{UPD_SRC_NONE, 0u, operand};
  else if (op == BMX_UPD_DELETE) w.S = UpdSrc{UPD_SRC_NONE, 0u, VAL_DELETED};
  else w.S = UpdSrc{src_field == base_field ? UPD_SRC_COLUMN : UPD_SRC_PROBE, src_field, op == BMX_UPD_ADD ? operand : 0};
  *out = w;
  return BMX_OK;
}

// the staging of one call: `scap` records and winner indices, the words between the passes, the merge's outputs; the counter shards are zero between two calls
int upd_ensure(bmx_ctx* ctx, uint64_t scap) {
  UpdScratch& s = ctx->upd;
  if (!s.counts) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (int rc = dev_alloc_all(ctx, {{s.counts, sizeof(UpdCounts)}, {s.ctr, UPD_CTR_SHARDS * UPD_CTR_STRIDE * sizeof(unsigned long long)}, {s.n_applied, sizeof(unsigned long long)},
                                     {s.stats, sizeof(bmx_merge_stats)}, {s.stage_res, sizeof(bmx_upd_res)}}))
      return rc;
    HIPCHK(hipMemsetAsync(s.ctr, 0, UPD_CTR_SHARDS * UPD_CTR_STRIDE * sizeof(unsigned long long), ctx->stream));
  }
  const uint64_t want = std::max<uint64_t>(scap, 1);
  if (want > s.cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.cap = 0;
    if (int rc = dev_alloc_all(ctx, {{s.recs, want * sizeof(bmx_delta_rec)}, {s.applied, want * sizeof(uint32_t)}, {s.ids, want * sizeof(uint64_t)}})) return rc;
    s.cap = want;
  }
  return BMX_OK;
}

// Pass 1 of one call on one context: the base index brought up to date, the mask of the WRITABLE positions from `start` on and the counts per block into the
// scans' scratch, the nodes without source and outside the range into the counter shards. The context has been entered.
int upd_mask(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, const UpdWant& w, uint64_t start) {
  return where_mask_pass(ctx, base_field, W, "launch k_scan_mask(update)", &ctx->upd.masked,
    [&](const auto& P) { using T = decltype(where_value(P)); constexpr bool C = where_clocks<decltype(P)>; return PredUpd<T, C>{PredRowsFrom<T, C>{P, start}, w.S, ctx->upd.ctr}; },
    [](bmx_ctx* x) { return upd_ensure(x, 0); });      // (the counter shards, in front of the launch that reads their address)
}

// Behind upd_mask: the emit pass into min(cap, index size) records, the one wait, the merge, the finish kernel. d_out_ids (may be null) and d_res are device
// memory; *hc receives the counts the host waited for.
int upd_write(bmx_ctx* ctx, const UpdWant& w, uint64_t cap, uint64_t* d_out_ids, bmx_upd_res* d_res, UpdCounts* hc) {
  UpdScratch& s = ctx->upd;
  const RowsScratch::Masked M = s.masked;
  const uint64_t scap = std::min<uint64_t>(cap, M.n);        // no more records can come
  if (int rc = upd_ensure(ctx, scap)) return rc;
  UpdArgs A{};
  A.ids = M.ids; A.v = M.v; A.slots = ctx->slots; A.nslots = ctx->nslots;
  A.recs = s.recs; A.counts = s.counts; A.ctr = s.ctr;
  A.cap = scap; A.n = M.n; A.layout = M.layout; A.ts = w.ts; A.S = w.S; A.target = w.target;
  by_width(M.fits32, [&](auto t) {
    emit_dispatch(M.nb, [&](auto B, uint32_t wgs) {
      hipLaunchKernelGGL((k_upd_emit<decltype(t), decltype(B)::value>), dim3(wgs), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.mask, ctx->scan.counts, M.nb, A);
    });
  });
  LAUNCHCHK("k_upd_emit");
  // the one wait: the merge's grid, its workspace and a growth of the table are sized on the host by the batch size
  HIPCHK(hipMemcpyAsync(hc, s.counts, sizeof(UpdCounts), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (hc->n_sent > scap) return fail(ctx, BMX_ERR_INTERNAL, "bmx_where_update: more records than room");
  if (hc->n_sent) {
    // The DEFAULT path (claims and lists), although the keys are unique by construction: a BMX_MERGE_UNIQUE_KEYS batch without force is not written into the
    // index change log (plan_change_log), so every maintained index, view and standing query would be rebuilt by its next use.
    const MergeMode mode = w.force ? MODE_PUT : MergeMode{BMX_INSERT_DELTA, false, false, false, false};
    if (int rc = merge_core(ctx, MergeIn{hc->n_sent, nullptr, nullptr, nullptr, nullptr, s.recs}, MergeOut{s.applied, reinterpret_cast<uint64_t*>(s.n_applied), nullptr, s.stats}, mode)) return rc;
  }
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((hc->n_sent + UPD_FIN_THREADS - 1) / UPD_FIN_THREADS, 1), 1024);
  hipLaunchKernelGGL(k_upd_finish, dim3(d_out_ids ? blocks : 1u), dim3(UPD_FIN_THREADS), 0, ctx->stream, s.recs, s.applied, s.n_applied, s.stats, s.counts, &ctx->ds->row_count,
                     d_out_ids, d_res, hc->n_sent ? 1u : 0u);
  LAUNCHCHK("k_upd_finish");
  return BMX_OK;
}

// a host-mode answer: the record and the ids through the staging, `at` ids into out_ids (room: cap)
int upd_write_host(bmx_ctx* ctx, const UpdWant& w, uint64_t cap, uint64_t at, uint64_t* out_ids, bmx_upd_res* res) {
  UpdScratch& s = ctx->upd;
  UpdCounts hc;
  if (int rc = upd_ensure(ctx, std::min<uint64_t>(cap, s.masked.n))) return rc;      // before s.ids is handed on: growing the staging moves it
  if (int rc = upd_write(ctx, w, cap, out_ids && cap ? s.ids : nullptr, s.stage_res, &hc)) return rc;
  bmx_upd_res r;
  HIPCHK(hipMemcpyAsync(&r, s.stage_res, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (r.n_applied > r.n_sent || r.n_sent > cap) return fail(ctx, BMX_ERR_INTERNAL, "bmx_where_update: more rows than room");
  if (out_ids && r.n_applied) {
    HIPCHK(hipMemcpyAsync(out_ids + at, s.ids, r.n_applied * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  *res = r;
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_where_update(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t target_field, uint32_t op,
                     uint32_t src_field, int64_t operand, int64_t ts, uint32_t flags, uint64_t start_pos, uint64_t cap, uint64_t* out_ids, bmx_upd_res* res, int mem) {
  WhereProg W;
  UpdWant w;
  std::string why;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int rc = upd_prepare(base_field, target_field, op, src_field, operand, ts, flags, cap, res, &w, &why)) return fail(ctx, rc, why);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (int rc = upd_mask(ctx, base_field, W, w, start_pos)) return rc;
  if (mem == BMX_MEM_HOST) return upd_write_host(ctx, w, cap, 0, out_ids, res);
  UpdCounts hc;
  return upd_write(ctx, w, cap, cap ? out_ids : nullptr, res, &hc);
}

int bmx_comm_where_update(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t target_field, uint32_t op,
                          uint32_t src_field, int64_t operand, int64_t ts, uint32_t flags, uint32_t start_shard, uint64_t start_pos, uint64_t cap, uint64_t* out_ids,
                          bmx_upd_res* res) {
  WhereProg W;
  UpdWant w;
  std::string why;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = upd_prepare(base_field, target_field, op, src_field, operand, ts, flags, cap, res, &w, &why)) return fail(c, rc, why);
  if (int rc = where_comm_guard(c, "bmx_comm_where_update", start_shard)) return rc;
  DevGuard guard;
  bmx_upd_res tot{};
  bool cut = false;                      // some shard had a writable node that was not sent: tot.next_shard / next_pos name the first such node
  bool failed = false;
  uint64_t sent = 0, applied = 0;
  const int rc = comm_two_phase(c,
    [&](uint32_t g, bmx_ctx* x) {         // every shard's index up to date (its stamp counts even in front of the cursor); the mask pass from the cursor on
      if (int erc = enter(x)) return erc;
      return g < start_shard ? where_stamp_only(x, base_field, &x->upd.masked) : upd_mask(x, base_field, W, w, g == start_shard ? start_pos : 0);
    },
    [&](uint32_t g, bmx_ctx* x) {         // shard after shard: its own nodes with the room that is left (none: the shard is counted only)
      tot.layout += x->upd.masked.layout;
      if (failed) return (int)BMX_OK;     // a shard in front could not write: the shards behind it are left as they are
      int crc = enter(x);
      if (g < start_shard) {
        uint64_t rows = 0;
        if (!crc) crc = bmx_row_count(x, &rows);
        tot.n_rows += rows;
        failed = crc != BMX_OK;
        return crc;
      }
      bmx_upd_res r;
      if (!crc) crc = upd_write_host(x, w, cap - sent, applied, out_ids, &r);
      if (crc) { failed = true; return crc; }
      tot.n_match += r.n_match; tot.n_nosrc += r.n_nosrc; tot.n_range += r.n_range; tot.n_rows += r.n_rows;
      sent += r.n_sent; applied += r.n_applied;
      page_note(cut, tot, g, r.next_pos, r.n_match - r.n_nosrc - r.n_range > r.n_sent);
      return (int)BMX_OK;
    });
  if (rc) return rc;
  tot.n_sent = sent; tot.n_applied = applied; tot.reserved = 0;
  *res = tot;
  return BMX_OK;
}

}  // extern "C"
