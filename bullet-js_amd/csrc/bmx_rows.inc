// bmx_rows.inc — row projection (bmx_rows.h): bmx_where_rows and its sharded form. The program, the mask pass (select.h's k_scan_mask over the predicate behind a
// cursor, into the scans' own mask and counts), the entry guards and the cursor steps of the sharded form are bmx_where.inc's (where_prepare, where_mask_pass,
// where_enter, where_comm_guard, where_stamp_only, page_note), the emit pass is rows_kernels.h's k_rows_emit in bmx_scan.inc's geometry (emit_dispatch). The
// context keeps the staging of a host-mode answer and what the mask pass leaves the emit pass (RowsScratch); rows_stage and rows_copy_cols, which grow that
// staging and copy columns out of it, serve the join projection as well. Included by bmx.hip (one translation unit), behind everything that was here before it.
namespace {

struct RowsWant { uint32_t nfields; const uint32_t* fields; uint32_t flags; };
inline uint32_t rows_cols(const RowsWant& w) { return w.nfields * ((w.flags & BMX_ROWS_TS) ? 2u : 1u); }     // columns of 8-byte cells behind the id column

const char* rows_bad_args(const RowsWant& w, uint64_t cap, const uint64_t* out_ids, const int64_t* out_val, const int64_t* out_ts, const bmx_rows_res* res) {
  if (w.nfields > BMX_ROWS_MAX_FIELDS) return "bmx_where_rows: more than BMX_ROWS_MAX_FIELDS fields";
  if (w.nfields && !w.fields) return "bmx_where_rows: null fields";
  if (w.flags & ~BMX_ROWS_TS) return "bmx_where_rows: unknown flag bits in flags";
  if (!res) return "bmx_where_rows: null result record";
  if (cap) {
    if (!out_ids) return "bmx_where_rows: null out_ids";
    if (w.nfields && !out_val) return "bmx_where_rows: null out_val";
    if (w.nfields && (w.flags & BMX_ROWS_TS) && !out_ts) return "bmx_where_rows: null out_ts";
  }
  return nullptr;
}

// Pass 1 of one call on one context: the base index brought up to date, the mask of the selected positions from `start` on and the counts per block into the
// scans' scratch. The context has been entered.
int rows_mask(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint64_t start) {
  return where_mask_pass(ctx, base_field, W, "launch k_scan_mask(rows)", &ctx->rows.masked, [&](const auto& P) { return PredRowsFrom<decltype(where_value(P)), where_clocks<decltype(P)>>{P, start}; });
}

// Pass 2 behind rows_mask: up to `cap` rows into the columns d_ids / d_val / d_ts of stride cap and the record into d_res (all device memory).
int rows_emit(bmx_ctx* ctx, uint32_t base_field, const RowsWant& w, uint64_t cap, uint64_t* d_ids, int64_t* d_val, int64_t* d_ts, bmx_rows_res* d_res) {
  const RowsScratch::Masked& M = ctx->rows.masked;
  RowsArgs A{};
  A.ids = M.ids; A.v = M.v; A.slots = ctx->slots; A.nslots = ctx->nslots;
  A.out_ids = d_ids; A.out_val = d_val; A.out_ts = d_ts; A.res = d_res;
  A.cap = cap; A.n = M.n; A.layout = M.layout;
  A.nfields = w.nfields; A.base_field = base_field; A.with_ts = (w.flags & BMX_ROWS_TS) ? 1u : 0u;
  A.nt = std::min<uint64_t>(cap, M.n) * 8 * (1 + rows_cols(w)) > SCAN_NT_BYTES ? 1u : 0u;
  for (uint32_t f = 0; f < w.nfields; f++) A.field[f] = w.fields[f];
  by_width(M.fits32, [&](auto t) {
    emit_dispatch(M.nb, [&](auto B, uint32_t wgs) {
      hipLaunchKernelGGL((k_rows_emit<decltype(t), decltype(B)::value>), dim3(wgs), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.mask, ctx->scan.counts, M.nb, A);
    });
  });
  LAUNCHCHK("k_rows_emit");
  return BMX_OK;
}

// room for `words` 8-byte words of staged columns, and the result record
int rows_stage(bmx_ctx* ctx, uint64_t words) {
  RowsScratch& s = ctx->rows;
  words = std::max<uint64_t>(words, 1);
  if (words > s.stage_words || !s.stage_res) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.stage_words = 0;
    if (int rc = dev_alloc_all(ctx, {{s.stage, words * 8}, {s.stage_res, sizeof(bmx_rows_res)}})) return rc;
    s.stage_words = words;
  }
  return BMX_OK;
}

// ... for a host-mode answer: into the context's staging, columns of stride `scap` (the caller's cap, cut at the index size: no more rows can come)
int rows_emit_staged(bmx_ctx* ctx, uint32_t base_field, const RowsWant& w, uint64_t scap) {
  if (int rc = rows_stage(ctx, scap * (1 + rows_cols(w)))) return rc;
  uint64_t* d_ids = reinterpret_cast<uint64_t*>(ctx->rows.stage);
  int64_t* d_val = reinterpret_cast<int64_t*>(ctx->rows.stage) + scap;
  return rows_emit(ctx, base_field, w, scap, d_ids, d_val, d_val + (uint64_t)w.nfields * scap, ctx->rows.stage_res);
}

// `m` rows of one block of staged columns (st: the id column, the values of w's fields, then their clocks; stride scap) to the caller's columns (stride cap),
// `at` rows in. Enqueued; the caller waits.
int rows_copy_cols(bmx_ctx* ctx, const RowsWant& w, const unsigned long long* st, uint64_t scap, uint64_t m, uint64_t cap, uint64_t at, uint64_t* out_ids, int64_t* out_val, int64_t* out_ts) {
  HIPCHK(hipMemcpyAsync(out_ids + at, st, m * 8, hipMemcpyDeviceToHost, ctx->stream));
  for (uint32_t f = 0; f < w.nfields; f++) {
    HIPCHK(hipMemcpyAsync(out_val + (uint64_t)f * cap + at, st + (1 + (uint64_t)f) * scap, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (w.flags & BMX_ROWS_TS) HIPCHK(hipMemcpyAsync(out_ts + (uint64_t)f * cap + at, st + (1 + (uint64_t)w.nfields + f) * scap, m * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  return BMX_OK;
}

// second half of a host-mode answer: the record, then the rows it says were written, column by column from the staging (stride scap) to the caller's columns
// (stride cap), `at` rows in
int rows_collect(bmx_ctx* ctx, const RowsWant& w, uint64_t scap, uint64_t cap, uint64_t at, uint64_t* out_ids, int64_t* out_val, int64_t* out_ts, bmx_rows_res* res) {
  HIPCHK(hipMemcpyAsync(res, ctx->rows.stage_res, sizeof(bmx_rows_res), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t m = res->n_out;
  if (!m) return BMX_OK;
  if (m > scap || at + m > cap) return fail(ctx, BMX_ERR_INTERNAL, "bmx_where_rows: more rows than room");
  if (int rc = rows_copy_cols(ctx, w, ctx->rows.stage, scap, m, cap, at, out_ids, out_val, out_ts)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_where_rows(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t nfields, const uint32_t* fields,
                   uint32_t flags, uint64_t start_pos, uint64_t cap, uint64_t* out_ids, int64_t* out_val, int64_t* out_ts, bmx_rows_res* res, int mem) {
  WhereProg W;
  const RowsWant w{nfields, fields, flags};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = rows_bad_args(w, cap, out_ids, out_val, out_ts, res)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (int rc = rows_mask(ctx, base_field, W, start_pos)) return rc;
  if (mem == BMX_MEM_DEVICE) return rows_emit(ctx, base_field, w, cap, out_ids, out_val, out_ts, res);
  const uint64_t scap = std::min<uint64_t>(cap, ctx->rows.masked.n);
  if (int rc = rows_emit_staged(ctx, base_field, w, scap)) return rc;
  bmx_rows_res r;
  if (int rc = rows_collect(ctx, w, scap, cap, 0, out_ids, out_val, out_ts, &r)) return rc;
  *res = r;
  return BMX_OK;
}

int bmx_comm_where_rows(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t nfields,
                        const uint32_t* fields, uint32_t flags, uint32_t start_shard, uint64_t start_pos, uint64_t cap, uint64_t* out_ids, int64_t* out_val,
                        int64_t* out_ts, bmx_rows_res* res) {
  WhereProg W;
  const RowsWant w{nfields, fields, flags};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = rows_bad_args(w, cap, out_ids, out_val, out_ts, res)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c, "bmx_comm_where_rows", start_shard)) return rc;
  DevGuard guard;
  bmx_rows_res tot{};
  bool cut = false;                      // some shard had a selected node that was not delivered: tot.next_shard / next_pos name the first such node
  uint64_t delivered = 0;
  const int rc = comm_two_phase(c,
    [&](uint32_t g, bmx_ctx* x) {         // every shard's index up to date (its stamp counts even in front of the cursor); the mask pass from the cursor on
      if (int erc = enter(x)) return erc;
      return g < start_shard ? where_stamp_only(x, base_field, &x->rows.masked) : rows_mask(x, base_field, W, g == start_shard ? start_pos : 0);
    },
    [&](uint32_t g, bmx_ctx* x) {         // shard after shard: the emit pass with the room that is left (none: the shard is counted only), then its rows
      tot.layout += x->rows.masked.layout;
      if (g < start_shard) return (int)BMX_OK;
      int crc = enter(x);
      const uint64_t room = cap - delivered, scap = std::min<uint64_t>(room, x->rows.masked.n);
      if (!crc) crc = rows_emit_staged(x, base_field, w, scap);
      bmx_rows_res r;
      if (!crc) crc = rows_collect(x, w, scap, cap, delivered, out_ids, out_val, out_ts, &r);
      if (crc) return crc;
      tot.n_match += r.n_match; delivered += r.n_out;
      page_note(cut, tot, g, r.next_pos, r.n_match > r.n_out);
      return (int)BMX_OK;
    });
  if (rc) return rc;
  tot.n_out = delivered; tot.reserved = 0;
  *res = tot;
  return BMX_OK;
}

}  // extern "C"
