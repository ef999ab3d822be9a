// bmx_rows.inc — row projection (bmx_rows.h): bmx_where_rows and its sharded form. The program is bmx_where.inc's (where_prepare), the predicate
// bmx_where_agg.inc's (where_pred) behind a cursor, the mask pass select.h's k_scan_mask into the scans' own mask and counts (ScanScratch), the emit pass
// rows_kernels.h's k_rows_emit. The context keeps the staging of a host-mode answer and what the mask pass leaves the emit pass (RowsScratch). Included by bmx.hip
// (one translation unit), behind everything that was here before it.
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
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  if (int rc = ctx->scan.ensure(ctx, std::max<uint64_t>(ix->n, 1), 0)) return rc;
  const uint32_t nb = (uint32_t)((std::max<uint64_t>(ix->n, 1) + SCAN_BLOCK_ELEMS - 1) / SCAN_BLOCK_ELEMS);
  if (ix->fits32) hipLaunchKernelGGL((k_scan_mask<PredRowsFrom<int32_t>, true>), dim3(nb), dim3(SEL_THREADS), 0, ctx->stream, PredRowsFrom<int32_t>{where_pred<int32_t>(ctx, ix, W), start}, ix->n, ctx->scan.mask, ctx->scan.counts);
  else hipLaunchKernelGGL((k_scan_mask<PredRowsFrom<int64_t>, true>), dim3(nb), dim3(SEL_THREADS), 0, ctx->stream, PredRowsFrom<int64_t>{where_pred<int64_t>(ctx, ix, W), start}, ix->n, ctx->scan.mask, ctx->scan.counts);
  LAUNCHCHK("k_scan_mask(rows)");
  ctx->rows.masked = RowsScratch::Masked{ix->ids, ix->fits32 ? static_cast<const void*>(ix->v32) : static_cast<const void*>(ix->v64), ix->n, ix->layout, ix->fits32, nb};
  return BMX_OK;
}

template <class T>
void rows_launch_emit(bmx_ctx* ctx, const RowsArgs& A, uint32_t nb) {
  const char* s8 = std::getenv("BMX_SCAN_SUB8_BLOCKS");       // the scans' measurement / test switch: blocks beyond which the emit pass takes eight per workgroup
  const uint32_t sub8_blocks = s8 ? (uint32_t)std::strtoul(s8, nullptr, 0) : SCAN_SUB8_BLOCKS;
  if (nb > sub8_blocks) hipLaunchKernelGGL((k_rows_emit<T, 8>), dim3((nb + 7) / 8), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.mask, ctx->scan.counts, nb, A);
  else hipLaunchKernelGGL((k_rows_emit<T, 1>), dim3(nb), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.mask, ctx->scan.counts, nb, A);
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
  if (M.fits32) rows_launch_emit<int32_t>(ctx, A, M.nb); else rows_launch_emit<int64_t>(ctx, A, M.nb);
  LAUNCHCHK("k_rows_emit");
  return BMX_OK;
}

// ... for a host-mode answer: into the context's staging, columns of stride `scap` (the caller's cap, cut at the index size: no more rows can come)
int rows_emit_staged(bmx_ctx* ctx, uint32_t base_field, const RowsWant& w, uint64_t scap) {
  RowsScratch& s = ctx->rows;
  const uint64_t words = std::max<uint64_t>(scap * (1 + rows_cols(w)), 1);
  if (words > s.stage_words || !s.stage_res) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.stage_words = 0;
    if (int rc = dev_alloc_all(ctx, {{s.stage, words * 8}, {s.stage_res, sizeof(bmx_rows_res)}})) return rc;
    s.stage_words = words;
  }
  uint64_t* d_ids = reinterpret_cast<uint64_t*>(s.stage);
  int64_t* d_val = reinterpret_cast<int64_t*>(s.stage) + scap;
  return rows_emit(ctx, base_field, w, scap, d_ids, d_val, d_val + (uint64_t)w.nfields * scap, s.stage_res);
}

// second half of a host-mode answer: the record, then the rows it says were written, column by column from the staging (stride scap) to the caller's columns
// (stride cap), `at` rows in
int rows_collect(bmx_ctx* ctx, const RowsWant& w, uint64_t scap, uint64_t cap, uint64_t at, uint64_t* out_ids, int64_t* out_val, int64_t* out_ts, bmx_rows_res* res) {
  const RowsScratch& s = ctx->rows;
  HIPCHK(hipMemcpyAsync(res, s.stage_res, sizeof(bmx_rows_res), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t m = res->n_out;
  if (!m) return BMX_OK;
  if (m > scap || at + m > cap) return fail(ctx, BMX_ERR_INTERNAL, "bmx_where_rows: more rows than room");
  const unsigned long long* st = s.stage;
  HIPCHK(hipMemcpyAsync(out_ids + at, st, m * 8, hipMemcpyDeviceToHost, ctx->stream));
  for (uint32_t f = 0; f < w.nfields; f++) {
    HIPCHK(hipMemcpyAsync(out_val + (uint64_t)f * cap + at, st + (1 + (uint64_t)f) * scap, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (w.flags & BMX_ROWS_TS) HIPCHK(hipMemcpyAsync(out_ts + (uint64_t)f * cap + at, st + (1 + (uint64_t)w.nfields + f) * scap, m * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
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
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
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
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  if (start_shard >= c->N) return fail(c, BMX_ERR_INVALID, "bmx_comm_where_rows: start_shard is no shard");
  DevGuard guard;
  bmx_rows_res tot{};
  bool cut = false;                      // some shard had a selected node that was not delivered: tot.next_shard / next_pos name the first such node
  uint64_t delivered = 0;
  const int rc = comm_two_phase(c,
    [&](uint32_t g, bmx_ctx* x) {         // every shard's index up to date (its stamp counts even in front of the cursor); the mask pass from the cursor on
      if (int erc = enter(x)) return erc;
      if (g >= start_shard) return rows_mask(x, base_field, W, g == start_shard ? start_pos : 0);
      Index* ix;
      if (int frc = fresh_index(x, base_field, &ix)) return frc;
      x->rows.masked.layout = ix->layout;
      return (int)BMX_OK;
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
      if (!cut) {
        tot.next_shard = g; tot.next_pos = r.next_pos;
        cut = r.n_match > r.n_out;
      }
      return (int)BMX_OK;
    });
  if (rc) return rc;
  tot.n_out = delivered; tot.reserved = 0;
  *res = tot;
  return BMX_OK;
}

}  // extern "C"
