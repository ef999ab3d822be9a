// bmx_join_rows.inc — join projection (bmx_join_rows.h): bmx_where_join_rows, bmx_where_map_rows and their sharded forms. The programs are bmx_where.inc's
// (where_prepare), and so are the width dispatch of the build sweep, the inner join's mask pass, the entry guards and the cursor steps of the sharded forms
// (where_sweep, where_mask_pass, where_enter, where_comm_guard, where_stamp_only, page_note); the left join's mask pass is bmx_rows.inc's (rows_mask), the emit
// pass's geometry bmx_scan.inc's (emit_dispatch), the map's scratch and its clean protocol bmx_join.inc's (join_scratch: the same table bmx_where_join_group
// uses), the kernels join_rows_kernels.h. A host-mode answer comes down through the row projection's staging columns (RowsScratch::stage, grown by rows_stage,
// copied out by rows_copy_cols) and the lookup joins' result record (JoinScratch::stage_res); a host-mode list goes up through JoinScratch::stage_keys /
// stage_vals. Included by bmx.hip (one translation unit), behind everything that was here before it.
namespace {

struct JRowsWant {
  uint32_t link_field; RowsWant o, in; uint32_t flags; uint64_t cap;
  uint64_t* out_ids; int64_t* out_val; int64_t* out_ts; uint64_t* out_in_ids; int64_t* out_in_val; int64_t* out_in_ts; bmx_jrows_res* res;
};
inline bool jrows_inner(const JRowsWant& w) { return (w.flags & BMX_JROWS_INNER) != 0u; }
inline uint32_t jrows_cols(const JRowsWant& w) { return 2u + rows_cols(w.o) + rows_cols(w.in); }   // staging columns: both id columns and the cells

const char* jrows_bad_args(const JRowsWant& w, uint64_t map_cap, const char* map_cap_text) {
  if (w.o.nfields > BMX_ROWS_MAX_FIELDS) return "more than BMX_ROWS_MAX_FIELDS fields";
  if (w.in.nfields > BMX_ROWS_MAX_FIELDS) return "more than BMX_ROWS_MAX_FIELDS inner fields";
  if (w.o.nfields && !w.o.fields) return "null fields";
  if (w.in.nfields && !w.in.fields) return "null in_fields";
  if (w.flags & ~(BMX_ROWS_TS | BMX_JROWS_INNER)) return "unknown flag bits in flags";
  if (!w.res) return "null result record";
  if (w.cap) {
    const bool ts = (w.flags & BMX_ROWS_TS) != 0u;
    if (!w.out_ids) return "null out_ids";
    if (w.o.nfields && !w.out_val) return "null out_val";
    if (w.o.nfields && ts && !w.out_ts) return "null out_ts";
    if (!w.out_in_ids) return "null out_in_ids";
    if (w.in.nfields && !w.out_in_val) return "null out_in_val";
    if (w.in.nfields && ts && !w.out_in_ts) return "null out_in_ts";
  }
  if (map_cap == 0 || map_cap > BMX_JOIN_MAX_MAP) return map_cap_text;
  if (w.link_field == BMX_AGG_NO_FIELD) return "no link field";
  return nullptr;
}

JRowsWant jrows_want(uint32_t link_field, uint32_t nfields, const uint32_t* fields, uint32_t n_in_fields, const uint32_t* in_fields, uint32_t flags, uint64_t cap,
                     uint64_t* out_ids, int64_t* out_val, int64_t* out_ts, uint64_t* out_in_ids, int64_t* out_in_val, int64_t* out_in_ts, bmx_jrows_res* res) {
  return JRowsWant{link_field, RowsWant{nfields, fields, flags & BMX_ROWS_TS}, RowsWant{n_in_fields, in_fields, flags & BMX_ROWS_TS}, flags, cap,
                   out_ids, out_val, out_ts, out_in_ids, out_in_val, out_in_ts, res};
}

// the map from the inner program: one sweep of the inner base field's index
int jrows_build(bmx_ctx* ctx, const JoinArgs& J, uint32_t in_base_field, const WhereProg& WI, uint32_t key_field) {
  Index* ix;
  if (int rc = fresh_index(ctx, in_base_field, &ix)) return rc;
  const uint32_t ksrc = where_agg_source(key_field, in_base_field);
  where_sweep_c(ctx, ix, WI, [&](const auto& P, uint32_t blocks) {
    hipLaunchKernelGGL((k_jrows_build<decltype(where_value(P)), where_clocks<decltype(P)>>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, J, key_field, ksrc);
  });
  LAUNCHCHK("k_jrows_build");
  return BMX_OK;
}

// the map from `n` pairs in device memory
int jrows_insert_list(bmx_ctx* ctx, const JoinArgs& J, const int64_t* d_keys, const uint64_t* d_ids, uint64_t n) {
  hipLaunchKernelGGL(k_jrows_insert, dim3(semi_grid(n)), dim3(JOIN_THREADS), 0, ctx->stream, reinterpret_cast<const long long*>(d_keys),
                     reinterpret_cast<const unsigned long long*>(d_ids), n, J);
  LAUNCHCHK("k_jrows_insert");
  return BMX_OK;
}

// ... from `n` pairs in HOST memory, through the staging of the map's scratch (n <= the cap the scratch was sized for)
int jrows_insert_staged(bmx_ctx* ctx, const JoinArgs& J, const int64_t* keys, const uint64_t* ids, uint64_t n) {
  HIPCHK(hipMemcpyAsync(ctx->join.stage_keys, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->join.stage_vals, ids, n * 8, hipMemcpyHostToDevice, ctx->stream));
  return jrows_insert_list(ctx, J, reinterpret_cast<const int64_t*>(ctx->join.stage_keys), reinterpret_cast<const uint64_t*>(ctx->join.stage_vals), n);
}

inline JRowsLink jrows_link(const JoinArgs& J, uint32_t link_field, uint32_t base_field) {
  return JRowsLink{J.map, J.S, J.slots, J.cap, link_field, where_agg_source(link_field, base_field)};
}

// Pass 1 behind a complete map: the left join's is the row projection's; the inner join's takes the link lookup into the selection. Leaves the emit pass what
// rows_mask leaves it (ctx->rows.masked).
int jrows_mask(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, const JRowsWant& w, const JoinArgs& J, uint64_t start) {
  if (!jrows_inner(w)) return rows_mask(ctx, base_field, W, start);
  const JRowsLink L = jrows_link(J, w.link_field, base_field);
  return where_mask_pass(ctx, base_field, W, "launch k_scan_mask(join rows)", &ctx->rows.masked, [&](const auto& P) {
    using T = decltype(where_value(P));
    constexpr bool C = where_clocks<decltype(P)>;
    return PredJRowsFrom<T, C>{PredRowsFrom<T, C>{P, start}, L};
  });
}

// the call's last kernel: the map back to empty, the record completed
int jrows_finish(bmx_ctx* ctx, const JoinArgs& J, bmx_jrows_res* d_res, uint32_t rows) {
  hipLaunchKernelGGL(k_jrows_finish, dim3(semi_finish_grid(J.slots)), dim3(JOIN_THREADS), 0, ctx->stream, J, d_res, rows);
  LAUNCHCHK("k_jrows_finish");
  ctx->join.clean = true;
  return BMX_OK;
}

// Pass 2 behind jrows_mask, and the finish: up to `cap` rows into six columns of stride cap and the record into d_res (all device memory).
int jrows_emit(bmx_ctx* ctx, uint32_t base_field, const JRowsWant& w, const JoinArgs& J, uint64_t cap, uint64_t* d_ids, int64_t* d_val, int64_t* d_ts,
               uint64_t* d_in_ids, int64_t* d_in_val, int64_t* d_in_ts, bmx_jrows_res* d_res) {
  const RowsScratch::Masked& M = ctx->rows.masked;
  JRowsArgs A{};
  RowsArgs& R = A.R;
  R.ids = M.ids; R.v = M.v; R.slots = ctx->slots; R.nslots = ctx->nslots;
  R.out_ids = d_ids; R.out_val = d_val; R.out_ts = d_ts; R.res = reinterpret_cast<bmx_rows_res*>(d_res);   // (its first four words are bmx_rows_res's)
  R.cap = cap; R.n = M.n; R.layout = M.layout;
  R.nfields = w.o.nfields; R.base_field = base_field; R.with_ts = (w.flags & BMX_ROWS_TS) ? 1u : 0u;
  R.nt = std::min<uint64_t>(cap, M.n) * 8 * jrows_cols(w) > SCAN_NT_BYTES ? 1u : 0u;
  for (uint32_t f = 0; f < w.o.nfields; f++) R.field[f] = w.o.fields[f];
  A.L = jrows_link(J, w.link_field, base_field);
  A.out_in_ids = d_in_ids; A.out_in_val = d_in_val; A.out_in_ts = d_in_ts;
  A.n_joined = &J.S->nout;
  A.n_in_fields = w.in.nfields;
  for (uint32_t g = 0; g < w.in.nfields; g++) A.in_field[g] = w.in.fields[g];
  by_width(M.fits32, [&](auto t) {
    emit_dispatch(M.nb, [&](auto B, uint32_t wgs) {
      hipLaunchKernelGGL((k_jrows_emit<decltype(t), decltype(B)::value>), dim3(wgs), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.mask, ctx->scan.counts, M.nb, A);
    });
  });
  LAUNCHCHK("k_jrows_emit");
  return jrows_finish(ctx, J, d_res, 1u);
}

static_assert(offsetof(bmx_jrows_res, next_pos) == offsetof(bmx_rows_res, next_pos) && offsetof(bmx_jrows_res, layout) == offsetof(bmx_rows_res, layout) &&
              offsetof(bmx_jrows_res, n_match) == 0 && offsetof(bmx_jrows_res, n_out) == 8, "rows_emit_block writes next_pos through a bmx_rows_res pointer");

// ... for a host-mode answer: into the staging, columns of stride `scap`: ids, the outer cells (values, then clocks), inner ids, the inner cells
int jrows_emit_staged(bmx_ctx* ctx, uint32_t base_field, const JRowsWant& w, const JoinArgs& J, uint64_t scap) {
  if (int rc = rows_stage(ctx, scap * jrows_cols(w))) return rc;
  const RowsScratch& s = ctx->rows;
  uint64_t* d_ids = reinterpret_cast<uint64_t*>(s.stage);
  int64_t* d_val = reinterpret_cast<int64_t*>(s.stage) + scap;
  int64_t* d_ts = d_val + (uint64_t)w.o.nfields * scap;
  uint64_t* d_in_ids = reinterpret_cast<uint64_t*>(s.stage) + (1 + (uint64_t)rows_cols(w.o)) * scap;
  int64_t* d_in_val = reinterpret_cast<int64_t*>(d_in_ids) + scap;
  return jrows_emit(ctx, base_field, w, J, scap, d_ids, d_val, d_ts, d_in_ids, d_in_val, d_in_val + (uint64_t)w.in.nfields * scap,
                    reinterpret_cast<bmx_jrows_res*>(ctx->join.stage_res));
}

// second half of a host-mode answer: the record, then the rows it says were written, column by column from the staging (stride scap) to the caller's columns
// (stride w.cap), `at` rows in. with_inner = false leaves the inner cells to the caller (the sharded forms' phase 3).
int jrows_collect(bmx_ctx* ctx, const JRowsWant& w, uint64_t scap, uint64_t at, bool with_inner, bmx_jrows_res* res) {
  HIPCHK(hipMemcpyAsync(res, ctx->join.stage_res, sizeof(bmx_jrows_res), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t m = res->n_out, cap = w.cap;
  if (!m) return BMX_OK;
  if (m > scap || at + m > cap) return fail(ctx, BMX_ERR_INTERNAL, "bmx_where_join_rows: more rows than room");
  const unsigned long long* st = ctx->rows.stage;
  if (int rc = rows_copy_cols(ctx, w.o, st, scap, m, cap, at, w.out_ids, w.out_val, w.out_ts)) return rc;
  // the inner block: its id column always, its cells with_inner
  if (int rc = rows_copy_cols(ctx, with_inner ? w.in : RowsWant{0, nullptr, 0}, st + (1 + (uint64_t)rows_cols(w.o)) * scap, scap, m, cap, at, w.out_in_ids, w.out_in_val, w.out_in_ts)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return BMX_OK;
}

// a host-mode answer of one context behind a map that is complete
int jrows_deliver(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, const JRowsWant& w, const JoinArgs& J, uint64_t start_pos) {
  if (int rc = jrows_mask(ctx, base_field, W, w, J, start_pos)) return rc;
  const uint64_t scap = std::min<uint64_t>(w.cap, ctx->rows.masked.n);
  if (int rc = jrows_emit_staged(ctx, base_field, w, J, scap)) return rc;
  bmx_jrows_res r;
  if (int rc = jrows_collect(ctx, w, scap, 0, true, &r)) return rc;
  *w.res = r;
  return BMX_OK;
}

// Phases 2 and 3 of both sharded forms: the `m` pairs (host memory) to every shard from the cursor's on, every mask pass enqueued, then the rows shard after
// shard as bmx_comm_where_rows delivers them; then the inner cells of the delivered rows from the shards that own the inner nodes. map_size, n_inner and
// n_keyed of *tot are the cursor's shard's (every shard was given the same list).
int comm_jrows_map(bmx_comm* c, uint32_t base_field, const WhereProg& W, const JRowsWant& w, const int64_t* keys, const uint64_t* ids, uint64_t m,
                   uint32_t start_shard, uint64_t start_pos, bmx_jrows_res* tot) {
  std::vector<JoinArgs> J(c->N);
  *tot = bmx_jrows_res{};
  bool cut = false;
  uint64_t delivered = 0;
  const int rc = comm_two_phase(c,
    [&](uint32_t g, bmx_ctx* x) {
      if (int erc = enter(x)) return erc;
      if (g < start_shard) return where_stamp_only(x, base_field, &x->rows.masked);
      if (int src = join_scratch(x, m, &J[g])) return src;
      if (int src = jrows_insert_staged(x, J[g], keys, ids, m)) return src;
      return jrows_mask(x, base_field, W, w, J[g], g == start_shard ? start_pos : 0);
    },
    [&](uint32_t g, bmx_ctx* x) {
      tot->layout += x->rows.masked.layout;
      if (g < start_shard) return (int)BMX_OK;
      int crc = enter(x);
      const uint64_t room = w.cap - delivered, scap = std::min<uint64_t>(room, x->rows.masked.n);
      if (!crc) crc = jrows_emit_staged(x, base_field, w, J[g], scap);
      bmx_jrows_res r;
      if (!crc) crc = jrows_collect(x, w, scap, delivered, false, &r);
      if (crc) return crc;
      if (g == start_shard) { tot->map_size = r.map_size; tot->n_inner = r.n_inner; tot->n_keyed = r.n_keyed; }
      tot->n_match += r.n_match; tot->n_joined += r.n_joined; delivered += r.n_out;
      page_note(cut, *tot, g, r.next_pos, r.n_match > r.n_out);
      return (int)BMX_OK;
    });
  if (rc) return rc;
  tot->n_out = delivered; tot->flags = 0;
  // phase 3: one point-read request per inner field for the rows that have an inner node
  if (!delivered || !w.in.nfields) return BMX_OK;
  const bool with_ts = (w.flags & BMX_ROWS_TS) != 0u;
  std::vector<uint64_t> row, want;
  for (uint64_t r = 0; r < delivered; r++) if (w.out_in_ids[r] != BMX_JROWS_NO_NODE) { row.push_back(r); want.push_back(w.out_in_ids[r]); }
  std::vector<uint32_t> fh(want.size());
  std::vector<int64_t> gt(want.size()), gv(want.size());
  std::vector<uint8_t> found(want.size());
  for (uint32_t g = 0; g < w.in.nfields; g++) {
    int64_t* val = w.out_in_val + (uint64_t)g * w.cap;
    int64_t* ts = with_ts ? w.out_in_ts + (uint64_t)g * w.cap : nullptr;
    for (uint64_t r = 0; r < delivered; r++) { val[r] = BMX_VAL_DELETED; if (ts) ts[r] = BMX_ROWS_NO_CLOCK; }
    if (want.empty()) continue;
    std::fill(fh.begin(), fh.end(), w.in.fields[g]);
    if (int grc = bmx_comm_get_rows(c, want.size(), want.data(), fh.data(), gt.data(), gv.data(), found.data())) return grc;
    for (size_t k = 0; k < want.size(); k++) if (found[k]) { val[row[k]] = gv[k]; if (ts) ts[row[k]] = gt[k]; }
  }
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_where_join_rows(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t nfields,
                        const uint32_t* fields, uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits, uint32_t key_field,
                        uint32_t n_in_fields, const uint32_t* in_fields, uint64_t map_cap, uint32_t flags, uint64_t start_pos, uint64_t cap, uint64_t* out_ids,
                        int64_t* out_val, int64_t* out_ts, uint64_t* out_in_ids, int64_t* out_in_val, int64_t* out_in_ts, bmx_jrows_res* res, int mem) {
  static const char FN[] = "bmx_where_join_rows";
  WhereProg W, WI;
  const JRowsWant w = jrows_want(link_field, nfields, fields, n_in_fields, in_fields, flags, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val, out_in_ts, res);
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "outer program: ", bad));
  if (const char* bad = where_prepare(in_base_field, in_nclauses, in_clause_len, in_lits, &WI)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "inner program: ", bad));
  if (const char* bad = jrows_bad_args(w, map_cap, JOIN_BAD_MAP_CAP)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", bad));
  if (key_field == BMX_AGG_NO_FIELD) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", "no key field"));
  if (int erc = where_enter(ctx, mem)) return erc;
  JoinArgs J;
  if (int rc = join_scratch(ctx, map_cap, &J)) return rc;
  if (int rc = jrows_build(ctx, J, in_base_field, WI, key_field)) return rc;
  if (mem == BMX_MEM_HOST) return jrows_deliver(ctx, base_field, W, w, J, start_pos);
  if (int rc = jrows_mask(ctx, base_field, W, w, J, start_pos)) return rc;
  return jrows_emit(ctx, base_field, w, J, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val, out_in_ts, res);
}

int bmx_where_map_rows(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t nfields,
                       const uint32_t* fields, const int64_t* keys, const uint64_t* node_ids, uint64_t npairs, uint32_t n_in_fields, const uint32_t* in_fields,
                       uint32_t flags, uint64_t start_pos, uint64_t cap, uint64_t* out_ids, int64_t* out_val, int64_t* out_ts, uint64_t* out_in_ids,
                       int64_t* out_in_val, int64_t* out_in_ts, bmx_jrows_res* res, int mem) {
  static const char FN[] = "bmx_where_map_rows";
  WhereProg W;
  const JRowsWant w = jrows_want(link_field, nfields, fields, n_in_fields, in_fields, flags, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val, out_in_ts, res);
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "outer program: ", bad));
  if (const char* bad = jrows_bad_args(w, npairs, JOIN_BAD_NPAIRS)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", bad));
  if (!keys) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", "null keys"));
  if (!node_ids) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", "null node_ids"));
  if (int erc = where_enter(ctx, mem)) return erc;
  JoinArgs J;
  if (int rc = join_scratch(ctx, npairs, &J)) return rc;
  if (mem == BMX_MEM_HOST) {
    if (int rc = jrows_insert_staged(ctx, J, keys, node_ids, npairs)) return rc;
    return jrows_deliver(ctx, base_field, W, w, J, start_pos);
  }
  if (int rc = jrows_insert_list(ctx, J, keys, node_ids, npairs)) return rc;
  if (int rc = jrows_mask(ctx, base_field, W, w, J, start_pos)) return rc;
  return jrows_emit(ctx, base_field, w, J, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val, out_in_ts, res);
}

int bmx_comm_where_join_rows(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field,
                             uint32_t nfields, const uint32_t* fields, uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len,
                             const bmx_lit* in_lits, uint32_t key_field, uint32_t n_in_fields, const uint32_t* in_fields, uint64_t map_cap, uint32_t flags,
                             uint32_t start_shard, uint64_t start_pos, uint64_t cap, uint64_t* out_ids, int64_t* out_val, int64_t* out_ts, uint64_t* out_in_ids,
                             int64_t* out_in_val, int64_t* out_in_ts, bmx_jrows_res* res) {
  static const char FN[] = "bmx_comm_where_join_rows";
  WhereProg W, WI;
  const JRowsWant w = jrows_want(link_field, nfields, fields, n_in_fields, in_fields, flags, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val, out_in_ts, res);
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, join_text(FN, "outer program: ", bad));
  if (const char* bad = where_prepare(in_base_field, in_nclauses, in_clause_len, in_lits, &WI)) return fail(c, BMX_ERR_INVALID, join_text(FN, "inner program: ", bad));
  if (const char* bad = jrows_bad_args(w, map_cap, JOIN_BAD_MAP_CAP)) return fail(c, BMX_ERR_INVALID, join_text(FN, "", bad));
  if (key_field == BMX_AGG_NO_FIELD) return fail(c, BMX_ERR_INVALID, join_text(FN, "", "no key field"));
  if (int rc = where_comm_guard(c, FN, start_shard)) return rc;
  DevGuard guard;
  // phase 1: every shard's own map, exported; the union on the host. The outer index is brought up to date as well: an overflow still reports its size and stamp.
  std::vector<std::pair<int64_t, int64_t>> all;     // (key, jrows_word(id)): the signed order of the words is the unsigned order of the ids
  std::vector<long long> pk, pv;
  uint64_t n_inner = 0, n_keyed = 0, lower = 0, layout = 0, last_n = 0;
  bool overflow = false;
  int rc = comm_two_phase(c,
    [&](uint32_t, bmx_ctx* x) {
      if (int erc = enter(x)) return erc;
      Index* ix;
      if (int frc = fresh_index(x, base_field, &ix)) return frc;
      x->rows.masked.layout = ix->layout; x->rows.masked.n = ix->n;
      JoinArgs J;
      if (int src = join_scratch(x, map_cap, &J)) return src;
      if (int src = jrows_build(x, J, in_base_field, WI, key_field)) return src;
      bmx_ctx* ctx = x;
      hipLaunchKernelGGL(k_join_export, dim3(semi_finish_grid(J.slots)), dim3(JOIN_THREADS), 0, ctx->stream, J, ctx->join.stage_keys, ctx->join.stage_vals);
      LAUNCHCHK("k_join_export");
      return jrows_finish(ctx, J, reinterpret_cast<bmx_jrows_res*>(ctx->join.stage_res), 0u);
    },
    [&](uint32_t, bmx_ctx* ctx) {
      if (int erc = enter(ctx)) return erc;
      layout += ctx->rows.masked.layout; last_n = ctx->rows.masked.n;
      bmx_jrows_res r;
      HIPCHK(hipMemcpyAsync(&r, ctx->join.stage_res, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      n_inner += r.n_inner; n_keyed += r.n_keyed;
      if (r.flags & BMX_JOIN_MAP_OVERFLOW) { overflow = true; lower = std::max<uint64_t>(lower, r.map_size); return (int)BMX_OK; }
      if (r.map_size > map_cap) return fail(ctx, BMX_ERR_INTERNAL, "bmx_comm_where_join_rows: more keys than map_cap without the overflow flag");
      pk.resize(r.map_size); pv.resize(r.map_size);
      if (r.map_size) {
        HIPCHK(hipMemcpy(pk.data(), ctx->join.stage_keys, r.map_size * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pv.data(), ctx->join.stage_vals, r.map_size * 8, hipMemcpyDeviceToHost));
      }
      for (size_t i = 0; i < pk.size(); i++) all.emplace_back((int64_t)pk[i], (int64_t)pv[i]);
      return (int)BMX_OK;
    });
  if (rc) return rc;
  std::sort(all.begin(), all.end());                 // equal keys: the smallest word first
  std::vector<int64_t> uk; std::vector<uint64_t> ui;
  for (const auto& p : all) if (uk.empty() || uk.back() != p.first) { uk.push_back(p.first); ui.push_back(jrows_id((long long)p.second)); }
  if (overflow || uk.size() > map_cap) {
    bmx_jrows_res o{};
    o.next_pos = last_n; o.layout = layout; o.next_shard = c->N - 1;
    o.map_size = std::max<uint64_t>(lower, uk.size()); o.n_inner = n_inner; o.n_keyed = n_keyed; o.flags = BMX_JOIN_MAP_OVERFLOW;
    *res = o;
    return BMX_OK;
  }
  const uint64_t map_size = uk.size();
  if (uk.empty()) { uk.push_back(INT64_MIN); ui.push_back(BMX_JROWS_NO_NODE); }   // (an empty map: one pair that is skipped)
  bmx_jrows_res tot;
  if ((rc = comm_jrows_map(c, base_field, W, w, uk.data(), ui.data(), uk.size(), start_shard, start_pos, &tot))) return rc;
  tot.map_size = map_size; tot.n_inner = n_inner; tot.n_keyed = n_keyed;
  *res = tot;
  return BMX_OK;
}

int bmx_comm_where_map_rows(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field,
                            uint32_t nfields, const uint32_t* fields, const int64_t* keys, const uint64_t* node_ids, uint64_t npairs, uint32_t n_in_fields,
                            const uint32_t* in_fields, uint32_t flags, uint32_t start_shard, uint64_t start_pos, uint64_t cap, uint64_t* out_ids, int64_t* out_val,
                            int64_t* out_ts, uint64_t* out_in_ids, int64_t* out_in_val, int64_t* out_in_ts, bmx_jrows_res* res) {
  static const char FN[] = "bmx_comm_where_map_rows";
  WhereProg W;
  const JRowsWant w = jrows_want(link_field, nfields, fields, n_in_fields, in_fields, flags, cap, out_ids, out_val, out_ts, out_in_ids, out_in_val, out_in_ts, res);
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, join_text(FN, "outer program: ", bad));
  if (const char* bad = jrows_bad_args(w, npairs, JOIN_BAD_NPAIRS)) return fail(c, BMX_ERR_INVALID, join_text(FN, "", bad));
  if (!keys) return fail(c, BMX_ERR_INVALID, join_text(FN, "", "null keys"));
  if (!node_ids) return fail(c, BMX_ERR_INVALID, join_text(FN, "", "null node_ids"));
  if (int rc = where_comm_guard(c, FN, start_shard)) return rc;
  DevGuard guard;
  bmx_jrows_res tot;
  if (int rc = comm_jrows_map(c, base_field, W, w, keys, node_ids, npairs, start_shard, start_pos, &tot)) return rc;
  *res = tot;
  return BMX_OK;
}

}  // extern "C"
