// bmx_group_top.inc — the first N nodes per group (bmx_group_top.h): bmx_where_group_top and its sharded form. Passes 1 and 2 are bmx_first.inc's (first_passes:
// the table, the words per position, the first node's id), the grouped-answer steps bmx_group.inc's (grouped_collect, comm_grouped), the rounds and the finish
// gtop_kernels.h. The context keeps what the form adds to GroupScratch and FirstScratch (GtopScratch): per slot the previous winner, the round's extreme and
// the rank counter, which every query's last kernel leaves at rest again (clean), `per` winner pairs per slot (grown on demand, no rest state), the rounds'
// counters and the staging of a host-mode answer. Included by bmx.hip (one translation unit), behind bmx_first.inc.
namespace {

struct GtopWant { uint32_t group_field, order_field, per, nfields; const uint32_t* fields; uint32_t flags; uint64_t cap; };
inline uint32_t gtop_cols(const GtopWant& w) { return w.nfields * ((w.flags & BMX_ROWS_TS) ? 2u : 1u); }     // columns of 8-byte cells beside the rows

const char* gtop_bad_args(const GtopWant& w, const bmx_gtop_grp* out, const bmx_gtop_row* out_rows, const int64_t* out_val, const int64_t* out_ts, const bmx_gtop_res* res) {
  if (!res) return "bmx_where_group_top: null result record";
  if (w.cap == 0 || w.cap > BMX_GTOP_MAX_CAP) return "bmx_where_group_top: cap outside 1..BMX_GTOP_MAX_CAP";
  if (w.per == 0 || w.per > BMX_GTOP_MAX_PER) return "bmx_where_group_top: per outside 1..BMX_GTOP_MAX_PER";
  if (w.cap * w.per > BMX_GTOP_MAX_ROWS) return "bmx_where_group_top: cap * per above BMX_GTOP_MAX_ROWS";
  if (!out) return "bmx_where_group_top: null output";
  if (!out_rows) return "bmx_where_group_top: null out_rows";
  if (w.nfields > BMX_ROWS_MAX_FIELDS) return "bmx_where_group_top: more than BMX_ROWS_MAX_FIELDS fields";
  if (w.nfields && !w.fields) return "bmx_where_group_top: null fields";
  if (w.nfields && !out_val) return "bmx_where_group_top: null out_val";
  if (w.nfields && (w.flags & BMX_ROWS_TS) && !out_ts) return "bmx_where_group_top: null out_ts";
  if (w.flags & ~(BMX_ROWS_TS | BMX_GTOP_DESC)) return "bmx_where_group_top: unknown flag bits in flags";
  if (w.group_field == BMX_AGG_NO_FIELD) return "bmx_where_group_top: no group field";
  if (w.order_field == BMX_AGG_NO_FIELD) return "bmx_where_group_top: no order field";
  return nullptr;
}

// the form's own scratch for a table of `slots` slots and `per` winners per slot (group_scratch and first_scratch have sized and cleaned theirs)
int gtop_scratch(bmx_ctx* ctx, uint64_t slots, uint32_t per) {
  GtopScratch& s = ctx->gtop;
  if (slots > s.slots) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.slots = 0;
    if (int rc = dev_alloc_all(ctx, {{s.pv, slots * sizeof(long long)}, {s.pid, slots * sizeof(unsigned long long)}, {s.ext, slots * sizeof(long long)},
                                     {s.rank, slots * sizeof(uint32_t)}, {s.state, sizeof(GtopState)}})) return rc;
    s.slots = slots; s.clean = false;
  }
  if (slots * per > s.win_rows) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.win_rows = 0;
    if (int rc = dev_alloc_all(ctx, {{s.win, slots * per * sizeof(bmx_gtop_row)}})) return rc;
    s.win_rows = slots * per;
  }
  if (!s.clean) {
    GtopArgs G{};
    G.pv = s.pv; G.pid = s.pid; G.ext = s.ext; G.rank = s.rank; G.T = s.state;
    hipLaunchKernelGGL(k_gtop_clear, dim3(group_finish_grid(s.slots)), dim3(256), 0, ctx->stream, G, s.slots);
    LAUNCHCHK("k_gtop_clear");
    s.clean = true;
  }
  return BMX_OK;
}

// room for the staged groups, their rows, `words` 8-byte words of staged columns and the result record
int gtop_stage(bmx_ctx* ctx, uint64_t cap, uint64_t rows, uint64_t words) {
  GtopScratch& s = ctx->gtop;
  words = std::max<uint64_t>(words, 1);
  if (cap > s.stage_cap || rows > s.stage_rows_cap || words > s.stage_words) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    cap = std::max(cap, s.stage_cap); rows = std::max(rows, s.stage_rows_cap); words = std::max(words, s.stage_words);
    s.stage_cap = 0; s.stage_rows_cap = 0; s.stage_words = 0;
    if (int rc = dev_alloc_all(ctx, {{s.stage, cap * sizeof(bmx_gtop_grp)}, {s.stage_rows, rows * sizeof(bmx_gtop_row)}, {s.stage_cols, words * 8},
                                     {s.stage_res, sizeof(bmx_gtop_res)}})) return rc;
    s.stage_cap = cap; s.stage_rows_cap = rows; s.stage_words = words;
  }
  return BMX_OK;
}

// Enqueue one query over a prepared program; the groups, the rows, the columns (stride w.cap * w.per) and the result record go to d_out / d_rows / d_val /
// d_ts / d_res (device memory), or, with d_out == nullptr, to the context's staging (gtop_collect fetches them). Every round is enqueued blind: nothing
// returns to the host between the kernels. The arguments have been checked and the context entered.
int gtop_enqueue(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, const GtopWant& w, bmx_gtop_grp* d_out, bmx_gtop_row* d_rows, int64_t* d_val, int64_t* d_ts,
                 bmx_gtop_res* d_res) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  GtopScratch& s = ctx->gtop;
  const uint64_t rows = w.cap * w.per;
  if (!d_out) {
    if (int rc = gtop_stage(ctx, w.cap, rows, rows * gtop_cols(w))) return rc;
    d_out = s.stage; d_rows = s.stage_rows; d_res = s.stage_res;
    d_val = reinterpret_cast<int64_t*>(s.stage_cols); d_ts = d_val + (uint64_t)w.nfields * rows;
  }
  if (int rc = gtop_scratch(ctx, group_slots(w.cap), w.per)) return rc;
  FirstArgs F;
  if (int rc = first_passes(ctx, ix, base_field, W, w.group_field, w.order_field, (w.flags & BMX_GTOP_DESC) != 0, w.cap, F)) return rc;
  const GroupArgs& A = F.G;
  GtopArgs G{};
  G.pv = s.pv; G.pid = s.pid; G.ext = s.ext; G.rank = s.rank; G.win = s.win; G.T = s.state; G.per = w.per;
  GtopOut O{};
  O.slots = ctx->slots; O.nslots = ctx->nslots;
  O.out = d_out; O.out_rows = d_rows; O.out_val = d_val; O.out_ts = d_ts; O.res = d_res;
  O.nfields = w.nfields; O.with_ts = (w.flags & BMX_ROWS_TS) ? 1u : 0u;
  for (uint32_t f = 0; f < w.nfields; f++) O.field[f] = w.fields[f];
  s.clean = false;
  const uint32_t rgrid = sweep_grid(ctx, ix->n, 8ull * FIRST_THREADS), sgrid = group_finish_grid(A.slots);
  for (uint32_t round = 0; round < w.per; round++) {
    if (round) {
      by_width(ix->fits32, [&](auto t) {
        using T = decltype(t);
        const T* col = sizeof(T) == 4 ? reinterpret_cast<const T*>(ix->v32) : reinterpret_cast<const T*>(ix->v64);
        hipLaunchKernelGGL((k_gtop_value<T>), dim3(rgrid), dim3(FIRST_THREADS), 0, ctx->stream, col, ix->ids, ix->n, F, G, round);
        hipLaunchKernelGGL((k_gtop_id<T>), dim3(rgrid), dim3(FIRST_THREADS), 0, ctx->stream, col, ix->ids, ix->n, F, G, round);
      });
      LAUNCHCHK("k_gtop_value / k_gtop_id");
    }
    hipLaunchKernelGGL(k_gtop_advance, dim3(sgrid), dim3(256), 0, ctx->stream, F, G, round);
    LAUNCHCHK("k_gtop_advance");
  }
  hipLaunchKernelGGL(k_gtop_finish, dim3(sgrid), dim3(256), 0, ctx->stream, F, G, O, A.m_src != AGG_SRC_PROBE ? 1u : 0u);
  LAUNCHCHK("k_gtop_finish");
  ctx->group.clean = true; ctx->first.clean = true; s.clean = true;
  return BMX_OK;
}

inline bool gtop_key_less(const bmx_gtop_grp& a, const bmx_gtop_grp& b) { return a.key < b.key; }

// Second half of a staged answer: the result record, the groups sorted by key, their rows (blocks of w.per, moved with the groups) and their gtop_cols(w)
// columns, packed with stride grps.size() * w.per into `cols`. Nothing of the caller's is written.
int gtop_collect(bmx_ctx* ctx, const GtopWant& w, std::vector<bmx_gtop_grp>& grps, std::vector<bmx_gtop_row>& rows, std::vector<int64_t>& cols, bmx_gtop_res* res) {
  const GtopScratch& s = ctx->gtop;
  std::vector<uint32_t> perm;
  if (int rc = grouped_collect(ctx, s.stage, s.stage_res, BMX_GTOP_OVERFLOW, w.cap, gtop_key_less, "bmx_where_group_top", grps, res, &perm)) return rc;
  const uint64_t per = w.per, m = grps.size() * per, nc = gtop_cols(w), stride = w.cap * per;
  rows.assign(m, bmx_gtop_row{});
  cols.assign(m * nc, 0);
  if (!m) return BMX_OK;
  std::vector<bmx_gtop_row> raw_rows(m);
  std::vector<int64_t> raw(m * nc);
  HIPCHK(hipMemcpyAsync(raw_rows.data(), s.stage_rows, m * sizeof(bmx_gtop_row), hipMemcpyDeviceToHost, ctx->stream));
  for (uint64_t c = 0; c < nc; c++)
    HIPCHK(hipMemcpyAsync(raw.data() + c * m, reinterpret_cast<const int64_t*>(s.stage_cols) + c * stride, m * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (uint64_t g = 0; g < grps.size(); g++) {
    std::memcpy(rows.data() + g * per, raw_rows.data() + perm[g] * per, per * sizeof(bmx_gtop_row));
    for (uint64_t c = 0; c < nc; c++) std::memcpy(cols.data() + c * m + g * per, raw.data() + c * m + perm[g] * per, per * 8);
  }
  return BMX_OK;
}

// does row a come before row b under the order (both have a node)?
inline bool gtop_before(const bmx_gtop_row& a, const bmx_gtop_row& b, bool desc) {
  if (a.val != b.val) return desc ? a.val > b.val : a.val < b.val;
  return a.id < b.id;
}

// the sharded merge: one row and where its cells are; one group and where its rows are (a block of `per` in the merge's pool)
struct GtopSrc { bmx_gtop_row r; uint32_t shard; uint64_t at; };
struct GtopKey { bmx_gtop_grp g; uint64_t block; };
struct GtopTot { uint64_t n_groups; uint32_t flags, reserved; uint64_t total, absent, n_ordered; };   // what comm_grouped folds (bmx_gtop_res without per / n_rows)

}  // namespace

extern "C" {

int bmx_where_group_top(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t group_field,
                        uint32_t order_field, uint32_t per, uint32_t nfields, const uint32_t* fields, uint32_t flags, uint64_t cap, bmx_gtop_grp* out,
                        bmx_gtop_row* out_rows, int64_t* out_val, int64_t* out_ts, bmx_gtop_res* res, int mem) {
  WhereProg W;
  const GtopWant w{group_field, order_field, per, nfields, fields, flags, cap};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = gtop_bad_args(w, out, out_rows, out_val, out_ts, res)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (mem == BMX_MEM_DEVICE) return gtop_enqueue(ctx, base_field, W, w, out, out_rows, out_val, out_ts, res);
  if (int rc = gtop_enqueue(ctx, base_field, W, w, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
  std::vector<bmx_gtop_grp> grps;
  std::vector<bmx_gtop_row> rows;
  std::vector<int64_t> cols;
  bmx_gtop_res r;
  if (int rc = gtop_collect(ctx, w, grps, rows, cols, &r)) return rc;
  const uint64_t m = rows.size(), stride = cap * per;
  if (m) {
    std::memcpy(out, grps.data(), grps.size() * sizeof(bmx_gtop_grp));
    std::memcpy(out_rows, rows.data(), m * sizeof(bmx_gtop_row));
    for (uint32_t f = 0; f < nfields; f++) {
      std::memcpy(out_val + (uint64_t)f * stride, cols.data() + (uint64_t)f * m, m * 8);
      if (flags & BMX_ROWS_TS) std::memcpy(out_ts + (uint64_t)f * stride, cols.data() + ((uint64_t)nfields + f) * m, m * 8);
    }
  }
  *res = r;
  return BMX_OK;
}

int bmx_comm_where_group_top(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t group_field,
                             uint32_t order_field, uint32_t per, uint32_t nfields, const uint32_t* fields, uint32_t flags, uint64_t cap, bmx_gtop_grp* out,
                             bmx_gtop_row* out_rows, int64_t* out_val, int64_t* out_ts, bmx_gtop_res* res) {
  WhereProg W;
  const GtopWant w{group_field, order_field, per, nfields, fields, flags, cap};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = gtop_bad_args(w, out, out_rows, out_val, out_ts, res)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  const bool desc = (flags & BMX_GTOP_DESC) != 0;
  const uint32_t nc = gtop_cols(w);
  std::vector<std::vector<int64_t>> cols;          // per shard, in shard order: its packed columns
  std::vector<uint64_t> strides;                   // ... and their stride (the shard's groups * per)
  std::vector<GtopSrc> pool;                       // blocks of `per` rows: a shard's group's, or a merged key's
  std::vector<bmx_gtop_grp> grps;
  std::vector<bmx_gtop_row> rows;
  std::vector<GtopKey> merged(cap);
  GtopTot tot;
  if (int rc = comm_grouped(c, cap, BMX_GTOP_OVERFLOW, [](const GtopKey& a, const GtopKey& b) { return a.g.key < b.g.key; }, merged.data(), &tot,
        [&](bmx_ctx* x) { return gtop_enqueue(x, base_field, W, w, nullptr, nullptr, nullptr, nullptr, nullptr); },
        [&](bmx_ctx* x, std::vector<GtopKey>& part, GtopTot* t) {
          cols.emplace_back();
          bmx_gtop_res r;
          const int crc = gtop_collect(x, w, grps, rows, cols.back(), &r);
          strides.push_back(crc ? 0 : rows.size());
          part.clear();
          if (crc) return crc;
          *t = GtopTot{r.n_groups, r.flags, 0u, r.total, r.absent, r.n_ordered};
          const uint32_t shard = (uint32_t)cols.size() - 1u;
          for (uint64_t g = 0; g < grps.size(); g++) {
            part.push_back(GtopKey{grps[g], pool.size()});
            for (uint64_t j = 0; j < per; j++) pool.push_back(GtopSrc{rows[g * per + j], shard, g * per + j});
          }
          return (int)BMX_OK;
        },
        [](uint32_t, GtopTot& t, const GtopTot& r) { t.total += r.total; t.absent += r.absent; t.n_ordered += r.n_ordered; },
        [&](GtopKey& m, const GtopKey& p) {            // counts add; the first `per` of both blocks under the order, each row with its shard's cells
          const uint64_t a0 = m.block, b0 = p.block, at = pool.size();
          uint64_t i = 0, j = 0;
          for (uint64_t k = 0; k < per; k++) {
            const bool ha = i < m.g.n_rows, hb = j < p.g.n_rows;
            if (!ha && !hb) { pool.push_back(GtopSrc{bmx_gtop_row{BMX_GTOP_NO_NODE, BMX_VAL_DELETED}, 0u, 0ull}); continue; }
            const bool take_b = hb && (!ha || gtop_before(pool[b0 + j].r, pool[a0 + i].r, desc));
            const GtopSrc src = take_b ? pool[b0 + j++] : pool[a0 + i++];
            pool.push_back(src);
          }
          m.g.n_match += p.g.n_match; m.g.n += p.g.n;
          m.g.n_rows = std::min<uint64_t>(per, m.g.n);
          m.block = at;
        })) return rc;
  bmx_gtop_res o{};
  o.n_groups = tot.n_groups; o.flags = tot.flags; o.per = per; o.total = tot.total; o.absent = tot.absent; o.n_ordered = tot.n_ordered;
  if (!(tot.flags & BMX_GTOP_OVERFLOW)) {
    const uint64_t stride = cap * per;
    for (uint64_t g = 0; g < tot.n_groups; g++) {
      const GtopKey& m = merged[g];
      out[g] = m.g;
      o.n_rows += m.g.n_rows;
      for (uint64_t j = 0; j < per; j++) {
        const GtopSrc& src = pool[m.block + j];
        out_rows[g * per + j] = src.r;
        const bool node = src.r.id != BMX_GTOP_NO_NODE;
        for (uint32_t k = 0; k < nc; k++) {
          int64_t* dst = k < nfields ? out_val + (uint64_t)k * stride : out_ts + (uint64_t)(k - nfields) * stride;
          dst[g * per + j] = node ? cols[src.shard][(uint64_t)k * strides[src.shard] + src.at] : (k < nfields ? BMX_VAL_DELETED : BMX_ROWS_NO_CLOCK);
        }
      }
    }
  }
  *res = o;
  return BMX_OK;
}

}  // extern "C"
