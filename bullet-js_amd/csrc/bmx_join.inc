// bmx_join.inc — lookup joins (bmx_join.h): bmx_where_join_group, bmx_where_map_group and their sharded forms. The programs are bmx_where.inc's (where_prepare),
// and so are the width dispatch of the sweeps and the entry guards (where_sweep, where_enter, where_comm_guard), the kernels join_kernels.h. The context keeps
// the map's scratch (JoinScratch): the table of pairs and its state record, which every query's last kernel leaves empty again (clean), and the staging of the
// host-mode and sharded forms. The records are aggregated in bmx_where_group's table (ctx->group, through group_scratch and its clean protocol), and a
// host-mode answer's records come down through its staging, collected, merged and combined over the shards by bmx_group.inc's grouped_collect, merge_sorted
// and comm_grouped. Included by bmx.hip (one translation unit), behind everything that was here before it.
namespace {

struct JoinWant { uint32_t link_field, measure_field; bmx_group_rec* out; uint64_t cap; bmx_join_res* res; };

const char* join_bad_args(const JoinWant& w, uint64_t map_cap, const char* map_cap_text) {
  if (!w.res) return "null result record";
  if (w.cap == 0 || w.cap > BMX_GROUP_MAX_CAP) return "cap outside 1..BMX_GROUP_MAX_CAP";
  if (!w.out) return "null output";
  if (map_cap == 0 || map_cap > BMX_JOIN_MAX_MAP) return map_cap_text;
  if (w.link_field == BMX_AGG_NO_FIELD) return "no link field";
  return nullptr;
}
const char* const JOIN_BAD_MAP_CAP = "map_cap outside 1..BMX_JOIN_MAX_MAP";
const char* const JOIN_BAD_NPAIRS = "npairs outside 1..BMX_JOIN_MAX_MAP";

static_assert(JOIN_THREADS == SEMI_THREADS, "the grids of the list, export, finish and clear kernels are bmx_semi.inc's (semi_grid, semi_finish_grid), and so is semi_slots");

// the scratch for a map of up to `cap` keys: grows to the largest cap asked so far, all or nothing. -> this query's arguments: the head of the table
int join_scratch(bmx_ctx* ctx, uint64_t cap, JoinArgs* J) {
  JoinScratch& s = ctx->join;
  if (cap > s.cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.cap = 0; s.slots = 0;
    const uint64_t slots = semi_slots(cap);
    if (int rc = dev_alloc_all(ctx, {{s.map, slots * sizeof(JoinPair)}, {s.state, sizeof(JoinState)}, {s.stage_keys, cap * sizeof(long long)},
                                     {s.stage_vals, cap * sizeof(long long)}, {s.stage_res, sizeof(bmx_join_res)}})) return rc;
    s.cap = cap; s.slots = slots; s.clean = false;
  }
  if (!s.clean) {     // a new table, or a query that did not get as far as its last kernel
    hipLaunchKernelGGL(k_join_clear, dim3(semi_finish_grid(s.slots)), dim3(JOIN_THREADS), 0, ctx->stream, s.map, s.slots, s.state);
    LAUNCHCHK("k_join_clear");
  }
  J->map = s.map; J->S = s.state; J->slots = semi_slots(cap); J->cap = cap;
  s.clean = false;
  return BMX_OK;
}

// the group table for `cap` records, empty, and this query's arguments for it (group = the LINK field: what k_join_group_sweep probes for)
int join_group_args(bmx_ctx* ctx, uint32_t base_field, const JoinWant& w, GroupArgs* A) {
  if (int rc = group_scratch(ctx, w.cap)) return rc;
  GroupScratch& s = ctx->group;
  *A = GroupArgs{};
  A->keys = s.keys; A->acc = s.acc; A->S = s.state;
  A->slots = group_slots(w.cap); A->cap = w.cap;
  A->measure = w.measure_field; A->group = w.link_field;
  A->m_src = where_agg_source(w.measure_field, base_field); A->g_src = where_agg_source(w.link_field, base_field);
  s.clean = false;
  return BMX_OK;
}

// the map from the inner program: one sweep of the inner base field's index
int join_build(bmx_ctx* ctx, const JoinArgs& J, uint32_t in_base_field, const WhereProg& WI, uint32_t key_field, uint32_t attr_field) {
  Index* ix;
  if (int rc = fresh_index(ctx, in_base_field, &ix)) return rc;
  const uint32_t ksrc = where_agg_source(key_field, in_base_field);
  const uint32_t asrc = attr_field == key_field ? JOIN_SRC_KEY : where_agg_source(attr_field, in_base_field);
  where_sweep_c(ctx, ix, WI, [&](const auto& P, uint32_t blocks) {
    hipLaunchKernelGGL((k_join_build<decltype(where_value(P)), where_clocks<decltype(P)>>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, J, key_field, ksrc, attr_field, asrc);
  });
  LAUNCHCHK("k_join_build");
  return BMX_OK;
}

// the map from `n` pairs in device memory
int join_insert_list(bmx_ctx* ctx, const JoinArgs& J, const long long* d_keys, const long long* d_vals, uint64_t n) {
  hipLaunchKernelGGL(k_join_insert, dim3(semi_grid(n)), dim3(JOIN_THREADS), 0, ctx->stream, d_keys, d_vals, n, J);
  LAUNCHCHK("k_join_insert");
  return BMX_OK;
}

// The group sweep over a map that has been built, and the call's last kernel. The records and the result record go to d_out / d_res (device memory), or, with
// d_out == nullptr, to the staging (the group scratch's records, this scratch's result record). A value-ordered view of the base field's index is neither read
// nor touched (where_run).
int join_sweep(bmx_ctx* ctx, const JoinArgs& J, uint32_t base_field, const WhereProg& W, const JoinWant& w, bmx_group_rec* d_out, bmx_join_res* d_res) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  GroupArgs A;
  if (int rc = join_group_args(ctx, base_field, w, &A)) return rc;
  where_sweep_c(ctx, ix, W, [&](const auto& P, uint32_t blocks) {
    hipLaunchKernelGGL((k_join_group_sweep<decltype(where_value(P)), where_clocks<decltype(P)>>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, A, J);
  });
  LAUNCHCHK("k_join_group_sweep");
  hipLaunchKernelGGL(k_join_finish, dim3(semi_finish_grid(std::max(A.slots, J.slots))), dim3(JOIN_THREADS), 0, ctx->stream, A, J, d_out ? d_out : ctx->group.stage,
                     d_out ? d_res : ctx->join.stage_res, A.m_src != AGG_SRC_PROBE ? 1u : 0u);
  LAUNCHCHK("k_join_finish");
  ctx->group.clean = true; ctx->join.clean = true;
  return BMX_OK;
}

// second half of a staged answer (grouped_collect): ANY flag of the record says that no records were written, the map's overflow as the groups'
int join_collect(bmx_ctx* ctx, uint64_t cap, std::vector<bmx_group_rec>& recs, bmx_join_res* res) {
  return grouped_collect(ctx, ctx->group.stage, ctx->join.stage_res, ~0u, cap, group_key_less, "bmx_where_join_group", recs, res);
}

// one shard's (or the one context's) bmx_where_map_group with the pairs in HOST memory, enqueued into the staging
int join_map_staged(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, const JoinWant& w, const int64_t* keys, const int64_t* vals, uint64_t npairs) {
  JoinArgs J;
  if (int rc = join_scratch(ctx, std::max<uint64_t>(npairs, 1), &J)) return rc;
  if (npairs) {
    HIPCHK(hipMemcpyAsync(ctx->join.stage_keys, keys, npairs * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->join.stage_vals, vals, npairs * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  if (int rc = join_insert_list(ctx, J, ctx->join.stage_keys, ctx->join.stage_vals, npairs)) return rc;
  return join_sweep(ctx, J, base_field, W, w, nullptr, nullptr);
}

int join_deliver(bmx_ctx* ctx, const JoinWant& w) {
  std::vector<bmx_group_rec> recs;
  bmx_join_res r;
  if (int rc = join_collect(ctx, w.cap, recs, &r)) return rc;
  if (!recs.empty()) std::memcpy(w.out, recs.data(), recs.size() * sizeof(bmx_group_rec));
  *w.res = r;
  return BMX_OK;
}

// phase 2 of both sharded forms: the `m` pairs (host memory) to every shard, every sweep enqueued, then the answers merged shard after shard. n_inner and
// n_keyed of *tot are shard 0's (every shard was given the same list).
int comm_join_map(bmx_comm* c, uint32_t base_field, const WhereProg& W, const JoinWant& w, const int64_t* keys, const int64_t* vals, uint64_t m, bmx_join_res* tot) {
  return comm_grouped(c, w.cap, BMX_JOIN_GROUP_OVERFLOW, group_key_less, w.out, tot,
    [&](bmx_ctx* x) { return join_map_staged(x, base_field, W, w, keys, vals, m); },
    [&](bmx_ctx* x, std::vector<bmx_group_rec>& part, bmx_join_res* r) { return join_collect(x, w.cap, part, r); },
    [](uint32_t g, bmx_join_res& t, const bmx_join_res& r) {
      if (g == 0) { t = r; t.flags = 0; t.n_groups = 0; }
      else { group_fold(t.absent, r.absent); group_fold(t.unmatched, r.unmatched); group_fold(t.total, r.total); }
    });
}

std::string join_text(const char* fn, const char* which, const char* bad) { return std::string(fn) + ": " + which + bad; }

constexpr bmx_agg JOIN_AGG_EMPTY = bmx_agg{0ull, 0ull, INT64_MAX, INT64_MIN, 0ull, 0ll};

}  // namespace

extern "C" {

int bmx_where_join_group(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t measure_field,
                         uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits, uint32_t key_field, uint32_t attr_field,
                         uint64_t map_cap, bmx_group_rec* out, uint64_t cap, bmx_join_res* res, int mem) {
  static const char FN[] = "bmx_where_join_group";
  WhereProg W, WI;
  const JoinWant w{link_field, measure_field, out, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "outer program: ", bad));
  if (const char* bad = where_prepare(in_base_field, in_nclauses, in_clause_len, in_lits, &WI)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "inner program: ", bad));
  if (const char* bad = join_bad_args(w, map_cap, JOIN_BAD_MAP_CAP)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", bad));
  if (key_field == BMX_AGG_NO_FIELD) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", "no key field"));
  if (attr_field == BMX_AGG_NO_FIELD) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", "no attribute field"));
  if (int erc = where_enter(ctx, mem)) return erc;
  JoinArgs J;
  if (int rc = join_scratch(ctx, map_cap, &J)) return rc;
  if (int rc = join_build(ctx, J, in_base_field, WI, key_field, attr_field)) return rc;
  if (mem == BMX_MEM_DEVICE) return join_sweep(ctx, J, base_field, W, w, out, res);
  if (int rc = join_sweep(ctx, J, base_field, W, w, nullptr, nullptr)) return rc;
  return join_deliver(ctx, w);
}

int bmx_where_map_group(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t measure_field,
                        const int64_t* keys, const int64_t* vals, uint64_t npairs, bmx_group_rec* out, uint64_t cap, bmx_join_res* res, int mem) {
  static const char FN[] = "bmx_where_map_group";
  WhereProg W;
  const JoinWant w{link_field, measure_field, out, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "outer program: ", bad));
  if (const char* bad = join_bad_args(w, npairs, JOIN_BAD_NPAIRS)) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", bad));
  if (!keys) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", "null keys"));
  if (!vals) return fail(ctx, BMX_ERR_INVALID, join_text(FN, "", "null vals"));
  if (int erc = where_enter(ctx, mem)) return erc;
  if (mem == BMX_MEM_DEVICE) {
    JoinArgs J;
    if (int rc = join_scratch(ctx, npairs, &J)) return rc;
    if (int rc = join_insert_list(ctx, J, reinterpret_cast<const long long*>(keys), reinterpret_cast<const long long*>(vals), npairs)) return rc;
    return join_sweep(ctx, J, base_field, W, w, out, res);
  }
  if (int rc = join_map_staged(ctx, base_field, W, w, keys, vals, npairs)) return rc;
  return join_deliver(ctx, w);
}

int bmx_comm_where_join_group(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field,
                              uint32_t measure_field, uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits,
                              uint32_t key_field, uint32_t attr_field, uint64_t map_cap, bmx_group_rec* out, uint64_t cap, bmx_join_res* res) {
  static const char FN[] = "bmx_comm_where_join_group";
  WhereProg W, WI;
  const JoinWant w{link_field, measure_field, out, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, join_text(FN, "outer program: ", bad));
  if (const char* bad = where_prepare(in_base_field, in_nclauses, in_clause_len, in_lits, &WI)) return fail(c, BMX_ERR_INVALID, join_text(FN, "inner program: ", bad));
  if (const char* bad = join_bad_args(w, map_cap, JOIN_BAD_MAP_CAP)) return fail(c, BMX_ERR_INVALID, join_text(FN, "", bad));
  if (key_field == BMX_AGG_NO_FIELD) return fail(c, BMX_ERR_INVALID, join_text(FN, "", "no key field"));
  if (attr_field == BMX_AGG_NO_FIELD) return fail(c, BMX_ERR_INVALID, join_text(FN, "", "no attribute field"));
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  // phase 1: every shard's own map, exported; the union on the host
  std::vector<std::pair<int64_t, int64_t>> all;
  std::vector<long long> pk, pv;
  uint64_t n_inner = 0, n_keyed = 0, lower = 0;                       // lower: the largest lower bound of the map's size any overflowing shard reported
  bool overflow = false;
  int rc = comm_two_phase(c,
    [&](uint32_t, bmx_ctx* x) {
      if (int erc = enter(x)) return erc;
      JoinArgs J;
      if (int src = join_scratch(x, map_cap, &J)) return src;
      if (int src = join_build(x, J, in_base_field, WI, key_field, attr_field)) return src;
      bmx_ctx* ctx = x;
      hipLaunchKernelGGL(k_join_export, dim3(semi_finish_grid(J.slots)), dim3(JOIN_THREADS), 0, ctx->stream, J, ctx->join.stage_keys, ctx->join.stage_vals);
      LAUNCHCHK("k_join_export");
      GroupArgs A;                                                       // (the group state record is read and put back; no group table is swept)
      if (int src = join_group_args(ctx, base_field, w, &A)) return src;
      A.slots = 0;
      hipLaunchKernelGGL(k_join_finish, dim3(semi_finish_grid(J.slots)), dim3(JOIN_THREADS), 0, ctx->stream, A, J, ctx->group.stage, ctx->join.stage_res, 1u);
      LAUNCHCHK("k_join_finish");
      ctx->group.clean = true; ctx->join.clean = true;
      return (int)BMX_OK;
    },
    [&](uint32_t, bmx_ctx* ctx) {
      if (int erc = enter(ctx)) return erc;
      bmx_join_res r;
      HIPCHK(hipMemcpyAsync(&r, ctx->join.stage_res, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      n_inner += r.n_inner; n_keyed += r.n_keyed;
      if (r.flags & BMX_JOIN_MAP_OVERFLOW) { overflow = true; lower = std::max<uint64_t>(lower, r.map_size); return (int)BMX_OK; }
      if (r.map_size > map_cap) return fail(ctx, BMX_ERR_INTERNAL, "bmx_comm_where_join_group: more keys than map_cap without the overflow flag");
      pk.resize(r.map_size); pv.resize(r.map_size);
      if (r.map_size) {
        HIPCHK(hipMemcpy(pk.data(), ctx->join.stage_keys, r.map_size * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pv.data(), ctx->join.stage_vals, r.map_size * 8, hipMemcpyDeviceToHost));
      }
      for (size_t i = 0; i < pk.size(); i++) all.emplace_back((int64_t)pk[i], (int64_t)pv[i]);
      return (int)BMX_OK;
    });
  if (rc) return rc;
  // equal keys: the minimum of their attributes (INT64_MAX = none sorts last)
  std::sort(all.begin(), all.end());
  std::vector<int64_t> uk, uv;
  for (const auto& p : all) if (uk.empty() || uk.back() != p.first) { uk.push_back(p.first); uv.push_back(p.second); }
  if (overflow || uk.size() > map_cap) {
    bmx_join_res o{};
    o.map_size = std::max<uint64_t>(lower, uk.size()); o.n_inner = n_inner; o.n_keyed = n_keyed; o.flags = BMX_JOIN_MAP_OVERFLOW;
    o.absent = JOIN_AGG_EMPTY; o.unmatched = JOIN_AGG_EMPTY; o.total = JOIN_AGG_EMPTY;
    *res = o;
    return BMX_OK;
  }
  bmx_join_res tot;
  if (uk.empty()) { uk.push_back(INT64_MIN); uv.push_back(INT64_MAX); }   // (an empty map: one pair outside the domain, which is skipped)
  if ((rc = comm_join_map(c, base_field, W, w, uk.data(), uv.data(), uk.size(), &tot))) return rc;
  tot.map_size = all.empty() ? 0 : tot.map_size; tot.n_inner = n_inner; tot.n_keyed = n_keyed;
  *res = tot;
  return BMX_OK;
}

int bmx_comm_where_map_group(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field,
                             uint32_t measure_field, const int64_t* keys, const int64_t* vals, uint64_t npairs, bmx_group_rec* out, uint64_t cap, bmx_join_res* res) {
  static const char FN[] = "bmx_comm_where_map_group";
  WhereProg W;
  const JoinWant w{link_field, measure_field, out, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, join_text(FN, "outer program: ", bad));
  if (const char* bad = join_bad_args(w, npairs, JOIN_BAD_NPAIRS)) return fail(c, BMX_ERR_INVALID, join_text(FN, "", bad));
  if (!keys) return fail(c, BMX_ERR_INVALID, join_text(FN, "", "null keys"));
  if (!vals) return fail(c, BMX_ERR_INVALID, join_text(FN, "", "null vals"));
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  bmx_join_res tot;
  if (int rc = comm_join_map(c, base_field, W, w, keys, vals, npairs, &tot)) return rc;
  *res = tot;
  return BMX_OK;
}

}  // extern "C"
