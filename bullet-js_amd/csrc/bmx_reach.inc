// bmx_reach.inc — graph traversal (bmx_reach.h): bmx_where_reach, bmx_where_reach_from and their sharded forms. The programs are bmx_where.inc's (where_prepare),
// and so are the width dispatch of the sweeps, the answer's mask pass and the entry guards (where_sweep, where_mask_pass, where_enter, where_comm_guard); the map
// is the lookup joins' (join_scratch and its clean protocol: joins, join projections and traversals interleave on one context), the emit pass's geometry
// bmx_scan.inc's (emit_dispatch), the kernels reach_kernels.h. The context keeps the traversal's own scratch (ReachScratch): one link word and one depth byte per
// position of the largest index traversed so far, the state record, which every call's last kernel leaves zero again (clean), and the staging of the host-mode
// and sharded forms. Nothing in it survives a call. Included by bmx.hip (one translation unit), behind everything that was here before it.
namespace {

struct ReachWant {
  uint32_t link_field, key_field, flags, max_depth; uint64_t set_cap;
  uint64_t* out_ids; uint8_t* out_depth; uint64_t cap; bmx_reach_res* res;
};

const char* reach_bad_args(const ReachWant& w) {
  if (!w.res) return "null result record";
  if (w.set_cap == 0 || w.set_cap > BMX_REACH_MAX_SET) return "set_cap outside 1..BMX_REACH_MAX_SET";
  if (w.max_depth == 0 || w.max_depth > BMX_REACH_MAX_DEPTH) return "max_depth outside 1..BMX_REACH_MAX_DEPTH";
  if (w.cap && !w.out_ids) return "null out_ids";
  if (w.cap && !w.out_depth) return "null out_depth";
  if (w.flags) return "flags must be 0";
  if (w.link_field == BMX_AGG_NO_FIELD) return "no link field";
  if (w.key_field == BMX_AGG_NO_FIELD) return "no key field";
  return nullptr;
}
const char* reach_bad_list(const int64_t* values, uint64_t nvalues) {
  if (nvalues == 0 || nvalues > BMX_REACH_MAX_SET) return "nvalues outside 1..BMX_REACH_MAX_SET";
  if (!values) return "null values";
  return nullptr;
}

// one call's device state: the head of the map, the per-position arrays, the base index as the prepare sweep saw it
struct ReachRun { JoinArgs J; ReachArgs A; ReachKey K; uint64_t n = 0; bool fits32 = false; };

// The map for `set_cap` values (its staging has room for `list` values as well) and the state record, both empty.
int reach_scratch(bmx_ctx* ctx, uint64_t set_cap, uint64_t list, ReachRun* R) {
  if (int rc = join_scratch(ctx, std::max(set_cap, list), &R->J)) return rc;
  R->J.slots = semi_slots(set_cap); R->J.cap = set_cap;                  // (the head of a table that may be larger)
  ReachScratch& s = ctx->reach;
  if (!s.state) {
    if (int rc = dev_alloc_all(ctx, {{s.state, sizeof(ReachState)}, {s.stage_res, sizeof(bmx_reach_res)}})) return rc;
    s.clean = false;
  }
  if (!s.clean) HIPCHK(hipMemsetAsync(s.state, 0, sizeof(ReachState), ctx->stream));     // new, or a call that did not get as far as its last kernel
  s.clean = false;
  R->A.S = s.state;
  return BMX_OK;
}

// the seeds from the seed program: one sweep of the seed base field's index
int reach_seed(bmx_ctx* ctx, const ReachRun& R, uint32_t seed_base_field, const WhereProg& WS, uint32_t seed_field) {
  Index* ix;
  if (int rc = fresh_index(ctx, seed_base_field, &ix)) return rc;
  const uint32_t src = where_agg_source(seed_field, seed_base_field);
  where_sweep_c(ctx, ix, WS, [&](const auto& P, uint32_t blocks) {
    hipLaunchKernelGGL((k_reach_seed<decltype(where_value(P)), where_clocks<decltype(P)>>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, R.J, R.A.S, seed_field, src);
  });
  LAUNCHCHK("k_reach_seed");
  return BMX_OK;
}

// `n` values in device memory into the map at `level`
int reach_list(bmx_ctx* ctx, const ReachRun& R, const long long* d_values, uint64_t n, uint32_t level, bool count) {
  hipLaunchKernelGGL(k_reach_list, dim3(semi_grid(n)), dim3(JOIN_THREADS), 0, ctx->stream, d_values, n, R.J, R.A.S, level, count ? 1u : 0u);
  LAUNCHCHK("k_reach_list");
  return BMX_OK;
}
// ... in HOST memory, through the staging of the map's scratch (n <= the `list` the scratch was sized for)
int reach_list_staged(bmx_ctx* ctx, const ReachRun& R, const int64_t* values, uint64_t n, uint32_t level, bool count) {
  HIPCHK(hipMemcpyAsync(ctx->join.stage_keys, values, n * 8, hipMemcpyHostToDevice, ctx->stream));
  return reach_list(ctx, R, ctx->join.stage_keys, n, level, count);
}

// The prepare sweep: the per-position arrays sized for the base index and filled. A value-ordered view of the base field's index is neither read nor touched.
int reach_prepare(bmx_ctx* ctx, ReachRun* R, uint32_t base_field, const WhereProg& W, const ReachWant& w) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  ReachScratch& s = ctx->reach;
  if (ix->n > s.pos_cap || !s.link) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.pos_cap = 0;
    const uint64_t cap = (std::max<uint64_t>(ix->n, 1) + ix->n / 4 + 15) & ~15ull;
    if (int rc = dev_alloc_all(ctx, {{s.link, cap * sizeof(long long)}, {s.depth, cap}})) return rc;
    s.pos_cap = cap;
  }
  R->A.link = s.link; R->A.depth = s.depth;
  R->n = ix->n; R->fits32 = ix->fits32;
  R->K = ReachKey{ix->ids, ix->fits32 ? static_cast<const void*>(ix->v32) : static_cast<const void*>(ix->v64), ctx->slots, ctx->nslots, w.key_field,
                  where_agg_source(w.key_field, base_field)};
  const uint32_t src = where_agg_source(w.link_field, base_field);
  where_sweep_c(ctx, ix, W, [&](const auto& P, uint32_t blocks) {
    hipLaunchKernelGGL((k_reach_prepare<decltype(where_value(P)), where_clocks<decltype(P)>>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, R->A, w.link_field, src);
  });
  LAUNCHCHK("k_reach_prepare");
  return BMX_OK;
}

// round r, enqueued blind: it returns at once on the device when the level before it brought nothing new
int reach_round(bmx_ctx* ctx, const ReachRun& R, uint32_t r) {
  const uint32_t grid = sweep_grid(ctx, (R.n + 1) / 2, 4ull * REACH_THREADS * REACH_U);
  by_width(R.fits32, [&](auto t) {
    hipLaunchKernelGGL((k_reach_round<decltype(t)>), dim3(grid), dim3(REACH_THREADS), 0, ctx->stream, R.n, R.A, R.J, R.K, r);
  });
  LAUNCHCHK("k_reach_round");
  return BMX_OK;
}

// room for `n` ids and depths of a host-mode answer on its way down
int reach_stage(bmx_ctx* ctx, uint64_t n) {
  ReachScratch& s = ctx->reach;
  if (n > s.stage_cap || !s.stage_ids) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.stage_cap = 0;
    const uint64_t cap = std::max<uint64_t>(n, 1);
    if (int rc = dev_alloc_all(ctx, {{s.stage_ids, cap * sizeof(uint64_t)}, {s.stage_depth, cap}})) return rc;
    s.stage_cap = cap;
  }
  return BMX_OK;
}

// The answer behind the last round, and the call's last kernel: mask, emit, finish. d_ids / d_depth / d_res are device memory; with d_res == nullptr the answer
// goes to the staging, sized here for min(w.cap, positions) entries.
int reach_answer(bmx_ctx* ctx, const ReachRun& R, uint32_t base_field, const WhereProg& W, const ReachWant& w, uint64_t* d_ids, uint8_t* d_depth, bmx_reach_res* d_res) {
  ReachScratch& s = ctx->reach;
  uint64_t d_cap = w.cap;
  if (!d_res) {
    d_cap = std::min<uint64_t>(w.cap, R.n);                               // (no more can come)
    if (int rc = reach_stage(ctx, d_cap)) return rc;
    d_ids = s.stage_ids; d_depth = s.stage_depth; d_res = s.stage_res;
    s.staged = d_cap;
  }
  RowsScratch::Masked M;
  const PredReach Q{R.A.depth, R.J.S, R.J.cap};
  if (int rc = where_mask_pass(ctx, base_field, W, "launch k_scan_mask(reach)", &M, [&](const auto&) { return Q; })) return rc;
  const ReachEmit E{M.ids, R.A.depth, d_ids, d_depth, R.A.S, d_cap, M.n};
  emit_dispatch(M.nb, [&](auto B, uint32_t wgs) {
    hipLaunchKernelGGL((k_reach_emit<decltype(B)::value>), dim3(wgs), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.mask, ctx->scan.counts, M.nb, E);
  });
  LAUNCHCHK("k_reach_emit");
  hipLaunchKernelGGL(k_reach_finish, dim3(semi_finish_grid(R.J.slots)), dim3(JOIN_THREADS), 0, ctx->stream, R.J, R.A.S, d_res, w.max_depth);
  LAUNCHCHK("k_reach_finish");
  ctx->join.clean = true; s.clean = true;
  return BMX_OK;
}

// ... without an answer: the finish alone (the sharded forms' overflow)
int reach_finish_only(bmx_ctx* ctx, const ReachRun& R, const ReachWant& w) {
  hipLaunchKernelGGL(k_reach_finish, dim3(semi_finish_grid(R.J.slots)), dim3(JOIN_THREADS), 0, ctx->stream, R.J, R.A.S, ctx->reach.stage_res, w.max_depth);
  LAUNCHCHK("k_reach_finish");
  ctx->join.clean = true; ctx->reach.clean = true;
  return BMX_OK;
}

// second half of a staged answer: the record, then the entries it says were delivered, at most `room` of them. -> *got entries written
int reach_collect(bmx_ctx* ctx, uint64_t* out_ids, uint8_t* out_depth, uint64_t room, bmx_reach_res* res, uint64_t* got) {
  const ReachScratch& s = ctx->reach;
  HIPCHK(hipMemcpyAsync(res, s.stage_res, sizeof(bmx_reach_res), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t k = std::min<uint64_t>(std::min<uint64_t>(res->n_match, s.staged), room);
  if (k) {
    HIPCHK(hipMemcpy(out_ids, s.stage_ids, k * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_depth, s.stage_depth, k, hipMemcpyDeviceToHost));
  }
  if (got) *got = k;
  return BMX_OK;
}

// everything behind the seeds on one context: prepare, all rounds blind, the answer
int reach_run(bmx_ctx* ctx, ReachRun* R, uint32_t base_field, const WhereProg& W, const ReachWant& w, int mem) {
  if (int rc = reach_prepare(ctx, R, base_field, W, w)) return rc;
  for (uint32_t r = 1; r <= w.max_depth; r++) if (int rc = reach_round(ctx, *R, r)) return rc;
  if (mem == BMX_MEM_DEVICE) return reach_answer(ctx, *R, base_field, W, w, w.out_ids, w.out_depth, w.res);
  if (int rc = reach_answer(ctx, *R, base_field, W, w, nullptr, nullptr, nullptr)) return rc;
  bmx_reach_res r;
  if (int rc = reach_collect(ctx, w.out_ids, w.out_depth, w.cap, &r, nullptr)) return rc;
  *w.res = r;
  return BMX_OK;
}

std::string reach_text(const char* fn, const char* which, const char* bad) { return std::string(fn) + ": " + which + bad; }

// Both sharded forms. seed(g, shard, run): enqueue the shard's seeds at level 0. The program form exports level 0 and unites it like every later level; the
// list form's `known` arrives complete (listed: the list's own count of values inside the domain) and no shard exports level 0.
template <class Seed>
int comm_reach(bmx_comm* c, uint32_t base_field, const WhereProg& W, const ReachWant& w, uint64_t list, bool seeds_exported, std::vector<int64_t> known, uint64_t listed,
               Seed&& seed) {
  std::vector<ReachRun> R(c->N);
  std::vector<int64_t> fresh;
  std::vector<long long> part;
  bool overflow = false;
  uint64_t lower = 0;                                                    // the largest lower bound of the set's size any overflowing shard reported
  // the keys of `level` from every shard, united; what is known taken out; the rest joins `known`
  auto gather = [&](uint32_t level) {
    fresh.clear();
    const int rc = comm_two_phase(c,
      [&](uint32_t g, bmx_ctx* ctx) {
        if (int erc = enter(ctx)) return erc;
        HIPCHK(hipMemsetAsync(&R[g].A.S->nout, 0, sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(k_reach_export, dim3(semi_finish_grid(R[g].J.slots)), dim3(JOIN_THREADS), 0, ctx->stream, R[g].J, R[g].A.S, (long long)level, ctx->join.stage_keys);
        LAUNCHCHK("k_reach_export");
        return (int)BMX_OK;
      },
      [&](uint32_t g, bmx_ctx* ctx) {
        if (int erc = enter(ctx)) return erc;
        JoinState m; unsigned long long nout = 0;
        HIPCHK(hipMemcpyAsync(&m, R[g].J.S, sizeof(m), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(&nout, &R[g].A.S->nout, sizeof(nout), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (m.overflow || m.claims > w.set_cap) { overflow = true; lower = std::max<uint64_t>(lower, m.claims); return (int)BMX_OK; }
        if (nout > w.set_cap) return fail(ctx, BMX_ERR_INTERNAL, "bmx_comm_where_reach: more keys of one level than set_cap without the overflow flag");
        part.resize(nout);
        if (nout) HIPCHK(hipMemcpy(part.data(), ctx->join.stage_keys, nout * 8, hipMemcpyDeviceToHost));
        fresh.insert(fresh.end(), part.begin(), part.end());
        return (int)BMX_OK;
      });
    if (rc) return rc;
    std::sort(fresh.begin(), fresh.end());
    fresh.erase(std::unique(fresh.begin(), fresh.end()), fresh.end());
    std::vector<int64_t> only(fresh.size());
    only.resize(std::set_difference(fresh.begin(), fresh.end(), known.begin(), known.end(), only.begin()) - only.begin());
    fresh.swap(only);
    std::vector<int64_t> all(known.size() + fresh.size());
    std::merge(known.begin(), known.end(), fresh.begin(), fresh.end(), all.begin());
    known.swap(all);
    if (known.size() > w.set_cap) overflow = true;
    return (int)BMX_OK;
  };
  // `fresh` to every shard at `level` (from a copy nobody touches before every shard's stream has been waited for: the next gather's fetch)
  std::vector<int64_t> sent;
  auto spread = [&](uint32_t level) {
    sent = fresh;
    for (uint32_t g = 0; g < c->N; g++) {
      bmx_ctx* ctx = c->sh[g];
      CSH(g, enter(ctx));
      CSH(g, reach_list_staged(ctx, R[g], sent.data(), sent.size(), level, false));
    }
    return (int)BMX_OK;
  };
  // every shard seeds and prepares
  for (uint32_t g = 0; g < c->N; g++) {
    bmx_ctx* ctx = c->sh[g];
    CSH(g, enter(ctx));
    CSH(g, reach_scratch(ctx, w.set_cap, list, &R[g]));
    CSH(g, seed(g, ctx, R[g]));
    CSH(g, reach_prepare(ctx, &R[g], base_field, W, w));
  }
  bool more = false;
  if (seeds_exported) {
    if (int rc = gather(0)) return rc;
    if (!overflow && !fresh.empty()) if (int rc = spread(0)) return rc;
  } else if (known.size() > w.set_cap) overflow = true;
  for (uint32_t r = 1; r <= w.max_depth && !overflow && !known.empty(); r++) {
    for (uint32_t g = 0; g < c->N; g++) { CSH(g, enter(c->sh[g])); CSH(g, reach_round(c->sh[g], R[g], r)); }
    if (int rc = gather(r)) return rc;
    if (overflow || fresh.empty()) break;
    if (r == w.max_depth) { more = true; break; }
    if (int rc = spread(r)) return rc;
  }
  // every shard's answer enqueued, then fetched shard after shard
  bmx_reach_res tot{};
  uint64_t delivered = 0;
  const int rc = comm_two_phase(c,
    [&](uint32_t g, bmx_ctx* ctx) {
      if (int erc = enter(ctx)) return erc;
      return overflow ? reach_finish_only(ctx, R[g], w) : reach_answer(ctx, R[g], base_field, W, w, nullptr, nullptr, nullptr);
    },
    [&](uint32_t, bmx_ctx* ctx) {
      bmx_reach_res r;
      uint64_t got = 0;
      int crc = enter(ctx);
      if (!crc) crc = reach_collect(ctx, overflow ? nullptr : (w.out_ids ? w.out_ids + delivered : nullptr), overflow ? nullptr : (w.out_depth ? w.out_depth + delivered : nullptr),
                                    overflow ? 0 : w.cap - delivered, &r, &got);
      if (crc) return crc;
      delivered += got;
      tot.n_match += r.n_match; tot.n_seed += r.n_seed; tot.n_edges += r.n_edges; tot.rounds = std::max(tot.rounds, r.rounds);
      return (int)BMX_OK;
    });
  if (rc) return rc;
  if (!seeds_exported) tot.n_seed = listed;
  tot.set_size = std::max<uint64_t>(lower, known.size());
  if (overflow) { tot.n_match = 0; tot.rounds = 0; tot.flags = BMX_REACH_OVERFLOW; }
  else tot.flags = more ? BMX_REACH_MORE : 0u;
  *w.res = tot;
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_where_reach(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t key_field,
                    uint32_t flags, uint32_t seed_base_field, uint32_t seed_nclauses, const uint32_t* seed_clause_len, const bmx_lit* seed_lits, uint32_t seed_field,
                    uint32_t max_depth, uint64_t set_cap, uint64_t* out_ids, uint8_t* out_depth, uint64_t cap, bmx_reach_res* res, int mem) {
  static const char FN[] = "bmx_where_reach";
  WhereProg W, WS;
  const ReachWant w{link_field, key_field, flags, max_depth, set_cap, out_ids, out_depth, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, reach_text(FN, "edge program: ", bad));
  if (const char* bad = where_prepare(seed_base_field, seed_nclauses, seed_clause_len, seed_lits, &WS)) return fail(ctx, BMX_ERR_INVALID, reach_text(FN, "seed program: ", bad));
  if (const char* bad = reach_bad_args(w)) return fail(ctx, BMX_ERR_INVALID, reach_text(FN, "", bad));
  if (seed_field == BMX_AGG_NO_FIELD) return fail(ctx, BMX_ERR_INVALID, reach_text(FN, "", "no seed field"));
  if (int erc = where_enter(ctx, mem)) return erc;
  ReachRun R;
  if (int rc = reach_scratch(ctx, set_cap, 0, &R)) return rc;
  if (int rc = reach_seed(ctx, R, seed_base_field, WS, seed_field)) return rc;
  return reach_run(ctx, &R, base_field, W, w, mem);
}

int bmx_where_reach_from(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t key_field,
                         uint32_t flags, const int64_t* values, uint64_t nvalues, uint32_t max_depth, uint64_t set_cap, uint64_t* out_ids, uint8_t* out_depth,
                         uint64_t cap, bmx_reach_res* res, int mem) {
  static const char FN[] = "bmx_where_reach_from";
  WhereProg W;
  const ReachWant w{link_field, key_field, flags, max_depth, set_cap, out_ids, out_depth, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, reach_text(FN, "edge program: ", bad));
  if (const char* bad = reach_bad_args(w)) return fail(ctx, BMX_ERR_INVALID, reach_text(FN, "", bad));
  if (const char* bad = reach_bad_list(values, nvalues)) return fail(ctx, BMX_ERR_INVALID, reach_text(FN, "", bad));
  if (int erc = where_enter(ctx, mem)) return erc;
  ReachRun R;
  if (int rc = reach_scratch(ctx, set_cap, mem == BMX_MEM_HOST ? nvalues : 0, &R)) return rc;
  if (mem == BMX_MEM_DEVICE) { if (int rc = reach_list(ctx, R, reinterpret_cast<const long long*>(values), nvalues, 0u, true)) return rc; }
  else if (int rc = reach_list_staged(ctx, R, values, nvalues, 0u, true)) return rc;
  return reach_run(ctx, &R, base_field, W, w, mem);
}

int bmx_comm_where_reach(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t key_field,
                         uint32_t flags, uint32_t seed_base_field, uint32_t seed_nclauses, const uint32_t* seed_clause_len, const bmx_lit* seed_lits, uint32_t seed_field,
                         uint32_t max_depth, uint64_t set_cap, uint64_t* out_ids, uint8_t* out_depth, uint64_t cap, bmx_reach_res* res) {
  static const char FN[] = "bmx_comm_where_reach";
  WhereProg W, WS;
  const ReachWant w{link_field, key_field, flags, max_depth, set_cap, out_ids, out_depth, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, reach_text(FN, "edge program: ", bad));
  if (const char* bad = where_prepare(seed_base_field, seed_nclauses, seed_clause_len, seed_lits, &WS)) return fail(c, BMX_ERR_INVALID, reach_text(FN, "seed program: ", bad));
  if (const char* bad = reach_bad_args(w)) return fail(c, BMX_ERR_INVALID, reach_text(FN, "", bad));
  if (seed_field == BMX_AGG_NO_FIELD) return fail(c, BMX_ERR_INVALID, reach_text(FN, "", "no seed field"));
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  return comm_reach(c, base_field, W, w, 0, true, {}, 0, [&](uint32_t, bmx_ctx* x, const ReachRun& R) { return reach_seed(x, R, seed_base_field, WS, seed_field); });
}

int bmx_comm_where_reach_from(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field,
                              uint32_t key_field, uint32_t flags, const int64_t* values, uint64_t nvalues, uint32_t max_depth, uint64_t set_cap, uint64_t* out_ids,
                              uint8_t* out_depth, uint64_t cap, bmx_reach_res* res) {
  static const char FN[] = "bmx_comm_where_reach_from";
  WhereProg W;
  const ReachWant w{link_field, key_field, flags, max_depth, set_cap, out_ids, out_depth, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, reach_text(FN, "edge program: ", bad));
  if (const char* bad = reach_bad_args(w)) return fail(c, BMX_ERR_INVALID, reach_text(FN, "", bad));
  if (const char* bad = reach_bad_list(values, nvalues)) return fail(c, BMX_ERR_INVALID, reach_text(FN, "", bad));
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  // the list's values inside the domain, counted and united on the host: every shard gets the same set at level 0
  std::vector<int64_t> known;
  for (uint64_t i = 0; i < nvalues; i++) if (values[i] >= -VAL_MAX && values[i] <= VAL_MAX) known.push_back(values[i]);
  const uint64_t listed = known.size();
  std::sort(known.begin(), known.end());
  known.erase(std::unique(known.begin(), known.end()), known.end());
  const std::vector<int64_t> seeds = known;
  return comm_reach(c, base_field, W, w, nvalues, false, known, listed, [&](uint32_t, bmx_ctx* x, const ReachRun& R) {
    return seeds.empty() ? (int)BMX_OK : reach_list_staged(x, R, seeds.data(), seeds.size(), 0u, true);
  });
}

}  // extern "C"
