// bmx_group_multi.inc — group-by over several fields (bmx_group_multi.h): bmx_where_group_multi and its sharded form. The program is bmx_where.inc's
// (where_prepare), and so are the width dispatch of the sweep and the entry guards (where_sweep, where_enter, where_comm_guard); the slot count, the finish
// grid, the fold of two records and the collect, merge and sharded combine of a grouped answer are bmx_group.inc's (group_slots, group_finish_grid, group_fold,
// grouped_collect, merge_sorted, comm_grouped), the kernels are mgroup_kernels.h. The context keeps their scratch (MGroupScratch):
// the tuple table, the dictionaries, the state records, which every query's last kernels leave empty again (clean), and the answer of a host-mode call on its
// way down. bmx_where_group's scratch (ctx->group) is neither read nor written. Included by bmx.hip (one translation unit), behind everything that was here
// before it.
namespace {

constexpr int64_t MGROUP_BIG = (1ll << 53) - 1;

const char* mgroup_bad_args(uint32_t nkeys, const bmx_group_key* keys, const bmx_mgroup_rec* out, uint64_t cap, const bmx_group_res* res) {
  if (!res) return "bmx_where_group_multi: null result record";
  if (!out) return "bmx_where_group_multi: null output";
  if (!keys) return "bmx_where_group_multi: null keys";
  if (nkeys < 1 || nkeys > BMX_MGROUP_MAX_KEYS) return "bmx_where_group_multi: nkeys outside 1..BMX_MGROUP_MAX_KEYS";
  for (uint32_t j = 0; j < nkeys; j++) {
    if (keys[j].field == BMX_AGG_NO_FIELD) return "bmx_where_group_multi: no key field";
    if (keys[j].flags != 0) return "bmx_where_group_multi: unknown key flag bits";
    if (keys[j].width < 1 || keys[j].width > MGROUP_BIG) return "bmx_where_group_multi: width outside 1..2^53 - 1";
    if (keys[j].origin < -MGROUP_BIG || keys[j].origin > MGROUP_BIG) return "bmx_where_group_multi: origin outside +-(2^53 - 1)";
  }
  if (cap == 0 || cap > BMX_GROUP_MAX_CAP) return "bmx_where_group_multi: cap outside 1..BMX_GROUP_MAX_CAP";
  if (nkeys == BMX_MGROUP_MAX_KEYS && cap > BMX_MGROUP_MAX_CAP4) return "bmx_where_group_multi: cap above BMX_MGROUP_MAX_CAP4 with four keys";
  return nullptr;
}

// the scratch for a query of `cap` records and `nkeys` dictionaries: grows to the largest asked so far, all or nothing
int mgroup_scratch(bmx_ctx* ctx, uint64_t cap, uint32_t nkeys) {
  MGroupScratch& s = ctx->mgroup;
  const uint64_t words = nkeys * group_slots(cap);
  if (cap > s.cap || words > s.dict_words) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const uint64_t ncap = std::max(cap, s.cap), nwords = std::max(words, s.dict_words), slots = group_slots(ncap);
    s.cap = 0; s.slots = 0; s.dict_words = 0;
    if (int rc = dev_alloc_all(ctx, {{s.keys, slots * sizeof(long long)}, {s.acc, slots * sizeof(AggRaw)}, {s.dict, nwords * sizeof(long long)},
                                     {s.state, (MGROUP_KEYS + 1) * sizeof(GroupState)}, {s.stage, ncap * sizeof(bmx_mgroup_rec)},
                                     {s.stage_res, sizeof(bmx_group_res)}})) return rc;
    s.cap = ncap; s.slots = slots; s.dict_words = nwords; s.clean = false;
  }
  if (!s.clean) {     // new tables, or a query that did not get as far as its last kernel
    hipLaunchKernelGGL(k_mgroup_clear, dim3(group_finish_grid(std::max(s.slots, s.dict_words))), dim3(256), 0, ctx->stream, s.dict, s.dict_words, s.state + 1, s.keys,
                       s.acc, s.slots, s.state);
    LAUNCHCHK("k_mgroup_clear");
  }
  return BMX_OK;
}

// Enqueue one query over a prepared program; the records and the result record go to d_out / d_res (device memory), or, with d_out == nullptr, to the context's
// staging buffers (mgroup_collect fetches them). The arguments have been checked and the context entered.
int mgroup_enqueue(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint32_t measure_field, uint32_t nkeys, const bmx_group_key* keys, uint64_t cap,
                   bmx_mgroup_rec* d_out, bmx_group_res* d_res) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  if (int rc = mgroup_scratch(ctx, cap, nkeys)) return rc;
  MGroupScratch& s = ctx->mgroup;
  MGroupArgs A{};
  A.T.keys = s.keys; A.T.acc = s.acc; A.T.S = s.state;
  A.T.slots = group_slots(cap); A.T.cap = cap;                      // (a query uses the head of tables that an earlier, larger one left empty)
  A.T.measure = measure_field; A.T.m_src = where_agg_source(measure_field, base_field);
  A.T.group = BMX_AGG_NO_FIELD; A.T.g_src = AGG_SRC_NONE;
  A.dict = s.dict; A.DS = s.state + 1; A.nkeys = nkeys;
  while ((1ull << A.shift) < A.T.slots) A.shift++;
  for (uint32_t j = 0; j < nkeys; j++) A.k[j] = MGroupKey{keys[j].origin, keys[j].width, keys[j].field, where_agg_source(keys[j].field, base_field)};
  s.clean = false;
  where_sweep_c(ctx, ix, W, [&](const auto& P, uint32_t blocks) {
    hipLaunchKernelGGL((k_mgroup_sweep<decltype(where_value(P)), where_clocks<decltype(P)>>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, A);
  });
  LAUNCHCHK("k_mgroup_sweep");
  hipLaunchKernelGGL(k_mgroup_finish, dim3(group_finish_grid(A.T.slots)), dim3(256), 0, ctx->stream, A, d_out ? d_out : s.stage, d_out ? d_res : s.stage_res,
                     A.T.m_src != AGG_SRC_PROBE ? 1u : 0u);
  LAUNCHCHK("k_mgroup_finish");
  // behind the finish, which read the keys back through them: the dictionaries and their state records
  hipLaunchKernelGGL(k_mgroup_clear, dim3(group_finish_grid(nkeys * A.T.slots)), dim3(256), 0, ctx->stream, s.dict, nkeys * A.T.slots, s.state + 1,
                     (long long*)nullptr, (AggRaw*)nullptr, (uint64_t)0, (GroupState*)nullptr);
  LAUNCHCHK("k_mgroup_clear");
  s.clean = true;
  return BMX_OK;
}

inline bool mgroup_key_less(const bmx_mgroup_rec& a, const bmx_mgroup_rec& b) { return std::lexicographical_compare(a.key, a.key + 4, b.key, b.key + 4); }

// second half of a host-mode query: the records sorted by tuple (grouped_collect)
int mgroup_collect(bmx_ctx* ctx, uint64_t cap, std::vector<bmx_mgroup_rec>& recs, bmx_group_res* res) {
  return grouped_collect(ctx, ctx->mgroup.stage, ctx->mgroup.stage_res, BMX_GROUP_OVERFLOW, cap, mgroup_key_less, "bmx_where_group_multi", recs, res);
}

}  // namespace

extern "C" {

int bmx_where_group_multi(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t measure_field,
                          uint32_t nkeys, const bmx_group_key* keys, bmx_mgroup_rec* out, uint64_t cap, bmx_group_res* res, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = mgroup_bad_args(nkeys, keys, out, cap, res)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (mem == BMX_MEM_DEVICE) return mgroup_enqueue(ctx, base_field, W, measure_field, nkeys, keys, cap, out, res);
  if (int rc = mgroup_enqueue(ctx, base_field, W, measure_field, nkeys, keys, cap, nullptr, nullptr)) return rc;
  std::vector<bmx_mgroup_rec> recs;
  bmx_group_res r;
  if (int rc = mgroup_collect(ctx, cap, recs, &r)) return rc;
  if (!recs.empty()) std::memcpy(out, recs.data(), recs.size() * sizeof(bmx_mgroup_rec));
  *res = r;
  return BMX_OK;
}

int bmx_comm_where_group_multi(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t measure_field,
                               uint32_t nkeys, const bmx_group_key* keys, bmx_mgroup_rec* out, uint64_t cap, bmx_group_res* res) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = mgroup_bad_args(nkeys, keys, out, cap, res)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  bmx_group_res tot;
  if (int rc = comm_grouped(c, cap, BMX_GROUP_OVERFLOW, mgroup_key_less, out, &tot,
        [&](bmx_ctx* x) { return mgroup_enqueue(x, base_field, W, measure_field, nkeys, keys, cap, nullptr, nullptr); },
        [&](bmx_ctx* x, std::vector<bmx_mgroup_rec>& part, bmx_group_res* r) { return mgroup_collect(x, cap, part, r); }, group_fold_res)) return rc;
  *res = tot;
  return BMX_OK;
}

}  // extern "C"
