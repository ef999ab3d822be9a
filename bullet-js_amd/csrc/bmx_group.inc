// bmx_group.inc — group-by over discovered values (bmx_group.h): bmx_where_group and its sharded form, and what every grouped answer shares (this one's, the
// group-by over several fields' and the lookup joins'): the staged answer's second half (grouped_collect), the merge of two sorted lists (merge_sorted) and
// the sharded combine (comm_grouped). The program, the width dispatch of the sweep and the entry guards are bmx_where.inc's (where_prepare, where_sweep,
// where_enter, where_comm_guard), the kernels are group_kernels.h. The context keeps their scratch (GroupScratch): the table, the state record, which every
// query's last kernel leaves empty again (clean), and the answer of a host-mode call on its way down. Included by bmx.hip (one translation unit), behind
// everything that was here before it.
namespace {

const char* group_bad_args(uint32_t group_field, const bmx_group_rec* out, uint64_t cap, const bmx_group_res* res) {
  if (!res) return "bmx_where_group: null result record";
  if (cap == 0 || cap > BMX_GROUP_MAX_CAP) return "bmx_where_group: cap outside 1..BMX_GROUP_MAX_CAP";
  if (!out) return "bmx_where_group: null output";
  if (group_field == BMX_AGG_NO_FIELD) return "bmx_where_group: no group field";
  return nullptr;
}

inline uint64_t group_slots(uint64_t cap) {
  uint64_t s = 64;
  while (s < 2 * cap) s <<= 1;
  return s;
}
// (every workgroup of k_group_finish ends with one returning atomic on one word: few workgroups, each with several rounds of slots)
inline uint32_t group_finish_grid(uint64_t slots) { return (uint32_t)std::min<uint64_t>((slots + 255) / 256, 256); }

// the scratch for a query of `cap` records: grows to the largest cap asked so far, all or nothing
int group_scratch(bmx_ctx* ctx, uint64_t cap) {
  GroupScratch& s = ctx->group;
  if (cap > s.cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.cap = 0; s.slots = 0;
    const uint64_t slots = group_slots(cap);
    if (int rc = dev_alloc_all(ctx, {{s.keys, slots * sizeof(long long)}, {s.acc, slots * sizeof(AggRaw)}, {s.state, sizeof(GroupState)},
                                     {s.stage, cap * sizeof(bmx_group_rec)}, {s.stage_res, sizeof(bmx_group_res)}})) return rc;
    s.cap = cap; s.slots = slots; s.clean = false;
  }
  if (!s.clean) {     // a new table, or a query that did not get as far as its last kernel
    hipLaunchKernelGGL(k_group_clear, dim3(group_finish_grid(s.slots)), dim3(256), 0, ctx->stream, s.keys, s.acc, s.slots, s.state);
    LAUNCHCHK("k_group_clear");
  }
  return BMX_OK;
}

// Enqueue one group-by over a prepared program; the records and the result record go to d_out / d_res (device memory), or, with d_out == nullptr, to the
// context's staging buffers (group_collect fetches them). The arguments have been checked and the context entered. A value-ordered view of the base field's
// index is neither read nor touched (where_run). EXPR: the measure is X's expression, as in where_agg_enqueue.
template <bool EXPR = false>
int group_enqueue(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint32_t measure_field, uint32_t group_field, uint64_t cap, bmx_group_rec* d_out,
                  bmx_group_res* d_res, const ExprArgs<EXPR>& X = ExprArgs<EXPR>()) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  if (int rc = group_scratch(ctx, cap)) return rc;
  GroupScratch& s = ctx->group;
  GroupArgs A{};
  A.keys = s.keys; A.acc = s.acc; A.S = s.state;
  A.slots = group_slots(cap); A.cap = cap;                         // (a query uses the head of a table that an earlier, larger one left empty)
  A.measure = measure_field; A.group = group_field;
  A.m_src = EXPR ? AGG_SRC_PROBE : where_agg_source(measure_field, base_field); A.g_src = where_agg_source(group_field, base_field);
  s.clean = false;
  where_sweep_c(ctx, ix, W, [&](const auto& P, uint32_t blocks) {
    hipLaunchKernelGGL((k_group_sweep<decltype(where_value(P)), where_clocks<decltype(P)>, EXPR>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, A, X);
  });
  LAUNCHCHK("k_group_sweep");
  hipLaunchKernelGGL(k_group_finish, dim3(group_finish_grid(A.slots)), dim3(256), 0, ctx->stream, A, d_out ? d_out : s.stage, d_out ? d_res : s.stage_res,
                     A.m_src != AGG_SRC_PROBE ? 1u : 0u);
  LAUNCHCHK("k_group_finish");
  s.clean = true;
  return BMX_OK;
}

inline bool group_key_less(const bmx_group_rec& a, const bmx_group_rec& b) { return a.key < b.key; }

// Second half of a staged grouped answer: the result record, then (if they fit) the records, sorted by `less`. `recs` gets them; nothing of the caller's is
// written. no_recs: the flag bits of the record that say no records were written. fn: the entry point, for the internal error's text. perm (optional) gets the
// sort's permutation: recs[i] was record perm[i] of the staging (a form that staged columns beside its records moves their rows the same way).
template <class Rec, class Res, class Less>
int grouped_collect(bmx_ctx* ctx, const Rec* stage, const Res* stage_res, uint32_t no_recs, uint64_t cap, Less less, const char* fn, std::vector<Rec>& recs, Res* res,
                    std::vector<uint32_t>* perm = nullptr) {
  HIPCHK(hipMemcpyAsync(res, stage_res, sizeof(Res), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  recs.clear();
  if (perm) perm->clear();
  if (res->flags & no_recs) return BMX_OK;
  if (res->n_groups > cap) return fail(ctx, BMX_ERR_INTERNAL, std::string(fn) + ": more records than cap without the overflow flag");
  recs.resize(res->n_groups);
  if (res->n_groups) {
    HIPCHK(hipMemcpyAsync(recs.data(), stage, res->n_groups * sizeof(Rec), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!perm) std::sort(recs.begin(), recs.end(), less);
    else {
      const std::vector<Rec> raw(recs);
      perm->resize(raw.size());
      for (uint32_t i = 0; i < raw.size(); i++) (*perm)[i] = i;
      std::sort(perm->begin(), perm->end(), [&](uint32_t a, uint32_t b) { return less(raw[a], raw[b]); });
      for (size_t i = 0; i < raw.size(); i++) recs[i] = raw[(*perm)[i]];
    }
  }
  return BMX_OK;
}
int group_collect(bmx_ctx* ctx, uint64_t cap, std::vector<bmx_group_rec>& recs, bmx_group_res* res) {
  return grouped_collect(ctx, ctx->group.stage, ctx->group.stage_res, BMX_GROUP_OVERFLOW, cap, group_key_less, "bmx_where_group", recs, res);
}

// ... and into the caller's host memory: what a host-mode call ends with
int group_collect_to(bmx_ctx* ctx, uint64_t cap, bmx_group_rec* out, bmx_group_res* res) {
  std::vector<bmx_group_rec> recs;
  bmx_group_res r;
  if (int rc = group_collect(ctx, cap, recs, &r)) return rc;
  if (!recs.empty()) std::memcpy(out, recs.data(), recs.size() * sizeof(bmx_group_rec));
  *res = r;
  return BMX_OK;
}

// a += b: counts and 128-bit sums add, minima and maxima fold (comm_agg_with's combine)
inline void group_fold(bmx_agg& o, const bmx_agg& p) {
  o.n_match += p.n_match; o.n += p.n;
  o.min = std::min(o.min, p.min); o.max = std::max(o.max, p.max);
  const unsigned __int128 s = (((unsigned __int128)(uint64_t)o.sum_hi << 64) | o.sum_lo) + (((unsigned __int128)(uint64_t)p.sum_hi << 64) | p.sum_lo);
  o.sum_lo = (uint64_t)s; o.sum_hi = (int64_t)(uint64_t)(s >> 64);
}
// the aggregates of shard g's result record into the communicator's: shard 0's start it
inline void group_fold_res(uint32_t g, bmx_group_res& tot, const bmx_group_res& r) {
  if (g == 0) { tot.absent = r.absent; tot.total = r.total; } else { group_fold(tot.absent, r.absent); group_fold(tot.total, r.total); }
}

// how two records of one key become one: the aggregates fold (every grouped answer whose record ends in a bmx_agg)
struct GroupRecFold {
  template <class Rec>
  void operator()(Rec& m, const Rec& p) const { group_fold(m.agg, p.agg); }
};

// all = all UNION part: two lists sorted by `less` into one, the records of equal keys folded by `recfold` (tmp: scratch of the caller's)
template <class Rec, class Less, class RecFold = GroupRecFold>
void merge_sorted(std::vector<Rec>& all, const std::vector<Rec>& part, std::vector<Rec>& tmp, Less less, RecFold recfold = RecFold()) {
  tmp.clear(); tmp.reserve(all.size() + part.size());
  size_t i = 0, j = 0;
  while (i < all.size() || j < part.size()) {
    if (j == part.size() || (i < all.size() && less(all[i], part[j]))) tmp.push_back(all[i++]);
    else if (i == all.size() || less(part[j], all[i])) tmp.push_back(part[j++]);
    else { Rec m = all[i++]; recfold(m, part[j++]); tmp.push_back(m); }
  }
  all.swap(tmp);
}

// A grouped answer over the shards: enqueue(x) on every shard (entered here), then shard after shard collect(x, part, &r) — its sorted list and its record — and
// fold(g, *tot, r), the form's own aggregates; the lists merged, equal keys folded. A shard that overflowed reports a lower bound of the number of groups: the
// answer overflows (`overflow`: the form's flag bit) with the largest bound any shard or the union gives. Otherwise the records go to `out`. recfold:
// merge_sorted's.
template <class Rec, class Res, class Less, class Enqueue, class Collect, class Fold, class RecFold = GroupRecFold>
int comm_grouped(bmx_comm* c, uint64_t cap, uint32_t overflow, Less less, Rec* out, Res* tot, Enqueue enqueue, Collect collect, Fold fold, RecFold recfold = RecFold()) {
  std::vector<Rec> all, part, tmp;
  uint64_t lower = 0;
  bool over = false;
  *tot = Res{};
  const int rc = comm_two_phase(c,
    [&](uint32_t, bmx_ctx* x) { const int erc = enter(x); return erc ? erc : enqueue(x); },
    [&](uint32_t g, bmx_ctx* x) {
      Res r;
      int crc = enter(x);
      if (!crc) crc = collect(x, part, &r);
      if (crc) return crc;
      fold(g, *tot, r);
      if (r.flags & overflow) { over = true; lower = std::max<uint64_t>(lower, r.n_groups); return (int)BMX_OK; }
      merge_sorted(all, part, tmp, less, recfold);
      return (int)BMX_OK;
    });
  if (rc) return rc;
  lower = std::max<uint64_t>(lower, all.size());
  if (over || all.size() > cap) { tot->flags = overflow; tot->n_groups = lower; }
  else { tot->flags = 0; tot->n_groups = all.size(); if (!all.empty()) std::memcpy(out, all.data(), all.size() * sizeof(Rec)); }
  tot->reserved = 0;
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_where_group(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t measure_field,
                    uint32_t group_field, bmx_group_rec* out, uint64_t cap, bmx_group_res* res, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = group_bad_args(group_field, out, cap, res)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (mem == BMX_MEM_DEVICE) return group_enqueue(ctx, base_field, W, measure_field, group_field, cap, out, res);
  if (int rc = group_enqueue(ctx, base_field, W, measure_field, group_field, cap, nullptr, nullptr)) return rc;
  return group_collect_to(ctx, cap, out, res);
}

int bmx_comm_where_group(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t measure_field,
                         uint32_t group_field, bmx_group_rec* out, uint64_t cap, bmx_group_res* res) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = group_bad_args(group_field, out, cap, res)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  bmx_group_res tot;
  if (int rc = comm_grouped(c, cap, BMX_GROUP_OVERFLOW, group_key_less, out, &tot,
        [&](bmx_ctx* x) { return group_enqueue(x, base_field, W, measure_field, group_field, cap, nullptr, nullptr); },
        [&](bmx_ctx* x, std::vector<bmx_group_rec>& part, bmx_group_res* r) { return group_collect(x, cap, part, r); }, group_fold_res)) return rc;
  *res = tot;
  return BMX_OK;
}

}  // extern "C"
