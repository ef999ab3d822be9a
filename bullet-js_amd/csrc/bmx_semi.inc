// bmx_semi.inc — semi-joins (bmx_semi.h): bmx_where_semijoin, bmx_where_in and their sharded forms. The programs are bmx_where.inc's (where_prepare), the
// width dispatch of both sweeps and the entry guards as well (where_sweep, where_enter, where_comm_guard), the kernels semi_kernels.h, and the probe sweep's
// answer is delivered by run_scan_t (bmx_scan.inc) like any scan's — always on its device route: into the caller's device buffer, or into the context's
// staging, from where the host form and the sharded forms fetch it behind the call's last kernel. The context keeps the scratch (SemiScratch): the table and
// the state record, which every query's last kernel leaves empty again (clean), and the staging. Included by bmx.hip (one translation unit), behind everything
// that was here before it.
namespace {

struct SemiWant { uint32_t link_field, flags; uint64_t* out_ids; uint64_t cap; bmx_semi_res* res; };

const char* semi_bad_args(const SemiWant& w, uint64_t set_cap, const char* set_cap_text) {
  if (!w.res) return "null result record";
  if (set_cap == 0 || set_cap > BMX_SEMI_MAX_SET) return set_cap_text;
  if (w.cap && !w.out_ids) return "null out_ids";
  if (w.flags & ~BMX_SEMI_ANTI) return "unknown flag bits in flags";
  if (w.link_field == BMX_AGG_NO_FIELD) return "no link field";
  return nullptr;
}
const char* const SEMI_BAD_SET_CAP = "set_cap outside 1..BMX_SEMI_MAX_SET";
const char* const SEMI_BAD_NVALUES = "nvalues outside 1..BMX_SEMI_MAX_SET";

inline uint64_t semi_slots(uint64_t cap) {
  uint64_t s = 64;
  while (s < 2 * cap) s <<= 1;
  return s;
}
inline uint32_t semi_grid(uint64_t work) { return (uint32_t)std::min<uint64_t>((std::max<uint64_t>(work, 1) + SEMI_THREADS - 1) / SEMI_THREADS, 1024); }
// (every workgroup of k_semi_finish ends with one returning atomic on one word: few workgroups, each with several rounds of slots)
inline uint32_t semi_finish_grid(uint64_t slots) { return (uint32_t)std::min<uint64_t>((slots + SEMI_THREADS - 1) / SEMI_THREADS, 256); }

// the scratch for a set of up to `cap` values: grows to the largest cap asked so far, all or nothing. -> this query's arguments: the head of the table
int semi_scratch(bmx_ctx* ctx, uint64_t cap, SemiArgs* A) {
  SemiScratch& s = ctx->semi;
  if (cap > s.cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.cap = 0; s.slots = 0;
    const uint64_t slots = semi_slots(cap);
    if (int rc = dev_alloc_all(ctx, {{s.keys, slots * sizeof(long long)}, {s.state, sizeof(SemiState)}, {s.stage_keys, cap * sizeof(long long)},
                                     {s.stage_res, sizeof(bmx_semi_res)}})) return rc;
    s.cap = cap; s.slots = slots; s.clean = false;
  }
  if (!s.clean) {     // a new table, or a query that did not get as far as its last kernel
    hipLaunchKernelGGL(k_semi_clear, dim3(semi_finish_grid(s.slots)), dim3(SEMI_THREADS), 0, ctx->stream, s.keys, s.slots, s.state);
    LAUNCHCHK("k_semi_clear");
  }
  A->keys = s.keys; A->S = s.state; A->slots = semi_slots(cap); A->cap = cap;
  s.clean = false;
  return BMX_OK;
}

// room for `n` ids of a host-mode answer on its way down
int semi_stage_ids(bmx_ctx* ctx, uint64_t n) {
  SemiScratch& s = ctx->semi;
  if (n > s.ids_cap || !s.stage_ids) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.ids_cap = 0;
    if (int rc = dev_alloc(ctx, &s.stage_ids, n)) return rc;
    s.ids_cap = std::max<uint64_t>(n, 1);
  }
  return BMX_OK;
}

// the set from the inner program: one sweep of the inner base field's index
int semi_build(bmx_ctx* ctx, const SemiArgs& A, uint32_t in_base_field, const WhereProg& WI, uint32_t key_field) {
  Index* ix;
  if (int rc = fresh_index(ctx, in_base_field, &ix)) return rc;
  const uint32_t src = where_agg_source(key_field, in_base_field);
  where_sweep_c(ctx, ix, WI, [&](const auto& P, uint32_t blocks) {
    hipLaunchKernelGGL((k_semi_build<decltype(where_value(P)), where_clocks<decltype(P)>>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, A, key_field, src);
  });
  LAUNCHCHK("k_semi_build");
  return BMX_OK;
}

// the set from a list of `n` values in device memory
int semi_insert_list(bmx_ctx* ctx, const SemiArgs& A, const long long* d_values, uint64_t n) {
  hipLaunchKernelGGL(k_semi_insert, dim3(semi_grid(n)), dim3(SEMI_THREADS), 0, ctx->stream, d_values, n, A);
  LAUNCHCHK("k_semi_insert");
  return BMX_OK;
}

template <class T, bool CLOCKS>
int semi_scan(bmx_ctx* ctx, const Index* ix, const PredWhere<T, true, CLOCKS>& P, const SemiArgs& A, uint32_t base_field, const SemiWant& w, uint64_t* d_ids, uint64_t d_cap) {
  PredSemi<T, CLOCKS> Q;
  Q.P = P;
  Q.keys = A.keys; Q.slots = A.slots; Q.S = A.S; Q.cap = A.cap;
  Q.link = w.link_field; Q.link_src = where_agg_source(w.link_field, base_field); Q.anti = w.flags & BMX_SEMI_ANTI;
  return run_scan_t<false>(ctx, Q, ix, d_cap ? d_ids : nullptr, d_cap, reinterpret_cast<uint64_t*>(&A.S->n_match), BMX_MEM_DEVICE, /*deferred=*/false);
}

// The probe sweep over a table that has been built, and the call's last kernel. d_ids (device memory, or nullptr: the context's staging, sized here) gets up to
// w.cap ids and d_res (or the staging's record) the result. A value-ordered view of the base field's index is neither read nor touched (where_run).
int semi_probe(bmx_ctx* ctx, const SemiArgs& A, uint32_t base_field, const WhereProg& W, const SemiWant& w, uint64_t* d_ids, bmx_semi_res* d_res) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  SemiScratch& s = ctx->semi;
  uint64_t d_cap = w.cap;
  if (!d_ids) {
    d_cap = std::min<uint64_t>(w.cap, ix->n);                           // (no more ids can come)
    if (d_cap) { if (int rc = semi_stage_ids(ctx, d_cap)) return rc; d_ids = s.stage_ids; }
    s.staged = d_cap;
  }
  if (int rc = where_sweep_c(ctx, ix, W, [&](const auto& P, uint32_t) { return semi_scan(ctx, ix, P, A, base_field, w, d_ids, d_cap); })) return rc;     // (the grid is run_scan_t's own)
  hipLaunchKernelGGL(k_semi_finish, dim3(semi_finish_grid(A.slots)), dim3(SEMI_THREADS), 0, ctx->stream, A, d_res ? d_res : s.stage_res);
  LAUNCHCHK("k_semi_finish");
  s.clean = true;
  return BMX_OK;
}

// second half of a staged answer: the record, then the ids it says were delivered, at most `room` of them. -> *got ids written to `out`
int semi_collect(bmx_ctx* ctx, uint64_t* out, uint64_t room, bmx_semi_res* res, uint64_t* got) {
  const SemiScratch& s = ctx->semi;
  HIPCHK(hipMemcpyAsync(res, s.stage_res, sizeof(bmx_semi_res), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t k = std::min<uint64_t>(std::min<uint64_t>(res->n_match, s.staged), room);
  if (k) HIPCHK(hipMemcpy(out, s.stage_ids, k * 8, hipMemcpyDeviceToHost));
  if (got) *got = k;
  return BMX_OK;
}

// one shard's (or the one context's) bmx_where_in with the values in HOST memory, enqueued into the staging
int semi_in_staged(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, const SemiWant& w, const int64_t* values, uint64_t nvalues) {
  SemiArgs A;
  if (int rc = semi_scratch(ctx, std::max<uint64_t>(nvalues, 1), &A)) return rc;
  if (nvalues) HIPCHK(hipMemcpyAsync(ctx->semi.stage_keys, values, nvalues * 8, hipMemcpyHostToDevice, ctx->stream));
  if (int rc = semi_insert_list(ctx, A, ctx->semi.stage_keys, nvalues)) return rc;
  return semi_probe(ctx, A, base_field, W, w, nullptr, nullptr);
}

std::string semi_text(const char* fn, const char* which, const char* bad) { return std::string(fn) + ": " + which + bad; }

// phase 2 of both sharded forms: the `m` values of `vals` (host memory) to every shard, every probe sweep enqueued, then the answers shard after shard
int comm_semi_in(bmx_comm* c, uint32_t base_field, const WhereProg& W, const SemiWant& w, const int64_t* vals, uint64_t m, bmx_semi_res* tot) {
  uint64_t delivered = 0;
  *tot = bmx_semi_res{};
  return comm_two_phase(c,
    [&](uint32_t, bmx_ctx* x) { const int erc = enter(x); return erc ? erc : semi_in_staged(x, base_field, W, w, vals, m); },
    [&](uint32_t g, bmx_ctx* x) {
      bmx_semi_res r;
      uint64_t got = 0;
      int crc = enter(x);
      if (!crc) crc = semi_collect(x, w.out_ids ? w.out_ids + delivered : nullptr, w.cap - delivered, &r, &got);
      if (crc) return crc;
      delivered += got; tot->n_match += r.n_match;
      if (g == 0) { tot->set_size = r.set_size; tot->n_inner = r.n_inner; }     // (every shard was given the same list)
      return (int)BMX_OK;
    });
}

}  // namespace

extern "C" {

int bmx_where_semijoin(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t flags,
                       uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits, uint32_t key_field, uint64_t set_cap,
                       uint64_t* out_ids, uint64_t cap, bmx_semi_res* res, int mem) {
  static const char FN[] = "bmx_where_semijoin";
  WhereProg W, WI;
  const SemiWant w{link_field, flags, out_ids, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, semi_text(FN, "outer program: ", bad));
  if (const char* bad = where_prepare(in_base_field, in_nclauses, in_clause_len, in_lits, &WI)) return fail(ctx, BMX_ERR_INVALID, semi_text(FN, "inner program: ", bad));
  if (const char* bad = semi_bad_args(w, set_cap, SEMI_BAD_SET_CAP)) return fail(ctx, BMX_ERR_INVALID, semi_text(FN, "", bad));
  if (key_field == BMX_AGG_NO_FIELD) return fail(ctx, BMX_ERR_INVALID, semi_text(FN, "", "no key field"));
  if (int erc = where_enter(ctx, mem)) return erc;
  SemiArgs A;
  if (int rc = semi_scratch(ctx, set_cap, &A)) return rc;
  if (int rc = semi_build(ctx, A, in_base_field, WI, key_field)) return rc;
  if (mem == BMX_MEM_DEVICE) return semi_probe(ctx, A, base_field, W, w, out_ids, res);
  if (int rc = semi_probe(ctx, A, base_field, W, w, nullptr, nullptr)) return rc;
  bmx_semi_res r;
  if (int rc = semi_collect(ctx, out_ids, cap, &r, nullptr)) return rc;
  *res = r;
  return BMX_OK;
}

int bmx_where_in(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t flags,
                 const int64_t* values, uint64_t nvalues, uint64_t* out_ids, uint64_t cap, bmx_semi_res* res, int mem) {
  static const char FN[] = "bmx_where_in";
  WhereProg W;
  const SemiWant w{link_field, flags, out_ids, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, semi_text(FN, "outer program: ", bad));
  if (const char* bad = semi_bad_args(w, nvalues, SEMI_BAD_NVALUES)) return fail(ctx, BMX_ERR_INVALID, semi_text(FN, "", bad));
  if (!values) return fail(ctx, BMX_ERR_INVALID, semi_text(FN, "", "null values"));
  if (int erc = where_enter(ctx, mem)) return erc;
  if (mem == BMX_MEM_DEVICE) {
    SemiArgs A;
    if (int rc = semi_scratch(ctx, nvalues, &A)) return rc;
    if (int rc = semi_insert_list(ctx, A, reinterpret_cast<const long long*>(values), nvalues)) return rc;
    return semi_probe(ctx, A, base_field, W, w, out_ids, res);
  }
  if (int rc = semi_in_staged(ctx, base_field, W, w, values, nvalues)) return rc;
  bmx_semi_res r;
  if (int rc = semi_collect(ctx, out_ids, cap, &r, nullptr)) return rc;
  *res = r;
  return BMX_OK;
}

int bmx_comm_where_semijoin(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t flags,
                            uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits, uint32_t key_field, uint64_t set_cap,
                            uint64_t* out_ids, uint64_t cap, bmx_semi_res* res) {
  static const char FN[] = "bmx_comm_where_semijoin";
  WhereProg W, WI;
  const SemiWant w{link_field, flags, out_ids, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, semi_text(FN, "outer program: ", bad));
  if (const char* bad = where_prepare(in_base_field, in_nclauses, in_clause_len, in_lits, &WI)) return fail(c, BMX_ERR_INVALID, semi_text(FN, "inner program: ", bad));
  if (const char* bad = semi_bad_args(w, set_cap, SEMI_BAD_SET_CAP)) return fail(c, BMX_ERR_INVALID, semi_text(FN, "", bad));
  if (key_field == BMX_AGG_NO_FIELD) return fail(c, BMX_ERR_INVALID, semi_text(FN, "", "no key field"));
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  // phase 1: every shard's own set, exported; the union on the host
  std::vector<int64_t> all;
  std::vector<long long> part;
  uint64_t n_inner = 0, lower = 0;                                    // lower: the largest lower bound of the set's size any overflowing shard reported
  bool overflow = false;
  int rc = comm_two_phase(c,
    [&](uint32_t, bmx_ctx* x) {
      if (int erc = enter(x)) return erc;
      SemiArgs A;
      if (int src = semi_scratch(x, set_cap, &A)) return src;
      if (int src = semi_build(x, A, in_base_field, WI, key_field)) return src;
      bmx_ctx* ctx = x;
      hipLaunchKernelGGL(k_semi_export, dim3(semi_finish_grid(A.slots)), dim3(SEMI_THREADS), 0, ctx->stream, A, ctx->semi.stage_keys);
      LAUNCHCHK("k_semi_export");
      hipLaunchKernelGGL(k_semi_finish, dim3(semi_finish_grid(A.slots)), dim3(SEMI_THREADS), 0, ctx->stream, A, ctx->semi.stage_res);
      LAUNCHCHK("k_semi_finish");
      ctx->semi.clean = true;
      return (int)BMX_OK;
    },
    [&](uint32_t, bmx_ctx* ctx) {
      if (int erc = enter(ctx)) return erc;
      bmx_semi_res r;
      HIPCHK(hipMemcpyAsync(&r, ctx->semi.stage_res, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      n_inner += r.n_inner;
      if (r.flags & BMX_SEMI_OVERFLOW) { overflow = true; lower = std::max<uint64_t>(lower, r.set_size); return (int)BMX_OK; }
      if (r.set_size > set_cap) return fail(ctx, BMX_ERR_INTERNAL, "bmx_comm_where_semijoin: more keys than set_cap without the overflow flag");
      part.resize(r.set_size);
      if (r.set_size) HIPCHK(hipMemcpy(part.data(), ctx->semi.stage_keys, r.set_size * 8, hipMemcpyDeviceToHost));
      all.insert(all.end(), part.begin(), part.end());
      return (int)BMX_OK;
    });
  if (rc) return rc;
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  if (overflow || all.size() > set_cap) {
    bmx_semi_res o{};
    o.set_size = std::max<uint64_t>(lower, all.size()); o.n_inner = n_inner; o.flags = BMX_SEMI_OVERFLOW;
    *res = o;
    return BMX_OK;
  }
  // phase 2
  bmx_semi_res tot;
  if ((rc = comm_semi_in(c, base_field, W, w, all.data(), all.size(), &tot))) return rc;
  tot.set_size = all.size(); tot.n_inner = n_inner;
  *res = tot;
  return BMX_OK;
}

int bmx_comm_where_in(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t link_field, uint32_t flags,
                      const int64_t* values, uint64_t nvalues, uint64_t* out_ids, uint64_t cap, bmx_semi_res* res) {
  static const char FN[] = "bmx_comm_where_in";
  WhereProg W;
  const SemiWant w{link_field, flags, out_ids, cap, res};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, semi_text(FN, "outer program: ", bad));
  if (const char* bad = semi_bad_args(w, nvalues, SEMI_BAD_NVALUES)) return fail(c, BMX_ERR_INVALID, semi_text(FN, "", bad));
  if (!values) return fail(c, BMX_ERR_INVALID, semi_text(FN, "", "null values"));
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  bmx_semi_res tot;
  if (int rc = comm_semi_in(c, base_field, W, w, values, nvalues, &tot)) return rc;
  *res = tot;
  return BMX_OK;
}

}  // extern "C"
