// bmx_where_agg.inc — aggregates and top-k over boolean filters (bmx_where_agg.h): bmx_where_aggregate, bmx_where_top and their sharded forms. The program is
// bmx_where.inc's, and so are the predicate, the sweep grid, the width dispatch and the entry guards (where_prepare, where_sweep, where_enter, where_comm_guard);
// the two sweeps are where_agg_kernels.h, and everything behind them is bmx_agg.inc's and bmx_top.inc's: the scratch with its `clean` protocol, k_agg_finish, the
// select's chain (top_launch_with), the collect halves, and bmx_comm.inc's combine steps. Included by bmx.hip (one translation unit), behind everything that was
// here before it.
namespace {

// agg_bad_args / top_bad_args without their term checks: the program stands where the terms stood and where_prepare has judged it
const bmx_term WHERE_AGG_NO_TERMS[1] = {};
const char* where_agg_bad_args(uint32_t group_field, uint32_t ngroups, const bmx_agg* out) { return agg_bad_args(1, WHERE_AGG_NO_TERMS, group_field, ngroups, out); }
const char* where_top_bad_args(uint32_t flags, uint32_t k, const bmx_top_rec* out) { return top_bad_args(1, WHERE_AGG_NO_TERMS, flags, k, out); }

// the sweep of one aggregate: flat, grouped in LDS, or grouped in device memory. EXPR: with a computed measure X (bmx_expr.inc), otherwise X is empty
template <class T, bool CLOCKS, bool EXPR>
void where_agg_launch(bmx_ctx* ctx, const Index* ix, const PredWhere<T, true, CLOCKS>& P, uint32_t blocks, const AggArgs& A, const ExprArgs<EXPR>& X) {
  if (A.ngroups == 0) hipLaunchKernelGGL((k_where_agg<T, 0, CLOCKS, EXPR>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, A, X);
  else if (A.ngroups <= AGG_LDS_GROUPS) hipLaunchKernelGGL((k_where_agg<T, 1, CLOCKS, EXPR>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, A, X);
  else hipLaunchKernelGGL((k_where_agg<T, 2, CLOCKS, EXPR>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, A, X);
}

// Enqueue one aggregate over a prepared program; the records go to d_out (device memory), or, with d_out == nullptr, to the context's staging buffer
// (agg_collect fetches them). The arguments have been checked and the context entered. A value-ordered view of the base field's index is neither read nor
// touched (where_run). EXPR: the measure is X's expression (bmx_expr.inc has made X and enqueues k_expr_finish behind this); measure_field is not read then, and
// n is counted per row: no class of node makes n == n_match, not even base * base.
template <bool EXPR = false>
int where_agg_enqueue(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint32_t measure_field, uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* d_out,
                      const ExprArgs<EXPR>& X = ExprArgs<EXPR>()) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  const uint32_t nrec = agg_records(ngroups);
  if (int rc = agg_scratch(ctx, nrec)) return rc;
  AggArgs A{};
  A.slots = ctx->slots; A.nslots = ctx->nslots; A.acc = ctx->agg.raw;
  A.group_lo = group_lo; A.ngroups = ngroups; A.measure = measure_field; A.group = group_field;
  A.m_src = EXPR ? AGG_SRC_PROBE : where_agg_source(measure_field, base_field); A.g_src = ngroups ? where_agg_source(group_field, base_field) : AGG_SRC_NONE;
  A.nterms = 0;
  ctx->agg.clean = false;
  where_sweep_c(ctx, ix, W, [&](const auto& P, uint32_t blocks) { where_agg_launch(ctx, ix, P, blocks, A, X); });
  LAUNCHCHK("k_where_agg");
  hipLaunchKernelGGL(k_agg_finish, dim3(std::min<uint32_t>((nrec + 255) / 256, 64)), dim3(256), 0, ctx->stream, ctx->agg.raw, d_out ? d_out : ctx->agg.stage, nrec,
                     A.m_src != AGG_SRC_PROBE ? 1u : 0u);
  LAUNCHCHK("k_agg_finish");
  ctx->agg.clean = true;
  return BMX_OK;
}

template <class T, bool PAIRS>
int where_top_launch(bmx_ctx* ctx, const Index* ix, const PredWhere<T, PAIRS>& P, const TopArgs& A, uint32_t k) {
  return top_launch_with<T, true>(ctx, ix, A, k, [&](const T*, uint32_t blocks, uint32_t) {
    hipLaunchKernelGGL((k_where_top0<T, PAIRS>), dim3(blocks), dim3(TOP_THREADS), 0, ctx->stream, ix->n, P, A);
  });
}

// Enqueue one top-k query over a prepared program; outputs as top_enqueue's
int where_top_enqueue(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint32_t flags, const bmx_top_rec* after, uint32_t k, bmx_top_rec* d_out, uint64_t* d_n_out,
                      uint64_t* d_n_eligible) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  if (int rc = top_scratch(ctx)) return rc;
  if (int rc = ctx->scan.ensure(ctx, std::max<uint64_t>(ix->n, 1), 0)) return rc;     // the scans' mask: one bit per index position
  TopArgs A{};     // (no terms: pass 0 decides with the program, the passes behind it read the mask)
  A.ids = ix->ids; A.mask = ctx->scan.mask; A.slots = ctx->slots; A.nslots = ctx->nslots; A.S = ctx->top.state;
  A.desc = flags & BMX_TOP_DESC;
  top_set_cursor(A, after);
  ctx->top.clean = false;
  if (int rc = where_sweep(ctx, ix, W, [&](const auto& P, uint32_t) { return where_plain_or_pairs(P, [&](const auto& Q) { return where_top_launch(ctx, ix, Q, A, k); }); })) return rc;     // (the grid is top_launch_with's own)
  return top_launch_finish(ctx, A, k, d_out, d_n_out, d_n_eligible);
}

}  // namespace

extern "C" {

int bmx_where_aggregate(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t measure_field,
                        uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* out, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = where_agg_bad_args(group_field, ngroups, out)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (int rc = where_agg_enqueue(ctx, base_field, W, measure_field, group_field, group_lo, ngroups, mem == BMX_MEM_DEVICE ? out : nullptr)) return rc;
  return mem == BMX_MEM_HOST ? agg_collect(ctx, agg_records(ngroups), out) : BMX_OK;
}

int bmx_where_top(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t flags, const bmx_top_rec* after,
                  uint32_t k, bmx_top_rec* out, uint64_t* n_out, uint64_t* n_eligible, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = where_top_bad_args(flags, k, out)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (mem == BMX_MEM_DEVICE) return where_top_enqueue(ctx, base_field, W, flags, after, k, out, n_out, n_eligible);
  if (int rc = where_top_enqueue(ctx, base_field, W, flags, after, k, nullptr, nullptr, nullptr)) return rc;
  return top_collect_to(ctx, k, out, n_out, n_eligible);
}

int bmx_comm_where_aggregate(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t measure_field,
                             uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* out) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = where_agg_bad_args(group_field, ngroups, out)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  return comm_agg_with(c, ngroups, out, [&](bmx_ctx* x) { return where_agg_enqueue(x, base_field, W, measure_field, group_field, group_lo, ngroups, nullptr); });
}

int bmx_comm_where_top(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t flags, const bmx_top_rec* after,
                       uint32_t k, bmx_top_rec* out, uint64_t* n_out, uint64_t* n_eligible) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = where_top_bad_args(flags, k, out)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  return comm_top_with(c, flags, k, out, n_out, n_eligible, [&](bmx_ctx* x) { return where_top_enqueue(x, base_field, W, flags, after, k, nullptr, nullptr, nullptr); });
}

}  // extern "C"
