// bmx_expr.inc — computed measures (bmx_expr.h): bmx_where_aggregate_expr, bmx_where_group_expr, bmx_where_quantiles_expr and their sharded forms. A measure
// that is value(a) op value(b) of the selected node changes one thing in each form, the sweep that fetches the measure (expr_kernels.h: k_where_agg,
// k_group_sweep and k_quant0 with EXPR = true); everything else is the plain form's and is called, not copied: the program and the entry guards (where_prepare,
// where_enter, where_comm_guard), the argument checks, the enqueue functions (where_agg_enqueue, group_enqueue, quant_enqueue / quant_enqueue0, which take the
// expression as their last argument), the collect halves (agg_collect, group_collect_to, quant_collect) and the sharded combines (comm_agg_with, comm_grouped,
// comm_quant_with). What this file adds is the expression's own checks, its kernel argument, and the two counters of bmx_expr_res: a state record of their own
// (ExprScratch) that the sweep adds to and k_expr_finish, enqueued behind the form's last kernel, writes out and leaves zero again (clean). Included by
// bmx.hip (one translation unit), behind everything that was here before it.
namespace {

const char* expr_bad_args(const bmx_expr* m) {
  if (!m) return "bmx_expr: null measure expression";
  if (m->op < BMX_EXPR_ADD || m->op > BMX_EXPR_MUL) return "bmx_expr: op outside BMX_EXPR_ADD..BMX_EXPR_MUL";
  if (m->reserved != 0) return "bmx_expr: reserved must be 0";
  if (m->a == BMX_AGG_NO_FIELD) return "bmx_expr: operand a is no field";
  if (m->b == BMX_AGG_NO_FIELD) return "bmx_expr: operand b is no field";
  return nullptr;
}

// The state record and the staging, zero before the sweep, and the kernel argument of one query on a context that has been entered. Every allocation comes
// before the first launch.
int expr_begin(bmx_ctx* ctx, uint32_t base_field, const bmx_expr& m, ExprArgs<true>* X) {
  ExprScratch& s = ctx->expr;
  if (!s.state) {
    if (int rc = dev_alloc_all(ctx, {{s.state, sizeof(ExprState)}, {s.stage, sizeof(bmx_expr_res)}})) return rc;
    s.clean = false;
  }
  if (!s.clean) HIPCHK(hipMemsetAsync(s.state, 0, sizeof(ExprState), ctx->stream));     // a new record, or a query that did not get as far as k_expr_finish
  s.clean = false;
  const uint32_t a_src = m.a == base_field ? 0u : AGG_SRC_PROBE;
  const uint32_t b_src = m.b == base_field ? 0u : (m.b == m.a ? EXPR_SRC_SAME : AGG_SRC_PROBE);      // (a == b: one probe)
  X->S = s.state; X->a = m.a; X->b = m.b; X->mode = a_src | b_src << 8 | m.op << 16;
  return BMX_OK;
}
// behind the form's last kernel: the counters to d_xres (device memory; nullptr: nowhere), the state record back to zero
int expr_finish(bmx_ctx* ctx, bmx_expr_res* d_xres) {
  hipLaunchKernelGGL(k_expr_finish, dim3(1), dim3(64), 0, ctx->stream, ctx->expr.state, d_xres);
  LAUNCHCHK("k_expr_finish");
  ctx->expr.clean = true;
  return BMX_OK;
}
// second half of a host-mode query, behind the form's own: the staged counters down
int expr_collect(bmx_ctx* ctx, bmx_expr_res* xres) {
  if (!xres) return BMX_OK;
  HIPCHK(hipMemcpyAsync(xres, ctx->expr.stage, sizeof(bmx_expr_res), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return BMX_OK;
}
// ... of a sharded query: every shard's staged counters, added up
int expr_comm_collect(bmx_comm* c, bmx_expr_res* xres) {
  if (!xres) return BMX_OK;
  DevGuard guard;
  bmx_expr_res tot{0, 0};
  for (uint32_t g = 0; g < c->N; g++) {
    bmx_ctx* x = c->sh[g];
    bmx_expr_res r{0, 0};
    CSH(g, enter(x));
    CSH(g, expr_collect(x, &r));
    tot.n_undef += r.n_undef; tot.n_range += r.n_range;
  }
  *xres = tot;
  return BMX_OK;
}

// one shard's (or the one context's) whole aggregate / group-by with the expression, into the staging buffers
int expr_agg_staged(bmx_ctx* x, uint32_t base_field, const WhereProg& W, const bmx_expr& m, uint32_t group_field, int64_t group_lo, uint32_t ngroups) {
  ExprArgs<true> X;
  if (int rc = expr_begin(x, base_field, m, &X)) return rc;
  if (int rc = where_agg_enqueue<true>(x, base_field, W, BMX_AGG_NO_FIELD, group_field, group_lo, ngroups, nullptr, X)) return rc;
  return expr_finish(x, x->expr.stage);
}
int expr_group_staged(bmx_ctx* x, uint32_t base_field, const WhereProg& W, const bmx_expr& m, uint32_t group_field, uint64_t cap) {
  ExprArgs<true> X;
  if (int rc = expr_begin(x, base_field, m, &X)) return rc;
  if (int rc = group_enqueue<true>(x, base_field, W, BMX_AGG_NO_FIELD, group_field, cap, nullptr, nullptr, X)) return rc;
  return expr_finish(x, x->expr.stage);
}

}  // namespace

extern "C" {

int bmx_where_aggregate_expr(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                             uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* out, bmx_expr_res* xres, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = expr_bad_args(m)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = where_agg_bad_args(group_field, ngroups, out)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (mem == BMX_MEM_HOST) {
    if (int rc = expr_agg_staged(ctx, base_field, W, *m, group_field, group_lo, ngroups)) return rc;
    if (int rc = agg_collect(ctx, agg_records(ngroups), out)) return rc;
    return expr_collect(ctx, xres);
  }
  ExprArgs<true> X;
  if (int rc = expr_begin(ctx, base_field, *m, &X)) return rc;
  if (int rc = where_agg_enqueue<true>(ctx, base_field, W, BMX_AGG_NO_FIELD, group_field, group_lo, ngroups, out, X)) return rc;
  return expr_finish(ctx, xres);
}

int bmx_where_group_expr(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                         uint32_t group_field, bmx_group_rec* out, uint64_t cap, bmx_group_res* res, bmx_expr_res* xres, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = expr_bad_args(m)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = group_bad_args(group_field, out, cap, res)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (mem == BMX_MEM_HOST) {
    if (int rc = expr_group_staged(ctx, base_field, W, *m, group_field, cap)) return rc;
    if (int rc = group_collect_to(ctx, cap, out, res)) return rc;
    return expr_collect(ctx, xres);
  }
  ExprArgs<true> X;
  if (int rc = expr_begin(ctx, base_field, *m, &X)) return rc;
  if (int rc = group_enqueue<true>(ctx, base_field, W, BMX_AGG_NO_FIELD, group_field, cap, out, res, X)) return rc;
  return expr_finish(ctx, xres);
}

int bmx_where_quantiles_expr(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                             uint32_t nq, const bmx_quant_q* qs, bmx_quant_rec* out, bmx_quant_res* res, bmx_expr_res* xres, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = expr_bad_args(m)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = quant_bad_args(nq, qs, out)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  const QuantQs q = quant_copy_qs(nq, qs);      // read now: the caller may reuse qs as soon as the call returns
  const bool dev = mem == BMX_MEM_DEVICE;
  ExprArgs<true> X;
  if (int rc = expr_begin(ctx, base_field, *m, &X)) return rc;
  if (int rc = quant_enqueue<true>(ctx, base_field, W, BMX_AGG_NO_FIELD, nq, q, dev ? out : nullptr, dev ? res : nullptr, X)) return rc;
  if (int rc = expr_finish(ctx, dev ? xres : ctx->expr.stage)) return rc;
  if (dev) return BMX_OK;
  if (int rc = quant_collect(ctx, nq, out, res)) return rc;
  return expr_collect(ctx, xres);
}

int bmx_comm_where_aggregate_expr(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                                  uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* out, bmx_expr_res* xres) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = expr_bad_args(m)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = where_agg_bad_args(group_field, ngroups, out)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  if (int rc = comm_agg_with(c, ngroups, out, [&](bmx_ctx* x) { return expr_agg_staged(x, base_field, W, *m, group_field, group_lo, ngroups); })) return rc;
  return expr_comm_collect(c, xres);
}

int bmx_comm_where_group_expr(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                              uint32_t group_field, bmx_group_rec* out, uint64_t cap, bmx_group_res* res, bmx_expr_res* xres) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = expr_bad_args(m)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = group_bad_args(group_field, out, cap, res)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  bmx_group_res tot;
  {
    DevGuard guard;
    if (int rc = comm_grouped(c, cap, BMX_GROUP_OVERFLOW, group_key_less, out, &tot,
          [&](bmx_ctx* x) { return expr_group_staged(x, base_field, W, *m, group_field, cap); },
          [&](bmx_ctx* x, std::vector<bmx_group_rec>& part, bmx_group_res* r) { return group_collect(x, cap, part, r); }, group_fold_res)) return rc;
  }
  *res = tot;
  return expr_comm_collect(c, xres);
}

int bmx_comm_where_quantiles_expr(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                                  uint32_t nq, const bmx_quant_q* qs, bmx_quant_rec* out, bmx_quant_res* res, bmx_expr_res* xres) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = expr_bad_args(m)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = quant_bad_args(nq, qs, out)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  // pass 0 is the only sweep that classifies: its counters are final when the select's first fold has waited for it; they come out behind the select
  if (int rc = comm_quant_with(c, nq, qs, out, res, [&](bmx_ctx* x, QuantSrc* src) {
        ExprArgs<true> X;
        if (int brc = expr_begin(x, base_field, *m, &X)) return brc;
        return quant_enqueue0<true>(x, base_field, W, BMX_AGG_NO_FIELD, src, X);
      })) return rc;
  {
    DevGuard guard;
    for (uint32_t g = 0; g < c->N; g++) {
      bmx_ctx* x = c->sh[g];
      CSH(g, enter(x));
      CSH(g, expr_finish(x, x->expr.stage));
    }
  }
  return expr_comm_collect(c, xres);
}

}  // extern "C"
