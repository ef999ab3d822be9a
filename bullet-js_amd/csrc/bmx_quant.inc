// bmx_quant.inc — exact quantiles over boolean filters (bmx_quant.h): bmx_where_quantiles and its sharded form. The program is bmx_where.inc's (where_prepare),
// and so are the width dispatch of pass 0 and the entry guards (where_sweep, where_enter, where_comm_guard), the kernels quant_kernels.h. The context keeps the scratch (QuantScratch):
// the state record, which every query's last kernel leaves empty again (clean), the value scratch of a probed measure, and the staging of a host-mode answer.
// One context enqueues the worst-case chain blind; the communicator steps the same sweeps and finds the bins on the host with the kernels' own helpers.
// Included by bmx.hip (one translation unit), behind everything that was here before it.
namespace {

const char* quant_bad_args(uint32_t nq, const bmx_quant_q* qs, const bmx_quant_rec* out) {
  if (nq == 0 || nq > BMX_QUANT_MAX) return "bmx_where_quantiles: nq outside 1..BMX_QUANT_MAX";
  if (!qs) return "bmx_where_quantiles: null qs";
  if (!out) return "bmx_where_quantiles: null output";
  for (uint32_t i = 0; i < nq; i++)
    if (qs[i].den == 0 || qs[i].den > BMX_QUANT_MAX_DEN || qs[i].num > qs[i].den) return "bmx_where_quantiles: a quantile outside 0 <= num <= den, 1 <= den <= BMX_QUANT_MAX_DEN";
  return nullptr;
}

constexpr size_t QUANT_STAGE_BYTES = QUANT_MAX * sizeof(bmx_quant_rec) + sizeof(bmx_quant_res);
constexpr uint32_t QUANT_HIST_BYTES = TOP_BINS * sizeof(uint32_t);              // one live prefix's histogram in LDS

// the state record, the staging and, for a probed measure, a value scratch of `rows` positions (0: none needed). Every allocation comes before the first
// launch: a call that cannot have its memory has done nothing.
int quant_scratch(bmx_ctx* ctx, uint64_t rows) {
  QuantScratch& s = ctx->quant;
  if (!s.state) {
    if (int rc = dev_alloc_all(ctx, {{s.state, sizeof(QuantState)}, {s.stage, QUANT_STAGE_BYTES}})) return rc;
    s.clean = false;
  }
  if (rows > s.vals_cap) {     // grown with the index, a quarter ahead of it
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.vals_cap = 0;
    const uint64_t cap = rows + rows / 4 + 1024;
    if (int rc = dev_alloc(ctx, &s.vals, cap)) return rc;
    s.vals_cap = cap;
  }
  if (!s.clean) {     // a new state record, or a query that did not get as far as its last kernel
    hipLaunchKernelGGL(k_quant_clear, dim3(64), dim3(256), 0, ctx->stream, s.state);
    LAUNCHCHK("k_quant_clear");
  }
  return BMX_OK;
}

// what the digit sweeps of one call read, fixed by its pass 0
struct QuantSrc { bool fits32 = false /* the 4-byte base column; otherwise 8-byte values: the int64 column or the value scratch */; const void* col = nullptr; uint64_t n = 0; uint32_t nt = 0, blocks = 1; };

template <class T, bool PAIRS, bool EXPR>
void quant_launch0(bmx_ctx* ctx, const Index* ix, const PredWhere<T, PAIRS>& P, uint32_t blocks, const QuantArgs& A, bool probe, const ExprArgs<EXPR>& X) {
  if (EXPR || probe) hipLaunchKernelGGL((k_quant0<T, true, PAIRS, EXPR>), dim3(blocks), dim3(TOP_THREADS), 0, ctx->stream, ix->n, P, A, X);
  else if constexpr (!EXPR) hipLaunchKernelGGL((k_quant0<T, false, PAIRS>), dim3(blocks), dim3(TOP_THREADS), 0, ctx->stream, ix->n, P, A, X);
}

// Pass 0 of one call over a prepared program, enqueued; *src: where its digit sweeps find the values. The context has been entered. A value-ordered view of the
// base field's index is neither read nor touched (where_run). EXPR: the sample value is X's expression (bmx_expr.inc has made X and enqueues k_expr_finish
// behind the query); measure_field is not read then, and the value goes through the scratch whatever the operands are.
template <bool EXPR = false>
int quant_enqueue0(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint32_t measure_field, QuantSrc* src, const ExprArgs<EXPR>& X = ExprArgs<EXPR>()) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  const bool probe = EXPR || measure_field != base_field;
  if (int rc = ctx->scan.ensure(ctx, std::max<uint64_t>(ix->n, 1), 0)) return rc;     // the scans' mask: one bit per index position
  if (int rc = quant_scratch(ctx, probe ? std::max<uint64_t>(ix->n, 1) : 0)) return rc;
  QuantArgs A{};
  A.mask = ctx->scan.mask; A.vals = ctx->quant.vals; A.S = ctx->quant.state; A.measure = measure_field;
  ctx->quant.clean = false;
  where_sweep(ctx, ix, W, [&](const auto& P, uint32_t blocks) { where_plain_or_pairs(P, [&](const auto& Q) { quant_launch0(ctx, ix, Q, blocks, A, probe, X); }); });
  LAUNCHCHK("k_quant0");
  src->fits32 = !probe && ix->fits32; src->n = ix->n;
  src->col = probe ? static_cast<const void*>(ctx->quant.vals) : (ix->fits32 ? static_cast<const void*>(ix->v32) : static_cast<const void*>(ix->v64));
  const uint64_t width = src->fits32 ? 4 : 8;
  src->nt = ix->n * width > SCAN_NT_BYTES ? 1u : 0u;
  src->blocks = sweep_grid(ctx, ix->n, 4ull * TOP_THREADS * TOP_U * (16 / width));    // (where_agg_grid's rule, for the width the sweep reads)
  return BMX_OK;
}

// one digit sweep with room for `np` histograms
int quant_digit(bmx_ctx* ctx, const QuantSrc& s, uint32_t np) {
  const uint32_t lds = np * QUANT_HIST_BYTES;
  if (s.fits32) hipLaunchKernelGGL((k_quant_digit<int32_t>), dim3(s.blocks), dim3(TOP_THREADS), lds, ctx->stream, static_cast<const int32_t*>(s.col), s.n, s.nt, (const uint32_t*)ctx->scan.mask, ctx->quant.state);
  else hipLaunchKernelGGL((k_quant_digit<int64_t>), dim3(s.blocks), dim3(TOP_THREADS), lds, ctx->stream, static_cast<const int64_t*>(s.col), s.n, s.nt, (const uint32_t*)ctx->scan.mask, ctx->quant.state);
  LAUNCHCHK("k_quant_digit");
  return BMX_OK;
}

int quant_finish(bmx_ctx* ctx, uint32_t nq, bmx_quant_rec* d_out, bmx_quant_res* d_res) {
  hipLaunchKernelGGL(k_quant_finish, dim3(1), dim3(64), 0, ctx->stream, ctx->quant.state, nq, d_out, d_res);
  LAUNCHCHK("k_quant_finish");
  ctx->quant.clean = true;
  return BMX_OK;
}

// Enqueue one whole query: the records go to d_out and the result to d_res (device memory; d_res may be null), or, with d_out == nullptr, both to the staging.
template <bool EXPR = false>
int quant_enqueue(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint32_t measure_field, uint32_t nq, const QuantQs& qs, bmx_quant_rec* d_out, bmx_quant_res* d_res,
                  const ExprArgs<EXPR>& X = ExprArgs<EXPR>()) {
  QuantSrc s;
  if (int rc = quant_enqueue0(ctx, base_field, W, measure_field, &s, X)) return rc;
  hipLaunchKernelGGL(k_quant_init, dim3(1), dim3(64), 0, ctx->stream, ctx->quant.state, nq, qs);
  LAUNCHCHK("k_quant_init");
  // the worst case of digits: 32 bits of (key - min) in the 4-byte column, the 54-bit value domain (a difference below 2^54) otherwise. The first digit has one
  // prefix; behind it the ranks may have parted, and nobody looks: room for nq
  const uint32_t passes = ((s.fits32 ? 32u : 54u) + TOP_DIGIT_BITS - 1) / TOP_DIGIT_BITS;
  static_assert((32u + TOP_DIGIT_BITS - 1) / TOP_DIGIT_BITS == 3u && (54u + TOP_DIGIT_BITS - 1) / TOP_DIGIT_BITS == 5u, "3 and 5 digit passes");
  for (uint32_t p = 0; p < passes; p++) {
    if (int rc = quant_digit(ctx, s, p == 0 ? 1u : nq)) return rc;
    hipLaunchKernelGGL(k_quant_find, dim3(1), dim3(SEL_THREADS), 0, ctx->stream, ctx->quant.state);
  }
  LAUNCHCHK("k_quant_find");
  if (!d_out) { d_out = reinterpret_cast<bmx_quant_rec*>(ctx->quant.stage); d_res = reinterpret_cast<bmx_quant_res*>(ctx->quant.stage + QUANT_MAX * sizeof(bmx_quant_rec)); }
  return quant_finish(ctx, nq, d_out, d_res);
}

QuantQs quant_copy_qs(uint32_t nq, const bmx_quant_q* qs) {
  QuantQs q{};
  for (uint32_t i = 0; i < nq; i++) q.q[i] = qs[i];
  return q;
}

// second half of a host-mode query: wait for it and copy its records and its result down
int quant_collect(bmx_ctx* ctx, uint32_t nq, bmx_quant_rec* out, bmx_quant_res* res) {
  uint8_t h[QUANT_STAGE_BYTES];
  HIPCHK(hipMemcpyAsync(h, ctx->quant.stage, QUANT_STAGE_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::memcpy(out, h, nq * sizeof(bmx_quant_rec));
  if (res) std::memcpy(res, h + QUANT_MAX * sizeof(bmx_quant_rec), sizeof(bmx_quant_res));
  return BMX_OK;
}

// The quantiles of the shards do not combine: the communicator runs the select itself. Pass 0 on every shard (enqueue0(shard, &its QuantSrc); the shard has been
// entered), the counts and the extremes folded here, then per digit the select record (live prefixes, the common minimum) up to every shard, every shard's
// sweep, the histograms down and added, the bins found here by quant_search / quant_step / quant_relist — what k_quant_find runs. At most 5 rounds of at most
// nq x 16 KB per shard. The arguments have been checked.
template <class Enqueue0>
int comm_quant_with(bmx_comm* c, uint32_t nq, const bmx_quant_q* qs, bmx_quant_rec* out, bmx_quant_res* res, Enqueue0 enqueue0) {
  DevGuard guard;
  std::vector<QuantSrc> src(c->N);
  unsigned long long n_match = 0, n = 0, kmin = ~0ull, kmax = 0;
  int rc = comm_two_phase(c,
    [&](uint32_t g, bmx_ctx* x) { const int erc = enter(x); return erc ? erc : enqueue0(x, &src[g]); },
    [&](uint32_t, bmx_ctx* ctx) {
      if (int erc = enter(ctx)) return erc;
      unsigned long long h[4];
      HIPCHK(hipMemcpyAsync(h, ctx->quant.state, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      n_match += h[0]; n += h[1]; kmin = std::min(kmin, h[2]); kmax = std::max(kmax, h[3]);
      return (int)BMX_OK;
    });
  if (rc) return rc;
  QuantSel Q;
  quant_sel_init(Q, n, kmin, kmax, nq, qs);
  std::vector<unsigned long long> hist((size_t)nq * TOP_BINS), part((size_t)nq * TOP_BINS);
  while (Q.sh) {
    const uint32_t w = quant_width(Q.sh), np = Q.np;
    const size_t words = (size_t)np * TOP_BINS;
    std::fill(hist.begin(), hist.begin() + words, 0ull);
    rc = comm_two_phase(c,
      [&](uint32_t g, bmx_ctx* ctx) {
        if (int erc = enter(ctx)) return erc;
        HIPCHK(hipMemcpyAsync(&ctx->quant.state->Q, &Q, sizeof(Q), hipMemcpyHostToDevice, ctx->stream));     // (Q stands still until every shard's stream has been waited for)
        return quant_digit(ctx, src[g], np);
      },
      [&](uint32_t, bmx_ctx* ctx) {
        if (int erc = enter(ctx)) return erc;
        HIPCHK(hipMemcpyAsync(part.data(), &ctx->quant.state->hist[0][0], words * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemsetAsync(&ctx->quant.state->hist[0][0], 0, words * 8, ctx->stream));                    // what k_quant_find does behind its read
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (size_t b = 0; b < words; b++) hist[b] += part[b];
        return (int)BMX_OK;
      });
    if (rc) return rc;
    for (uint32_t i = 0; i < nq; i++) {
      uint32_t bin; unsigned long long cb, in_bin;
      if (!quant_search(&hist[(size_t)Q.slot[i] * TOP_BINS], TOP_BINS, 0ull, Q.rank[i] - Q.below[i], &bin, &cb, &in_bin))
        return fail(c, BMX_ERR_INTERNAL, "bmx_comm_where_quantiles: the shards' histograms do not hold a rank");
      quant_step(Q, i, bin, cb, in_bin, w);
    }
    quant_relist(Q, Q.sh - w);
  }
  for (uint32_t g = 0; g < c->N; g++) {       // every shard's state record back to empty
    bmx_ctx* ctx = c->sh[g];
    CSH(g, enter(ctx));
    CSH(g, quant_finish(ctx, 0, nullptr, nullptr));
  }
  for (uint32_t i = 0; i < nq; i++) out[i] = quant_record(Q, i);
  if (res) *res = quant_result(n_match, n, kmin, kmax);
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_where_quantiles(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t measure_field, uint32_t nq,
                        const bmx_quant_q* qs, bmx_quant_rec* out, bmx_quant_res* res, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = quant_bad_args(nq, qs, out)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  const QuantQs q = quant_copy_qs(nq, qs);      // read now: the caller may reuse qs as soon as the call returns
  if (mem == BMX_MEM_DEVICE) return quant_enqueue(ctx, base_field, W, measure_field, nq, q, out, res);
  if (int rc = quant_enqueue(ctx, base_field, W, measure_field, nq, q, nullptr, nullptr)) return rc;
  return quant_collect(ctx, nq, out, res);
}

// bmx_where_quantiles over the shards (host memory): comm_quant_with
int bmx_comm_where_quantiles(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t measure_field, uint32_t nq,
                             const bmx_quant_q* qs, bmx_quant_rec* out, bmx_quant_res* res) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = quant_bad_args(nq, qs, out)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  return comm_quant_with(c, nq, qs, out, res, [&](bmx_ctx* x, QuantSrc* src) { return quant_enqueue0(x, base_field, W, measure_field, src); });
}

}  // extern "C"
