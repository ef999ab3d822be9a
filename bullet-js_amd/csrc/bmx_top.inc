// bmx_top.inc — ordered, limited queries (bmx_top.h): bmx_scan_top over one context. The kernels are top_kernels.h; included by bmx.hip (one translation unit),
// which keeps their scratch (TopScratch): the select's state record, left ready by every query's last kernel, the candidate list, and the two counts and the
// records of a host-mode answer on their way down. bmx_comm_scan_top (bmx_comm.inc) enqueues and collects through the same two halves.
namespace {

// what every caller's arguments must satisfy before anything touches a device (bmx_comm_scan_top asks the same)
const char* top_bad_args(uint32_t nterms, const bmx_term* terms, uint32_t flags, uint32_t k, const bmx_top_rec* out) {
  if (const char* bad = bad_terms(nterms, terms, "bmx_scan_top needs 1..8 terms")) return bad;
  if (!out) return "bmx_scan_top: null output";
  if (k == 0 || k > BMX_TOP_MAX_K) return "bmx_scan_top: k outside 1..BMX_TOP_MAX_K";
  if (flags & ~BMX_TOP_DESC) return "bmx_scan_top: unknown flag bits";
  return nullptr;
}

int top_scratch(bmx_ctx* ctx) {
  TopScratch& s = ctx->top;
  if (!s.state) {
    if (int rc = dev_alloc_all(ctx, {{s.state, sizeof(TopState)}, {s.cand_u, TOP_CAND * sizeof(unsigned long long)}, {s.cand_id, TOP_CAND * sizeof(unsigned long long)},
                                     {s.stage, 2 * sizeof(unsigned long long) + BMX_TOP_MAX_K * sizeof(bmx_top_rec)}})) return rc;
    s.clean = false;
  }
  if (!s.clean) {     // a new state record, or a query that did not get as far as its last kernel
    hipLaunchKernelGGL(k_top_clear, dim3(1), dim3(256), 0, ctx->stream, s.state);
    LAUNCHCHK("k_top_clear");
  }
  return BMX_OK;
}

// the whole chain of one query on the column of width T: pass 0, the state, the worst case of digit passes (those behind "done" return at once), the compaction.
// pass0(col, blocks, nt) launches the query's own pass 0: k_top_sweep0 for an AND of terms (top_launch), k_where_top0 for a program (bmx_where_agg.inc).
template <class T, bool PROBE, class Pass0>
int top_launch_with(bmx_ctx* ctx, const Index* ix, const TopArgs& A, uint32_t k, Pass0&& pass0) {
  const T* col = sizeof(T) == 4 ? reinterpret_cast<const T*>(ix->v32) : reinterpret_cast<const T*>(ix->v64);
  const uint32_t nt = ix->n * sizeof(T) > SCAN_NT_BYTES ? 1u : 0u;
  // no workgroup with fewer than four rounds of loads to spread its one flush over
  const uint32_t blocks = sweep_grid(ctx, ix->n, 4ull * TOP_THREADS * TOP_U * (16 / sizeof(T)));
  pass0(col, blocks, nt);
  LAUNCHCHK("k_top_sweep0 / k_where_top0");
  hipLaunchKernelGGL(k_top_init, dim3(1), dim3(64), 0, ctx->stream, A.S, k);
  // digits of the value (key - min: at most 32 bits in the 4-byte column, 64 in the 8-byte one), then of the id
  const uint32_t passes = (uint32_t)((sizeof(T) * 8 + TOP_DIGIT_BITS - 1) / TOP_DIGIT_BITS + (64 + TOP_DIGIT_BITS - 1) / TOP_DIGIT_BITS);
  for (uint32_t p = 0; p < passes; p++) {
    hipLaunchKernelGGL((k_top_digit<T, PROBE>), dim3(blocks), dim3(TOP_THREADS), 0, ctx->stream, col, ix->n, nt, A);
    hipLaunchKernelGGL(k_top_find, dim3(1), dim3(SEL_THREADS), 0, ctx->stream, A.S);
  }
  LAUNCHCHK("k_top_digit / k_top_find");
  hipLaunchKernelGGL((k_top_compact<T, PROBE>), dim3(blocks), dim3(TOP_THREADS), 0, ctx->stream, col, ix->n, nt, A, ctx->top.cand_u, ctx->top.cand_id);
  LAUNCHCHK("k_top_compact");
  return BMX_OK;
}
template <class T, bool PROBE>
int top_launch(bmx_ctx* ctx, const Index* ix, const TopArgs& A, uint32_t k) {
  return top_launch_with<T, PROBE>(ctx, ix, A, k, [&](const T* col, uint32_t blocks, uint32_t nt) {
    hipLaunchKernelGGL((k_top_sweep0<T, PROBE>), dim3(blocks), dim3(TOP_THREADS), 0, ctx->stream, col, ix->n, nt, A);
  });
}

// the cursor as the kernels take it
inline void top_set_cursor(TopArgs& A, const bmx_top_rec* after) {
  if (!after) return;
  const unsigned long long u = (unsigned long long)after->val ^ 0x8000000000000000ull;
  A.has_after = 1u; A.au = A.desc ? ~u : u; A.aid = after->id;
}
// the last kernel of a query: records and counts to the caller's device memory, or, with d_out == nullptr, to the staging buffer
int top_launch_finish(bmx_ctx* ctx, const TopArgs& A, uint32_t k, bmx_top_rec* d_out, uint64_t* d_n_out, uint64_t* d_n_eligible) {
  unsigned long long* st = reinterpret_cast<unsigned long long*>(ctx->top.stage);
  hipLaunchKernelGGL(k_top_finish, dim3(1), dim3(TOP_SORT_THREADS), 0, ctx->stream, ctx->top.state, (const unsigned long long*)ctx->top.cand_u, (const unsigned long long*)ctx->top.cand_id,
                     d_out ? d_out : reinterpret_cast<bmx_top_rec*>(st + 2), d_out ? reinterpret_cast<unsigned long long*>(d_n_out) : st,
                     d_out ? reinterpret_cast<unsigned long long*>(d_n_eligible) : st + 1, k, A.desc);
  LAUNCHCHK("k_top_finish");
  ctx->top.clean = true;
  return BMX_OK;
}

// Enqueue one query; records and counts go to the caller's device memory (d_out; d_n_out and d_n_eligible may be null), or, with d_out == nullptr, to the
// context's staging buffer (top_collect fetches them). The arguments have been checked (top_bad_args) and the context entered. The value-ordered view of the
// index, if there is one, is neither read nor touched: fresh_index keeps the dense columns current whether or not a view exists.
int top_enqueue(bmx_ctx* ctx, uint32_t nterms, const bmx_term* terms, uint32_t flags, const bmx_top_rec* after, uint32_t k, bmx_top_rec* d_out,
                uint64_t* d_n_out, uint64_t* d_n_eligible) {
  Index* ix;
  if (int rc = fresh_index(ctx, terms[0].field, &ix)) return rc;
  if (int rc = top_scratch(ctx)) return rc;
  const bool probe = nterms > 1;
  if (probe) if (int rc = ctx->scan.ensure(ctx, std::max<uint64_t>(ix->n, 1), 0)) return rc;     // the scans' mask: one bit per index position
  TopArgs A{};
  A.ids = ix->ids; A.mask = ctx->scan.mask; A.slots = ctx->slots; A.nslots = ctx->nslots; A.S = ctx->top.state;
  A.desc = flags & BMX_TOP_DESC; A.nterms = nterms;
  copy_terms(A.t, terms, nterms);
  A.lo = A.t[0].lo; A.hi = A.t[0].hi;
  if (ix->fits32) { const Range32 r = clamp_i32(A.lo, A.hi); A.lo = r.lo; A.hi = r.hi; }    // the 4-byte column
  top_set_cursor(A, after);
  ctx->top.clean = false;
  int rc;
  if (ix->fits32) rc = probe ? top_launch<int32_t, true>(ctx, ix, A, k) : top_launch<int32_t, false>(ctx, ix, A, k);
  else rc = probe ? top_launch<int64_t, true>(ctx, ix, A, k) : top_launch<int64_t, false>(ctx, ix, A, k);
  if (rc) return rc;
  return top_launch_finish(ctx, A, k, d_out, d_n_out, d_n_eligible);
}

// second half of a host-mode query: wait for it, copy the counts and the records down; recs gets the min(k, n_eligible) records
int top_collect(bmx_ctx* ctx, uint32_t k, std::vector<bmx_top_rec>& recs, uint64_t* n_eligible) {
  std::vector<unsigned long long> h(2 + 2 * (size_t)k);
  HIPCHK(hipMemcpyAsync(h.data(), ctx->top.stage, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t m = std::min<uint64_t>(h[0], k);
  recs.resize(m);
  if (m) std::memcpy(recs.data(), h.data() + 2, m * sizeof(bmx_top_rec));
  *n_eligible = h[1];
  return BMX_OK;
}
// ... into the caller's host memory
int top_collect_to(bmx_ctx* ctx, uint32_t k, bmx_top_rec* out, uint64_t* n_out, uint64_t* n_eligible) {
  std::vector<bmx_top_rec> recs; uint64_t ne = 0;
  if (int rc = top_collect(ctx, k, recs, &ne)) return rc;
  if (!recs.empty()) std::memcpy(out, recs.data(), recs.size() * sizeof(bmx_top_rec));
  if (n_out) *n_out = recs.size();
  if (n_eligible) *n_eligible = ne;
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_scan_top(bmx_ctx* ctx, uint32_t nterms, const bmx_term* terms, uint32_t flags, const bmx_top_rec* after, uint32_t k, bmx_top_rec* out, uint64_t* n_out,
                 uint64_t* n_eligible, int mem) {
  if (const char* bad = top_bad_args(nterms, terms, flags, k, out)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  if (mem == BMX_MEM_DEVICE) return top_enqueue(ctx, nterms, terms, flags, after, k, out, n_out, n_eligible);
  if (int rc = top_enqueue(ctx, nterms, terms, flags, after, k, nullptr, nullptr, nullptr)) return rc;
  return top_collect_to(ctx, k, out, n_out, n_eligible);
}

}  // extern "C"
