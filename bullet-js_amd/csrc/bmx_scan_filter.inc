// bmx_scan_filter.inc — the scans that first use run_scan_t with positions and with PredFilter: bmx_scan_range_pos and the declarative filter with its clamping
// rules (the rest of the scans is bmx_scan.inc). Included by bmx.hip (one translation unit) behind its own entry points, where these two always sat (the include list).
extern "C" {

int bmx_scan_range_pos(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, uint32_t* out_pos, uint64_t cap, uint64_t* n_out, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  return scan_range_impl_t<true>(ctx, field, lo, hi, out_pos, cap, n_out, mem);
}

}  // extern "C"

namespace {

// bmx_scan_filter and the first half of bmx_comm_scan_filter
int scan_filter_impl(bmx_ctx* ctx, uint32_t nterms, const bmx_term* terms, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem, bool deferred = false) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (const char* bad = bad_terms(nterms, terms, "filter needs 1..8 terms")) return fail(ctx, BMX_ERR_INVALID, bad);
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  int rc = fresh_index(ctx, terms[0].field, &ix);
  if (rc) return rc;
  PredFilter P;
  P.v = ix->v64; P.ids = ix->ids; P.slots = ctx->slots; P.nslots = ctx->nslots; P.nterms = nterms;
  copy_terms(P.t, terms, nterms);
  // with a value-ordered view of the first term's index: its run is the candidate list, the other terms are probed for those ids only (no order)
  if ((n_out || out_ids) && ensure_ordered_view(ctx, ix)) {
    const int src = run_scan_t<false>(ctx, P, ix, out_ids, cap, n_out, mem, deferred, true, P.t[0].lo, P.t[0].hi);
    if (!src) view_after_query(ctx, ix);
    return src;
  }
  return run_scan_t<false>(ctx, P, ix, out_ids, cap, n_out, mem, deferred);
}

}  // namespace

extern "C" {

int bmx_scan_filter(bmx_ctx* ctx, uint32_t nterms, const bmx_term* terms, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem) {
  return scan_filter_impl(ctx, nterms, terms, out_ids, cap, n_out, mem);
}

}  // extern "C"
