// bmx_where.inc — boolean filters (bmx_where.h): bmx_scan_where over one context. The predicate is where_kernels.h PredWhere; run_scan_t (bmx_scan.inc) delivers
// the answer as it delivers every scan's. Included by bmx.hip (one translation unit). bmx_comm_scan_where (bmx_comm.inc) prepares the program once and enqueues it on every shard through where_run's
// deferred form and fetches with scan_collect, like bmx_comm_scan_filter.
namespace {

// The caller's program as the kernel takes it: the field table (fields other than the base field, in order of first use), per literal its slot, per clause its
// literal range (inside a clause the literals on the base field first), per field the set of its literals, the bounds clamped to the value domain (a lower bound of -VAL_MAX keeps tombstones out of every range; an
// upper bound of VAL_MAX changes no answer). Host arithmetic only. nullptr: the program is fine; otherwise why it is refused (nothing is written then).
const char* where_prepare(uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, WhereProg* out) {
  if (nclauses == 0 || nclauses > WHERE_MAX_CLAUSES) return "bmx_scan_where needs 1..8 clauses";
  if (!clause_len || !lits) return "bmx_scan_where: null clause_len or lits";
  uint32_t total = 0;
  for (uint32_t c = 0; c < nclauses; c++) {
    if (clause_len[c] == 0 || clause_len[c] > 8u) return "bmx_scan_where: a clause needs 1..8 literals";
    total += clause_len[c];
  }
  if (total > WHERE_MAX_LITS) return "bmx_scan_where: more than 32 literals";
  WhereProg W{};
  W.nclauses = nclauses;
  uint32_t l = 0, first = 0;                  // l: the kernel's literal number; first: the clause's first literal in the caller's list
  for (uint32_t c = 0; c < nclauses; first += clause_len[c], c++) {
    W.cbeg[c] = l;
    // an AND does not care for its order: the literals on the base field go in front, so a lane whose column value fails one leaves the clause before any probe
    for (int probed = 0; probed < 2; probed++) {
      for (uint32_t k = 0; k < clause_len[c]; k++) {
        const bmx_lit& in = lits[first + k];
        if (in.flags & ~BMX_LIT_NOT) return "bmx_scan_where: unknown flag bits";
        if ((in.field != base_field) != (probed != 0)) continue;
        WhereLit& o = W.lit[l];
        o.neg = in.flags & BMX_LIT_NOT;
        o.lo = above_tombstones(in.lo);
        o.hi = std::min<int64_t>(in.hi, VAL_MAX);
        if (!probed) { o.slot = 0; W.base_lits |= 1u << l; l++; continue; }
        uint32_t s = 0;
        while (s < W.nfields && W.field[s] != in.field) s++;
        if (s == W.nfields) {
          if (s == WHERE_MAX_FIELDS) return "bmx_scan_where: more than 8 fields besides the base field";
          W.field[W.nfields++] = in.field;
        }
        o.slot = s + 1u;
        W.flits[s] |= 1u << l;
        l++;
      }
    }
  }
  for (uint32_t c = nclauses; c <= WHERE_MAX_CLAUSES; c++) W.cbeg[c] = l;
  *out = W;
  return nullptr;
}

template <class T>
int where_scan(bmx_ctx* ctx, const Index* ix, const WhereProg& W, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem, bool deferred) {
  PredWhere<T> P;
  P.v = sizeof(T) == 4 ? reinterpret_cast<const T*>(ix->v32) : reinterpret_cast<const T*>(ix->v64);
  P.ids = ix->ids; P.slots = ctx->slots; P.nslots = ctx->nslots; P.nt = ix->n * sizeof(T) > SCAN_NT_BYTES; P.W = W;
  return run_scan_t<false>(ctx, P, ix, out_ids, cap, n_out, mem, deferred);
}

// One prepared program over one context: bmx_scan_where, and the first half of bmx_comm_scan_where on every shard (deferred). A value-ordered view of the base
// field's index is neither read nor touched: fresh_index keeps the dense columns current whether or not a view exists.
int where_run(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem, bool deferred) {
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  return ix->fits32 ? where_scan<int32_t>(ctx, ix, W, out_ids, cap, n_out, mem, deferred) : where_scan<int64_t>(ctx, ix, W, out_ids, cap, n_out, mem, deferred);
}

}  // namespace

extern "C" {

int bmx_scan_where(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint64_t* out_ids, uint64_t cap,
                   uint64_t* n_out, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  return where_run(ctx, base_field, W, out_ids, cap, n_out, mem, /*deferred=*/false);
}

}  // extern "C"
