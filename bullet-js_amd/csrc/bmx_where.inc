// bmx_where.inc — boolean filters (bmx_where.h): bmx_scan_where over one context, and the host steps every query form over a boolean filter shares: the program
// (where_prepare), the predicate and the sweep grid in the width of the index's column (where_pred, where_agg_grid, where_sweep), the entry guards (where_enter,
// where_comm_guard), the mask pass in front of an emit pass (where_mask_pass) and the cursor steps of the paged sharded forms (where_stamp_only, page_note). The
// predicate is where_kernels.h PredWhere; run_scan_t (bmx_scan.inc) delivers bmx_scan_where's answer as it delivers every scan's. Included by bmx.hip (one
// translation unit) in front of every other query form over a filter. bmx_comm_scan_where (bmx_comm.inc) prepares the program once and enqueues it on every
// shard through where_run's deferred form and fetches with scan_collect, like bmx_comm_scan_filter.
namespace {

// The caller's program as the kernel takes it: the field table (fields other than the base field and ordered field pairs, in order of first use), per literal its slot, per clause its
// literal range (inside a clause the literals on the base field first), per field the set of its literals, the bounds clamped to the value domain (a lower bound of -VAL_MAX keeps tombstones out of every range; an
// upper bound of VAL_MAX changes no answer). A clock literal goes to the plain slot of its field (the base field has one for its clock literals) with the bounds as given. A MINUS entry and the SUBTRAHEND entry behind it become one literal on the slot of their pair (A, B), with the
// bounds as given. Host arithmetic only. nullptr: the program is fine; otherwise why it is refused (nothing is written then).
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
    // the entries one by one: the flag bits, and a MINUS entry and its SUBTRAHEND entry next to each other inside the clause
    for (uint32_t k = 0; k < clause_len[c]; k++) {
      const bmx_lit& in = lits[first + k];
      if (in.flags & ~(BMX_LIT_NOT | BMX_LIT_MINUS | BMX_LIT_SUBTRAHEND | BMX_LIT_CLOCK | BMX_LIT_CLOCK_TOMB)) return "bmx_scan_where: unknown flag bits";
      if (in.flags & (BMX_LIT_CLOCK | BMX_LIT_CLOCK_TOMB)) {       // a clock literal ranges over one row's clock, never over a difference
        if (in.flags & BMX_LIT_MINUS) return "bmx_scan_where: a clock literal goes with no BMX_LIT_MINUS";
        if (in.flags & BMX_LIT_SUBTRAHEND) return "bmx_scan_where: a clock literal goes with no BMX_LIT_SUBTRAHEND";
      }
      if (in.flags & BMX_LIT_SUBTRAHEND) {
        if (in.flags != BMX_LIT_SUBTRAHEND) return "bmx_scan_where: BMX_LIT_SUBTRAHEND goes with no other flag";
        if (in.lo != 0 || in.hi != 0) return "bmx_scan_where: a BMX_LIT_SUBTRAHEND entry has lo = hi = 0";
        if (k == 0 || !(lits[first + k - 1].flags & BMX_LIT_MINUS)) return "bmx_scan_where: a BMX_LIT_SUBTRAHEND entry follows no BMX_LIT_MINUS entry";
        if (in.field == lits[first + k - 1].field) return "bmx_scan_where: a field minus itself";
      } else if (in.flags & BMX_LIT_MINUS) {
        if (k + 1 == clause_len[c]) return "bmx_scan_where: a BMX_LIT_MINUS entry ends its clause";
        if (!(lits[first + k + 1].flags & BMX_LIT_SUBTRAHEND)) return "bmx_scan_where: a BMX_LIT_MINUS entry is followed by no BMX_LIT_SUBTRAHEND entry";
      }
    }
    // an AND does not care for its order: the literals on the base field go in front, so a lane whose column value fails one leaves the clause before any probe
    for (int probed = 0; probed < 2; probed++) {
      for (uint32_t k = 0; k < clause_len[c]; k++) {
        const bmx_lit& in = lits[first + k];
        if (in.flags & BMX_LIT_SUBTRAHEND) continue;               // (taken with the MINUS entry in front of it)
        const bool pair = in.flags & BMX_LIT_MINUS;                // A - B: always among the probed, also when A is the base field
        const bool clock = in.flags & (BMX_LIT_CLOCK | BMX_LIT_CLOCK_TOMB);      // the row's clock: always among the probed, the index column holds no clocks
        if ((pair || clock || in.field != base_field) != (probed != 0)) continue;
        WhereLit& o = W.lit[l];
        o.flags = (in.flags & BMX_LIT_NOT ? WHERE_LIT_NOT : 0u) | (in.flags & BMX_LIT_CLOCK ? WHERE_LIT_CLOCK_DATA : 0u) | (in.flags & BMX_LIT_CLOCK_TOMB ? WHERE_LIT_CLOCK_TOMB : 0u);
        o.lo = pair || clock ? in.lo : above_tombstones(in.lo);    // (a difference or a clock is no stored value: its bounds are taken as given)
        o.hi = pair || clock ? in.hi : std::min<int64_t>(in.hi, VAL_MAX);
        if (!probed) { o.slot = 0; W.base_lits |= 1u << l; l++; continue; }
        const uint32_t second = pair ? lits[first + k + 1].field : 0u;
        uint32_t s = 0;
        while (s < W.nfields && (W.field[s] != in.field || ((W.pairs >> s) & 1u) != (uint32_t)pair || (pair && W.field2[s] != second))) s++;
        if (s == W.nfields) {
          if (s == WHERE_MAX_FIELDS) return pair ? "bmx_scan_where: no slot left for a field pair (8 fields and pairs besides the base field)"
                                                 : "bmx_scan_where: more than 8 fields besides the base field";
          W.field[W.nfields++] = in.field;
          if (pair) {
            W.field2[s] = second;
            W.pairs |= (1u | (in.field == base_field ? 1u << WHERE_PAIR_A_BASE : 0u) | (second == base_field ? 1u << WHERE_PAIR_B_BASE : 0u)) << s;
          }
        }
        if (clock) W.pairs |= 1u << (WHERE_SLOT_CLOCK + s);       // (a field's value literals and clock literals share its plain slot and its one probe)
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
PredWhere<T> where_pred(bmx_ctx* ctx, const Index* ix, const WhereProg& W) {
  PredWhere<T> P;
  P.v = sizeof(T) == 4 ? reinterpret_cast<const T*>(ix->v32) : reinterpret_cast<const T*>(ix->v64);
  P.ids = ix->ids; P.slots = ctx->slots; P.nslots = ctx->nslots; P.nt = ix->n * sizeof(T) > SCAN_NT_BYTES; P.W = W;
  return P;
}
template <class T, bool PAIRS, bool CLOCKS>
T where_value(const PredWhere<T, PAIRS, CLOCKS>&);      // (never defined) decltype(where_value(P)): the width of a predicate
// For the kernels that are built with and without the pair path and the clock literals (where_kernels.h PredWhere's PAIRS): f(the predicate), those compiled in
// only when the program has a pair slot or a clock literal (either sets bits of W.pairs), so a program of plain literals runs the registers and the occupancy it
// always ran.
template <class P>
constexpr bool where_clocks = std::decay_t<P>::HAS_CLOCKS;      // where_clocks<decltype(P)>: is the clock literals' code compiled into this predicate
template <bool PAIRS, bool CLOCKS, class T>
PredWhere<T, PAIRS, CLOCKS> where_pred_as(const PredWhere<T>& P) {
  PredWhere<T, PAIRS, CLOCKS> Q;
  Q.v = P.v; Q.ids = P.ids; Q.slots = P.slots; Q.nslots = P.nslots; Q.nt = P.nt; Q.W = P.W;
  return Q;
}
template <class T, class F>
decltype(auto) where_plain_or_pairs(const PredWhere<T>& P, F&& f) {
  if (P.W.pairs) return f(P);
  return f(where_pred_as<false, false>(P));
}
// ... and three ways, for the id scan (the other sweeps choose between the last two: where_sweep_c, where_mask_pass): a program of plain literals, one with pair slots and no clock literal, one with a clock literal. Each runs the code it
// needs and no more; the first two run what they ran before there were clock literals.
template <class T, class F>
decltype(auto) where_by_paths(const PredWhere<T>& P, F&& f) {
  if (!P.W.pairs) return f(where_pred_as<false, false>(P));
  if (!(P.W.pairs >> WHERE_SLOT_CLOCK)) return f(where_pred_as<true, false>(P));
  return f(P);
}
// the grid of the sweeps: no workgroup with fewer than four rounds of loads to spread its one flush over
template <class T>
uint32_t where_agg_grid(bmx_ctx* ctx, const Index* ix) { return sweep_grid(ctx, ix->n, 4ull * TOP_THREADS * TOP_U * (16 / sizeof(T))); }
// where a sweep finds a field's value: the base field's column (0), a probe of its own, or nowhere
inline uint32_t where_agg_source(uint32_t field, uint32_t base_field) { return field == BMX_AGG_NO_FIELD ? AGG_SRC_NONE : (field == base_field ? 0u : AGG_SRC_PROBE); }

// One sweep of a prepared program over an index: f(predicate, grid) in the width of the index's column; f's result is handed on.
template <class F>
auto where_sweep(bmx_ctx* ctx, const Index* ix, const WhereProg& W, F&& f) {
  return by_width(ix->fits32, [&](auto t) { using T = decltype(t); return f(where_pred<T>(ctx, ix, W), where_agg_grid<T>(ctx, ix)); });
}

// ... for the sweeps whose kernels are built with and without the clock literals (their CLOCKS argument): f gets the build without them, which is the code these
// kernels ran before there were clock literals, unless the program has one.
template <class F>
auto where_sweep_c(bmx_ctx* ctx, const Index* ix, const WhereProg& W, F&& f) {
  return where_sweep(ctx, ix, W, [&](const auto& P, uint32_t grid) {
    if (W.pairs >> WHERE_SLOT_CLOCK) return f(P, grid);
    return f(where_pred_as<true, false>(P), grid);
  });
}

// What every entry point over one context ends its own checks with, in this order: the mem kind, the context, the context entered.
inline int where_bad_mem(bmx_ctx* ctx, int mem) { return mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE ? fail(ctx, BMX_ERR_INVALID, "bad mem kind") : (int)BMX_OK; }
inline int where_enter(bmx_ctx* ctx, int mem) {
  if (int rc = where_bad_mem(ctx, mem)) return rc;
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  return enter(ctx);
}
// ... and every sharded one: the communicator and, for a form with a cursor (fn: its name), the cursor's shard.
inline int where_comm_guard(bmx_comm* c, const char* fn = nullptr, uint32_t start_shard = 0) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  if (fn && start_shard >= c->N) return fail(c, BMX_ERR_INVALID, std::string(fn) + ": start_shard is no shard");
  return BMX_OK;
}

// Pass 1 of the forms that emit rows, on a context that has been entered: the base index brought up to date, the scans' scratch sized, then k_scan_mask over
// make(where_pred<T>) — the program behind whatever the form adds to it — into the scans' own mask and counts. *out: what the emit pass needs of the index as
// this pass saw it. what: "launch k_scan_mask(<form>)", for a launch error's text. `ready` (optional) runs between the scratch and the launch.
template <class Make>
int where_mask_pass(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, const char* what, RowsScratch::Masked* out, Make&& make, int (*ready)(bmx_ctx*) = nullptr) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  if (int rc = ctx->scan.ensure(ctx, std::max<uint64_t>(ix->n, 1), 0)) return rc;
  if (ready) if (int rc = ready(ctx)) return rc;
  const uint32_t nb = (uint32_t)((std::max<uint64_t>(ix->n, 1) + SCAN_BLOCK_ELEMS - 1) / SCAN_BLOCK_ELEMS);
  by_width(ix->fits32, [&](auto t) {
    const auto launch = [&](const auto& Q) {                        // (the clock literals' code only for a program that has one, as where_sweep_c)
      auto P = make(Q);
      hipLaunchKernelGGL((k_scan_mask<decltype(P), true>), dim3(nb), dim3(SEL_THREADS), 0, ctx->stream, P, ix->n, ctx->scan.mask, ctx->scan.counts);
    };
    const auto P0 = where_pred<decltype(t)>(ctx, ix, W);
    if (W.pairs >> WHERE_SLOT_CLOCK) launch(P0); else launch(where_pred_as<true, false>(P0));
  });
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(ctx, e, what);      // (LAUNCHCHK with a text that is no literal)
  *out = RowsScratch::Masked{ix->ids, ix->fits32 ? static_cast<const void*>(ix->v32) : static_cast<const void*>(ix->v64), ix->n, ix->layout, ix->fits32, nb};
  return BMX_OK;
}

// The paged sharded forms. A shard in front of the cursor only refreshes its index: its layout stamp counts in the answer's.
int where_stamp_only(bmx_ctx* ctx, uint32_t base_field, RowsScratch::Masked* masked) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  masked->layout = ix->layout;
  return BMX_OK;
}
// ... and behind every shard that delivered: the answer's cursor names the first node that was selected and not delivered (more: shard g has one, at next_pos)
template <class Res>
void page_note(bool& cut, Res& tot, uint32_t g, uint64_t next_pos, bool more) {
  if (cut) return;
  tot.next_shard = g; tot.next_pos = next_pos;
  cut = more;
}

// One prepared program over one context that has been entered: bmx_scan_where, and the first half of bmx_comm_scan_where on every shard (deferred). A
// value-ordered view of the base field's index is neither read nor touched: fresh_index keeps the dense columns current whether or not a view exists.
int where_run(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem, bool deferred) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  return where_sweep(ctx, ix, W, [&](const auto& P, uint32_t) { return where_by_paths(P, [&](const auto& Q) { return run_scan_t<false>(ctx, Q, ix, out_ids, cap, n_out, mem, deferred); }); });
}

}  // namespace

extern "C" {

int bmx_scan_where(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint64_t* out_ids, uint64_t cap,
                   uint64_t* n_out, int mem) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  return where_run(ctx, base_field, W, out_ids, cap, n_out, mem, /*deferred=*/false);
}

}  // extern "C"
