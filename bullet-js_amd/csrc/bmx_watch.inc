// bmx_watch.inc — standing queries (bmx_watch.h): bmx_watch_* over one context and bmx_comm_watch_* over the shards. Kernels: watch_kernels.h, and select.h's
// k_scan_emit as the scans use it, in bmx_scan.inc's geometry (emit_dispatch). The program, the predicate in the width of the index's column and the mem-kind and
// communicator checks are bmx_where.inc's (where_prepare, where_sweep, where_bad_mem, where_comm_guard). Included by bmx.hip (one translation unit), which keeps the state
// (Watch, WatchState). A poll is two halves, watch_diff (enqueue the comparison) and watch_finish (emit the lists, commit, deliver): bmx_watch_poll runs them back
// to back, bmx_comm_watch_poll reads every shard's counts (watch_counts) in between.
namespace {

int WatchState::ensure(bmx_ctx* ctx, uint64_t nb) {
  if (nb <= blocks_cap) return BMX_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  blocks_cap = 0;
  const uint64_t cap = nb + nb / 4 + 16;
  left = nullptr;       // (the second half of the one allocation)
  if (int rc = dev_alloc_all(ctx, {{entered, 2 * cap * (SCAN_BLOCK_ELEMS / 32) * sizeof(uint32_t)}, {counts, 3 * cap * sizeof(uint32_t)}})) return rc;
  left = entered + cap * (SCAN_BLOCK_ELEMS / 32);
  blocks_cap = cap;
  return BMX_OK;
}

const char* watch_bad_poll_args(const uint64_t* entered, uint64_t cap_entered, const uint64_t* left, uint64_t cap_left, const bmx_watch_res* res) {
  if (!res) return "bmx_watch_poll: null res";
  if ((!entered && cap_entered) || (!left && cap_left)) return "bmx_watch_poll: a null list needs a cap of 0";
  return nullptr;
}
bool watch_live(const bmx_ctx* ctx, uint32_t id) { return id < BMX_WATCH_MAX && ctx->watch.w[id].live; }

// A prepared program becomes a watch: the lowest free id. The first watch of a context allocates the words the polls share.
int watch_create_prepared(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint32_t* watch_out) {
  if (int erc = enter(ctx)) return erc;
  WatchState& S = ctx->watch;
  uint32_t id = 0;
  while (id < BMX_WATCH_MAX && S.w[id].live) id++;
  if (id == BMX_WATCH_MAX) return fail(ctx, BMX_ERR_INVALID, "bmx_watch_create: 16 watches are live on this context");
  if (!S.committed) {
    if (int rc = dev_alloc_all(ctx, {{S.committed, BMX_WATCH_MAX * sizeof(unsigned long long)}, {S.tot, 2 * sizeof(WatchTotals)}})) return rc;
    HIPCHK(hipMemsetAsync(S.tot, 0, 2 * sizeof(WatchTotals), ctx->stream));
  }
  HIPCHK(hipMemsetAsync(S.committed + id, 0, sizeof(unsigned long long), ctx->stream));     // committed under no layout: the first poll is a RESET poll
  Watch& w = S.w[id];
  w.live = true; w.base_field = base_field; w.W = W; w.layout = 0;
  *watch_out = id;
  return BMX_OK;
}

int watch_destroy(bmx_ctx* ctx, uint32_t id) {
  if (!watch_live(ctx, id)) return fail(ctx, BMX_ERR_INVALID, "bmx_watch_destroy: no such watch");
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipStreamSynchronize(ctx->stream));          // a poll that was only enqueued may still be reading the bitmap
  Watch& w = ctx->watch.w[id];
  dev_free(w.prev); w.prev_words = 0; w.live = false;
  if (ctx->watch.pend.on && ctx->watch.pend.watch == id) ctx->watch.pend.on = false;
  return BMX_OK;
}

// First half of a poll: the index is brought up to date as bmx_scan_where does it (a value-ordered view is neither read nor touched), the watch's bitmap is made
// to fit the index's layout, and the comparison and its totals are enqueued. Leaves ctx->watch.pend for watch_counts / watch_finish; nothing else may run on the
// context in between (the two scratch masks are the context's).
int watch_diff(bmx_ctx* ctx, uint32_t id) {
  if (!watch_live(ctx, id)) return fail(ctx, BMX_ERR_INVALID, "bmx_watch_poll: no such watch");
  if (int erc = enter(ctx)) return erc;
  WatchState& S = ctx->watch;
  Watch& w = S.w[id];
  S.pend.on = false;
  Index* ix;
  if (int rc = fresh_index(ctx, w.base_field, &ix)) return rc;
  if (w.layout != ix->layout) {
    // The index was laid out anew since this watch last looked (or this is its first poll): positions mean other rows now, so the committed set is emptied and the
    // bitmap is sized for the new columns. One bit per position up to the columns' CAPACITY, not their length, in whole 8192-row blocks: between two layouts rows
    // are only appended, appended rows fit under `cap` by construction (bmx_index_refresh.inc apply_refresh_result: when they do not, the index is rebuilt, which is
    // a new layout and brings the poll here again), and a bit behind the index's length has never been set, so the appended rows read zero.
    const uint64_t words = std::max<uint64_t>((ix->cap + SCAN_BLOCK_ELEMS - 1) / SCAN_BLOCK_ELEMS, 1) * (SCAN_BLOCK_ELEMS / 32);
    if (words > w.prev_words) {
      HIPCHK(hipStreamSynchronize(ctx->stream));
      w.prev_words = 0;
      if (int rc = dev_alloc(ctx, &w.prev, words)) return rc;
      w.prev_words = words;
    }
    HIPCHK(hipMemsetAsync(w.prev, 0, w.prev_words * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync(S.committed + id, 0, sizeof(unsigned long long), ctx->stream));
    w.layout = ix->layout;
  }
  const uint32_t nb = (uint32_t)((std::max<uint64_t>(ix->n, 1) + SCAN_BLOCK_ELEMS - 1) / SCAN_BLOCK_ELEMS);
  if ((uint64_t)nb * (SCAN_BLOCK_ELEMS / 32) > w.prev_words) return fail(ctx, BMX_ERR_INTERNAL, "bmx_watch_poll: the index outgrew its columns without a new layout");
  if (int rc = S.ensure(ctx, nb)) return rc;
  where_sweep(ctx, ix, w.W, [&](const auto& P, uint32_t) {      // (one workgroup per block, as the scans' mask pass: the sweep grid is not used)
    where_plain_or_pairs(P, [&](const auto& Q) {
      hipLaunchKernelGGL((k_watch_mask<std::decay_t<decltype(Q)>>), dim3(nb), dim3(SEL_THREADS), 0, ctx->stream, Q, ix->n, (const uint32_t*)w.prev, S.entered, S.counts, (uint32_t)S.blocks_cap);
    });
  });
  LAUNCHCHK("k_watch_mask");
  hipLaunchKernelGGL(k_watch_totals, dim3(1), dim3(SEL_THREADS), 0, ctx->stream, (const uint32_t*)S.counts, (const uint32_t*)(S.counts + S.blocks_cap),
                     (const uint32_t*)(S.counts + 2 * S.blocks_cap), nb, (const unsigned long long*)(S.committed + id), (unsigned long long)ix->layout, S.tot);
  LAUNCHCHK("k_watch_totals");
  S.pend = WatchState::Pending{true, id, ix->n, nb, ix->ids, ix->layout};
  return BMX_OK;
}

// Between the halves (bmx_comm_watch_poll): wait for the comparison and read its totals.
int watch_counts(bmx_ctx* ctx, WatchTotals* out) {
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->watch.pend.on) return fail(ctx, BMX_ERR_INTERNAL, "bmx_watch_poll: no comparison is pending");
  HIPCHK(hipMemcpyAsync(out, ctx->watch.tot, sizeof(WatchTotals), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return BMX_OK;
}

// one list out of its mask, in position order: select.h k_scan_emit exactly as run_scan_t launches it (BMX_SCAN_SUB8_BLOCKS included); the total is k_watch_totals'
int watch_emit(bmx_ctx* ctx, const WatchState::Pending& P, const uint32_t* mask, const uint32_t* counts, uint64_t* d_out, uint64_t d_cap) {
  EmitIds Em{P.ids, d_out, d_cap, P.n * sizeof(uint64_t) > SCAN_NT_BYTES, SCAN_STREAM_MIN, SCAN_NTX_DEFAULT};
  FinishCount Fin{nullptr};
  emit_dispatch(P.nb, [&](auto B, uint32_t wgs) {
    hipLaunchKernelGGL((k_scan_emit<EmitIds, FinishCount, decltype(B)::value>), dim3(wgs), dim3(SEL_THREADS), 0, ctx->stream, mask, counts, P.n, P.nb, Em, Fin);
  });
  LAUNCHCHK("k_scan_emit(watch)");
  return BMX_OK;
}

// Second half of a poll: the two lists, the commit, and the way to the caller. BMX_MEM_DEVICE: the kernels write the caller's buffers and record; nothing waits.
// BMX_MEM_HOST: lists of at most SCAN_PIN_IDS ids in all come back through the mapped small-answer buffer, a caller's page-locked list is written by the kernels
// themselves, anything else is staged in the scans' download buffer; the record comes through a mapped word of the watches' own (or is downloaded).
int watch_finish(bmx_ctx* ctx, uint32_t id, uint64_t* entered, uint64_t cap_entered, uint64_t* left, uint64_t cap_left, bmx_watch_res* res, int mem) {
  HIPCHK(hipSetDevice(ctx->device));
  WatchState& S = ctx->watch;
  const WatchState::Pending P = S.pend;
  S.pend.on = false;
  if (!P.on || P.watch != id) return fail(ctx, BMX_ERR_INTERNAL, "bmx_watch_poll: no comparison of this watch is pending");
  uint64_t* d_e = entered; uint64_t* d_l = left;
  uint64_t room_e = entered ? cap_entered : 0, room_l = left ? cap_left : 0;
  bmx_watch_res* d_res = res;
  bool pinned = false, staged_e = false, staged_l = false;
  if (mem == BMX_MEM_HOST) {
    room_e = std::min<uint64_t>(room_e, P.n); room_l = std::min<uint64_t>(room_l, P.n);     // (a list is a subset of the positions)
    if (room_e + room_l <= SCAN_PIN_IDS && ensure_pinned(ctx)) {
      pinned = true;
      d_e = reinterpret_cast<uint64_t*>(ctx->host.pin_out); d_l = d_e + room_e;
    } else {
      d_e = room_e ? static_cast<uint64_t*>(mapped_host(entered)) : nullptr;
      d_l = room_l ? static_cast<uint64_t*>(mapped_host(left)) : nullptr;
      staged_e = room_e && !d_e; staged_l = room_l && !d_l;
      if (staged_e || staged_l) {
        if (int rc = ctx->scan.ensure(ctx, std::max<uint64_t>(P.n, 1), (staged_e ? room_e : 0) + (staged_l ? room_l : 0))) return rc;
        if (staged_e) d_e = ctx->scan.out;
        if (staged_l) d_l = ctx->scan.out + (staged_e ? room_e : 0);
      }
    }
    if (!S.hres && hipHostMalloc(reinterpret_cast<void**>(&S.hres), sizeof(bmx_watch_res), hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); S.hres = nullptr; }
    d_res = S.hres ? S.hres : reinterpret_cast<bmx_watch_res*>(S.tot + 1);
  }
  const uint32_t* cnt_e = S.counts; const uint32_t* cnt_l = S.counts + S.blocks_cap;
  if (room_e) if (int rc = watch_emit(ctx, P, S.entered, cnt_e, d_e, room_e)) return rc;
  if (room_l) if (int rc = watch_emit(ctx, P, S.left, cnt_l, d_l, room_l)) return rc;
  const uint64_t nquads = (uint64_t)P.nb * (SCAN_BLOCK_ELEMS / 128);
  const uint32_t cblocks = (uint32_t)std::min<uint64_t>((nquads + 255) / 256, 2048);
  hipLaunchKernelGGL(k_watch_commit, dim3(cblocks), dim3(256), 0, ctx->stream, reinterpret_cast<const uint4*>(S.entered), reinterpret_cast<const uint4*>(S.left),
                     reinterpret_cast<uint4*>(S.w[id].prev), nquads, (const WatchTotals*)S.tot, cap_entered, cap_left, S.committed + id, (unsigned long long)P.layout, d_res);
  LAUNCHCHK("k_watch_commit");
  if (mem != BMX_MEM_HOST) return BMX_OK;
  bmx_watch_res r;
  if (!S.hres) HIPCHK(hipMemcpyAsync(&r, d_res, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (S.hres) std::memcpy(&r, S.hres, sizeof(r));
  const uint64_t k_e = std::min<uint64_t>(r.n_entered, room_e), k_l = std::min<uint64_t>(r.n_left, room_l);
  if (pinned) {
    if (k_e) std::memcpy(entered, d_e, k_e * 8);
    if (k_l) std::memcpy(left, d_l, k_l * 8);
  } else {
    if (staged_e && k_e) HIPCHK(hipMemcpy(entered, d_e, k_e * 8, hipMemcpyDeviceToHost));
    if (staged_l && k_l) HIPCHK(hipMemcpy(left, d_l, k_l * 8, hipMemcpyDeviceToHost));
  }
  *res = r;
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_watch_create(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t* watch_out) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (!watch_out) return fail(ctx, BMX_ERR_INVALID, "bmx_watch_create: null watch_out");
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  return watch_create_prepared(ctx, base_field, W, watch_out);
}

int bmx_watch_poll(bmx_ctx* ctx, uint32_t watch, uint64_t* entered, uint64_t cap_entered, uint64_t* left, uint64_t cap_left, bmx_watch_res* res, int mem) {
  if (int rc = where_bad_mem(ctx, mem)) return rc;
  if (const char* bad = watch_bad_poll_args(entered, cap_entered, left, cap_left, res)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int rc = watch_diff(ctx, watch)) return rc;
  return watch_finish(ctx, watch, entered, cap_entered, left, cap_left, res, mem);
}

int bmx_watch_destroy(bmx_ctx* ctx, uint32_t watch) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  return watch_destroy(ctx, watch);
}

// One watch id on every shard: the shards are given the same creates and destroys in the same order, so each hands out the same lowest free id.
int bmx_comm_watch_create(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t* watch_out) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (!watch_out) return fail(c, BMX_ERR_INVALID, "bmx_watch_create: null watch_out");
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  uint32_t id0 = 0;
  for (uint32_t g = 0; g < c->N; g++) {
    uint32_t id = 0;
    const int rc = watch_create_prepared(c->sh[g], base_field, W, &id);
    if (rc || (g && id != id0)) {        // nothing half-made stays behind
      const std::string msg = rc ? shard_msg(c, g) : "bmx_comm_watch_create: the shards hand out different ids (a watch was created on one shard alone)";
      if (!rc) (void)watch_destroy(c->sh[g], id);
      for (uint32_t k = 0; k < g; k++) (void)watch_destroy(c->sh[k], id0);
      return fail(c, rc ? rc : BMX_ERR_INVALID, msg);
    }
    id0 = id;
  }
  *watch_out = id0;
  return BMX_OK;
}

int bmx_comm_watch_poll(bmx_comm* c, uint32_t watch, uint64_t* entered, uint64_t cap_entered, uint64_t* left, uint64_t cap_left, bmx_watch_res* res) {
  if (const char* bad = watch_bad_poll_args(entered, cap_entered, left, cap_left, res)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  std::vector<WatchTotals> t(c->N);
  if (int rc = comm_two_phase(c, [&](uint32_t, bmx_ctx* x) { return watch_diff(x, watch); }, [&](uint32_t g, bmx_ctx* x) { return watch_counts(x, &t[g]); })) {
    for (uint32_t g = 0; g < c->N; g++) c->sh[g]->watch.pend.on = false;
    return rc;
  }
  bmx_watch_res sum{};
  for (uint32_t g = 0; g < c->N; g++) { sum.n_entered += t[g].n_entered; sum.n_left += t[g].n_left; sum.n_match += t[g].n_match; sum.flags |= t[g].flags; }
  if (sum.n_entered > cap_entered || sum.n_left > cap_left) {       // no shard commits: the halves that would are not run
    for (uint32_t g = 0; g < c->N; g++) c->sh[g]->watch.pend.on = false;
    sum.flags |= BMX_WATCH_OVERFLOW;
    *res = sum;
    return BMX_OK;
  }
  uint64_t off_e = 0, off_l = 0;
  for (uint32_t g = 0; g < c->N; g++) {       // every shard's lists fit its slice exactly, so every shard commits
    bmx_watch_res r;
    CSH(g, watch_finish(c->sh[g], watch, t[g].n_entered ? entered + off_e : nullptr, t[g].n_entered, t[g].n_left ? left + off_l : nullptr, t[g].n_left, &r, BMX_MEM_HOST));
    off_e += t[g].n_entered; off_l += t[g].n_left;
  }
  *res = sum;
  return BMX_OK;
}

int bmx_comm_watch_destroy(bmx_comm* c, uint32_t watch) {
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  int first = BMX_OK; std::string msg;
  for (uint32_t g = 0; g < c->N; g++) {
    const int rc = watch_destroy(c->sh[g], watch);
    if (rc && !first) { first = rc; msg = shard_msg(c, g); }
  }
  return first ? fail(c, first, msg) : BMX_OK;
}

}  // extern "C"
