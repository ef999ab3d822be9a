// bmx_view_sort.inc — the view's sort (bmx.h bmx_index_set_ordered; the rest of the view is bmx_view.inc): when a stale view is sorted again, the two sorts, and the
// bmx_index_*ordered* entry points. It stays behind refresh_from_log (bmx_index_refresh.inc): kernel templates are laid out in the gfx950 code object in the order the
// source first uses them, and this sort's kernels follow the patch's (in front, they would land elsewhere). Included by bmx.hip (one translation unit).
namespace {

// The policy. Is the view of `ix` usable for the query at hand? A stale one is sorted again by the ordered_after-th query since the columns last changed — the
// queries in front of that one scan the column as ever (one sort of a 100M-row column costs what ~20 scans cost). Owns the view's count of stale queries.
enum ViewState { VIEW_USABLE, VIEW_SCAN_INSTEAD, VIEW_SORT_NOW };
ViewState view_state(bmx_ctx* ctx, Index* ix) {
  OrderedView& v = ix->view;
  if (!v.ordered_after || ix->n == 0 || ix->n > 0xFFFFFFFFull) return VIEW_SCAN_INSTEAD;
  if (v.ord_content == ix->content && v.s_val) { finish_rewrite(ctx, v, /*wait=*/false); return VIEW_USABLE; }   // (a finished rewrite becomes main; an unfinished one changes nothing)
  finish_rewrite(ctx, v, /*wait=*/true);
  uint32_t after = v.ordered_after;
  if (after == BMX_INDEX_ORDERED_AUTO) {
    // rent or buy: sort once the scans answered since the change have cost what a sort costs — then whatever the caller does next, at most twice
    // the best possible was spent. A scan moves the value column at ~6 TB/s (+ two launches); a sort costs what the last one cost (first time: 60 us per 10^6 rows).
    const double scan_us = 8.0 + (double)ix->n * (ix->fits32 ? 4.0 : 8.0) / 6.0e6;
    const double sort_us = v.last_sort_us > 0 ? v.last_sort_us : 200.0 + (double)ix->n * 0.00006;
    after = (uint32_t)std::min<double>(1.0e6, std::max<double>(2.0, std::ceil(sort_us / scan_us)));
  }
  if (v.stale_content != ix->content) { v.stale_content = ix->content; v.stale_queries = 0; }   // the count starts with every change of the columns
  return ++v.stale_queries < after ? VIEW_SCAN_INSTEAD : VIEW_SORT_NOW;
}

// The two sorts: the columns of `ix` -> the view's (s_val, s_pos, s_ids), which have room. Synchronous; false = a HIP call failed or the scratch could not be had
// (the caller gives the view up). Their scratch goes back before they return.
// A/B arm (BMX_VIEW_SORT=own): the whole column through the patch path's sort — (value, position) keys, 4096-key tiles in LDS, then log2(n / 4096) merge-path passes between
// the view's columns and a scratch pair; a tombstone is the column type's minimum and sorts in front like every other value
bool sort_view_own(bmx_ctx* ctx, const Index* ix) {
  const OrderedView& v = ix->view;
  const uint64_t n = ix->n;
  const size_t vb = ix->fits32 ? sizeof(int32_t) : sizeof(int64_t);
  void* tv = nullptr; uint32_t* tp = nullptr;
  if (!alloc_all({{tv, n * vb}, {tp, n * sizeof(uint32_t)}})) return false;
  const uint32_t gbo = (uint32_t)std::min<uint64_t>((n + 255) / 256, 8192);
  unsigned passes = 0; for (uint64_t L = VIEW_SORT_TILE; L < n; L *= 2) passes++;
  auto run = [&](auto tag) {
    using T = decltype(tag);
    const T* col = sizeof(T) == 4 ? reinterpret_cast<const T*>(ix->v32) : reinterpret_cast<const T*>(ix->v64);
    T* bufv[2] = {static_cast<T*>(v.s_val), static_cast<T*>(tv)}; uint32_t* bufp[2] = {v.s_pos, tp};
    const int first = passes & 1;                                     // the tile sort writes into the buffer from which `passes` swaps end in the view's columns
    uint32_t* iota = bufp[first ^ 1];                                 // (the other position buffer is free until the first pass writes it)
    hipLaunchKernelGGL(k_iota_u32, dim3(gbo), dim3(256), 0, ctx->stream, iota, n);
    sort_view_keys<T>(ctx->stream, col, iota, bufv, bufp, n, 0, first);
  };
  if (ix->fits32) run(int32_t{}); else run(int64_t{});
  hipLaunchKernelGGL(k_view_gather_ids, dim3(gbo), dim3(256), 0, ctx->stream, (const uint32_t*)v.s_pos, (uint32_t)n, (const uint64_t*)ix->ids, v.s_ids);
  hipError_t eo = hipGetLastError();
  if (eo == hipSuccess) eo = hipStreamSynchronize(ctx->stream);
  dev_free(tv); dev_free(tp);
  return eo == hipSuccess;
}
// rocPRIM's radix sort of (value, position) pairs
bool sort_view_rocprim(bmx_ctx* ctx, const Index* ix) {
  const OrderedView& v = ix->view;
  const uint64_t n = ix->n;
  // the column's value range decides how many bits the sort has to look at (csrc/ordered_sort.hip: keys rebased to min = 1, tombstones = 0)
  const uint32_t gb = (uint32_t)std::min<uint64_t>((n + 255) / 256, 8192);
  long long mm[2] = {INT64_MAX, INT64_MIN};
  long long* d_mm = reinterpret_cast<long long*>(ctx->ds->ord_ab);
  hipError_t e = hipMemcpyAsync(d_mm, mm, sizeof(mm), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    if (ix->fits32) hipLaunchKernelGGL((k_col_minmax<int32_t>), dim3(std::min<uint32_t>(gb, 2048)), dim3(256), 0, ctx->stream, (const int32_t*)ix->v32, n, d_mm);
    else hipLaunchKernelGGL((k_col_minmax<int64_t>), dim3(std::min<uint32_t>(gb, 2048)), dim3(256), 0, ctx->stream, (const int64_t*)ix->v64, n, d_mm);
    e = hipMemcpyAsync(mm, d_mm, sizeof(mm), hipMemcpyDeviceToHost, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return false;
  if (mm[0] > mm[1]) { mm[0] = 0; mm[1] = 0; }                   // nothing but tombstones
  const unsigned long long span = (unsigned long long)mm[1] - (unsigned long long)mm[0] + 1ull;     // largest rebased key
  unsigned bits = 1; while (bits < 64 && (span >> bits)) bits++;
  bits = std::min<unsigned>(bits, ix->fits32 ? 32u : 64u);
  uint32_t* iota = nullptr; void* tmp = nullptr; size_t tmp_bytes = 0;
  e = ix->fits32 ? sort_pairs_i32(nullptr, &tmp_bytes, nullptr, 0, bits, nullptr, nullptr, nullptr, n, ctx->stream)
                 : sort_pairs_i64(nullptr, &tmp_bytes, nullptr, 0, bits, nullptr, nullptr, nullptr, n, ctx->stream);
  if (e != hipSuccess || !alloc_all({{iota, n * sizeof(uint32_t)}, {tmp, std::max<size_t>(tmp_bytes, 16)}})) return false;
  hipLaunchKernelGGL(k_iota_u32, dim3(gb), dim3(256), 0, ctx->stream, iota, n);
  e = ix->fits32 ? sort_pairs_i32(tmp, &tmp_bytes, ix->v32, (int32_t)mm[0], bits, static_cast<uint32_t*>(v.s_val), iota, v.s_pos, n, ctx->stream)
                 : sort_pairs_i64(tmp, &tmp_bytes, ix->v64, (int64_t)mm[0], bits, static_cast<uint64_t*>(v.s_val), iota, v.s_pos, n, ctx->stream);
  if (e == hipSuccess) {
    if (ix->fits32) hipLaunchKernelGGL((k_gather_ids<int32_t, uint32_t>), dim3(gb), dim3(256), 0, ctx->stream, (const uint64_t*)ix->ids, (const uint32_t*)v.s_pos, v.s_ids, n, static_cast<uint32_t*>(v.s_val), (int32_t)mm[0]);
    else hipLaunchKernelGGL((k_gather_ids<int64_t, uint64_t>), dim3(gb), dim3(256), 0, ctx->stream, (const uint64_t*)ix->ids, (const uint32_t*)v.s_pos, v.s_ids, n, static_cast<uint64_t*>(v.s_val), (int64_t)mm[0]);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);       // the scratch goes back below
  dev_free(iota); dev_free(tmp);
  return e == hipSuccess;
}

// Is the view of `ix` usable for the query at hand (view_state)? Where it is time to, the view is sorted first — never while it cannot be had (no memory: the index
// goes on without it). Synchronous where it sorts. Room for the view, giving it up and the bookkeeping of a finished sort are here, once for both sorts.
bool ensure_ordered_view(bmx_ctx* ctx, Index* ix) {
  const ViewState st = view_state(ctx, ix);
  if (st != VIEW_SORT_NOW) return st == VIEW_USABLE;
  OrderedView& v = ix->view;
  const auto t_sort = std::chrono::steady_clock::now();
  v.npd = v.npi = 0;                          // a fresh sort of the columns: whatever patch was pending is in them
  const uint64_t n = ix->n;
  bool ok = true;
  if (n > v.ord_cap || v.ord_fits32 != ix->fits32) {
    v.release();
    const uint64_t cap = n + n / 8 + 1024;
    ok = alloc_all({{v.s_val, cap * (ix->fits32 ? sizeof(int32_t) : sizeof(int64_t))}, {v.s_pos, cap * sizeof(uint32_t)}, {v.s_ids, cap * sizeof(uint64_t)}});
    if (ok) { v.ord_cap = cap; v.ord_fits32 = ix->fits32; }
  }
  ok = ok && ((ctx->view.own_sort && n < 0xFFFFFFFFull) ? sort_view_own(ctx, ix) : sort_view_rocprim(ctx, ix));
  if (!ok) { (void)hipGetLastError(); v.release(); v.stale_queries = 0; return false; }
  v.ord_n = n; v.ord_content = ix->content; v.stale_queries = 0; v.ord_sorts++;
  v.last_sort_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_sort).count();
  return true;
}

}  // namespace

extern "C" {

int bmx_index_set_ordered(bmx_ctx* ctx, uint32_t field, uint32_t after_queries) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  int rc = fresh_index(ctx, field, &ix);      // (creates the index like a first query would)
  if (rc) return rc;
  ix->view.ordered_after = after_queries;
  ix->view.stale_queries = 0;
  if (!after_queries) { HIPCHK(hipStreamSynchronize(ctx->stream)); ix->view.release(); }
  return BMX_OK;
}
int bmx_index_ordered_info(bmx_ctx* ctx, uint32_t field, uint32_t* after_queries, int* valid_now, uint64_t* sorts) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  Index* ix = find_index(ctx, field);
  if (!ix) return fail(ctx, BMX_ERR_INVALID, "bmx_index_ordered_info: no index on this field");
  const OrderedView& v = ix->view;
  if (after_queries) *after_queries = v.ordered_after;
  if (valid_now) *valid_now = v.ordered_after && v.s_val && v.ord_content == ix->content && ix->version == ctx->version;
  if (sorts) *sorts = v.ord_sorts;
  return BMX_OK;
}

int bmx_index_ordered_stats(bmx_ctx* ctx, uint32_t field, uint64_t* sorts, uint64_t* patches, uint64_t* keys_patched, double* last_sort_us, double* last_patch_us, uint64_t* rewrites, uint64_t* pending_keys) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  Index* ix = find_index(ctx, field);
  if (!ix) return fail(ctx, BMX_ERR_INVALID, "bmx_index_ordered_stats: no index on this field");
  const OrderedView& v = ix->view;
  if (sorts) *sorts = v.ord_sorts;
  if (patches) *patches = v.ord_patches;
  if (keys_patched) *keys_patched = v.ord_patched_keys;
  if (last_sort_us) *last_sort_us = v.last_sort_us;
  if (last_patch_us) *last_patch_us = v.last_patch_us;
  if (rewrites) *rewrites = v.ord_merges;
  if (pending_keys) *pending_keys = v.npd + v.npi;
  return BMX_OK;
}

}  // extern "C"
