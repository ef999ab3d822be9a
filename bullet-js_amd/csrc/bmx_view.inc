// bmx_view.inc — host side of the value-ordered index view (include/bmx.h bmx_index_set_ordered; kernels: view_kernels.h, csrc/ordered_sort.hip):
// the patch under writes with its pending runs and the rewrite of main behind the answer, and the ordered queries. Included by bmx.hip (one
// translation unit), which keeps the view's state (OrderedView per index, ViewShared per context). The view's sort and the bmx_index_*ordered* entry points are
// bmx_view_sort.inc, behind the index refresh that calls the patch here (bmx.hip, the include list).
namespace {

void ViewShared::read_env() {   // at create: the A/B switches, the test hook and the diagnostic prints
  { const char* vp = std::getenv("BMX_VIEW_PATCH"); if (vp && vp[0] == '0' && !vp[1]) patching = false; }
  { const char* vf = std::getenv("BMX_TEST_VIEW_FAIL"); if (vf && (vf[0] == '1' || vf[0] == '2') && !vf[1]) test_fail = vf[0] - '0'; }
  { const char* vs = std::getenv("BMX_VIEW_SORT"); if (vs && std::strcmp(vs, "own") == 0) own_sort = true; }
  { const char* vp = std::getenv("BMX_VIEW_PENDING"); if (vp && vp[0] == '0' && !vp[1]) pending = false; }
  debug = std::getenv("BMX_VIEW_DEBUG") != nullptr;
}
void ViewShared::release() {
  for (int i = 0; i < 2; i++) { dev_free(vk_v[i]); dev_free(vk_p[i]); }
  dev_free(vk_sv); dev_free(vk_sp); dev_free(vk_d0); dev_free(vk_y0);
  if (err_host) (void)hipHostFree(err_host); if (ev) (void)hipEventDestroy(ev);
}
void OrderedView::release_pending() {
  for (int i = 0; i < 2; i++) { dev_free(pd_v[i]); dev_free(pd_p[i]); dev_free(pi_v[i]); dev_free(pi_p[i]); dev_free(pi_ids[i]); }
  dev_free(pi_dead);
  npd = npi = 0; pend_cap = 0; pcur = 0; icur = 0; rewrite_due = false; rewrite_inflight = false;
}
void OrderedView::release() {
  release_pending();
  dev_free(s_val); dev_free(s_pos); dev_free(s_ids); dev_free(s_val2); dev_free(s_pos2); dev_free(s_ids2);
  dev_free(cl_pos); dev_free(cl_old); dev_free(cl2_pos); dev_free(cl2_old);
  ord_cap = 0; ord_n = 0; ord_content = ~0ull; ord_cap2 = 0; cl_cap = 0;
}

// the page-locked error word and the event through which a background rewrite reports (false: not to be had, no rewrite runs behind an answer)
bool ensure_rewrite_report(ViewShared& sh) {
  if (!sh.err_host && hipHostMalloc(reinterpret_cast<void**>(&sh.err_host), sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); sh.err_host = nullptr; }
  if (!sh.ev && hipEventCreateWithFlags(&sh.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); sh.ev = nullptr; }
  return sh.err_host && sh.ev;
}

// ---- the value-ordered view kept current (view_kernels.h) ----
constexpr uint64_t VIEW_PATCH_MAX_LOG = 1ull << 24;     // a longer change log is not captured: the view goes stale and is sorted again (a sort of 10^8 rows costs less than a patch that large)
// the change run's capture buffers for a log of `ub` entries; without room there the refresh captures nothing and the view goes stale
int ensure_change_run(bmx_ctx* ctx, OrderedView& v, uint64_t ub) {
  if (v.cl_cap >= ub) return BMX_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  v.cl_cap = 0;
  const uint64_t cap = (ub + ub / 2 + (1u << 16) + 255) & ~255ull;
  if (alloc_all({{v.cl_pos, cap * sizeof(uint32_t)}, {v.cl_old, cap * sizeof(int64_t)}, {v.cl2_pos, cap * sizeof(uint32_t)}, {v.cl2_old, cap * sizeof(int64_t)}})) v.cl_cap = cap;
  return BMX_OK;
}
int ensure_view_scratch(bmx_ctx* ctx, uint64_t keys, uint64_t tiles) {
  ViewShared& sh = ctx->view;
  if (keys > sh.vk_cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    sh.vk_cap = 0;
    const uint64_t cap = (keys + keys / 4 + (1u << 16) + 255) & ~255ull;
    if (!alloc_all({{sh.vk_v[0], cap * 8}, {sh.vk_p[0], cap * 4}, {sh.vk_v[1], cap * 8}, {sh.vk_p[1], cap * 4}})) return fail(ctx, BMX_ERR_NOMEM, "view patch: out of device memory");
    sh.vk_cap = cap;
  }
  if (tiles + 1 > sh.vk_tiles_cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    sh.vk_tiles_cap = 0;
    const uint64_t cap = tiles + tiles / 4 + 1024;
    if (!alloc_all({{sh.vk_sv, cap * 8}, {sh.vk_sp, cap * 4}, {sh.vk_d0, cap * 4}, {sh.vk_y0, cap * 4}})) return fail(ctx, BMX_ERR_NOMEM, "view patch: out of device memory");
    sh.vk_tiles_cap = cap;
  }
  return BMX_OK;
}
// Sort (value, position) keys in two segments, [0, n0) and [n0, n0 + n1) (n1 = 0: one segment): k_view_tile_sort from (iv, ip) into buffer `first` of the pair
// (bv, bp), then merge-path passes between the two buffers until the runs span their segments. Returns the buffer that holds the result. Enqueue only.
template <class T>
int sort_view_keys(hipStream_t st, const T* iv, const uint32_t* ip, T* const bv[2], uint32_t* const bp[2], uint64_t n0, uint64_t n1, int first) {
  ViewSegs S{}; S.base[0] = 0; S.len[0] = (uint32_t)n0; S.base[1] = (uint32_t)n0; S.len[1] = (uint32_t)n1;
  const uint32_t t0 = (uint32_t)((n0 + VIEW_SORT_TILE - 1) / VIEW_SORT_TILE), t1 = (uint32_t)((n1 + VIEW_SORT_TILE - 1) / VIEW_SORT_TILE);
  S.blk0[0] = 0; S.blk0[1] = t0; S.blk0[2] = t0 + t1;
  hipLaunchKernelGGL((k_view_tile_sort<T>), dim3(t0 + t1), dim3(VIEW_SORT_THREADS), 0, st, iv, ip, bv[first], bp[first], S);
  ViewSegs P = S; P.blk0[1] = (uint32_t)((n0 + VIEW_PASS_KEYS - 1) / VIEW_PASS_KEYS); P.blk0[2] = P.blk0[1] + (uint32_t)((n1 + VIEW_PASS_KEYS - 1) / VIEW_PASS_KEYS);
  int cur = first;
  for (uint64_t L = VIEW_SORT_TILE; L < std::max<uint64_t>(n0, n1); L *= 2) {
    hipLaunchKernelGGL((k_view_merge_pass<T>), dim3(P.blk0[2]), dim3(256), 0, st, (const T*)bv[cur], (const uint32_t*)bp[cur], bv[cur ^ 1], bp[cur ^ 1], P, (uint32_t)L);
    cur ^= 1;
  }
  return cur;
}
// Z = (X without the sorted keys D, all of which are keys of X) merged with the sorted keys Y — k_view_merge over the tiles of X, with its sample and tile offsets
// in the context's scratch. X may be empty (then D is, and Z = Y). Enqueue only; a deleted key that is not in X raises ds->view_err.
template <class T, bool HAS_IDS>
void launch_run_merge(bmx_ctx* ctx, ViewRun<T> X, uint64_t nx, const T* dv, const uint32_t* dp, uint64_t nd, const T* yv, const uint32_t* yp, uint64_t ny, const uint64_t* ix_ids, ViewRun<T> Z) {
  hipStream_t st = ctx->stream;
  if (nx == 0) {
    if (ny) {
      (void)hipMemcpyAsync(Z.v, yv, ny * sizeof(T), hipMemcpyDeviceToDevice, st); (void)hipMemcpyAsync(Z.p, yp, ny * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
      if (HAS_IDS) hipLaunchKernelGGL(k_view_gather_ids, dim3((uint32_t)std::min<uint64_t>((ny + 255) / 256, 4096)), dim3(256), 0, st, yp, (uint32_t)ny, ix_ids, Z.ids);
    }
    return;
  }
  const uint32_t ntiles = (uint32_t)((nx + VIEW_TILE - 1) / VIEW_TILE);
  T* sv = static_cast<T*>(ctx->view.vk_sv);
  hipLaunchKernelGGL((k_view_sample<T>), dim3((ntiles + 255) / 256), dim3(256), 0, st, (const T*)X.v, (const uint32_t*)X.p, ntiles, sv, ctx->view.vk_sp);
  hipLaunchKernelGGL((k_view_tile_offsets<T>), dim3((ntiles + 1 + 255) / 256), dim3(256), 0, st, (const T*)sv, (const uint32_t*)ctx->view.vk_sp, ntiles, dv, dp, (uint32_t)nd, yv, yp, (uint32_t)ny, ctx->view.vk_d0, ctx->view.vk_y0);
  hipLaunchKernelGGL((k_view_merge<T, HAS_IDS>), dim3(ntiles), dim3(256), 0, st, X, (uint32_t)nx, dv, dp, yv, yp, ix_ids, Z, (const uint32_t*)ctx->view.vk_d0, (const uint32_t*)ctx->view.vk_y0, &ctx->ds->view_err);
}
// the pending patch's buffers for at least `need` keys in each run (what is there is kept)
template <class T>
int ensure_pending(bmx_ctx* ctx, OrderedView& v, uint64_t need) {
  if (need <= v.pend_cap) return BMX_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t cap = need + need / 8 + (1u << 16);
  void* nv[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; uint32_t* np[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; uint64_t* ni[2] = {nullptr, nullptr}; uint8_t* nd = nullptr;
  if (!alloc_all({{nd, cap}, {nv[0][0], cap * sizeof(T)}, {np[0][0], cap * 4}, {nv[1][0], cap * sizeof(T)}, {np[1][0], cap * 4}, {ni[0], cap * 8},
                  {nv[0][1], cap * sizeof(T)}, {np[0][1], cap * 4}, {nv[1][1], cap * sizeof(T)}, {np[1][1], cap * 4}, {ni[1], cap * 8}}))
    return fail(ctx, BMX_ERR_NOMEM, "view patch: out of device memory");
  const int c = v.pcur, ci = v.icur;
  if (v.npd) { HIPCHK(hipMemcpy(nv[0][c], v.pd_v[c], v.npd * sizeof(T), hipMemcpyDeviceToDevice)); HIPCHK(hipMemcpy(np[0][c], v.pd_p[c], v.npd * 4, hipMemcpyDeviceToDevice)); }
  if (v.npi) { HIPCHK(hipMemcpy(nv[1][ci], v.pi_v[ci], v.npi * sizeof(T), hipMemcpyDeviceToDevice)); HIPCHK(hipMemcpy(np[1][ci], v.pi_p[ci], v.npi * 4, hipMemcpyDeviceToDevice));
                HIPCHK(hipMemcpy(ni[ci], v.pi_ids[ci], v.npi * 8, hipMemcpyDeviceToDevice)); }
  std::swap(v.pd_v, nv[0]); std::swap(v.pd_p, np[0]); std::swap(v.pi_v, nv[1]); std::swap(v.pi_p, np[1]); std::swap(v.pi_ids, ni); std::swap(v.pi_dead, nd);
  for (int i = 0; i < 2; i++) { dev_free(nv[0][i]); dev_free(np[0][i]); dev_free(nv[1][i]); dev_free(np[1][i]); dev_free(ni[i]); }   // (the old buffers)
  dev_free(nd); v.pend_cap = cap;
  return BMX_OK;
}
// the second set of the view's columns, for `nz` rows
template <class T>
bool ensure_view_spare(bmx_ctx* ctx, OrderedView& v, uint64_t nz) {
  if (nz <= v.ord_cap2 && v.s_val2) return true;
  if (v.s_val2) (void)hipStreamSynchronize(ctx->stream);
  v.ord_cap2 = 0;
  const uint64_t cap = std::max<uint64_t>(v.ord_cap, nz + nz / 8 + 1024);
  if (!alloc_all({{v.s_val2, cap * sizeof(T)}, {v.s_pos2, cap * sizeof(uint32_t)}, {v.s_ids2, cap * sizeof(uint64_t)}})) return false;
  v.ord_cap2 = cap;
  return true;
}
// the second set of columns, main - pd + pi with `nz` keys, becomes main
void take_spare(OrderedView& v, uint64_t nz) {
  std::swap(v.s_val, v.s_val2); std::swap(v.s_pos, v.s_pos2); std::swap(v.s_ids, v.s_ids2); std::swap(v.ord_cap, v.ord_cap2);
  v.ord_n = nz; v.npd = v.npi = 0; v.ord_merges++;
}
// ---- the rewrite of a view's main run, behind the answer ----
// finish_rewrite: a rewrite in flight whose event has completed (wait = true: wait for it) is looked at: error word 0 -> the second set of columns becomes main and the
// pending patch is empty; otherwise main and the patch stay what they are (they were never touched). Called in front of anything that reads or changes the view.
void finish_rewrite(bmx_ctx* ctx, OrderedView& v, bool wait) {
  if (!v.rewrite_inflight) return;
  if (wait) (void)hipEventSynchronize(ctx->view.ev);
  else if (hipEventQuery(ctx->view.ev) != hipSuccess) { (void)hipGetLastError(); return; }
  v.rewrite_inflight = false;
  if (*ctx->view.err_host == 0 && ctx->view.test_fail != 2) take_spare(v, v.rewrite_nz);
}
// start_rewrite: enqueue main - pd + pi -> the second set of columns, then the copy of the error word and the event. Nothing waits.
template <class T>
void start_rewrite(bmx_ctx* ctx, Index& ix) {
  OrderedView& v = ix.view;
  v.rewrite_due = false;
  if (v.rewrite_inflight || v.npd + v.npi == 0 || v.npd > v.ord_n) return;
  if (!ensure_rewrite_report(ctx->view)) return;
  for (auto& o : ctx->indexes) if (o.view.rewrite_inflight) return;                 // one at a time: they share the error word and the event
  const uint64_t nz = v.ord_n - v.npd + v.npi;
  const uint32_t ntiles = (uint32_t)((v.ord_n + VIEW_TILE - 1) / VIEW_TILE);
  if (ntiles + 1 > ctx->view.vk_tiles_cap || !ensure_view_spare<T>(ctx, v, nz)) return;
  const int q = v.pcur, qi = v.icur;
  (void)hipMemsetAsync(&ctx->ds->view_err, 0, sizeof(uint32_t), ctx->stream);
  ViewRun<T> X{static_cast<T*>(v.s_val), v.s_pos, v.s_ids}, Z{static_cast<T*>(v.s_val2), v.s_pos2, v.s_ids2};
  launch_run_merge<T, true>(ctx, X, v.ord_n, static_cast<const T*>(v.pd_v[q]), v.pd_p[q], v.npd, static_cast<const T*>(v.pi_v[qi]), v.pi_p[qi], v.npi, (const uint64_t*)ix.ids, Z);
  *ctx->view.err_host = 1u;                                                       // (overwritten by the copy below: an event that somehow completed without it reads as a failure)
  if (hipMemcpyAsync(ctx->view.err_host, &ctx->ds->view_err, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipEventRecord(ctx->view.ev, ctx->stream) != hipSuccess) {
    (void)hipGetLastError(); (void)hipStreamSynchronize(ctx->stream); return;    // nothing was swapped: main and the patch go on answering
  }
  v.rewrite_inflight = true; v.rewrite_nz = nz;
}
void view_after_query(bmx_ctx* ctx, Index* ix) {         // behind the answer of an ordered query
  if (!ix->view.rewrite_due) return;
  const auto t0 = std::chrono::steady_clock::now();
  if (ix->view.ord_fits32) start_rewrite<int32_t>(ctx, *ix); else start_rewrite<int64_t>(ctx, *ix);
  if (ctx->view.debug) std::fprintf(stderr, "bmx: rewrite enqueued in %.1f us\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
}

// Patch the view of `ix` with the change run k_ix_update captured (c changed rows: ix.view.cl2_pos / cl2_old) and the rows appended at positions [n0, n0 + added).
// 0 = the (logical) view equals a fresh sort of the columns again; 1 = it could not be patched (no memory, or a deleted key was not where it should be): the caller
// leaves it stale and the next queries scan / re-sort as ever. Synchronous at its end (one or two words come back).
//   1. the run's deleted keys (old value, position) and inserted keys (value, position) are sorted;
//   2. they join the view's PENDING patch (pd, pi): a deleted key that is a pending inserted key cancels it, the others are deleted keys of main; the inserted keys are
//      merged into pi. All on runs of a few million keys: L2 / Infinity-Cache traffic;
//   3. once the pending patch holds more than ord_n / 16 keys, main is rewritten BEHIND the answer of the query that brought the refresh about: one streaming pass,
//      main - pd + pi (start_rewrite / finish_rewrite). Only a run of more than ord_n / 4 keys is merged into main at once, in front of the answer.
// A 1M-delta merge into a 10^8-row index: steps 1-2 on every refresh, step 3 behind every fourth; into a 10^7-row index: step 3 behind every answer.
template <class T>
int patch_view_t(bmx_ctx* ctx, Index& ix, uint64_t c, uint64_t n0, uint64_t added) {
  const auto t0 = std::chrono::steady_clock::now();
  OrderedView& v = ix.view;
  if (ctx->view.test_fail == 1) return 1;
  finish_rewrite(ctx, v, /*wait=*/true);            // a rewrite still in flight is looked at first: the change run's keys are keys of the view as it is NOW
  const uint64_t m = c + added, ktot = c + m, nx = v.ord_n;
  if (nx + m >= 0xFFFFFFFFull || ktot >= 0xFFFFFFFFull) return 1;
  auto soft = [&](int line) {
    if (ctx->view.debug) std::fprintf(stderr, "bmx: view patch of field %u gave up (bmx_view.inc:%d): %s\n", ix.field, line, ctx->err.c_str());
    g_err.clear(); ctx->err.clear(); (void)hipGetLastError(); return 1;
  };
  const uint64_t thr = std::max<uint64_t>(nx / 16, 1u << 16);                 // a pending patch beyond this many keys makes a rewrite of main due (behind the answer)
  const uint64_t thr_direct = std::max<uint64_t>(nx / 4, 1u << 16);          // a run beyond this many keys is merged into main at once, in front of the answer
  const uint32_t ntiles_main = (uint32_t)((nx + VIEW_TILE - 1) / VIEW_TILE);
  if (!ensure_hres(ctx) || ensure_view_scratch(ctx, ktot, std::max<uint64_t>(ntiles_main, (v.npi + v.npd + VIEW_TILE) / VIEW_TILE + 2))) return soft(__LINE__);
  hipStream_t st = ctx->stream;
  T* kv[2] = {static_cast<T*>(ctx->view.vk_v[0]), static_cast<T*>(ctx->view.vk_v[1])};
  uint32_t* kp[2] = {ctx->view.vk_p[0], ctx->view.vk_p[1]};
  const T* col = sizeof(T) == 4 ? reinterpret_cast<const T*>(ix.v32) : reinterpret_cast<const T*>(ix.v64);
  hipLaunchKernelGGL((k_view_keys<T>), dim3((uint32_t)std::min<uint64_t>((ktot + 255) / 256, 4096)), dim3(256), 0, st, (const uint32_t*)v.cl2_pos, (const int64_t*)v.cl2_old, (uint32_t)c, col,
                     (uint32_t)n0, (uint32_t)added, kv[0], kp[0]);
  // 1. sort the deleted keys [0, c) and the inserted keys [c, c + m): tiles in LDS, then merge-path passes
  const int cur = sort_view_keys<T>(st, kv[0], kp[0], kv, kp, c, m, 1);
  const T* Dv = kv[cur]; const uint32_t* Dp = kp[cur]; const T* Iv = kv[cur] + c; const uint32_t* Ip = kp[cur] + c;
  (void)hipMemsetAsync(&ctx->ds->view_err, 0, sizeof(uint32_t), st);
  ViewRun<T> X{static_cast<T*>(v.s_val), v.s_pos, v.s_ids};
  auto finish = [&]() -> int {       // the error word comes back; 0 = everything enqueued above did what it should
    hipError_t e = hipGetLastError();
    ctx->host.hres[HRES_ERR] = 1;
    if (e == hipSuccess) e = hipMemcpyAsync(const_cast<unsigned long long*>(&ctx->host.hres[HRES_ERR]), &ctx->ds->view_err, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return (e != hipSuccess || (uint32_t)ctx->host.hres[HRES_ERR]) ? 1 : 0;
  };
  auto rewrite_main = [&](const T* dv, const uint32_t* dp, uint64_t nd, const T* yv, const uint32_t* yp, uint64_t ny) -> bool {   // step 3
    const uint64_t nz = nx - nd + ny;
    if (!ensure_view_spare<T>(ctx, v, nz)) return false;
    ViewRun<T> Z{static_cast<T*>(v.s_val2), v.s_pos2, v.s_ids2};
    launch_run_merge<T, true>(ctx, X, nx, dv, dp, nd, yv, yp, ny, (const uint64_t*)ix.ids, Z);
    if (finish()) return false;
    take_spare(v, nz);                                                  // (the pending patch is empty on this path)
    return true;
  };
  const bool have = v.npd + v.npi > 0;
  if (!ctx->view.pending || (!have && ktot > thr_direct)) {
    // the run is a large part of the view (joining it to a patch would cost what the rewrite costs), or the pending patch is switched off (BMX_VIEW_PENDING=0).
    // A run between thr and thr_direct keys joins the (empty) patch and makes the rewrite due at once: the same work, but BEHIND the answer
    if (have) return soft(__LINE__);
    if (c > nx || !rewrite_main(Dv, Dp, c, Iv, Ip, m)) return soft(__LINE__);
  } else {
    // room for the patch at its largest (a rewrite falls due beyond thr keys; the run that crosses the line is still taken in), allocated once: a growing
    // buffer would put its reallocation in front of some query's answer
    if (ensure_pending<T>(ctx, v, std::max<uint64_t>(std::max<uint64_t>(v.npd + c, v.npi + m), thr + 2 * std::max<uint64_t>(c, m)))) return soft(__LINE__);
    (void)ensure_rewrite_report(ctx->view);
    if (!v.s_val2 && !ensure_view_spare<T>(ctx, v, nx + thr + 2 * m)) return soft(__LINE__);     // (the rewrite's target, also allocated now rather than in front of a later answer)
    T* pdv[2] = {static_cast<T*>(v.pd_v[0]), static_cast<T*>(v.pd_v[1])}; T* piv[2] = {static_cast<T*>(v.pi_v[0]), static_cast<T*>(v.pi_v[1])};
    auto merge2 = [&](bool ids, ViewRun<T> A, uint64_t la, const T* bv, const uint32_t* bp, uint64_t lb, ViewRun<T> Z) {
      if (la + lb == 0) return;
      const uint32_t g = (uint32_t)((la + lb + VIEW_PASS_KEYS - 1) / VIEW_PASS_KEYS);
      if (ids) hipLaunchKernelGGL((k_view_merge2<T, true>), dim3(g), dim3(256), 0, st, A, (uint32_t)la, bv, bp, (uint32_t)lb, (const uint64_t*)ix.ids, Z);
      else hipLaunchKernelGGL((k_view_merge2<T, false>), dim3(g), dim3(256), 0, st, A, (uint32_t)la, bv, bp, (uint32_t)lb, (const uint64_t*)nullptr, Z);
    };
    if (!have) {
      const int dc = v.pcur, ic = v.icur;
      (void)hipMemcpyAsync(pdv[dc], Dv, c * sizeof(T), hipMemcpyDeviceToDevice, st); (void)hipMemcpyAsync(v.pd_p[dc], Dp, c * 4, hipMemcpyDeviceToDevice, st);
      ViewRun<T> none{nullptr, nullptr, nullptr}, Zi{piv[ic], v.pi_p[ic], v.pi_ids[ic]};
      merge2(true, none, 0, Iv, Ip, m, Zi);                             // (the inserted keys with their ids)
      if (hipGetLastError() != hipSuccess) return soft(__LINE__);       // (nothing here raises the error word, and everything that reads the patch is behind it on this stream: no synchronisation)
      v.npd = c; v.npi = m;
    } else {
      // 2. which deleted keys are pending inserted keys (they cancel), which are keys of main (they join pd)? one flag per key, two ordered selects by flag
      T* sel_v = kv[cur ^ 1]; uint32_t* sel_p = kp[cur ^ 1];              // the sort's other buffer: [0, c) keys of main, [c, 2c) pending inserted keys, behind them the flags
      uint8_t* flag = reinterpret_cast<uint8_t*>(sel_v + 2 * c);
      const int dc = v.pcur, ic = v.icur;
      unsigned long long hc[2] = {0, 0};
      if (c) {
        ctx->host.hres[HRES_SPLIT] = ctx->host.hres[HRES_SPLIT + 1] = ~0ull;
        (void)hipMemsetAsync(v.pi_dead, 0, v.npi, st);
        hipLaunchKernelGGL((k_view_flag_in<T>), dim3((uint32_t)((c + 255) / 256)), dim3(256), 0, st, Dv, Dp, (uint32_t)c, (const T*)piv[ic], (const uint32_t*)v.pi_p[ic], (uint32_t)v.npi, flag, v.pi_dead);
        SelGeom g = sel_geom<1>(c);
        for (uint32_t want = 0; want < 2; want++) {
          PredFlag PF{flag, want};
          EmitKeys<T> EK{Dv, Dp, sel_v + (want ? c : 0), sel_p + (want ? c : 0)};
          FinishCount FC{const_cast<unsigned long long*>(&ctx->host.hres[HRES_SPLIT + want])};
          hipLaunchKernelGGL((k_sel_count<PredFlag>), dim3(g.blocks), dim3(SEL_THREADS), 0, st, PF, c, g.tiles_per_block, ctx->scan.block_counts);
          hipLaunchKernelGGL((k_sel_write<PredFlag, EmitKeys<T>, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, st, PF, EK, FC, c, g.tiles_per_block, ctx->scan.block_counts);
        }
        if (hipStreamSynchronize(st) != hipSuccess) return soft(__LINE__);
        hc[0] = ctx->host.hres[HRES_SPLIT]; hc[1] = ctx->host.hres[HRES_SPLIT + 1];
        if (hc[0] + hc[1] != c || hc[1] > v.npi) return soft(__LINE__);
      }
      const uint64_t cX = hc[0], cI = hc[1];
      // pi' = pi - (deleted keys that were pending inserts) + inserted keys;  pd' = pd + (deleted keys of main): balanced two-run merges (k_view_merge2)
      int ia = ic; uint64_t na = v.npi;
      if (cI) {                                                           // the cancelled inserts leave pi: an ordered select into the other set
        PredFlag PN{(const uint8_t*)v.pi_dead, 0u};                           // (k_view_flag_in marked them while it looked the deleted keys up)
        EmitRun<T> ER{(const T*)piv[ic], (const uint32_t*)v.pi_p[ic], (const uint64_t*)v.pi_ids[ic], piv[ic ^ 1], v.pi_p[ic ^ 1], v.pi_ids[ic ^ 1]};
        FinishCount FC{&ctx->ds->view_tmp[0]};
        SelGeom g = sel_geom<1>(v.npi);
        hipLaunchKernelGGL((k_sel_count<PredFlag>), dim3(g.blocks), dim3(SEL_THREADS), 0, st, PN, v.npi, g.tiles_per_block, ctx->scan.block_counts);
        hipLaunchKernelGGL((k_sel_write<PredFlag, EmitRun<T>, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, st, PN, ER, FC, v.npi, g.tiles_per_block, ctx->scan.block_counts);
        ia = ic ^ 1; na = v.npi - cI;
      }
      ViewRun<T> Ai{piv[ia], v.pi_p[ia], v.pi_ids[ia]}, Zi{piv[ia ^ 1], v.pi_p[ia ^ 1], v.pi_ids[ia ^ 1]};
      if (m) merge2(true, Ai, na, Iv, Ip, m, Zi);
      ViewRun<T> Ad{pdv[dc], v.pd_p[dc], nullptr}, Zd{pdv[dc ^ 1], v.pd_p[dc ^ 1], nullptr};
      if (cX) merge2(false, Ad, v.npd, (const T*)sel_v, (const uint32_t*)sel_p, cX, Zd);
      if (hipGetLastError() != hipSuccess) return soft(__LINE__);       // (nothing here raises the error word, and everything that reads the patch is behind it on this stream: no synchronisation)
      v.icur = m ? ia ^ 1 : ia; if (cX) v.pcur = dc ^ 1;
      v.npd += cX; v.npi = na + m;
    }
    // 3. the pending patch has grown: main will be rewritten BEHIND the answer of the query that brought this refresh about (view_after_query), not in front of it
    if (v.npd + v.npi > thr) v.rewrite_due = true;
  }
  v.ord_patches++; v.ord_patched_keys += ktot;
  v.last_patch_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// ---- the ordered queries ----
// the query itself: two searches + one contiguous copy; lo/hi are already clamped like the scans' (tombstones sort in front of every legal value)
template <bool POS, class OutT, class T>
void launch_ordered_t(bmx_ctx* ctx, const OrderedView& v, T l, T h, OutT* d_out, uint64_t d_cap, unsigned long long* d_n, const PredFilter* filter) {
  unsigned long long* ab = ctx->ds->ord_ab;
  const T* sv = static_cast<const T*>(v.s_val);
  const bool pending = v.npd + v.npi > 0;           // the logical view = main - pd + pi (patch_view_t)
  const int q = v.pcur, qi = v.icur;
  const T* dv = static_cast<const T*>(v.pd_v[q]); const T* iv = static_cast<const T*>(v.pi_v[qi]);
  if (pending) hipLaunchKernelGGL((k_ordered_bounds_p<T>), dim3(1), dim3(384), 0, ctx->stream, sv, v.ord_n, dv, v.npd, iv, v.npi, l, h, ab, d_n, filter ? 1u : 0u);
  else hipLaunchKernelGGL((k_ordered_bounds<T>), dim3(1), dim3(128), 0, ctx->stream, sv, v.ord_n, l, h, ab, d_n, filter ? 1u : 0u);
  if (filter) {             // every candidate of the run is looked at whatever the caller can take: the count is the number of survivors
    if constexpr (!POS) {
      const uint32_t fb = (uint32_t)std::min<uint64_t>((v.ord_n + v.npi + 2047) / 2048, 4096);
      if (pending) hipLaunchKernelGGL((k_ordered_filter_p<T, PredFilter>), dim3(fb), dim3(256), 0, ctx->stream, sv, (const uint32_t*)v.s_pos, (const uint64_t*)v.s_ids, dv, (const uint32_t*)v.pd_p[q],
                                      (const uint64_t*)v.pi_ids[qi], (const unsigned long long*)ab, *filter, d_out, d_out ? d_cap : 0, d_n);
      else hipLaunchKernelGGL((k_ordered_filter<PredFilter>), dim3(fb), dim3(256), 0, ctx->stream, (const uint64_t*)v.s_ids, (const unsigned long long*)ab, *filter, d_out, d_out ? d_cap : 0, d_n);
    }
    return;
  }
  if (!d_out || !d_cap) return;
  // the match count is the device's: a grid for the most the caller can take, whose workgroups beyond the matches leave at once
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((std::min<uint64_t>(d_cap, v.ord_n + v.npi) + 2047) / 2048, 8192);
  if (pending) {
    if constexpr (POS) hipLaunchKernelGGL((k_ordered_copy_p<T, uint32_t>), dim3(blocks), dim3(256), 0, ctx->stream, sv, (const uint32_t*)v.s_pos, (const uint32_t*)v.s_pos, dv, (const uint32_t*)v.pd_p[q],
                                          (const uint32_t*)v.pi_p[qi], (const unsigned long long*)ab, d_out, d_cap);
    else hipLaunchKernelGGL((k_ordered_copy_p<T, uint64_t>), dim3(blocks), dim3(256), 0, ctx->stream, sv, (const uint32_t*)v.s_pos, (const uint64_t*)v.s_ids, dv, (const uint32_t*)v.pd_p[q],
                            (const uint64_t*)v.pi_ids[qi], (const unsigned long long*)ab, d_out, d_cap);
  } else {
    if constexpr (POS) hipLaunchKernelGGL((k_ordered_copy<uint32_t>), dim3(blocks), dim3(256), 0, ctx->stream, (const uint32_t*)v.s_pos, (const unsigned long long*)ab, d_out, d_cap);
    else hipLaunchKernelGGL((k_ordered_copy<uint64_t>), dim3(blocks), dim3(256), 0, ctx->stream, (const uint64_t*)v.s_ids, (const unsigned long long*)ab, d_out, d_cap);
  }
}
template <bool POS, class OutT>
void launch_ordered(bmx_ctx* ctx, const Index* ix, int64_t lo, int64_t hi, OutT* d_out, uint64_t d_cap, unsigned long long* d_n, const PredFilter* filter = nullptr) {
  if (filter && !d_n) d_n = &ctx->ds->n_out;       // (the filter appends through a counter even when nobody asked for the count)
  const OrderedView& v = ix->view;
  if (v.ord_fits32) {     // the view was sorted from the 4-byte column: bounds clamped into int32 like the scans' (an empty range stays empty)
    const Range32 r = clamp_i32(lo, hi);
    launch_ordered_t<POS, OutT, int32_t>(ctx, v, (int32_t)r.lo, (int32_t)r.hi, d_out, d_cap, d_n, filter);
  } else launch_ordered_t<POS, OutT, int64_t>(ctx, v, lo, hi, d_out, d_cap, d_n, filter);
}

}  // namespace
