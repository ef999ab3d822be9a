// bmx_host.inc — the paths of BMX_MEM_HOST calls: copy streams, the two staging sets (bmx_merge_submit / bmx_merge_collect), the small-batch path through
// mapped host memory, merge_host, the mapped result words and the point reads' columns. Included by bmx.hip (one translation unit), which keeps their
// state (HostIO).
namespace {

int HostIO::create(bmx_ctx* ctx) {
  int rc;
  if ((rc = dev_alloc_all(ctx, {{stg[0].n_out, sizeof(unsigned long long)}, {stg[0].stats, sizeof(bmx_merge_stats)},
                                {stg[1].n_out, sizeof(unsigned long long)}, {stg[1].stats, sizeof(bmx_merge_stats)}})))
    return rc;
  for (Staging& S : stg) {
    HIPCHK(hipMemsetAsync(S.n_out, 0, sizeof(unsigned long long), ctx->stream));
    HIPCHK(hipMemsetAsync(S.stats, 0, sizeof(bmx_merge_stats), ctx->stream));
  }
  if (hipHostMalloc(reinterpret_cast<void**>(&tails), 2 * sizeof(SmallOut), hipHostMallocMapped) == hipSuccess) {
    std::memset(tails, 0, 2 * sizeof(SmallOut));
    for (int i = 0; i < 2; i++) stg[i].tail = tails + i;
  } else { tails = nullptr; (void)hipGetLastError(); }
  return BMX_OK;
}
void HostIO::release() {
  if (copy_stream) (void)hipStreamSynchronize(copy_stream);
  if (down_stream) (void)hipStreamSynchronize(down_stream);
  for (Staging& S : stg) {
    dev_free(S.id); dev_free(S.field); dev_free(S.ts); dev_free(S.val); dev_free(S.applied); dev_free(S.flags); dev_free(S.n_out); dev_free(S.stats);
    if (S.up) (void)hipEventDestroy(S.up);
    if (S.done) (void)hipEventDestroy(S.done);
    S.up = S.done = nullptr; S.tail = nullptr; S.cap = 0;
  }
  dev_free(pr_id); dev_free(pr_field); dev_free(pr_ts); dev_free(pr_val); dev_free(pr_found); pr_cap = 0;
  if (copy_stream) (void)hipStreamDestroy(copy_stream);
  if (down_stream) (void)hipStreamDestroy(down_stream);
  copy_stream = down_stream = nullptr;
  if (hres) (void)hipHostFree(const_cast<unsigned long long*>(hres));
  if (tails) (void)hipHostFree(tails);
  if (pin_in) (void)hipHostFree(pin_in);
  if (pin_out) (void)hipHostFree(pin_out);
  hres = nullptr; tails = nullptr; pin_in = pin_out = nullptr;
}

// The copy streams exist only once a host batch is submitted: HIP maps streams onto a few hardware queues, and a device-mode caller
// that overlaps its own streams (the sharded pipeline: exchange beside merge) must not find them sharing a queue with idle ones of ours
// (measured: with two extra streams per context the exchange kernel serialised behind the merge kernels, 164 vs 125 us per step).
// ensure_staging: the copy streams, and room for n deltas in staging set k
int ensure_staging(bmx_ctx* ctx, int k, uint64_t n) {
  if (!ctx->host.copy_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->host.copy_stream, hipStreamNonBlocking));
  if (!ctx->host.down_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->host.down_stream, hipStreamNonBlocking));
  HostIO::Staging& S = ctx->host.stg[k];
  if (n <= S.cap) return BMX_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->host.copy_stream));
  HIPCHK(hipStreamSynchronize(ctx->host.down_stream));
  uint64_t cap = std::max<uint64_t>(n, 1u << 16);
  cap = (cap + 255) & ~255ull;
  S.cap = 0;
  if (int rc = dev_alloc_all(ctx, {{S.id, cap * 8}, {S.field, cap * 4}, {S.ts, cap * 8}, {S.val, cap * 8}, {S.applied, cap * 4}, {S.flags, cap}})) return rc;
  S.cap = (uint32_t)cap;
  return BMX_OK;
}

// persistent device columns of the host-mode point reads and dumps
int ensure_point_read(bmx_ctx* ctx, uint64_t n) {
  HostIO& H = ctx->host;
  if (n <= H.pr_cap) return BMX_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  H.pr_cap = 0;
  const uint64_t cap = (std::max<uint64_t>(n + n / 4, 1u << 12) + 255) & ~255ull;
  if (int rc = dev_alloc_all(ctx, {{H.pr_id, cap * 8}, {H.pr_field, cap * 4}, {H.pr_ts, cap * 8}, {H.pr_val, cap * 8}, {H.pr_found, cap}})) return rc;
  H.pr_cap = cap;
  return BMX_OK;
}

// Host batches go through two staging sets. submit: upload on the copy stream, then the merge on the main stream behind an event;
// collect: results back on the copy stream once the batch's kernels are done. While the host uploads batch b+1 (a pageable
// hipMemcpyAsync keeps the calling thread busy for the whole transfer) the GPU merges batch b.
__global__ void k_noop() {}
__global__ void k_small_tail(const unsigned long long* n_applied, const bmx_merge_stats* stats, const uint32_t* status, SmallOut* out) {
  if (threadIdx.x == 0) { out->n_applied = *n_applied; out->stats = *stats; out->status = *status; }
}
int submit_host(bmx_ctx* ctx, const MergeIn& in, const MergeMode& mode, bool want_flags, uint64_t* ticket, bool inputs_free_on_return) {
  const uint64_t n = in.n;
  int k = -1;
  for (int i = 0; i < 2; i++) if (!ctx->host.stg[i].busy) { k = i; break; }
  if (k < 0) return fail(ctx, BMX_ERR_INVALID, "two batches are already in flight: collect the oldest first (bmx_merge_collect)");
  HostIO::Staging& S = ctx->host.stg[k];
  int rc = ensure_staging(ctx, k, n);
  if (rc) return rc;
  if (n) {
    HIPCHK(hipMemcpyAsync(S.id, in.id, n * 8, hipMemcpyHostToDevice, ctx->host.copy_stream));
    HIPCHK(hipMemcpyAsync(S.field, in.field, n * 4, hipMemcpyHostToDevice, ctx->host.copy_stream));
    HIPCHK(hipMemcpyAsync(S.ts, in.ts, n * 8, hipMemcpyHostToDevice, ctx->host.copy_stream));
    HIPCHK(hipMemcpyAsync(S.val, in.val, n * 8, hipMemcpyHostToDevice, ctx->host.copy_stream));
    HIPCHK(hipEventRecord(S.up, ctx->host.copy_stream));
    HIPCHK(hipStreamWaitEvent(ctx->stream, S.up, 0));
    // a copy from page-locked memory (bmx_host_alloc) is truly asynchronous: bmx_merge_submit promises that the arrays may be reused on return
    if (inputs_free_on_return) HIPCHK(hipEventSynchronize(S.up));
  }
  rc = merge_core(ctx, MergeIn{n, S.id, S.field, S.ts, S.val, nullptr}, MergeOut{S.applied, reinterpret_cast<uint64_t*>(S.n_out), want_flags ? S.flags : nullptr, S.stats}, mode);
  if (rc) return rc;
  if (S.tail) {
    hipLaunchKernelGGL(k_small_tail, dim3(1), dim3(64), 0, ctx->stream, (const unsigned long long*)S.n_out, (const bmx_merge_stats*)S.stats, (const uint32_t*)&ctx->ds->status, S.tail);
    LAUNCHCHK("k_small_tail");
  }
  HIPCHK(hipEventRecord(S.done, ctx->stream));
  S.n = n; S.want_flags = want_flags; S.busy = true; S.ticket = ctx->host.next_ticket++;
  *ticket = S.ticket;
  return BMX_OK;
}

int collect_host(bmx_ctx* ctx, uint64_t ticket, uint32_t* applied_idx, uint64_t* n_applied, uint8_t* flags, bmx_merge_stats* stats) {
  int k = -1;
  for (int i = 0; i < 2; i++) if (ctx->host.stg[i].busy && ctx->host.stg[i].ticket == ticket) k = i;
  if (k < 0) return fail(ctx, BMX_ERR_INVALID, "unknown or already collected ticket");
  if (ctx->host.stg[1 - k].busy && ctx->host.stg[1 - k].ticket < ticket) return fail(ctx, BMX_ERR_INVALID, "collect tickets in submission order");
  HostIO::Staging& S = ctx->host.stg[k];
  S.busy = false;
  bmx_merge_stats hs; std::memset(&hs, 0, sizeof(hs));
  uint32_t st = 0;
  if (S.tail) {                         // count, stats and status are in mapped host memory once the batch's last launch is done
    HIPCHK(hipEventSynchronize(S.done));
    hs = S.tail->stats; st = S.tail->status;
  } else {
    HIPCHK(hipStreamWaitEvent(ctx->host.down_stream, S.done, 0));
    HIPCHK(hipMemcpyAsync(&hs, S.stats, sizeof(hs), hipMemcpyDeviceToHost, ctx->host.down_stream));
    HIPCHK(hipMemcpyAsync(&st, &ctx->ds->status, sizeof(st), hipMemcpyDeviceToHost, ctx->host.down_stream));
    HIPCHK(hipStreamSynchronize(ctx->host.down_stream));
  }
  if (st) return check_status(ctx);     // sticky device error of this (or an earlier, uncollected) batch
  if (S.n == 0) std::memset(&hs, 0, sizeof(hs));
  if (applied_idx && hs.n_applied) HIPCHK(hipMemcpyAsync(applied_idx, S.applied, hs.n_applied * 4, hipMemcpyDeviceToHost, ctx->host.down_stream));
  if (flags && S.n && S.want_flags) HIPCHK(hipMemcpyAsync(flags, S.flags, S.n, hipMemcpyDeviceToHost, ctx->host.down_stream));
  HIPCHK(hipStreamSynchronize(ctx->host.down_stream));
  if (!ctx->host.stg[1 - k].busy && S.n) ctx->rows_ub = hs.n_rows;   // exact again once nothing else is in flight
  if (n_applied) *n_applied = hs.n_applied;
  if (stats) *stats = hs;
  return BMX_OK;
}

// Small host batch (the reference's sync chunks hold 50 entries, src/bullet-network-sync.js:18): the general path costs ~115 us per call whatever
// the size (four pageable uploads, two extra streams, three downloads); here the columns are packed into mapped host memory that the kernels read
// over PCIe, and winners, count, stats and the device status come back through mapped host memory as well.
constexpr uint64_t SMALL_HOST_N = 32768;
constexpr int SMALL_PATH_UNAVAILABLE = 1;
constexpr size_t SMALL_IN_BYTES = SMALL_HOST_N * 28, SMALL_OUT_APPLIED = 0, SMALL_OUT_FLAGS = SMALL_HOST_N * 4, SMALL_OUT_TAIL = SMALL_HOST_N * 5,
                 SMALL_OUT_BYTES = SMALL_OUT_TAIL + sizeof(SmallOut);
// result words in mapped host memory: a kernel's last workgroup (or one copy) writes them, the host reads them after the synchronisation it needs anyway
constexpr int HRES_TOTALS = 0 /* 2 per maintained index */, HRES_RUN = PART_MAX_SHARDS /* one per index */, HRES_ERR = HRES_RUN + PART_MAX_SHARDS / 2, HRES_SPLIT = HRES_ERR + 1 /* 2 */,
              HRES_SCAN_N = HRES_SPLIT + 2, HRES_WORDS = HRES_SCAN_N + 1;
bool ensure_hres(bmx_ctx* ctx) {
  if (ctx->host.hres) return true;
  void* p = nullptr;
  if (hipHostMalloc(&p, HRES_WORDS * sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return false; }
  std::memset(p, 0, HRES_WORDS * sizeof(unsigned long long));
  ctx->host.hres = static_cast<volatile unsigned long long*>(p);
  return true;
}
// a caller's host buffer that the device can write itself (bmx_host_alloc, hipHostMalloc, a registered range): its device address, or nullptr
void* mapped_host(void* p) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) return at.devicePointer;
  (void)hipGetLastError();
  return nullptr;
}
bool ensure_pinned(bmx_ctx* ctx) {   // the two mapped host buffers of the small-call paths (merge, point reads, scans); false = fall back to copies
  if (ctx->host.pin_in) return true;
  { const char* t = std::getenv("BMX_TEST_FAIL_PINNED"); if (t && t[0] == '1') return false; }   // test hook: as if the page-locked allocation had failed
  if (hipHostMalloc(reinterpret_cast<void**>(&ctx->host.pin_in), SMALL_IN_BYTES, hipHostMallocMapped) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&ctx->host.pin_out), SMALL_OUT_BYTES, hipHostMallocMapped) != hipSuccess) {
    (void)hipGetLastError();
    if (ctx->host.pin_in) { (void)hipHostFree(ctx->host.pin_in); ctx->host.pin_in = nullptr; }
    ctx->host.pin_out = nullptr;
    return false;
  }
  return true;
}
int merge_host_small(bmx_ctx* ctx, const MergeIn& in, const MergeMode& mode, const MergeOut& out) {
  if (!ensure_pinned(ctx)) return SMALL_PATH_UNAVAILABLE;
  const uint64_t n = in.n;
  // the previous small batch's kernels are done (every call ends with a synchronisation): the buffers are free
  uint64_t* p_id = reinterpret_cast<uint64_t*>(ctx->host.pin_in);
  int64_t* p_ts = reinterpret_cast<int64_t*>(ctx->host.pin_in + n * 8);
  int64_t* p_val = reinterpret_cast<int64_t*>(ctx->host.pin_in + n * 16);
  uint32_t* p_field = reinterpret_cast<uint32_t*>(ctx->host.pin_in + n * 24);
  std::memcpy(p_id, in.id, n * 8); std::memcpy(p_ts, in.ts, n * 8); std::memcpy(p_val, in.val, n * 8); std::memcpy(p_field, in.field, n * 4);
  uint32_t* o_applied = reinterpret_cast<uint32_t*>(ctx->host.pin_out + SMALL_OUT_APPLIED);
  uint8_t* o_flags = ctx->host.pin_out + SMALL_OUT_FLAGS;
  SmallOut* o_tail = reinterpret_cast<SmallOut*>(ctx->host.pin_out + SMALL_OUT_TAIL);
  // count and stats go through device scalars first (the merge's last workgroup read-modify-writes them), then one thread copies them out
  int rc = merge_core(ctx, MergeIn{n, p_id, p_field, p_ts, p_val, nullptr},
                      MergeOut{out.applied_idx ? o_applied : nullptr, reinterpret_cast<uint64_t*>(&ctx->ds->n_out), out.flags ? o_flags : nullptr, &ctx->ds->stats}, mode);
  if (rc) return rc;
  hipLaunchKernelGGL(k_small_tail, dim3(1), dim3(64), 0, ctx->stream, (const unsigned long long*)&ctx->ds->n_out, (const bmx_merge_stats*)&ctx->ds->stats,
                     (const uint32_t*)&ctx->ds->status, o_tail);
  LAUNCHCHK("k_small_tail");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (o_tail->status) return check_status(ctx);
  const bmx_merge_stats hs = o_tail->stats;
  if (out.applied_idx && hs.n_applied) std::memcpy(out.applied_idx, o_applied, hs.n_applied * 4);
  if (out.flags) std::memcpy(out.flags, o_flags, n);
  ctx->rows_ub = hs.n_rows; ctx->inflight.clear();
  if (out.n_applied) *out.n_applied = hs.n_applied;
  if (out.stats) *out.stats = hs;
  return BMX_OK;
}

int merge_host(bmx_ctx* ctx, const MergeIn& in, const MergeMode& mode, const MergeOut& out) {
  for (int i = 0; i < 2; i++)
    if (ctx->host.stg[i].busy) return fail(ctx, BMX_ERR_INVALID, "a submitted batch is still in flight: collect it before a synchronous merge");
  if (in.n && in.n <= SMALL_HOST_N) {
    int src = merge_host_small(ctx, in, mode, out);
    if (src != SMALL_PATH_UNAVAILABLE) return src;
  }
  uint64_t ticket = 0;
  int rc = submit_host(ctx, in, mode, out.flags != nullptr, &ticket, false);   // collect_host waits for the whole batch
  if (rc) return rc;
  return collect_host(ctx, ticket, out.applied_idx, out.n_applied, out.flags, out.stats);
}

}  // namespace
