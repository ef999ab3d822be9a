// bmx_exchange.inc — the exchange between contexts and processes (bmx.h "partition", "direct exchange", "sequence words"): partition by owner into records or slabs,
// IPC-mapped memory, the sequence-word signals and waits, and the slab protocol's hooks into the merge. Included by bmx.hip (one translation unit), which keeps
// the state (PartScratch, SlabProtocol); the merge reads SlabProtocol in bmx_merge.inc.
namespace {

int partition_impl(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val,
                   uint32_t nshards, uint64_t slab, bmx_delta_rec* recs_out, uint64_t* counts_out_dev, const PartOut* split = nullptr, uint32_t aux_base = 0) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (nshards == 0 || nshards > PART_MAX_SHARDS || n > 0xFFFFFFFFull || !counts_out_dev || slab * nshards > 0xFFFFFFFFull)
    return fail(ctx, BMX_ERR_INVALID, "bad arguments (1..16 shards)");
  if (n && (!id || !field || !ts || !val || (!recs_out && !split))) return fail(ctx, BMX_ERR_INVALID, "null pointer");
  PartOut po;
  if (split) po = *split; else std::memset(&po, 0, sizeof(po));
  po.split = split ? 1u : 0u; po.aux_base = aux_base;
  if (int erc = enter(ctx)) return erc;
  uint32_t per_block = (uint32_t)((n + PART_BLOCKS - 1) / PART_BLOCKS);
  per_block = std::max<uint32_t>(PART_TILE, (per_block + PART_TILE - 1) / PART_TILE * PART_TILE);
  if (n > ctx->part.owner_cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->part.owner_cap = 0;
    int rc = dev_alloc(ctx, &ctx->part.owner, n + 256);
    if (rc) return rc;
    ctx->part.owner_cap = n;
  }
  hipLaunchKernelGGL(k_part_count, dim3(PART_BLOCKS), dim3(256), 0, ctx->stream, id, (uint32_t)n, nshards, per_block, ctx->part.counts, ctx->part.owner);
  LAUNCHCHK("k_part_count");
  hipLaunchKernelGGL(k_part_scatter, dim3(PART_BLOCKS), dim3(256), 0, ctx->stream, id, field, ts, val, (const uint8_t*)ctx->part.owner, (uint32_t)n, nshards, per_block, ctx->part.counts,
                     recs_out, reinterpret_cast<unsigned long long*>(counts_out_dev), (uint32_t)slab, &ctx->ds->status, po);
  LAUNCHCHK("k_part_scatter");
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_partition_by_owner(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val,
                           uint32_t nshards, bmx_delta_rec* recs_out, uint64_t* counts_out_dev) {
  return partition_impl(ctx, n, id, field, ts, val, nshards, 0, recs_out, counts_out_dev);
}

int bmx_partition_by_owner_slabs(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val,
                                 uint32_t nshards, uint64_t slab_records, bmx_delta_rec* recs_out, uint64_t* counts_out_dev) {
  if (slab_records == 0) return fail(ctx, BMX_ERR_INVALID, "slab_records must be > 0");
  return partition_impl(ctx, n, id, field, ts, val, nshards, slab_records, recs_out, counts_out_dev);
}

/* ---- direct exchange between processes (one process per GPU): IPC-mapped receive slabs, arrival words, no collective on the data path ---- */
int bmx_ipc_alloc(bmx_ctx* ctx, uint64_t bytes, uint32_t flags, void** dev_ptr, uint8_t handle_out[64]) {
  if (!ctx || !dev_ptr || !handle_out || bytes == 0) return fail(ctx, BMX_ERR_INVALID, "bmx_ipc_alloc: bad arguments");
  static_assert(sizeof(hipIpcMemHandle_t) <= 64, "IPC handle fits the 64-byte carrier");
  if (int erc = enter(ctx)) return erc;
  void* p = nullptr;
  // BMX_IPC_UNCACHED: memory other GPUs store into while kernels here poll or read it must not be served from this GPU's L2 (a line cached
  // before the peer's store would stay stale: the L2 is only coherent for this GPU's own writes)
  hipError_t e = (flags & BMX_IPC_UNCACHED) ? hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached) : hipMalloc(&p, bytes);
  if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? BMX_ERR_NOMEM : BMX_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  e = hipMemset(p, 0, bytes);
  hipIpcMemHandle_t h;
  if (e == hipSuccess) e = hipIpcGetMemHandle(&h, p);
  if (e != hipSuccess) { (void)hipFree(p); return fail_hip(ctx, e, "hipIpcGetMemHandle"); }
  std::memset(handle_out, 0, 64);
  std::memcpy(handle_out, &h, sizeof(h));
  *dev_ptr = p;
  return BMX_OK;
}
int bmx_ipc_open(bmx_ctx* ctx, const uint8_t handle[64], int peer_device, void** dev_ptr) {
  if (!ctx || !handle || !dev_ptr) return fail(ctx, BMX_ERR_INVALID, "bmx_ipc_open: bad arguments");
  if (int erc = enter(ctx)) return erc;
  if (peer_device >= 0 && peer_device != ctx->device) {       // peer access first: the mapping below is only usable from this GPU with it
    int can = 0;
    HIPCHK(hipDeviceCanAccessPeer(&can, ctx->device, peer_device));
    if (!can) return fail(ctx, BMX_ERR_HIP, "bmx_ipc_open: no peer access between the two GPUs");
    hipError_t pe = hipDeviceEnablePeerAccess(peer_device, 0);
    if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) return fail_hip(ctx, pe, "hipDeviceEnablePeerAccess");
    (void)hipGetLastError();
  }
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle, sizeof(h));
  void* p = nullptr;
  HIPCHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  *dev_ptr = p;
  return BMX_OK;
}
int bmx_ipc_close(bmx_ctx* ctx, void* dev_ptr) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (!dev_ptr) return BMX_OK;
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipIpcCloseMemHandle(dev_ptr));
  return BMX_OK;
}
int bmx_ipc_free(bmx_ctx* ctx, void* dev_ptr) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (!dev_ptr) return BMX_OK;
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipFree(dev_ptr));
  return BMX_OK;
}

int bmx_partition_scatter(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val,
                          uint32_t nshards, uint64_t slab_records, void* const* dst, uint64_t* counts_out_dev, uint64_t* const* arrive_words, uint64_t arrive_value,
                          const uint64_t* wait_words_dev, uint32_t n_wait, uint64_t wait_at_least) {
  if (!ctx || !dst || slab_records == 0 || nshards == 0 || nshards > PART_MAX_SHARDS) return fail(ctx, BMX_ERR_INVALID, "bmx_partition_scatter: bad arguments (1..16 shards, slab_records > 0)");
  // A/B switch, OFF by default: BMX_PART_WAIT_FOLD=1 folds the wait into the scatter pass (every workgroup polls before its first store) instead of a one-wave launch in
  // front of the count pass. Measured (profiles/r05_sharded_ab.log): 95.0 / 96.9 against 102.1 / 96.4 us per step — inside the run-to-run spread — and one run with the
  // deferred compaction beside it took 75 ms per step: 1024 spinning workgroups hold the LDS and wave slots the kernel that frees the slabs needs. A one-wave wait cannot do that.
  static const bool fold_wait = [] { const char* v = std::getenv("BMX_PART_WAIT_FOLD"); return v && v[0] == '1' && !v[1]; }();
  if (wait_words_dev && n_wait && (!fold_wait || n_wait > 64)) { int wrc = bmx_seq_wait_all(ctx, nullptr, wait_words_dev, n_wait, wait_at_least); if (wrc) return wrc; }
  PartOut po; std::memset(&po, 0, sizeof(po));
  if (wait_words_dev && n_wait && fold_wait && n_wait <= 64) {
    po.wait_words = reinterpret_cast<const unsigned long long*>(wait_words_dev); po.n_wait = n_wait; po.wait_at_least = wait_at_least; po.wait_diag = ctx->ds->seq_diag;
  }
  for (uint32_t g = 0; g < nshards; g++) {
    if (!dst[g]) return fail(ctx, BMX_ERR_INVALID, "bmx_partition_scatter: null destination slab");
    po.base[g] = static_cast<bmx_delta_rec*>(dst[g]);
  }
  int rc = partition_impl(ctx, n, id, field, ts, val, nshards, slab_records, nullptr, counts_out_dev, &po, 0);
  if (rc || !arrive_words) return rc;
  // the arrival words, from a launch of their own behind the scatter: its kernel boundary is the release (every record is stored and written
  // back, peer memory included) — fences inside the scatter's 1024 workgroups write the whole L2 back a thousand times (measured: +100 us)
  SeqPtrs w; std::memset(&w, 0, sizeof(w));
  for (uint32_t g = 0; g < nshards; g++) w.p[g] = reinterpret_cast<unsigned long long*>(arrive_words[g]);
  hipLaunchKernelGGL(k_seq_signal_multi, dim3(1), dim3(64), 0, ctx->stream, w, nshards, (unsigned long long)arrive_value);
  LAUNCHCHK("k_seq_signal_multi");
  return BMX_OK;
}

int bmx_seq_signal(bmx_ctx* ctx, void* hip_stream, uint64_t* seq_dev, uint64_t value) {
  if (!ctx || !seq_dev) return fail(ctx, BMX_ERR_INVALID, "bmx_seq_signal: null context or sequence word");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->stream;
  // a signal on the context's own stream says "every merge enqueued before this is done, outputs included": a compaction that is only recorded
  // (or still on the side stream) is ordered in front of it (ADVICE r4: a consumer stream woken by the word read a stale n_applied)
  if (st == ctx->stream) { if (int frc = flush_pending(ctx)) return frc; }
  hipLaunchKernelGGL(k_seq_signal, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long*>(seq_dev), (unsigned long long)value);
  LAUNCHCHK("k_seq_signal");
  return BMX_OK;
}

int bmx_seq_wait(bmx_ctx* ctx, void* hip_stream, const uint64_t* seq_dev, uint64_t at_least) {
  if (!ctx || !seq_dev) return fail(ctx, BMX_ERR_INVALID, "bmx_seq_wait: null context or sequence word");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->stream;
  hipLaunchKernelGGL(k_seq_wait, dim3(1), dim3(64), 0, st, reinterpret_cast<const unsigned long long*>(seq_dev), (unsigned long long)at_least,
                     &ctx->ds->status, ctx->ds->seq_diag);
  LAUNCHCHK("k_seq_wait");
  return BMX_OK;
}

int bmx_seq_wait_all(bmx_ctx* ctx, void* hip_stream, const uint64_t* words_dev, uint32_t nwords, uint64_t at_least) {
  if (!ctx || !words_dev || nwords == 0 || nwords > 64) return fail(ctx, BMX_ERR_INVALID, "bmx_seq_wait_all: 1..64 words");
  HIPCHK(hipSetDevice(ctx->device));      // (no flush: a wait in front of the next merge must not pull the recorded compaction onto this stream)
  hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->stream;
  hipLaunchKernelGGL(k_seq_wait_all, dim3(1), dim3(64), 0, st, reinterpret_cast<const unsigned long long*>(words_dev), nwords, (unsigned long long)at_least,
                     &ctx->ds->status, ctx->ds->seq_diag);
  LAUNCHCHK("k_seq_wait_all");
  return BMX_OK;
}

int bmx_merge_tail_wait(bmx_ctx* ctx, const uint64_t* words_dev, uint32_t nwords, uint64_t at_least) {
  if (!ctx || nwords > 64 || (nwords && !words_dev)) return fail(ctx, BMX_ERR_INVALID, "bmx_merge_tail_wait: at most 64 words");
  ctx->slab.tail_armed.words = reinterpret_cast<const unsigned long long*>(words_dev); ctx->slab.tail_armed.n = nwords; ctx->slab.tail_armed.at_least = at_least;
  return BMX_OK;
}

int bmx_merge_notify(bmx_ctx* ctx, uint64_t* const* words, uint32_t nwords) {
  if (!ctx || nwords > PART_MAX_SHARDS || (nwords && !words)) return fail(ctx, BMX_ERR_INVALID, "bmx_merge_notify: at most 16 words");
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::memset(&ctx->slab.notify, 0, sizeof(ctx->slab.notify));
  for (uint32_t k = 0; k < nwords; k++) ctx->slab.notify.p[k] = reinterpret_cast<unsigned long long*>(words[k]);
  ctx->slab.n_notify = nwords; ctx->slab.notify_seq = 0;
  return BMX_OK;
}

int bmx_merge_records_after(bmx_ctx* ctx, const uint64_t* wait_words_dev, uint32_t n_wait, uint64_t wait_at_least, uint64_t n, const bmx_delta_rec* recs,
                            int insert_mode, uint32_t* applied_idx, uint64_t* n_applied, uint8_t* flags, bmx_merge_stats* stats) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  SlabProtocol& sp = ctx->slab;
  if (wait_words_dev && n_wait) {
    const bool done = sp.tail_waited.n == n_wait && sp.tail_waited.words == reinterpret_cast<const unsigned long long*>(wait_words_dev) && sp.tail_waited.at_least >= wait_at_least;
    sp.tail_waited = SlabProtocol::TailWait{};
    if (!done) { int wrc = bmx_seq_wait_all(ctx, nullptr, wait_words_dev, n_wait, wait_at_least); if (wrc) return wrc; }   // (done: the resolve kernel of the merge before waited for exactly this)
  }
  sp.notify_armed = true;      // THIS merge reads a receive slab set: it (and no other merge of the context) tells the origins when the set is free again
  const int rc = bmx_merge_records(ctx, n, recs, insert_mode, applied_idx, n_applied, flags, stats);
  sp.notify_armed = false;
  return rc;
}

}  // extern "C"
