// bmx_merge.inc — the host side of the merge: workspace and table (MergeWs::ensure, alloc_table_tuned, grow_table), the row-count bound, the deferred compaction, merge_core
// as a list of named steps, the row loads. Included by bmx.hip (one translation unit), which keeps its state (MergeWs, Deferral, bmx_ctx), where this code always sat: the
// code object lays kernel templates out in the order the source first uses them (bmx.hip, the include list).
namespace {

int refresh_rows(bmx_ctx* ctx) {
  unsigned long long r = 0;
  if (ctx->host_rows && ctx->batch_seq > 0) {      // every change of the row count went through a merge, whose last workgroup mirrored it to the host
    HIPCHK(hipStreamSynchronize(ctx->stream));
    r = __atomic_load_n(ctx->host_rows, __ATOMIC_ACQUIRE);
  } else {
    HIPCHK(hipMemcpyAsync(&r, &ctx->ds->row_count, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  ctx->rows_ub = r;
  ctx->inflight.clear();
  return BMX_OK;
}

// rows_ub from the mirror the merges write, no sync: rows the host has seen + every delta of the batches enqueued after that one
void tighten_rows_ub(bmx_ctx* ctx) {
  if (!ctx->host_rows) return;
  const uint64_t seen_seq = __atomic_load_n(ctx->host_rows + 1, __ATOMIC_ACQUIRE);
  const uint64_t seen_rows = __atomic_load_n(ctx->host_rows, __ATOMIC_RELAXED);   // this count, or a later one: still an upper bound with the sum below
  if (seen_seq == 0) return;
  while (!ctx->inflight.empty() && ctx->inflight.front().first <= seen_seq) ctx->inflight.pop_front();
  uint64_t pending = 0;
  for (const auto& b : ctx->inflight) pending += b.second;
  ctx->rows_ub = std::min<uint64_t>(ctx->rows_ub, seen_rows + pending);
}

int flush_pending(bmx_ctx* ctx);
// (merge_core's capacity guard) Blocks the CALLER, not the device: until the row reports of enough batches in flight have arrived for the bound to clear,
// or none is left. A report that does not come within two seconds (a wedged queue) leaves the decision to the synchronising path.
int wait_for_row_reports(bmx_ctx* ctx, uint64_t n) {
  if (!ctx->host_rows) return BMX_OK;
  const auto t0 = std::chrono::steady_clock::now();
  while ((ctx->rows_ub + n >= ctx->nslots || ctx->rows_ub > ctx->capacity_rows) && !ctx->inflight.empty()) {
    if (ctx->inflight.size() == 1 && ctx->defer.pend.on) { if (int frc = flush_pending(ctx)) return frc; }   // the only report outstanding is that of a compaction not launched yet
    const uint64_t want = ctx->inflight.front().first;
    uint32_t spins = 0;
    while (__atomic_load_n(ctx->host_rows + 1, __ATOMIC_ACQUIRE) < want) {
      if ((++spins & 1023u) == 0) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) return BMX_OK;
        std::this_thread::yield();
      }
    }
    tighten_rows_ub(ctx);
    ctx->n_row_waits++;
  }
  return BMX_OK;
}
int MergeWs::ensure(bmx_ctx* ctx, uint64_t n) {
  if (n <= cap) return BMX_OK;
  if (int frc = flush_pending(ctx)) return frc;      // a compaction not launched yet reads the workspace this call frees
  HIPCHK(hipStreamSynchronize(ctx->stream));
  uint64_t c = std::max<uint64_t>(n, std::min<uint64_t>((uint64_t)cap * 2, MAX_BATCH));
  c = std::max<uint64_t>(c, 1u << 16);
  c = (c + 255) & ~255ull;
  const uint64_t half = (c / 256 + 16 + 3) & ~3ull;   // a multiple of four entries: every segment stays 16-byte aligned for the compaction's wide loads
  cap = 0;
  if (int rc = dev_alloc_all(ctx, {{next, c * 4}, {wflag[0], c + 16}, {slot_of[0], c * 4}, {fld[0], c * 4}, {wflag[1], c + 16}, {slot_of[1], c * 4}, {fld[1], c * 4},
                                   {wflag[2], c + 16}, {slot_of[2], c * 4}, {fld[2], c * 4}, {blk_info, BLK_SEGS * half * 4}, {blk_follow, (c / 256 + 16) * 4}}))
    return rc;
  HIPCHK(hipMemsetAsync(next, 0, c * sizeof(uint32_t), ctx->stream));
  HIPCHK(hipMemsetAsync(blk_follow, 0, (c / 256 + 16) * sizeof(uint32_t), ctx->stream));
  blk_half = (uint32_t)half;
  HIPCHK(hipMemsetAsync(blk_info, 0, BLK_SEGS * (size_t)blk_half * sizeof(uint32_t), ctx->stream));
  for (uint32_t h = 0; h < BLK_SEGS; h++) blk_clean[h] = true;
  cap = (uint32_t)c;
  return BMX_OK;
}

// Slots of a table that holds `capacity_rows` rows at load factor <= load_pct %. 0 = does not fit the 32-bit slot indices the
// per-delta workspace (slot_of[]) carries: 2^32 slots x 32 B = 137 GB would fit the 288 GB of HBM, so it is refused explicitly.
uint64_t slots_for(uint64_t capacity_rows, uint32_t load_pct) {
  if (capacity_rows > (1ull << 40)) return 0;
  uint64_t nslots = std::max<uint64_t>(4096, (capacity_rows * 100 + load_pct - 1) / load_pct);
  nslots = (nslots + 3) & ~3ull;
  return nslots >= (1ull << 32) ? 0 : nslots;   // the last 32-bit value is a sentinel (STRICT_NO_ROW)
}

// Where a table lands matters: the same kernels on the same rows take 68-72 us per 1M-delta launch on some allocations of a 1.4 GB table and 77-80 us on
// others made in the same process minutes apart — a property of the allocation that stays for its lifetime (profiles/r04_placement_probe.log: six tables alive at
// once, three passes; which ones are fast changes from run to run). So a large table is allocated up to PLACEMENT_TRIES times (fewer once a clearly faster candidate has turned up), every candidate is timed with
// the probe kernel's own request mix (k_placement_probe: 2^20 random slot reads + head exchanges + 16-byte stores, best of three launches, ~0.25 ms per
// candidate), the fastest is kept and the others are freed. Candidates stay allocated while the next one is made (otherwise the allocator hands the same range
// back); tables too large for that many copies get fewer tries. BMX_TABLE_PLACEMENT_TRIES=1 switches it off. -> the chosen allocation (uninitialised)
constexpr int PLACEMENT_TRIES = 4;   // at create (BMX_CTX_PLACEMENT_TRIES(n) in bmx_create_ex's flags, then BMX_TABLE_PLACEMENT_TRIES in the environment, override: 1..8);
                                     // round 4 tried up to eight: the transient footprint (8 x 1.4 GB) bought ~1 us over four (profiles/r04_placement_probe.log)
constexpr int PLACEMENT_TRIES_GROW = 3;  // while the old table is alive as well: old + 3 candidates = 4 x the table at the peak
constexpr uint64_t PLACEMENT_MIN_BYTES = 256ull << 20;     // below the Infinity Cache's size a table's lines are served on-die wherever they live
int alloc_table_tuned(bmx_ctx* ctx, uint64_t nslots, Slot** out, bool growing = false) {
  *out = nullptr;
  int tries = growing ? PLACEMENT_TRIES_GROW : PLACEMENT_TRIES;
  if (ctx->placement_tries_asked) tries = growing ? std::min<int>(ctx->placement_tries_asked, PLACEMENT_TRIES_GROW) : (int)ctx->placement_tries_asked;
  if (const char* t = std::getenv("BMX_TABLE_PLACEMENT_TRIES")) { const int v = std::atoi(t); if (v >= 1 && v <= 8) tries = v; }
  const uint64_t bytes = nslots * sizeof(Slot);
  if (bytes < PLACEMENT_MIN_BYTES) tries = 1;
  else {
    // never more than HALF of what is free right now for the candidates together (other contexts, torch's allocator and other processes share the
    // device: ADVICE r4), and never without 2 GB to spare
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) { while (tries > 1 && ((uint64_t)tries * bytes > free_b / 2 || (uint64_t)tries * bytes + (2ull << 30) > free_b)) tries--; } else (void)hipGetLastError();
  }
  int rc;
  if (tries == 1) return dev_alloc(ctx, out, nslots);
  std::vector<Slot*> cand;
  std::vector<float> us;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { (void)hipGetLastError(); if (e0) (void)hipEventDestroy(e0); return dev_alloc(ctx, out, nslots); }
  constexpr uint32_t PN = 1u << 20;
  const char* cenv = std::getenv("BMX_TABLE_CONTIGUOUS");
  const int n_contig = cenv ? std::atoi(cenv) : 0;         // measurement switch: the first n candidates are asked for as physically contiguous memory
  for (int k = 0; k < tries; k++) {
    Slot* p = nullptr;
    if (k < n_contig) {
      if (hipExtMallocWithFlags(reinterpret_cast<void**>(&p), bytes, hipDeviceMallocContiguous) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
      if (std::getenv("BMX_PLACEMENT_DEBUG")) fprintf(stderr, "bmx placement: candidate %d: contiguous allocation %s\n", k, p ? "granted" : "refused");
    }
    if (!p && (rc = dev_alloc(ctx, &p, nslots))) { if (cand.empty()) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return rc; } break; }
    float best = 1e30f;
    for (int rep = 0; rep < 4; rep++) {                    // (the first launch on a fresh allocation also pays its page-table walk misses: not counted)
      (void)hipEventRecord(e0, ctx->stream);
      hipLaunchKernelGGL(k_placement_probe, dim3(PN / 64), dim3(64), 0, ctx->stream, p, nslots, PN, (uint32_t)(k * 16 + rep), ctx->claim_team ? 1u : 0u);
      (void)hipEventRecord(e1, ctx->stream);
      float ms = 0;
      if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { (void)hipGetLastError(); ms = 1e9f; }
      if (rep > 0) best = std::min(best, ms * 1000.f);
    }
    cand.push_back(p); us.push_back(best);
    if (std::getenv("BMX_PLACEMENT_DEBUG")) fprintf(stderr, "bmx placement: candidate %d at %p (%llu MB): probe %.2f us\n", k, (void*)p, (unsigned long long)(bytes >> 20), best);
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  size_t pick = 0;
  for (size_t k = 1; k < cand.size(); k++) if (us[k] < us[pick]) pick = k;
  for (size_t k = 0; k < cand.size(); k++) if (k != pick) (void)hipFree(cand[k]);
  ctx->placement_tries = (uint32_t)cand.size(); ctx->placement_us_best = us[pick];
  ctx->placement_us_worst = *std::max_element(us.begin(), us.end());
  *out = cand[pick];
  return BMX_OK;
}

// Rehash into a table for `capacity_rows` rows. Synchronous.
int grow_table(bmx_ctx* ctx, uint64_t capacity_rows) {
  if (capacity_rows <= ctx->capacity_rows) return BMX_OK;
  int rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t nslots = slots_for(capacity_rows, ctx->load_pct);
  if (!nslots) return fail(ctx, BMX_ERR_INVALID, "table would need more than 2^32 slots (slot indices are 32-bit): shard the graph over more contexts");
  Slot* fresh = nullptr;
  if ((rc = alloc_table_tuned(ctx, nslots, &fresh, /*growing=*/true))) return rc;
  hipLaunchKernelGGL(k_init_slots, dim3(2048), dim3(256), 0, ctx->stream, fresh, nslots);
  hipLaunchKernelGGL(k_rehash, dim3(2048), dim3(256), 0, ctx->stream, ctx->slots, ctx->nslots, fresh, nslots, &ctx->ds->status);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { dev_free(fresh); return fail_hip(ctx, e, "grow_table"); }
  dev_free(ctx->slots);
  ctx->slots = fresh; ctx->nslots = nslots; ctx->capacity_rows = capacity_rows;
  // the batch epoch keeps counting: next[] still holds links tagged with earlier epochs; the new heads are all 0
  ctx->version++;          // indices are rebuilt on their next use
  ctx->chg.valid = false;  // every row moved: the recorded slot positions mean nothing any more
  dev_free(ctx->chg.slot_pos); ctx->chg.slot_pos_n = 0;
  for (auto& ix : ctx->indexes) ix.has_pos = false;
  return check_status(ctx);
}

// ---- deferred compaction ---------------------------------------------------------------------------------------------------------------
// K3 (k_compact_winners) reads only per-batch workspace — winner bytes, block counts, the claimers' slots — and writes what the CALLER reads
// after bmx_sync(): applied_idx, n_applied, stats. Nothing the next batch's probe kernel needs. So for a stream of device-resident batches the
// compaction of batch b runs on a second, high-priority stream UNDER the probe kernel of batch b + 1 (which is bound by memory-side requests in
// flight, not by CUs), and the context's stream carries K1 -> K2 -> K1 -> K2 ... only. Ordering without command-processor markers (an event
// record between two kernels holds a stream ~10 us, bmx.h "bmx_seq_signal"):
//   side stream:  k_seq_wait(seqw[0] >= q + 1)  ->  K3(q)  ->  k_seq_signal(seqw[1] = q)
//   main stream:  K1(q + 1) [block 0 stores seqw[0] = q + 1 when it starts: K2(q) is done]  ->  K2(q + 1) [block 0 returns once seqw[1] >= q]
// so K3(q) is complete before K1(q + 2) overwrites the workspace half it read, whatever the side stream's queue does. K3 is launched LATE: a
// merge only records it (ctx->defer.pend); the next deferring merge puts it on the side stream, anything else (bmx_sync, a scan, a host batch, a
// merge on another path, ...) launches it on the context's own stream first (flush_pending, called by every entry point) — after which that
// stream is ordered behind everything, because the K2 in front of it waited for the only compaction that could still be running on the side.
void launch_k3(bmx_ctx* ctx, const Deferral::PendingK3& P, hipStream_t ks) {
  hipLaunchKernelGGL((k_compact_winners<FinishMerge>), dim3((uint32_t)(((uint64_t)P.n + 4095) / 4096)), dim3(SEL_THREADS), 0, ks, P.wflag, P.blk, P.n,
                     P.applied, P.Fin, P.L, P.mark_created);
  if (P.notify_after) hipLaunchKernelGGL(k_seq_signal_multi, dim3(1), dim3(64), 0, ks, ctx->slab.notify, ctx->slab.n_notify, (unsigned long long)P.notify_seq);
}
// The deferral protocol lets a one-wave kernel on the side stream wait for a kernel on the context's stream to START. Where the runtime or a tool runs
// kernels strictly one at a time — rocprofv3 counter collection (--pmc serialises every dispatch of the device), HIP_LAUNCH_BLOCKING,
// AMD_SERIALIZE_KERNEL — that wait would never end (it expires after ~60 s and raises BMX_ERR_INTERNAL). Such processes keep every launch in stream order.
bool launches_are_serialized() {
  auto on = [](const char* name) { const char* v = std::getenv(name); return v && v[0] && !(v[0] == '0' && !v[1]) && std::strcmp(v, "False") && std::strcmp(v, "false"); };
  return on("ROCPROF_COUNTER_COLLECTION") || on("HIP_LAUNCH_BLOCKING") || on("AMD_SERIALIZE_KERNEL") || on("BMX_NO_DEFERRED_COMPACTION");
}
int flush_pending(bmx_ctx* ctx) {
  if (ctx->defer.side_last) {
    // the resolve kernel at the end of this stream waited for the compaction launched on the side stream TWO batches ago only: the last one may still be
    // running there (it was released when the last probe kernel started, so this one-wave wait is a formality, and it cannot starve anything)
    hipLaunchKernelGGL(k_seq_wait, dim3(1), dim3(64), 0, ctx->stream, (const unsigned long long*)&ctx->ds->seqw[1], (unsigned long long)ctx->defer.side_last, &ctx->ds->status, ctx->ds->seq_diag);
    LAUNCHCHK("k_seq_wait");
    ctx->defer.side_last = ctx->defer.side_prev = 0;
  }
  if (!ctx->defer.pend.on) return BMX_OK;
  ctx->defer.pend.on = false;
  launch_k3(ctx, ctx->defer.pend, ctx->stream);
  LAUNCHCHK("k_compact_winners");
  return BMX_OK;
}
// every entry point that is not a deferring merge: bind the device, launch a compaction that is still only recorded
int enter(bmx_ctx* ctx) {
  HIPCHK(hipSetDevice(ctx->device));
  return flush_pending(ctx);
}
constexpr uint64_t DEFER_MIN_N = 1u << 16;   // below this a batch is launch-bound: the side stream's three extra launches would cost more than the compaction
// ---- the merge proper ---------------------------------------------------------------------------------------------------------------------
// One batch as the host side hands it on (what the kernels see is MergeArgs, merge_kernels.h). Every pointer is a device pointer.
struct MergeIn { uint64_t n; const uint64_t* id; const uint32_t* field; const int64_t* ts; const int64_t* val; const bmx_delta_rec* recs; };   // recs != nullptr: records (AOS) instead of the columns
struct MergeOut { uint32_t* applied_idx; uint64_t* n_applied; uint8_t* flags; bmx_merge_stats* stats; };   // each may be null
struct MergeMode { int rule /* BMX_INSERT_REFERENCE | BMX_INSERT_DELTA */; bool unique, strict, mark_created, force; };
constexpr MergeMode MODE_LOAD{BMX_INSERT_DELTA, false, false, false, false};            // bmx_load_rows
constexpr MergeMode MODE_PUT{BMX_INSERT_DELTA, /*unique*/ true, false, false, /*force*/ true};   // bmx_put_rows: unique keys, stored as given; no caller's insert_mode says this
// A caller's insert_mode as a MergeMode, for every public entry point: what bmx.h documents is BMX_INSERT_* plus the three optional bits. -> nullptr, or the message
// of BMX_ERR_INVALID. (unique + strict, the one documented combination no kernel implements, is refused by merge_core: behind the batch-size check, as ever.)
const char* merge_mode_of(int insert_mode, MergeMode* m) {
  *m = MergeMode{insert_mode & BMX_INSERT_DELTA, (insert_mode & BMX_MERGE_UNIQUE_KEYS) != 0, (insert_mode & BMX_MERGE_STRICT_FLAGS) != 0, (insert_mode & BMX_MERGE_MARK_CREATED) != 0, false};
  return (insert_mode & ~(BMX_INSERT_DELTA | BMX_MERGE_UNIQUE_KEYS | BMX_MERGE_STRICT_FLAGS | BMX_MERGE_MARK_CREATED)) ? "bad insert_mode" : nullptr;
}
constexpr const char* BATCH_TOO_LARGE = "batch larger than 2^24 deltas: split it (sequential semantics are preserved)";
// ---- the steps of one merge, in the order merge_steps runs them: what state each owns, and what it leaves the next ----
// Capacity guard, physical (never let probing run out of empty slots) and logical (capacity_rows). Owns rows_ub, inflight and, when it grows the table, the table.
// Three stages, each only if the one before left the bound too high: tighten it from the mirror the merges write; wait for row reports; the exact count, then
// grow or BMX_ERR_FULL. Afterwards a batch of n deltas fits even if every one of them creates a row.
int ensure_room(bmx_ctx* ctx, uint64_t n) {
  auto too_high = [&]() { return ctx->rows_ub + n >= ctx->nslots || ctx->rows_ub > ctx->capacity_rows; };
  if (too_high()) tighten_rows_ub(ctx);
  // The bound counts every delta of every batch still in flight as a new row. A host that runs many batches ahead of the device (a stream of
  // device batches: ~10 us per call against ~80 us per batch) reaches it long before the table is full: wait for the OLDEST batch in flight to
  // report its row count (its compaction writes the host-visible mirror) and look again — the device keeps its queue, nothing drains. Only when
  // nothing is left in flight does the exact count decide (below).
  if (too_high()) if (int rc = wait_for_row_reports(ctx, n)) return rc;
  if (!too_high()) return BMX_OK;
  if (int rc = flush_pending(ctx)) return rc;                 // the exact row count is the last compaction's
  if (int rc = refresh_rows(ctx)) return rc;
  if (!too_high()) return BMX_OK;
  if (ctx->fixed_capacity) return fail(ctx, BMX_ERR_FULL, "resident table is full (capacity_rows exceeded)");
  return grow_table(ctx, std::max<uint64_t>(ctx->capacity_rows * 2, ctx->rows_ub + n + n / 2));   // amortised doubling
}
// Owns the workspace rotation (ws.par, ws.blk_seg, ws.blk_clean), the epoch and the creation of the side stream. Afterwards the workspace holds n deltas, and A names the table, the
// batch's epoch, its workspace set (A.wflag, A.slot_of, A.shard_ctr: what the compaction reads later) and its block-summary segment, all zero on the stream, with the next batch's (A.blk_next).
int begin_batch(bmx_ctx* ctx, uint64_t n, const MergeMode& mode, bool deferring, MergeArgs& A) {
  if (int rc = ctx->ws.ensure(ctx, n)) return rc;
  if (deferring && !ctx->defer.side) {
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));      // hi = the numerically smallest = highest priority: a hardware queue of its own
    HIPCHK(hipStreamCreateWithPriority(&ctx->defer.side, hipStreamNonBlocking, hi));
  }
  if (++ctx->epoch > EPOCH_MAX) {  // tags wrap: forget every claim
    hipLaunchKernelGGL(k_sweep_heads, dim3(2048), dim3(256), 0, ctx->stream, ctx->slots, ctx->nslots);
    LAUNCHCHK("k_sweep_heads");
    HIPCHK(hipMemsetAsync(ctx->ws.next, 0, (size_t)ctx->ws.cap * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->ws.blk_follow, 0, ((size_t)ctx->ws.cap / 256 + 16) * sizeof(uint32_t), ctx->stream));
    ctx->epoch = 1;
  }
  // this batch's workspace set and block-summary segment
  const uint32_t par = (ctx->ws.par = (ctx->ws.par + 1u) % MergeWs::SETS);
  const uint32_t seg = ctx->ws.blk_seg, seg_next = (seg + 1u) % MergeWs::BLK_SEGS;
  ctx->ws.blk_seg = seg_next;
  A.slots = ctx->slots; A.nslots = ctx->nslots;
  A.n = (uint32_t)n; A.epoch = ctx->epoch;
  A.next = ctx->ws.next; A.wflag = ctx->ws.wflag[par];
  A.slot_of = ctx->ws.slot_of[par]; A.blk_follow = ctx->ws.blk_follow; A.shard_ctr = ctx->ws.shard_ctr + (size_t)par * CTR_SHARDS * CTR_STRIDE; A.status = &ctx->ds->status;
  A.blk_info = ctx->ws.blk_info + (size_t)seg * ctx->ws.blk_half; A.blk_next = ctx->ws.blk_info + (size_t)seg_next * ctx->ws.blk_half; A.blk_ents = ctx->ws.blk_half;
  const bool wave_k1 = !mode.strict;       // k_probe_apply: adds into its segment, zeroes the next one
  if (wave_k1 && !ctx->ws.blk_clean[seg]) HIPCHK(hipMemsetAsync(A.blk_info, 0, (size_t)ctx->ws.blk_half * sizeof(uint32_t), ctx->stream));   // a batch on another path used this segment last
  ctx->ws.blk_clean[seg] = false; ctx->ws.blk_clean[seg_next] = wave_k1;
  return BMX_OK;
}
// The index change log of this batch (written by its compaction). Owns chg.valid, chg.par and chg.ub. Decided before the probe kernel is launched because a deferred compaction reads the
// deltas' fields from a copy that kernel makes (A.fld_out). -> what the compaction logs (chg == nullptr: nothing); A.log_slots tells the probe kernel to keep every first claimer's slot for it.
ChgLog plan_change_log(bmx_ctx* ctx, const MergeIn& in, const MergeMode& mode, bool deferring, MergeArgs& A) {
  ChgLog L{};
  if (ctx->chg.valid) {
    if (!mode.strict && (!mode.unique || mode.force) && ctx->chg.ub + in.n <= ctx->chg.cap && ctx->nslots < (1ull << 31)) {
      L.chg = ctx->chg.log; L.base = &ctx->ds->chg_n[ctx->chg.par]; L.next = &ctx->ds->chg_n[ctx->chg.par ^ 1u];
      L.slot_of = A.slot_of; L.field = in.field; L.recs = in.recs; L.cap = ctx->chg.cap;
      if (deferring) { A.fld_out = ctx->ws.fld[ctx->ws.par]; L.field = A.fld_out; L.recs = nullptr; }   // the caller's columns need not outlive this call's kernels
      ctx->chg.par ^= 1u; ctx->chg.ub += in.n;
    } else ctx->chg.valid = false;   // this batch is not in the log (another merge path, or the log is full): the next scan rebuilds
  }
  A.log_slots = (L.chg != nullptr) ? 1u : 0u;
  return L;
}
// What this batch's kernels signal and wait for beyond stream order. Owns defer.seq and the notify words of the pending compaction (side_k3: it goes to the side stream under this batch's
// probe kernel); reads defer.side_last and tail_armed. Afterwards A carries the deferral protocol's words (block comment above) and the armed tail wait. -> the resolve kernel polls the tail words.
bool arm_deferral(bmx_ctx* ctx, const MergeMode& mode, bool deferring, bool side_k3, MergeArgs& A) {
  if (deferring) {
    ++ctx->defer.seq;
    A.started = &ctx->ds->seqw[0]; A.started_val = ctx->defer.seq;
    if (side_k3) {
      // this batch's resolve kernel ends only once the compaction launched on the side stream BEFORE the one that goes there now is done: the next probe
      // kernel then reuses nothing a compaction still reads (three workspace sets), and that compaction has had two probe kernels' time
      if (ctx->defer.side_last) { A.k3_done = &ctx->ds->seqw[1]; A.k3_wait = ctx->defer.side_last; }
      FinishMerge& PF = ctx->defer.pend.Fin;
      if (PF.n_notify) { A.notify = PF.notify; A.n_notify = PF.n_notify; A.notify_value = PF.notify_value; PF.n_notify = 0; }   // the slab set of the batch before is free the moment this probe kernel starts: said there, not under it
    }
  }
  if (!ctx->slab.tail_armed.n || mode.strict || mode.unique) return false;     // (paths without a resolve kernel leave it armed for nobody: the later wait launch is then not skipped)
  A.tail_words = ctx->slab.tail_armed.words; A.tail_n = ctx->slab.tail_armed.n; A.tail_at_least = ctx->slab.tail_armed.at_least; A.tail_diag = ctx->ds->seq_diag;
  return true;
}
// K1 on the context's stream: the strict path's link kernel, or k_probe_apply for this rule / unique at the occupancy BMX_K1_WAVES asks for. Owns nothing.
template <bool AOS>
int launch_probe(bmx_ctx* ctx, const MergeArgs& A, const MergeMode& mode) {
  if (mode.strict) {
    hipLaunchKernelGGL((k_probe_link_strict<AOS>), dim3((A.n + 255u) / 256u), dim3(256), 0, ctx->stream, A);
  } else {
    constexpr int NT = 64;    // every wave its own workgroup (profiles/r03_ab_inserts.log)
    const dim3 grid((A.n + NT - 1u) / NT);
    const int kw = ctx->k1_waves;   // resident waves per SIMD the probe kernel may take (8 = all; 6 / 5 leave room for the kernels that run beside it)
    const bool team = ctx->claim_team;   // claim mode: a unique-key batch claims nothing, so only the general kernel has the team form
#define BMX_LAUNCH_K1(KERN) do { if (mode.rule == BMX_INSERT_REFERENCE) { \
        if (mode.unique) hipLaunchKernelGGL((KERN<AOS, BMX_INSERT_REFERENCE, true, NT>), grid, dim3(NT), 0, ctx->stream, A); \
        else if (team) hipLaunchKernelGGL((KERN<AOS, BMX_INSERT_REFERENCE, false, NT, true>), grid, dim3(NT), 0, ctx->stream, A); \
        else hipLaunchKernelGGL((KERN<AOS, BMX_INSERT_REFERENCE, false, NT>), grid, dim3(NT), 0, ctx->stream, A); \
      } else { \
        if (mode.unique) hipLaunchKernelGGL((KERN<AOS, BMX_INSERT_DELTA, true, NT>), grid, dim3(NT), 0, ctx->stream, A); \
        else if (team) hipLaunchKernelGGL((KERN<AOS, BMX_INSERT_DELTA, false, NT, true>), grid, dim3(NT), 0, ctx->stream, A); \
        else hipLaunchKernelGGL((KERN<AOS, BMX_INSERT_DELTA, false, NT>), grid, dim3(NT), 0, ctx->stream, A); \
      } } while (0)
    if (kw == 6) BMX_LAUNCH_K1(k_probe_apply_w6); else if (kw == 5) BMX_LAUNCH_K1(k_probe_apply_w5); else if (kw == 4) BMX_LAUNCH_K1(k_probe_apply_w4);
    else if (kw == 3) BMX_LAUNCH_K1(k_probe_apply_w3); else BMX_LAUNCH_K1(k_probe_apply);
#undef BMX_LAUNCH_K1
  }
  LAUNCHCHK("k_probe_apply");
  return BMX_OK;
}
// The compaction of the batch BEFORE, on the side stream: wait for this batch's probe kernel to start, K3, signal. Called with that probe kernel enqueued: the
// wait cannot be left without its signal. Owns defer.pend.on, side_prev / side_last and n_side; afterwards nothing is pending.
int launch_side_compaction(bmx_ctx* ctx) {
  Deferral& D = ctx->defer;
  hipLaunchKernelGGL(k_seq_wait, dim3(1), dim3(64), 0, D.side, (const unsigned long long*)&ctx->ds->seqw[0], (unsigned long long)D.seq, &ctx->ds->status, ctx->ds->seq_diag);
  launch_k3(ctx, D.pend, D.side);
  hipLaunchKernelGGL(k_seq_signal, dim3(1), dim3(64), 0, D.side, &ctx->ds->seqw[1], (unsigned long long)D.pend.seq);
  D.side_prev = D.side_last; D.side_last = D.pend.seq; D.pend.on = false; D.n_side++;
  LAUNCHCHK("deferred k_compact_winners");
  return BMX_OK;
}
// K2 on the context's stream, one lane per delta. Strict: flags for every delta against the untouched rows, then the final state by the last claimers. Otherwise
// the claim lists, which can only exist without the caller's guarantee of unique keys. Owns nothing.
template <bool AOS>
int launch_resolve(bmx_ctx* ctx, const MergeArgs& A, const MergeMode& mode) {
  const dim3 rblocks((A.n + 255u) / 256u);
  if (mode.strict) {
    if (mode.rule == BMX_INSERT_REFERENCE) {
      if (A.flags) hipLaunchKernelGGL((k_resolve_strict<AOS, BMX_INSERT_REFERENCE, false>), rblocks, dim3(256), 0, ctx->stream, A);
      hipLaunchKernelGGL((k_resolve_strict<AOS, BMX_INSERT_REFERENCE, true>), rblocks, dim3(256), 0, ctx->stream, A);
    } else {
      if (A.flags) hipLaunchKernelGGL((k_resolve_strict<AOS, BMX_INSERT_DELTA, false>), rblocks, dim3(256), 0, ctx->stream, A);
      hipLaunchKernelGGL((k_resolve_strict<AOS, BMX_INSERT_DELTA, true>), rblocks, dim3(256), 0, ctx->stream, A);
    }
  } else if (!mode.unique) {
    if (mode.rule == BMX_INSERT_REFERENCE) hipLaunchKernelGGL((k_resolve_lists<AOS, BMX_INSERT_REFERENCE>), rblocks, dim3(256), 0, ctx->stream, A);
    else hipLaunchKernelGGL((k_resolve_lists<AOS, BMX_INSERT_DELTA>), rblocks, dim3(256), 0, ctx->stream, A);
  }
  LAUNCHCHK("k_resolve_lists");
  return BMX_OK;
}
// K3: ordered compaction of the winner bytes (+ the index change log while an index is being maintained), launched behind K2 or only recorded (deferring: the next call launches it,
// flush_pending or launch_side_compaction). Owns batch_seq / inflight, notify_seq, defer.pend and the counts the next call's guards read (nbatch, rows_ub, version).
int finish_batch(bmx_ctx* ctx, const MergeArgs& A, const MergeOut& out, const ChgLog& L, const MergeMode& mode, bool deferring) {
  Deferral::PendingK3 P;
  P.wflag = A.wflag; P.blk = A.blk_info; P.n = A.n; P.applied = out.applied_idx; P.L = L; P.mark_created = mode.mark_created ? 1u : 0u;
  P.Fin = FinishMerge{reinterpret_cast<unsigned long long*>(out.n_applied), out.stats, A.shard_ctr, &ctx->ds->row_count};
  if (ctx->host_rows) { P.Fin.host_mirror = ctx->host_rows; P.Fin.seq = ++ctx->batch_seq; ctx->inflight.emplace_back(P.Fin.seq, A.n); }
  const bool notifying = ctx->slab.n_notify && ctx->slab.notify_armed;
  P.notify_after = notifying && L.chg && !deferring;   // a change log read from the caller's columns: the compaction's workgroups still read the batch, so the peers are told from a launch behind it
  if (notifying) { P.notify_seq = ++ctx->slab.notify_seq; if (!P.notify_after) { P.Fin.notify = ctx->slab.notify; P.Fin.n_notify = ctx->slab.n_notify; P.Fin.notify_value = ctx->slab.notify_seq; } }
  if (deferring) { P.on = true; P.seq = ctx->defer.seq; ctx->defer.pend = P; ctx->defer.n_deferred++; }
  else { launch_k3(ctx, P, ctx->stream); LAUNCHCHK("k_compact_winners"); }
  ctx->nbatch++; ctx->rows_ub += A.n; ctx->version++;
  return BMX_OK;
}
// One merge as the list of its steps; only enqueues work. `defer`: the caller reads applied_idx / n_applied / stats only after bmx_sync() or another bmx_* call on this context (the BMX_MEM_DEVICE
// contract), so the compaction may be deferred (above). A template over the input's layout so that the code object keeps the records' kernels in front of the columns': merge_core picks.
template <bool AOS>
int merge_steps(bmx_ctx* ctx, const MergeIn& in, const MergeOut& out, const MergeMode& mode, bool defer) {
  if (in.n > MAX_BATCH) return fail(ctx, BMX_ERR_INVALID, BATCH_TOO_LARGE);
  if (mode.unique && mode.strict) return fail(ctx, BMX_ERR_INVALID, "BMX_MERGE_STRICT_FLAGS cannot be combined with BMX_MERGE_UNIQUE_KEYS");
  int rc;
  hipEvent_t* pe = (ctx->prof.on && ctx->prof.n < PROF_MAX_CALLS) ? &ctx->prof.ev[4 * ctx->prof.n] : nullptr;
  // the compaction of THIS batch is deferred iff the default path runs (K1 + K2) on a batch big enough to hide it behind; per-kernel profiling brackets every launch
  const bool deferring = defer && ctx->defer.enabled && !mode.strict && !mode.unique && !pe && in.n >= DEFER_MIN_N;
  if (!deferring && (rc = flush_pending(ctx))) return rc;     // everything else sees the stream in order
  if (in.n == 0) {
    if (out.n_applied) HIPCHK(hipMemsetAsync(out.n_applied, 0, sizeof(uint64_t), ctx->stream));
    if (out.stats) HIPCHK(hipMemsetAsync(out.stats, 0, sizeof(bmx_merge_stats), ctx->stream));
    return BMX_OK;
  }
  if ((rc = ensure_room(ctx, in.n))) return rc;
  MergeArgs A;
  if ((rc = begin_batch(ctx, in.n, mode, deferring, A))) return rc;
  A.id = in.id; A.field = in.field; A.ts = in.ts; A.val = in.val; A.recs = in.recs; A.flags = out.flags; A.force = mode.force ? 1u : 0u;
  const ChgLog L = plan_change_log(ctx, in, mode, deferring, A);
  const bool side_k3 = deferring && ctx->defer.pend.on;     // the compaction of the batch before goes to the side stream, under this batch's probe kernel
  const bool tail_used = arm_deferral(ctx, mode, deferring, side_k3, A);
  if (pe) HIPCHK(hipEventRecord(pe[0], ctx->stream));
  if ((rc = launch_probe<AOS>(ctx, A, mode))) return rc;
  if (side_k3 && (rc = launch_side_compaction(ctx))) return rc;
  if (pe) HIPCHK(hipEventRecord(pe[1], ctx->stream));
  if ((rc = launch_resolve<AOS>(ctx, A, mode))) return rc;
  if (tail_used) ctx->slab.tail_waited = ctx->slab.tail_armed;
  ctx->slab.tail_armed = SlabProtocol::TailWait{};       // (armed for the next default-path merge only)
  if (pe) HIPCHK(hipEventRecord(pe[2], ctx->stream));
  if ((rc = finish_batch(ctx, A, out, L, mode, deferring))) return rc;
  if (pe) { HIPCHK(hipEventRecord(pe[3], ctx->stream)); ctx->prof.n++; }
  return BMX_OK;
}
int merge_core(bmx_ctx* ctx, const MergeIn& in, const MergeOut& out, const MergeMode& mode, bool defer = false) {
  return in.recs ? merge_steps<true>(ctx, in, out, mode, defer) : merge_steps<false>(ctx, in, out, mode, defer);
}
// records already on the device, for callers INSIDE the library (the communicator): the compaction is never deferred
int merge_records_internal(bmx_ctx* ctx, uint64_t n, const bmx_delta_rec* recs, const MergeMode& mode, uint32_t* applied_idx, uint64_t* n_applied, bmx_merge_stats* stats) {
  HIPCHK(hipSetDevice(ctx->device));
  return merge_core(ctx, MergeIn{n, nullptr, nullptr, nullptr, nullptr, recs}, MergeOut{applied_idx, n_applied, nullptr, stats}, mode);
}
// Row loads go in chunks of 2^22 rows: one(chunk) for each, until one fails. (bmx_vc.inc keeps a loop of its own: another engine.)
constexpr uint64_t LOAD_CHUNK = 1u << 22;
template <class F>
int in_load_chunks(uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val, F one) {
  for (uint64_t off = 0; off < n; off += LOAD_CHUNK)
    if (int rc = one(MergeIn{std::min<uint64_t>(LOAD_CHUNK, n - off), id + off, field + off, ts + off, val + off, nullptr})) return rc;
  return BMX_OK;
}
int merge_host(bmx_ctx* ctx, const MergeIn& in, const MergeMode& mode, const MergeOut& out);   // bmx_host.inc
// bmx_load_rows (MODE_LOAD) / bmx_put_rows (MODE_PUT)
int load_rows(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val, int mem, const MergeMode& mode) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (n && (!id || !field || !ts || !val)) return fail(ctx, BMX_ERR_INVALID, "null input column");
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (int erc = enter(ctx)) return erc;
  auto one = [&](const MergeIn& part) { return mem == BMX_MEM_DEVICE ? merge_core(ctx, part, MergeOut{}, mode) : merge_host(ctx, part, mode, MergeOut{}); };
  if (int rc = in_load_chunks(n, id, field, ts, val, one)) return rc;
  return mem == BMX_MEM_DEVICE ? BMX_OK : check_status(ctx);
}

}  // namespace
