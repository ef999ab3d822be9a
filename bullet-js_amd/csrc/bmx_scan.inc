// bmx_scan.inc — the scans over one index (bmx.h bmx_scan_*): how an answer leaves the device (ScanDelivery: plan_delivery, deliver, scan_collect), run_scan_t as
// plan / scratch / launch / deliver, the width and emit-geometry dispatch every two-pass form shares (by_width, emit_dispatch: the one reader of
// BMX_SCAN_SUB8_BLOCKS), and the range scans with their clamping rules. The position scan and the declarative filter are bmx_scan_filter.inc, behind
// bmx.hip's own entry points (bmx.hip, the include list). Kernels: scan_kernels.h; the ordered queries' launches are bmx_view.inc. Included by bmx.hip (one
// translation unit), which keeps the scratch (ScanScratch) and the delivery plan's type.
namespace {

// scratch of the scans for an index of `rows` rows: one match bit per row + one count per 8192-row block (+1 for the total); `out_n` > 0: a device
// buffer for that many ids of a host-mode answer on its way down
int ScanScratch::ensure(bmx_ctx* ctx, uint64_t rows, uint64_t out_n) {
  if (out_n > out_cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    out_cap = 0;
    if (int rc = dev_alloc(ctx, &out, out_n)) return rc;
    out_cap = out_n;
  }
  const uint64_t nb = (rows + SCAN_BLOCK_ELEMS - 1) / SCAN_BLOCK_ELEMS;
  if (nb > blocks_cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    blocks_cap = 0;
    const uint64_t cap = nb + nb / 4 + 16;
    if (int rc = dev_alloc_all(ctx, {{mask, cap * (SCAN_BLOCK_ELEMS / 32) * sizeof(uint32_t)}, {counts, (cap + 1) * sizeof(uint32_t)}})) return rc;
    blocks_cap = cap;
  }
  return BMX_OK;
}

// a value column above this size is read with nontemporal loads: it cannot stay in the 256 MiB Infinity Cache between two scans anyway (scan_kernels.h)
constexpr uint64_t SCAN_NT_BYTES = 256ull << 20;
constexpr uint32_t SCAN_NTX_DEFAULT = 0;      // EmitIds::ntx (profiles/r05_scan_nt_emit_ab.log)

// small host-mode answers (count only, or room for at most SCAN_PIN_IDS ids) come back through mapped host memory: no download, one synchronisation
constexpr uint64_t SCAN_PIN_IDS = 16384;
static_assert(SCAN_PIN_IDS * 8 + 8 <= SMALL_OUT_BYTES, "pinned scan answer fits the small-call buffer");

// the word behind a host-side home of the count (COUNT_CALLER has none: it is the caller's own device word)
unsigned long long* count_word(bmx_ctx* ctx, ScanDelivery::CountHome home) {
  switch (home) {
    case ScanDelivery::COUNT_PIN_OUT: return reinterpret_cast<unsigned long long*>(ctx->host.pin_out + SCAN_PIN_IDS * 8);
    case ScanDelivery::COUNT_HRES: return const_cast<unsigned long long*>(&ctx->host.hres[HRES_SCAN_N]);
    case ScanDelivery::COUNT_DEV_SCALAR: return &ctx->ds->n_out;
    case ScanDelivery::COUNT_CALLER: break;
  }
  return nullptr;
}

// How the answer of one scan leaves the device: decided once, in front of the launch, from the caller's arguments alone. Launches nothing (the mapped buffers it
// chooses are allocated on first use). `out` null = count only. `deferred`: the caller is bmx_comm_scan_*, which fetches with scan_collect. `count_by_atomics`: the
// kernel builds the count up with one atomic add per wave instead of storing it once.
// A staged or deferred plan has d_out = nullptr until ScanScratch::ensure has made room for d_cap ids (run_scan_t).
ScanDelivery plan_delivery(bmx_ctx* ctx, const Index* ix, void* out, uint64_t cap, uint64_t* n_out, int mem, bool deferred, bool count_by_atomics) {
  ScanDelivery D;
  if (mem != BMX_MEM_HOST) {
    D.route = ScanDelivery::DEVICE; D.d_out = out; D.d_cap = cap; D.count = ScanDelivery::COUNT_CALLER; D.d_n = reinterpret_cast<unsigned long long*>(n_out);
    return D;
  }
  D.d_cap = out ? std::min<uint64_t>(cap, ix->n) : cap;
  if (deferred) D.route = ScanDelivery::DEFERRED;
  else if ((!out || D.d_cap <= SCAN_PIN_IDS) && ensure_pinned(ctx)) { D.route = ScanDelivery::PINNED_SMALL; if (out) D.d_out = ctx->host.pin_out; }
  // a caller's buffer in page-locked memory (bmx_host_alloc, hipHostMalloc, a registered range) is written by the kernels themselves: no staging copy behind the answer
  else if (out && (D.d_out = mapped_host(out))) D.route = ScanDelivery::CALLER_PINNED;
  else D.route = ScanDelivery::STAGED;       // (also a count without the small-answer buffer: nothing to stage, the count comes as below)
  // The count. The small answer carries its own word; a deferred scan's stays on the device until scan_collect asks for it. Every other host-mode answer gets it in a
  // mapped result word, which the kernel's last store fills in without a download — except where the kernel counts by atomics (the ordered PredFilter appends its
  // survivors through the counter): thousands of read-modify-writes of one word belong in device memory, not across the bus, so that count is downloaded.
  if (D.route == ScanDelivery::PINNED_SMALL) D.count = ScanDelivery::COUNT_PIN_OUT;
  else if (D.route != ScanDelivery::DEFERRED && !count_by_atomics && ensure_hres(ctx)) D.count = ScanDelivery::COUNT_HRES;
  else D.count = ScanDelivery::COUNT_DEV_SCALAR;
  D.d_n = count_word(ctx, D.count);
  return D;
}

// Wait for the scan and read its count from its home: the one synchronisation of a host-mode answer (a count in device memory is downloaded in front of it).
int await_count(bmx_ctx* ctx, ScanDelivery::CountHome home, unsigned long long* m) {
  const unsigned long long* w = count_word(ctx, home);
  if (home == ScanDelivery::COUNT_DEV_SCALAR) HIPCHK(hipMemcpyAsync(m, w, sizeof(*m), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (home != ScanDelivery::COUNT_DEV_SCALAR) *m = *static_cast<const volatile unsigned long long*>(w);
  return BMX_OK;
}

// Behind the launch: the answer reaches the caller's `out` (up to d_cap entries of OutT) and `n_out` as the plan says.
template <class OutT>
int deliver(bmx_ctx* ctx, const ScanDelivery& D, OutT* out, uint64_t* n_out) {
  unsigned long long m = 0;
  switch (D.route) {
    case ScanDelivery::DEVICE: return BMX_OK;                    // the kernels wrote the caller's buffer and word; nothing waits
    case ScanDelivery::DEFERRED:                                 // the caller fetches with scan_collect()
      ctx->scan.deferred = ScanScratch::DeferredAnswer{out ? D.d_cap : 0, D.count};
      return BMX_OK;
    case ScanDelivery::PINNED_SMALL:
      if (int rc = await_count(ctx, D.count, &m)) return rc;
      if (out && m) std::memcpy(out, D.d_out, std::min<uint64_t>(m, D.d_cap) * sizeof(OutT));
      break;
    case ScanDelivery::CALLER_PINNED:                            // the ids are where the caller wants them
      if (int rc = await_count(ctx, D.count, &m)) return rc;
      break;
    case ScanDelivery::STAGED:
      if (int rc = await_count(ctx, D.count, &m)) return rc;
      if (out && m) HIPCHK(hipMemcpy(out, ctx->scan.out, std::min<uint64_t>(m, D.d_cap) * sizeof(OutT), hipMemcpyDeviceToHost));
      break;
  }
  if (n_out) *n_out = m;
  return BMX_OK;
}

// second half of a deferred host-mode scan: wait for the scan enqueued on the deferred route, deliver the count and up to `cap` ids
int scan_collect(bmx_ctx* ctx, uint64_t* out_ids, uint64_t cap, uint64_t* n_out) {
  if (int erc = enter(ctx)) return erc;
  unsigned long long m = 0;
  if (int rc = await_count(ctx, ctx->scan.deferred.count, &m)) return rc;
  const uint64_t k = std::min<uint64_t>(std::min<uint64_t>(m, ctx->scan.deferred.cap), cap);
  if (out_ids && k) HIPCHK(hipMemcpy(out_ids, ctx->scan.out, k * 8, hipMemcpyDeviceToHost));
  if (n_out) *n_out = m;
  return BMX_OK;
}

// f(T{}) with T the width of an index's value column
template <class F>
auto by_width(bool fits32, F&& f) {
  if (fits32) return f(int32_t{});
  return f(int64_t{});
}

// The geometry of an emit pass over `nb` blocks: f(std::integral_constant<int, B>, workgroups) with B = 8 blocks per workgroup on an eighth of the workgroups beyond
// SCAN_SUB8_BLOCKS blocks (a large column: each sums the counts in front of it once, no offsets launch), B = 1 otherwise. BMX_SCAN_SUB8_BLOCKS is a measurement
// and test switch and is read on every call: the tests set and clear it inside one process.
template <class F>
void emit_dispatch(uint32_t nb, F&& f) {
  const char* s8 = std::getenv("BMX_SCAN_SUB8_BLOCKS");
  const uint32_t sub8_blocks = s8 ? (uint32_t)std::strtoul(s8, nullptr, 0) : SCAN_SUB8_BLOCKS;
  if (nb > sub8_blocks) f(std::integral_constant<int, 8>{}, (nb + 7) / 8);
  else f(std::integral_constant<int, 1>{}, nb);
}

// Run one predicate over an index and deliver ids (POS = false: u64 node ids gathered from the id column) or index positions (POS = true: u32,
// no gather) / the count according to `mem`. `out` is uint64_t* or uint32_t* accordingly. Plan, scratch, launch, deliver.
template <bool POS, class Pred>
int run_scan_t(bmx_ctx* ctx, const Pred& P, const Index* ix, void* out_v, uint64_t cap, uint64_t* n_out, int mem, bool deferred, bool ordered = false, int64_t olo = 0, int64_t ohi = 0) {
  using OutT = typename std::conditional<POS, uint32_t, uint64_t>::type;
  ScanDelivery D = plan_delivery(ctx, ix, out_v, cap, n_out, mem, deferred, ordered && std::is_same<Pred, PredFilter>::value);
  const bool stage = out_v && (D.route == ScanDelivery::STAGED || D.route == ScanDelivery::DEFERRED);
  if (int rc = ctx->scan.ensure(ctx, std::max<uint64_t>(ix->n, 1), stage ? std::max<uint64_t>(D.d_cap, 1) : 0)) return rc;
  if (stage) D.d_out = ctx->scan.out;
  OutT* d_out = static_cast<OutT*>(D.d_out);
  const uint64_t d_cap = D.d_cap;
  unsigned long long* d_n = D.d_n;
  const uint32_t nb = (uint32_t)((std::max<uint64_t>(ix->n, 1) + SCAN_BLOCK_ELEMS - 1) / SCAN_BLOCK_ELEMS);
  hipEvent_t* se = (ctx->prof.on && ctx->prof.scan_n < PROF_MAX_CALLS && !ctx->prof.scan_ev.empty()) ? &ctx->prof.scan_ev[3 * ctx->prof.scan_n] : nullptr;
  if (se) HIPCHK(hipEventRecord(se[0], ctx->stream));
  if (ordered) {
    if constexpr (std::is_same<Pred, PredFilter>::value) launch_ordered<POS>(ctx, ix, olo, ohi, d_out, d_cap, d_n, &P);
    else launch_ordered<POS>(ctx, ix, olo, ohi, d_out, d_cap, d_n);
    LAUNCHCHK("k_ordered_bounds / k_ordered_copy");
    if (se) HIPCHK(hipEventRecord(se[1], ctx->stream));
  } else if (d_out) {
    // pass 1: one read of the column -> match mask + block counts; pass 2: ids / positions from the mask
    hipLaunchKernelGGL((k_scan_mask<Pred, true>), dim3(nb), dim3(SEL_THREADS), 0, ctx->stream, P, ix->n, ctx->scan.mask, ctx->scan.counts);
    LAUNCHCHK("k_scan_mask");
    if (se) HIPCHK(hipEventRecord(se[1], ctx->stream));
    typename std::conditional<POS, EmitPos, EmitIds>::type Em;
    if constexpr (POS) Em = EmitPos{d_out, d_cap};
    else {
      const char* sm = std::getenv("BMX_SCAN_STREAM_MIN");      // measurement switch: matches per block from which the id column is streamed (0xFFFFFFFF: never)
      const char* nx = std::getenv("BMX_SCAN_NT");               // measurement switch: EmitIds::ntx
      Em = EmitIds{ix->ids, d_out, d_cap, ix->n * sizeof(uint64_t) > SCAN_NT_BYTES, sm ? (uint32_t)std::strtoul(sm, nullptr, 0) : SCAN_STREAM_MIN, nx ? (uint32_t)std::strtoul(nx, nullptr, 0) : SCAN_NTX_DEFAULT};
    }
    using EmT = decltype(Em);
    FinishCount Fin{d_n};
    emit_dispatch(nb, [&](auto B, uint32_t wgs) {
      hipLaunchKernelGGL((k_scan_emit<EmT, FinishCount, decltype(B)::value>), dim3(wgs), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.mask, ctx->scan.counts, ix->n, nb, Em, Fin);
    });
    LAUNCHCHK("k_scan_emit");
  } else if (d_n) {
    hipLaunchKernelGGL((k_scan_mask<Pred, false>), dim3(nb), dim3(SEL_THREADS), 0, ctx->stream, P, ix->n, ctx->scan.mask, ctx->scan.counts);
    LAUNCHCHK("k_scan_mask(count)");
    if (se) HIPCHK(hipEventRecord(se[1], ctx->stream));
    hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.counts, nb, d_n);
    LAUNCHCHK("k_sum_counts");
  } else if (se) {
    HIPCHK(hipEventRecord(se[1], ctx->stream));
  }
  if (se) { HIPCHK(hipEventRecord(se[2], ctx->stream)); ctx->prof.scan_n++; }
  return deliver<OutT>(ctx, D, static_cast<OutT*>(out_v), n_out);
}

template <bool POS>
int scan_range_impl_t(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, void* out, uint64_t cap, uint64_t* n_out, int mem, bool deferred = false) {
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  Index* ix;
  int rc = fresh_index(ctx, field, &ix);
  if (rc) return rc;
  const bool ordered = (n_out || out) && ensure_ordered_view(ctx, ix);     // (it was sorted from columns of the width they have now: a widened index has a new `content`)
  if (ix->fits32) {
    const Range32 r = clamp_i32(lo, hi);     // every value fits int32: scan the 4-byte column
    PredRange32 P{ix->v32, (int32_t)r.lo, (int32_t)r.hi, ix->n * sizeof(int32_t) > SCAN_NT_BYTES};
    rc = run_scan_t<POS>(ctx, P, ix, out, cap, n_out, mem, deferred, ordered, r.lo, r.hi);
  } else {
    PredRange64 P{ix->v64, above_tombstones(lo), hi, ix->n * sizeof(int64_t) > SCAN_NT_BYTES};
    rc = run_scan_t<POS>(ctx, P, ix, out, cap, n_out, mem, deferred, ordered, P.lo, P.hi);
  }
  if (ordered && !rc) view_after_query(ctx, ix);
  return rc;
}
// bmx_scan_range and the first half of bmx_comm_scan_range (deferred: host mode, fetched with scan_collect)
int scan_range_impl(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem, bool deferred = false) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  return scan_range_impl_t<false>(ctx, field, lo, hi, out_ids, cap, n_out, mem, deferred);
}

}  // namespace

extern "C" {

int bmx_scan_range(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem) {
  return scan_range_impl(ctx, field, lo, hi, out_ids, cap, n_out, mem);
}
int bmx_scan_equals(bmx_ctx* ctx, uint32_t field, int64_t value, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem) {
  return bmx_scan_range(ctx, field, value, value, out_ids, cap, n_out, mem);
}
int bmx_scan_count(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, uint64_t* n_out, int mem) {
  return bmx_scan_range(ctx, field, lo, hi, nullptr, 0, n_out, mem);
}

}  // extern "C"
