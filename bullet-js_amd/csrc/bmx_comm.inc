// bmx_comm.inc — one process, N shards (include/bmx.h "bmx_comm_*"): the graph is split by node-id hash over N contexts, one per GPU
// (or several on one GPU: logical shards, which is how a one-GPU box tests N = 2, 4, 8). Included at the end of bmx.hip.
//
// Replaces the gossip fan-out of src/bullet-network.js:378-418 inside one node: instead of every peer merging every delta, a delta
// goes to the one shard that owns its node id (owner = bmx_owner_of(id, N)), so all fields of a node stay on one GPU. One `Bullet`
// instance owns all shards through this handle (SURVEY §8(e)).
//
//   host batch   (bmx_comm_merge / bmx_comm_load_rows / bmx_comm_put_rows): the batch is uploaded to shard 0 and partitioned by owner there (K7,
//                stable: a shard sees its deltas in ascending batch order, so the sequential semantics — smallest index wins ties / creates a
//                row — hold globally); the scatter pass writes every owner's run straight into that owner's receive buffer (one padded slab per
//                owner; peer stores when the owner is another GPU); every shard merges what it received; the winners come back as ascending
//                indices into the caller's batch. One shard: the context's own host-batch path.
//   device batch (bmx_comm_merge_dev): every shard originates a device-resident batch; its owner partition writes fixed-size slabs
//                STRAIGHT into the owners' receive buffers (peer-mapped stores: no copy kernel, no host round trip); each shard then
//                merges its N slabs (padding skipped). A slab that is too small is a sticky error (BMX_ERR_OVERFLOW at bmx_comm_sync).
//   scans        every shard scans its own rows; results are concatenated (no collective).
// Cross-device ordering uses HIP events (record on the origin's stream, wait on the owner's).

struct bmx_comm {
  uint32_t N = 0;
  std::vector<int> dev;
  std::vector<bmx_ctx*> sh;
  struct Shard {
    uint64_t in_cap = 0;
    uint64_t* id = nullptr; uint32_t* field = nullptr; int64_t* ts = nullptr; int64_t* val = nullptr;   // this shard's slice of a host batch
    unsigned long long* counts = nullptr;        // PART_MAX_SHARDS counts (device)
    uint64_t recv_cap = 0;
    bmx_delta_rec* recv = nullptr;               // what this shard merges
    uint32_t* applied = nullptr;                 // winners: positions in recv
    unsigned long long* n_applied = nullptr;     // device
    bmx_merge_stats* stats = nullptr;            // device
    hipEvent_t routed = nullptr;                 // this shard's partition (and scatter) of the current step is done
    hipEvent_t merged = nullptr;                 // this shard's merge of the previous step is done (its receive buffer may be overwritten)
    uint64_t slab = 0;                           // device path: records per (origin, owner) slab
    void release() {                             // (with the shard's device current and idle)
      dev_free(id); dev_free(field); dev_free(ts); dev_free(val); dev_free(counts); dev_free(recv); dev_free(applied); dev_free(n_applied); dev_free(stats);
      if (routed) (void)hipEventDestroy(routed);
      if (merged) (void)hipEventDestroy(merged);
      routed = merged = nullptr; in_cap = recv_cap = 0;
    }
  };
  std::vector<Shard> s;
  // winners of a host batch in the caller's index space: every shard marks its winners' batch indices in ONE byte map on shard 0's GPU
  // (peer stores), shard 0 compacts the map in order (k_count_winners + k_compact_winners): no host-side merge of N sorted lists
  struct WinnerMap {
    uint64_t cap = 0;
    uint8_t* flag = nullptr; uint32_t* blk = nullptr; uint32_t* applied = nullptr; unsigned long long* n = nullptr;
    hipEvent_t zeroed = nullptr;
    void release() {                             // (with shard 0's device current and idle)
      dev_free(flag); dev_free(blk); dev_free(applied); dev_free(n);
      if (zeroed) (void)hipEventDestroy(zeroed);
      zeroed = nullptr; cap = 0;
    }
  } win;
  bool dev_step_pending = false;
  std::string err;
};

namespace {
// bmx_comm_* calls hop over the shards' devices: the calling thread gets its current device back
struct DevGuard {
  int d = -1;
  DevGuard() { if (hipGetDevice(&d) != hipSuccess) { d = -1; (void)hipGetLastError(); } }
  ~DevGuard() { if (d >= 0) (void)hipSetDevice(d); }
};
// the one place that words a shard's error for the communicator's caller (a shard that could not be created left its text in bmx_last_error(NULL))
std::string shard_msg(const bmx_comm* c, uint32_t g) { return std::string("shard ") + std::to_string(g) + ": " + bmx_last_error(c->sh[g]); }
#define CSH(g, call) do { int rc__ = (call); if (rc__) return fail(c, rc__, shard_msg(c, g)); } while (0)

__global__ void k_mark_aux(const bmx_delta_rec* recs, const uint32_t* applied, const unsigned long long* n_applied, uint8_t* flag) {
  const uint64_t n = *n_applied;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) flag[recs[applied[i]].aux] = 1;
}

// Buffers that the shards' kernels read and write across devices are regrown only when every shard's device is idle (peers may still be writing the old ones):
// one all-or-nothing group from device `d`, which is the current device afterwards.
int comm_regrow(bmx_comm* c, int d, uint64_t* cap_word, uint64_t cap, std::initializer_list<DevBuf> bufs) {
  *cap_word = 0;
  for (uint32_t i = 0; i < c->N; i++) { HIPCHK_ON(c, hipSetDevice(c->dev[i])); HIPCHK_ON(c, hipDeviceSynchronize()); }
  HIPCHK_ON(c, hipSetDevice(d));
  if (int rc = dev_alloc_all(c, bufs)) return rc;
  *cap_word = cap;
  return BMX_OK;
}
int comm_ensure_global(bmx_comm* c, uint64_t n) {
  bmx_comm::WinnerMap& W = c->win;
  if (n <= W.cap) return BMX_OK;
  const uint64_t cap = (std::max<uint64_t>(n, 1u << 16) + 4095) & ~4095ull;
  return comm_regrow(c, c->dev[0], &W.cap, cap, {{W.flag, cap + 16}, {W.blk, (cap / 256 + 16) * sizeof(uint32_t)}, {W.applied, cap * sizeof(uint32_t)}});
}
int comm_ensure_in(bmx_comm* c, uint32_t g, uint64_t n) {
  bmx_comm::Shard& S = c->s[g];
  if (n <= S.in_cap) return BMX_OK;
  const uint64_t cap = (std::max<uint64_t>(n, 1u << 12) + 255) & ~255ull;
  return comm_regrow(c, c->dev[g], &S.in_cap, cap, {{S.id, cap * 8}, {S.field, cap * 4}, {S.ts, cap * 8}, {S.val, cap * 8}});
}
int comm_ensure_recv(bmx_comm* c, uint32_t g, uint64_t n) {
  bmx_comm::Shard& S = c->s[g];
  if (n <= S.recv_cap) return BMX_OK;
  const uint64_t cap = (std::max<uint64_t>(n + n / 4, 1u << 12) + 255) & ~255ull;
  return comm_regrow(c, c->dev[g], &S.recv_cap, cap, {{S.recv, cap * sizeof(bmx_delta_rec)}, {S.applied, cap * sizeof(uint32_t)}});
}

// The sharded queries' two phases. `enqueue(g, shard)` runs on shards 0..N-1 and the first error ends the call (what the shards before it were given finishes on
// their own streams); then `collect(g, shard)` runs on EVERY shard, also after an error, and the first error is the call's: N GPUs work at the same time, and
// the host waits once per shard for work that is already running.
template <class Enqueue, class Collect>
int comm_two_phase(bmx_comm* c, Enqueue enqueue, Collect collect) {
  for (uint32_t g = 0; g < c->N; g++) CSH(g, enqueue(g, c->sh[g]));
  int first = BMX_OK; std::string msg;
  for (uint32_t g = 0; g < c->N; g++) {
    const int rc = collect(g, c->sh[g]);
    if (rc && !first) { first = rc; msg = shard_msg(c, g); }
  }
  return first ? fail(c, first, msg) : BMX_OK;
}

// A small host batch (<= COMM_SMALL_N deltas): routed on the HOST — owner of every delta, stable split into per-shard sub-batches — and merged
// through each shard's small-batch path (mapped host memory, ~30 us per shard that got anything). Keys never straddle shards and the split keeps
// the batch order inside a shard, so the sequential semantics hold as in the device-routed path, which costs 1.2-2.3 ms per call whatever the size.
constexpr uint64_t COMM_SMALL_N = 32768;
int comm_host_small(bmx_comm* c, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val, const MergeMode& mode,
                    uint32_t* applied_idx, uint64_t* n_applied, bmx_merge_stats* stats) {
  const uint32_t N = c->N;
  if (c->dev_step_pending) { int rc = bmx_comm_sync(c); if (rc) return rc; }
  std::vector<std::vector<uint32_t>> back(N);
  for (uint64_t j = 0; j < n; j++) back[N == 1 ? 0 : bmx_owner_of(id[j], N)].push_back((uint32_t)j);
  std::vector<uint32_t> winners;
  bmx_merge_stats tot; std::memset(&tot, 0, sizeof(tot));
  std::vector<uint64_t> gi; std::vector<uint32_t> gf, ga; std::vector<int64_t> gt, gv;
  for (uint32_t g = 0; g < N; g++) {
    const size_t m = back[g].size();
    bmx_merge_stats st; std::memset(&st, 0, sizeof(st));
    if (m == 0) { uint64_t r = 0; CSH(g, bmx_row_count(c->sh[g], &r)); tot.n_rows += r; continue; }
    gi.resize(m); gf.resize(m); gt.resize(m); gv.resize(m); ga.resize(m);
    for (size_t x = 0; x < m; x++) { const uint32_t j = back[g][x]; gi[x] = id[j]; gf[x] = field[j]; gt[x] = ts[j]; gv[x] = val[j]; }
    uint64_t na = 0;
    HIPCHK_ON(c, hipSetDevice(c->dev[g]));
    CSH(g, merge_host(c->sh[g], MergeIn{m, gi.data(), gf.data(), gt.data(), gv.data(), nullptr}, mode, MergeOut{applied_idx ? ga.data() : nullptr, &na, nullptr, &st}));
    if (applied_idx) for (uint64_t x = 0; x < na; x++) winners.push_back(back[g][ga[x]]);
    tot.n_applied += st.n_applied; tot.n_conflicts += st.n_conflicts; tot.n_rows += st.n_rows;
  }
  if (applied_idx) {
    if (N > 1) std::sort(winners.begin(), winners.end());          // N ascending runs of a small batch
    if (!winners.empty()) std::memcpy(applied_idx, winners.data(), winners.size() * sizeof(uint32_t));
  }
  if (n_applied) *n_applied = tot.n_applied;
  if (stats) *stats = tot;
  return BMX_OK;
}

// One host batch through the shards. want = winners wanted (merge) or not (load).
int comm_host_batch(bmx_comm* c, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val, const MergeMode& mode,
                    uint32_t* applied_idx, uint64_t* n_applied, bmx_merge_stats* stats) {
  const uint32_t N = c->N;
  if (n > MAX_BATCH) return fail(c, BMX_ERR_INVALID, BATCH_TOO_LARGE);   // before a partition is launched
  if (n_applied) *n_applied = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n && (!id || !field || !ts || !val)) return fail(c, BMX_ERR_INVALID, "null input column");
  if (n && n <= COMM_SMALL_N) return comm_host_small(c, n, id, field, ts, val, mode, applied_idx, n_applied, stats);
  if (c->dev_step_pending) { int rc0 = bmx_comm_sync(c); if (rc0) return rc0; }
  if (N == 1 && n) {   // one shard owns everything: nothing to route, no winner map to build — the context's own host-batch path (two staging sets, three streams)
    HIPCHK_ON(c, hipSetDevice(c->dev[0]));
    bmx_merge_stats st; std::memset(&st, 0, sizeof(st));
    uint64_t na = 0;
    CSH(0, merge_host(c->sh[0], MergeIn{n, id, field, ts, val, nullptr}, mode, MergeOut{applied_idx, &na, nullptr, &st}));
    if (n_applied) *n_applied = na;
    if (stats) *stats = st;
    return BMX_OK;
  }
  // 1. the whole batch goes to shard 0 (four uploads whatever N is: the pageable copies block the calling thread one after the other anyway) and is
  //    partitioned THERE, once, by owner: the stable partition of 1M deltas takes ~17 us, and its scatter pass writes every owner's run straight into
  //    that owner's receive buffer — peer stores when the owner is another GPU — as ONE slab per owner, padded with reserved ids. No compact send
  //    buffer, no N x N device-to-device copies (round 2: 64 of them at N = 8). `aux` carries the index in the caller's batch.
  int rc;
  if ((rc = comm_ensure_in(c, 0, n))) return rc;
  bmx_comm::Shard& S0 = c->s[0];
  HIPCHK_ON(c, hipSetDevice(c->dev[0]));
  hipStream_t s0 = reinterpret_cast<hipStream_t>(bmx_get_stream(c->sh[0]));
  HIPCHK_ON(c, hipMemcpyAsync(S0.id, id, n * 8, hipMemcpyHostToDevice, s0));
  HIPCHK_ON(c, hipMemcpyAsync(S0.field, field, n * 4, hipMemcpyHostToDevice, s0));
  HIPCHK_ON(c, hipMemcpyAsync(S0.ts, ts, n * 8, hipMemcpyHostToDevice, s0));
  HIPCHK_ON(c, hipMemcpyAsync(S0.val, val, n * 8, hipMemcpyHostToDevice, s0));
  if (applied_idx) {   // the byte map of this batch's winners, zeroed before any shard marks it
    if ((rc = comm_ensure_global(c, n))) return rc;
    HIPCHK_ON(c, hipSetDevice(c->dev[0]));
    HIPCHK_ON(c, hipMemsetAsync(c->win.flag, 0, n, s0));
  }
  // 2. slab size: the mean run plus six standard deviations of a uniform owner hash; the exact counts come back with the partition, and a batch
  //    that does not fit (skewed node ids) is partitioned once more into slabs of the largest run — nothing has been merged by then
  std::vector<unsigned long long> cnt(N, 0);
  uint64_t slab = n / N + 6 * (uint64_t)std::sqrt((double)(n / N + 1)) + 64;
  for (int attempt = 0; attempt < 2; attempt++) {
    if (slab > 0xFFFFFFFFull / N) return fail(c, BMX_ERR_INVALID, "batch too large for one exchange slab per shard");
    for (uint32_t g = 0; g < N; g++) if ((rc = comm_ensure_recv(c, g, slab))) return rc;
    HIPCHK_ON(c, hipSetDevice(c->dev[0]));
    PartOut po; std::memset(&po, 0, sizeof(po));
    for (uint32_t g = 0; g < N; g++) po.base[g] = c->s[g].recv;
    CSH(0, partition_impl(c->sh[0], n, S0.id, S0.field, S0.ts, S0.val, N, slab, nullptr, reinterpret_cast<uint64_t*>(S0.counts), &po, 0));
    HIPCHK_ON(c, hipMemcpyAsync(cnt.data(), S0.counts, N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s0));
    HIPCHK_ON(c, hipStreamSynchronize(s0));
    uint64_t mx = 0;
    for (uint32_t g = 0; g < N; g++) mx = std::max<uint64_t>(mx, cnt[g]);
    if (mx <= slab) break;
    (void)bmx_sync(c->sh[0]);            // clears the sticky "slab too small" status of the first attempt
    if (attempt == 1) return fail(c, BMX_ERR_INTERNAL, "owner partition overflowed a slab sized from its own counts");
    slab = mx;
  }
  HIPCHK_ON(c, hipEventRecord(S0.routed, s0));    // the slabs are in place (and the winner map is zeroed)
  // 3. every owner merges its slab and marks its winners in the map; all on the owner's stream
  std::vector<uint64_t> m(N, 0);
  hipEvent_t routed0 = S0.routed;
  for (uint32_t g = 0; g < N; g++) {
    m[g] = cnt[g];
    bmx_comm::Shard& G = c->s[g];
    HIPCHK_ON(c, hipSetDevice(c->dev[g]));
    hipStream_t st = reinterpret_cast<hipStream_t>(bmx_get_stream(c->sh[g]));
    if (g) HIPCHK_ON(c, hipStreamWaitEvent(st, routed0, 0));
    if (m[g]) {
      CSH(g, merge_records_internal(c->sh[g], slab, G.recv, mode, applied_idx ? G.applied : nullptr, reinterpret_cast<uint64_t*>(G.n_applied), G.stats));
      if (applied_idx) {
        hipLaunchKernelGGL(k_mark_aux, dim3(256), dim3(256), 0, st, (const bmx_delta_rec*)G.recv, (const uint32_t*)G.applied, (const unsigned long long*)G.n_applied, c->win.flag);
        HIPCHK_ON(c, hipGetLastError());
      }
    }
    if (g) HIPCHK_ON(c, hipEventRecord(G.merged, st));       // "this shard's part of the host batch is done" (shard 0 orders itself)
  }
  if (applied_idx && n) {   // shard 0 compacts the byte map once every shard has marked
    HIPCHK_ON(c, hipSetDevice(c->dev[0]));
    for (uint32_t g = 1; g < N; g++) HIPCHK_ON(c, hipStreamWaitEvent(s0, c->s[g].merged, 0));
    hipLaunchKernelGGL(k_count_winners, dim3((uint32_t)((n + 4095) / 4096)), dim3(256), 0, s0, (const uint8_t*)c->win.flag, (uint32_t)n, c->win.blk);
    FinishCount Fin{c->win.n};
    hipLaunchKernelGGL((k_compact_winners<FinishCount>), dim3((uint32_t)((n + 4095) / 4096)), dim3(SEL_THREADS), 0, s0, (const uint8_t*)c->win.flag, (const uint32_t*)c->win.blk,
                       (uint32_t)n, c->win.applied, Fin, ChgLog{});
    HIPCHK_ON(c, hipGetLastError());
  }
  // 5. results: one wait per shard, then the winners (already in ascending batch order) from shard 0
  uint64_t total = 0;
  bmx_merge_stats tot; std::memset(&tot, 0, sizeof(tot));
  std::vector<bmx_merge_stats> hs(N);
  for (uint32_t g = 0; g < N; g++) {
    std::memset(&hs[g], 0, sizeof(bmx_merge_stats));
    HIPCHK_ON(c, hipSetDevice(c->dev[g]));
    HIPCHK_ON(c, hipMemcpyAsync(&hs[g], c->s[g].stats, sizeof(bmx_merge_stats), hipMemcpyDeviceToHost, reinterpret_cast<hipStream_t>(bmx_get_stream(c->sh[g]))));
  }
  for (uint32_t g = 0; g < N; g++) {
    CSH(g, bmx_sync(c->sh[g]));             // waits for the shard's stream and reports its sticky device errors
    if (!m[g]) { uint64_t r = 0; CSH(g, bmx_row_count(c->sh[g], &r)); std::memset(&hs[g], 0, sizeof(bmx_merge_stats)); hs[g].n_rows = r; }
    tot.n_applied += hs[g].n_applied; tot.n_conflicts += hs[g].n_conflicts; tot.n_rows += hs[g].n_rows;
  }
  if (applied_idx && n) {
    unsigned long long w = 0;
    HIPCHK_ON(c, hipSetDevice(c->dev[0]));
    HIPCHK_ON(c, hipMemcpy(&w, c->win.n, sizeof(w), hipMemcpyDeviceToHost));
    if (w != tot.n_applied) return fail(c, BMX_ERR_INTERNAL, "winner map and per-shard winner counts disagree");
    if (w) HIPCHK_ON(c, hipMemcpy(applied_idx, c->win.applied, w * 4, hipMemcpyDeviceToHost));
  }
  total = tot.n_applied;
  if (n_applied) *n_applied = total;
  if (stats) *stats = tot;
  return BMX_OK;
}
// bmx_comm_load_rows (MODE_LOAD) / bmx_comm_put_rows (MODE_PUT)
int comm_load_rows(bmx_comm* c, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val, const MergeMode& mode) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  DevGuard guard;
  return in_load_chunks(n, id, field, ts, val, [&](const MergeIn& p) { return comm_host_batch(c, p.n, p.id, p.field, p.ts, p.val, mode, nullptr, nullptr, nullptr); });
}
}  // namespace

extern "C" {

const char* bmx_comm_last_error(const bmx_comm* c) { return c ? c->err.c_str() : g_comm_err.c_str(); }
uint32_t bmx_comm_nshards(const bmx_comm* c) { return c ? c->N : 0; }
bmx_ctx* bmx_comm_shard(bmx_comm* c, uint32_t i) { return (c && i < c->N) ? c->sh[i] : nullptr; }

int bmx_comm_create(uint32_t nshards, const int* devices, uint64_t capacity_rows_per_shard, uint32_t flags, bmx_comm** out) {
  if (!out || nshards == 0 || nshards > PART_MAX_SHARDS || !devices || capacity_rows_per_shard == 0)
    return fail<bmx_comm>(nullptr, BMX_ERR_INVALID, "bmx_comm_create: bad arguments (1..16 shards)");
  *out = nullptr;
  DevGuard guard;
  bmx_comm* c = new (std::nothrow) bmx_comm();
  if (!c) return fail<bmx_comm>(nullptr, BMX_ERR_NOMEM, "out of host memory");
  c->N = nshards; c->dev.assign(devices, devices + nshards); c->sh.assign(nshards, nullptr); c->s.resize(nshards);
  auto bail = [&](int rc) { std::string m = c->err; bmx_comm_destroy(c); g_comm_err = m; return rc; };
  for (uint32_t g = 0; g < nshards; g++) {
    if (int rc = bmx_create(devices[g], capacity_rows_per_shard, flags, &c->sh[g])) return bail(fail(c, rc, shard_msg(c, g)));
    c->sh[g]->defer.enabled = false;   // the communicator orders its shards' streams with events right behind their merges: every compaction stays on its stream
    bmx_comm::Shard& S = c->s[g];
    HIPCHK_BAIL(c, hipSetDevice(devices[g]));
    if (int rc = dev_alloc_all(c, {{S.counts, PART_MAX_SHARDS * sizeof(unsigned long long)}, {S.n_applied, sizeof(unsigned long long)}, {S.stats, sizeof(bmx_merge_stats)}})) return bail(rc);
    HIPCHK_BAIL(c, hipMemset(S.n_applied, 0, sizeof(unsigned long long)));
    HIPCHK_BAIL(c, hipMemset(S.stats, 0, sizeof(bmx_merge_stats)));
    HIPCHK_BAIL(c, hipEventCreateWithFlags(&S.routed, hipEventDisableTiming));
    HIPCHK_BAIL(c, hipEventCreateWithFlags(&S.merged, hipEventDisableTiming));
  }
  HIPCHK_BAIL(c, hipSetDevice(devices[0]));
  if (int rc = dev_alloc(c, &c->win.n, 1)) return bail(rc);
  HIPCHK_BAIL(c, hipEventCreateWithFlags(&c->win.zeroed, hipEventDisableTiming));
  // peer access between distinct devices (the device path stores straight into the owners' receive buffers)
  for (uint32_t a = 0; a < nshards; a++)
    for (uint32_t b = 0; b < nshards; b++)
      if (devices[a] != devices[b]) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, devices[a], devices[b]) != hipSuccess || !can) return bail(fail(c, BMX_ERR_HIP, "bmx_comm_create: GPUs of one communicator must be peer-accessible"));
        (void)hipSetDevice(devices[a]);
        hipError_t e = hipDeviceEnablePeerAccess(devices[b], 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return bail(fail(c, BMX_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e)));
        (void)hipGetLastError();
      }
  *out = c;
  return BMX_OK;
}

void bmx_comm_destroy(bmx_comm* c) {
  if (!c) return;
  DevGuard guard;
  for (uint32_t g = 0; g < c->N; g++) { if (c->sh[g]) { (void)hipSetDevice(c->dev[g]); (void)hipDeviceSynchronize(); } }
  for (uint32_t g = 0; g < c->N; g++) {
    (void)hipSetDevice(c->dev[g]);
    c->s[g].release();
    if (c->sh[g]) bmx_destroy(c->sh[g]);
  }
  if (c->N) (void)hipSetDevice(c->dev[0]);
  c->win.release();
  delete c;
}

int bmx_comm_sync(bmx_comm* c) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  DevGuard guard;
  int first = BMX_OK; std::string msg;
  for (uint32_t g = 0; g < c->N; g++) {
    int rc = bmx_sync(c->sh[g]);
    if (rc && !first) { first = rc; msg = shard_msg(c, g); }
  }
  c->dev_step_pending = false;
  return first ? fail(c, first, msg) : BMX_OK;
}

int bmx_comm_load_rows(bmx_comm* c, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val) { return comm_load_rows(c, n, id, field, ts, val, MODE_LOAD); }
int bmx_comm_put_rows(bmx_comm* c, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val) { return comm_load_rows(c, n, id, field, ts, val, MODE_PUT); }

int bmx_comm_merge(bmx_comm* c, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val, int insert_mode,
                   uint32_t* applied_idx, uint64_t* n_applied, bmx_merge_stats* stats) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  DevGuard guard;
  MergeMode mode; if (const char* bad = merge_mode_of(insert_mode, &mode)) return fail(c, BMX_ERR_INVALID, bad);
  if (mode.strict) return fail(c, BMX_ERR_INVALID, "bmx_comm_merge: per-delta flags are not collected across shards");
  return comm_host_batch(c, n, id, field, ts, val, mode, applied_idx, n_applied, stats);
}

int bmx_comm_merge_dev(bmx_comm* c, const uint64_t* n, const uint64_t* const* id, const uint32_t* const* field, const int64_t* const* ts,
                       const int64_t* const* val, int insert_mode, uint64_t slab_records) {
  if (!c || !n || !id || !field || !ts || !val) return fail(c, BMX_ERR_INVALID, "bmx_comm_merge_dev: null argument");
  MergeMode mode; if (const char* bad = merge_mode_of(insert_mode, &mode)) return fail(c, BMX_ERR_INVALID, bad);   // before anything is routed; the shards' bmx_merge_records take insert_mode as it is
  DevGuard guard;
  const uint32_t N = c->N;
  uint64_t nmax = 0;
  for (uint32_t i = 0; i < N; i++) { if (n[i] > MAX_BATCH) return fail(c, BMX_ERR_INVALID, "batch larger than 2^24 deltas"); nmax = std::max(nmax, n[i]); }
  if (slab_records == 0) slab_records = nmax / N + nmax / (8 * N) + 64;          // 12.5 % head room over the mean run
  if (slab_records * N > 0xFFFFFFFFull) return fail(c, BMX_ERR_INVALID, "slab too large");
  int rc;
  for (uint32_t g = 0; g < N; g++) {
    if ((rc = comm_ensure_recv(c, g, (uint64_t)N * slab_records))) return rc;
    c->s[g].slab = slab_records;
  }
  // 1. every origin scatters straight into its owners' receive slabs (slab i of every receive buffer belongs to origin i); the owners'
  //    previous merges must have finished reading those buffers
  for (uint32_t i = 0; i < N; i++) {
    HIPCHK_ON(c, hipSetDevice(c->dev[i]));
    hipStream_t st = reinterpret_cast<hipStream_t>(bmx_get_stream(c->sh[i]));
    for (uint32_t g = 0; g < N; g++) if (g != i) HIPCHK_ON(c, hipStreamWaitEvent(st, c->s[g].merged, 0));
    PartOut po; std::memset(&po, 0, sizeof(po));
    for (uint32_t g = 0; g < N; g++) po.base[g] = c->s[g].recv + (size_t)i * slab_records;
    CSH(i, partition_impl(c->sh[i], n[i], id[i], field[i], ts[i], val[i], N, slab_records, nullptr, reinterpret_cast<uint64_t*>(c->s[i].counts), &po, 0));
    HIPCHK_ON(c, hipEventRecord(c->s[i].routed, st));
  }
  // 2. every owner merges its N slabs once all origins have scattered
  for (uint32_t g = 0; g < N; g++) {
    HIPCHK_ON(c, hipSetDevice(c->dev[g]));
    hipStream_t st = reinterpret_cast<hipStream_t>(bmx_get_stream(c->sh[g]));
    for (uint32_t i = 0; i < N; i++) if (i != g) HIPCHK_ON(c, hipStreamWaitEvent(st, c->s[i].routed, 0));
    CSH(g, bmx_merge_records(c->sh[g], (uint64_t)N * slab_records, c->s[g].recv, insert_mode, c->s[g].applied, reinterpret_cast<uint64_t*>(c->s[g].n_applied), nullptr, c->s[g].stats));
    HIPCHK_ON(c, hipEventRecord(c->s[g].merged, st));
  }
  c->dev_step_pending = true;
  return BMX_OK;
}

int bmx_comm_shard_result(bmx_comm* c, uint32_t shard, const bmx_delta_rec** recs_dev, const uint32_t** applied_dev, const uint64_t** n_applied_dev,
                          const bmx_merge_stats** stats_dev, uint64_t* n_records) {
  if (!c || shard >= c->N) return fail(c, BMX_ERR_INVALID, "bad shard");
  const bmx_comm::Shard& S = c->s[shard];
  if (recs_dev) *recs_dev = S.recv;
  if (applied_dev) *applied_dev = S.applied;
  if (n_applied_dev) *n_applied_dev = reinterpret_cast<const uint64_t*>(S.n_applied);
  if (stats_dev) *stats_dev = S.stats;
  if (n_records) *n_records = (uint64_t)c->N * S.slab;
  return BMX_OK;
}

int bmx_comm_row_count(bmx_comm* c, uint64_t* n_out) {
  if (!c || !n_out) return fail(c, BMX_ERR_INVALID, "bad arguments");
  DevGuard guard;
  uint64_t tot = 0;
  for (uint32_t g = 0; g < c->N; g++) { uint64_t r = 0; CSH(g, bmx_row_count(c->sh[g], &r)); tot += r; }
  *n_out = tot;
  return BMX_OK;
}

int bmx_comm_get_rows(bmx_comm* c, uint64_t n, const uint64_t* id, const uint32_t* field, int64_t* ts, int64_t* val, uint8_t* found) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  DevGuard guard;
  if (n == 0) return BMX_OK;
  if (!id || !field || !ts || !val || !found) return fail(c, BMX_ERR_INVALID, "null pointer");
  std::vector<std::vector<uint64_t>> pos(c->N);
  for (uint64_t j = 0; j < n; j++) pos[bmx_owner_of(id[j], c->N)].push_back(j);
  for (uint32_t g = 0; g < c->N; g++) {
    const size_t k = pos[g].size();
    if (!k) continue;
    std::vector<uint64_t> gi(k); std::vector<uint32_t> gf(k); std::vector<int64_t> gt(k), gv(k); std::vector<uint8_t> gfd(k);
    for (size_t x = 0; x < k; x++) { gi[x] = id[pos[g][x]]; gf[x] = field[pos[g][x]]; }
    CSH(g, bmx_get_rows(c->sh[g], k, gi.data(), gf.data(), gt.data(), gv.data(), gfd.data(), BMX_MEM_HOST));
    for (size_t x = 0; x < k; x++) { ts[pos[g][x]] = gt[x]; val[pos[g][x]] = gv[x]; found[pos[g][x]] = gfd[x]; }
  }
  return BMX_OK;
}

int bmx_comm_dump_rows(bmx_comm* c, uint64_t cap, uint64_t* id, uint32_t* field, int64_t* ts, int64_t* val, uint64_t* n_out) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  DevGuard guard;
  uint64_t tot = 0;
  for (uint32_t g = 0; g < c->N; g++) {
    uint64_t m = 0;
    const uint64_t room = cap > tot ? cap - tot : 0;
    CSH(g, bmx_dump_rows(c->sh[g], room, room ? id + tot : nullptr, room ? field + tot : nullptr, room ? ts + tot : nullptr, room ? val + tot : nullptr, &m, BMX_MEM_HOST));
    tot += m;
  }
  if (n_out) *n_out = tot;
  return BMX_OK;
}

int bmx_comm_index_build(bmx_comm* c, uint32_t field) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  DevGuard guard;
  for (uint32_t g = 0; g < c->N; g++) CSH(g, bmx_index_build(c->sh[g], field));
  return BMX_OK;
}

// value-ordered views on every shard's index of `field` (bmx.h bmx_index_set_ordered): each shard answers from its own sorted copy, concatenated as ever
int bmx_comm_index_set_ordered(bmx_comm* c, uint32_t field, uint32_t after_queries) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  DevGuard guard;
  for (uint32_t g = 0; g < c->N; g++) CSH(g, bmx_index_set_ordered(c->sh[g], field, after_queries));
  return BMX_OK;
}

// Sharded scan (src/bullet-query.js:221-261, 186-210 on a graph split over shards): every shard scans its own rows, the results are
// concatenated in shard order. Two phases: the scans of ALL shards are enqueued first (each into its context's own result buffer), then the
// results are fetched shard by shard — N GPUs scan at the same time, and the host waits once per shard for work that is already running.
}  // extern "C"
namespace {
// (bmx_where.inc sits behind this file in bmx.hip's include list)
const char* where_prepare(uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, WhereProg* out);
int where_run(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem, bool deferred);
template <class Enqueue>   // enqueue(shard context, want, cap): the shard's deferred host-mode scan
int comm_scan_with(bmx_comm* c, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, Enqueue enqueue) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  DevGuard guard;
  uint64_t* want = (out_ids && cap) ? out_ids : nullptr;
  uint64_t tot = 0;
  const int rc = comm_two_phase(c,
    [&](uint32_t, bmx_ctx* x) { return enqueue(x, want, cap); },
    [&](uint32_t, bmx_ctx* x) {
      uint64_t m = 0;
      const uint64_t room = (want && cap > tot) ? cap - tot : 0;
      const int crc = scan_collect(x, room ? out_ids + tot : nullptr, room, &m);
      tot += m;
      return crc;
    });
  if (rc) return rc;
  if (n_out) *n_out = tot;
  return BMX_OK;
}
}  // namespace
extern "C" {
static int comm_scan(bmx_comm* c, uint32_t field, int64_t lo, int64_t hi, uint32_t nterms, const bmx_term* terms, uint64_t* out_ids, uint64_t cap, uint64_t* n_out) {
  return comm_scan_with(c, out_ids, cap, n_out, [&](bmx_ctx* x, uint64_t* want, uint64_t wcap) {
    return terms ? scan_filter_impl(x, nterms, terms, want, wcap, nullptr, BMX_MEM_HOST, /*deferred=*/true) : scan_range_impl(x, field, lo, hi, want, wcap, nullptr, BMX_MEM_HOST, /*deferred=*/true);
  });
}
int bmx_comm_scan_range(bmx_comm* c, uint32_t field, int64_t lo, int64_t hi, uint64_t* out_ids, uint64_t cap, uint64_t* n_out) {
  return comm_scan(c, field, lo, hi, 0, nullptr, out_ids, cap, n_out);
}
int bmx_comm_scan_equals(bmx_comm* c, uint32_t field, int64_t value, uint64_t* out_ids, uint64_t cap, uint64_t* n_out) {
  return comm_scan(c, field, value, value, 0, nullptr, out_ids, cap, n_out);
}
int bmx_comm_scan_count(bmx_comm* c, uint32_t field, int64_t lo, int64_t hi, uint64_t* n_out) {
  return comm_scan(c, field, lo, hi, 0, nullptr, nullptr, 0, n_out);
}
int bmx_comm_scan_filter(bmx_comm* c, uint32_t nterms, const bmx_term* terms, uint64_t* out_ids, uint64_t cap, uint64_t* n_out) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  if (nterms == 0 || !terms) return fail(c, BMX_ERR_INVALID, "filter needs 1..8 terms");
  return comm_scan(c, 0, 0, 0, nterms, terms, out_ids, cap, n_out);
}

// bmx_scan_where over the shards (bmx_where.h, host memory): the program is checked and prepared once, then every shard sweeps its own index of the base field. A node's rows
// all live on the shard that owns its id, so every literal of a candidate is decided on its own shard.
int bmx_comm_scan_where(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint64_t* out_ids, uint64_t cap,
                        uint64_t* n_out) {
  WhereProg W;
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  return comm_scan_with(c, out_ids, cap, n_out, [&](bmx_ctx* x, uint64_t* want, uint64_t wcap) {
    const int erc = enter(x);
    return erc ? erc : where_run(x, base_field, W, want, wcap, nullptr, BMX_MEM_HOST, /*deferred=*/true);
  });
}

}  // extern "C"
namespace {
// The shards' aggregate records combined into `out` (host memory). A node's rows all live on the shard that owns its id, so a node is selected, measured and
// grouped by one shard alone and the shards' records combine exactly: the counts and the 128-bit sums add, the minima and maxima fold. enqueue(shard) enqueues
// the query into the shard's staging buffer; every shard's query is enqueued before the first shard's records are fetched.
template <class Enqueue>
int comm_agg_with(bmx_comm* c, uint32_t ngroups, bmx_agg* out, Enqueue enqueue) {
  DevGuard guard;
  const uint32_t nrec = agg_records(ngroups);
  std::vector<bmx_agg> part(nrec);
  return comm_two_phase(c,
    [&](uint32_t, bmx_ctx* x) { const int rc = enter(x); return rc ? rc : enqueue(x); },
    [&](uint32_t g, bmx_ctx* x) {
      int rc = enter(x);
      if (!rc) rc = agg_collect(x, nrec, g == 0 ? out : part.data());
      if (rc || g == 0) return rc;
      for (uint32_t r = 0; r < nrec; r++) {
        bmx_agg& o = out[r]; const bmx_agg& p = part[r];
        o.n_match += p.n_match; o.n += p.n;
        o.min = std::min(o.min, p.min); o.max = std::max(o.max, p.max);
        const unsigned __int128 s = (((unsigned __int128)(uint64_t)o.sum_hi << 64) | o.sum_lo) + (((unsigned __int128)(uint64_t)p.sum_hi << 64) | p.sum_lo);
        o.sum_lo = (uint64_t)s; o.sum_hi = (int64_t)(uint64_t)(s >> 64);
      }
      return BMX_OK;
    });
}

// The shards' top-k answers merged into `out` (host memory). A node lives on one shard and the order (value, id) is total, so the first k of the whole graph are
// the first k of the shards' first k: every shard's query is enqueued (enqueue(shard), into the shard's staging buffer) before the first answer is fetched, the
// answers (each ordered, <= k records) are merged on the host and the shards' n_eligible add up.
template <class Enqueue>
int comm_top_with(bmx_comm* c, uint32_t flags, uint32_t k, bmx_top_rec* out, uint64_t* n_out, uint64_t* n_eligible, Enqueue enqueue) {
  DevGuard guard;
  const bool desc = (flags & BMX_TOP_DESC) != 0;
  auto before = [desc](const bmx_top_rec& a, const bmx_top_rec& b) { return a.val != b.val ? (desc ? a.val > b.val : a.val < b.val) : a.id < b.id; };
  std::vector<bmx_top_rec> all, part, tmp;
  uint64_t tot = 0;
  const int rc = comm_two_phase(c,
    [&](uint32_t, bmx_ctx* x) { const int erc = enter(x); return erc ? erc : enqueue(x); },
    [&](uint32_t, bmx_ctx* x) {
      uint64_t ne = 0;
      int crc = enter(x);
      if (!crc) crc = top_collect(x, k, part, &ne);
      if (crc) return crc;
      tot += ne;
      tmp.resize(all.size() + part.size());
      std::merge(all.begin(), all.end(), part.begin(), part.end(), tmp.begin(), before);
      if (tmp.size() > k) tmp.resize(k);
      all.swap(tmp);
      return BMX_OK;
    });
  if (rc) return rc;
  if (!all.empty()) std::memcpy(out, all.data(), all.size() * sizeof(bmx_top_rec));
  if (n_out) *n_out = all.size();
  if (n_eligible) *n_eligible = tot;
  return BMX_OK;
}
}  // namespace
extern "C" {

// bmx_scan_aggregate over the shards (host memory): comm_agg_with
int bmx_comm_scan_aggregate(bmx_comm* c, uint32_t nterms, const bmx_term* terms, uint32_t measure_field, uint32_t group_field, int64_t group_lo, uint32_t ngroups,
                            bmx_agg* out) {
  if (const char* bad = agg_bad_args(nterms, terms, group_field, ngroups, out)) return fail(c, BMX_ERR_INVALID, bad);
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  return comm_agg_with(c, ngroups, out, [&](bmx_ctx* x) { return agg_enqueue(x, nterms, terms, measure_field, group_field, group_lo, ngroups, nullptr); });
}

// bmx_scan_top over the shards (bmx_top.h, host memory): comm_top_with
int bmx_comm_scan_top(bmx_comm* c, uint32_t nterms, const bmx_term* terms, uint32_t flags, const bmx_top_rec* after, uint32_t k, bmx_top_rec* out, uint64_t* n_out,
                      uint64_t* n_eligible) {
  if (const char* bad = top_bad_args(nterms, terms, flags, k, out)) return fail(c, BMX_ERR_INVALID, bad);
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  return comm_top_with(c, flags, k, out, n_out, n_eligible, [&](bmx_ctx* x) { return top_enqueue(x, nterms, terms, flags, after, k, nullptr, nullptr, nullptr); });
}

// Replica reconciliation over the shards (bmx.h). The shards' key sets are disjoint and the digest is a sum, so the digest of the sharded graph is the
// element-wise sum of the shards' vectors — the same vectors one context holding all the rows would give. Host memory.
int bmx_comm_digest(bmx_comm* c, uint32_t log2_buckets, uint32_t flags, uint64_t* sums, uint64_t* counts) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  if (log2_buckets > 16 || !sums || !counts) return fail(c, BMX_ERR_INVALID, "bmx_comm_digest: log2_buckets > 16 or null output");
  DevGuard guard;
  const uint64_t B = 1ull << log2_buckets;
  std::vector<uint64_t> s(B), n(B);
  std::memset(sums, 0, B * sizeof(uint64_t)); std::memset(counts, 0, B * sizeof(uint64_t));
  for (uint32_t g = 0; g < c->N; g++) {
    CSH(g, bmx_digest(c->sh[g], log2_buckets, flags, s.data(), n.data(), BMX_MEM_HOST));
    for (uint64_t b = 0; b < B; b++) { sums[b] += s[b]; counts[b] += n[b]; }
  }
  return BMX_OK;
}

// bmx_export_rows shard after shard into one host array (like bmx_comm_dump_rows): shard order, table order inside a shard
int bmx_comm_export_rows(bmx_comm* c, int64_t since_ts, uint32_t log2_buckets, const uint64_t* bucket_bits, uint32_t flags, bmx_delta_rec* out, uint64_t cap,
                         uint64_t* n_out) {
  if (!c) return fail(c, BMX_ERR_INVALID, "null communicator");
  DevGuard guard;
  uint64_t tot = 0;
  for (uint32_t g = 0; g < c->N; g++) {
    uint64_t m = 0;
    const uint64_t room = (out && cap > tot) ? cap - tot : 0;
    CSH(g, bmx_export_rows(c->sh[g], since_ts, log2_buckets, bucket_bits, flags, room ? out + tot : nullptr, room, &m, BMX_MEM_HOST));
    tot += m;
  }
  if (n_out) *n_out = tot;
  return BMX_OK;
}

}  // extern "C"
