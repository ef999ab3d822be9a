// bmx.hip — C ABI (include/bmx.h) over the gfx950 kernels. One context = one GPU + one HIP stream.
// No CPU fallback exists: every entry point fails with BMX_ERR_NO_DEVICE / BMX_ERR_HIP when there is no GPU.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <deque>
#include <initializer_list>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/bmx.h"
#include "merge_kernels.h"
#include "scan_kernels.h"
#include "select.h"
#include "slot.h"
#include "sync_kernels.h"
#include "view_kernels.h"
#include "agg_kernels.h"

namespace bmx {   // csrc/ordered_sort.hip (rocPRIM's radix sort, an object of its own)
hipError_t sort_pairs_i32(void* tmp, size_t* tmp_bytes, const int32_t* kin, int32_t lo, unsigned bits, uint32_t* kout, const uint32_t* vin, uint32_t* vout, size_t n, hipStream_t s);
hipError_t sort_pairs_i64(void* tmp, size_t* tmp_bytes, const int64_t* kin, int64_t lo, unsigned bits, uint64_t* kout, const uint32_t* vin, uint32_t* vout, size_t n, hipStream_t s);
}

using namespace bmx;

// count, stats and device status of one host batch, written by k_small_tail into mapped host memory
struct SmallOut { unsigned long long n_applied; bmx_merge_stats stats; uint32_t status; uint32_t pad; };

namespace {

struct DevScalars {  // one small device allocation; zeroed at create
  unsigned long long row_count;
  unsigned long long n_out;        // scratch count for host-mode calls
  unsigned long long part_totals[PART_MAX_SHARDS];
  bmx_merge_stats stats;           // scratch stats for host-mode calls
  uint32_t status;
  uint32_t wide;
  unsigned long long seq_diag[3];  // k_seq_wait expiry: {sequence word address, value waited for, value last seen}
  unsigned long long chg_n[2];     // entries in the index change log: batch k reads [k&1], its compaction writes [(k+1)&1]
  unsigned long long ord_ab[6];    // value-ordered view: [first match, one past the last) of the query being answered in the view's main run, its pending deleted keys, its pending inserted keys
  unsigned long long view_cl_n[8]; // keys in the change run of maintained index k (k_ix_update capture mode: view_kernels.h)
  uint32_t view_err, view_pad;     // a deleted key was not found in the view it is patched into
  unsigned long long view_tmp[2];  // how a change run's deleted keys split: keys of main / pending inserted keys
  unsigned long long seqw[2];      // deferred compaction: [0] = number of the latest probe kernel that has started, [1] = of the latest compaction finished on the side stream
};

// The value-ordered view of one index (bmx.h bmx_index_set_ordered): the columns once more, sorted by (value, position), and kept current under writes.
// Its code is bmx_view.inc and ensure_ordered_view. Copied with its Index (ctx->indexes is a vector): no destructor, release() gives the buffers back.
struct OrderedView {
  uint32_t ordered_after = 0;     // 0 = off; N: a stale view is sorted again by the N-th query since the columns last changed
  uint32_t stale_queries = 0;     // queries answered by the column scan since the columns last CHANGED (not: since the last sort)
  uint64_t stale_content = ~0ull; // the `content` value that count belongs to: a new change starts it again
  double last_sort_us = 0;        // what the last sort of the view cost the caller (BMX_INDEX_ORDERED_AUTO weighs it against the scans it saves)
  uint64_t ord_content = ~0ull;   // `content` the view was sorted from
  uint64_t ord_n = 0, ord_cap = 0, ord_sorts = 0;
  bool ord_fits32 = false;
  void* s_val = nullptr;          // int32_t[ord_n] or int64_t[ord_n], ascending
  uint32_t* s_pos = nullptr;      // position in the index columns
  uint64_t* s_ids = nullptr;      // node id
  // kept current under writes (view_kernels.h): the second set of columns a patch merges into (allocated by the first patch, then the two sets swap),
  // the change run k_ix_update captures, and what the patches did
  void* s_val2 = nullptr; uint32_t* s_pos2 = nullptr; uint64_t* s_ids2 = nullptr; uint64_t ord_cap2 = 0;
  uint32_t* cl_pos = nullptr; int64_t* cl_old = nullptr; uint64_t cl_cap = 0;      // the captured change run, one entry per log entry (holes: POS_NONE)
  uint32_t* cl2_pos = nullptr; int64_t* cl2_old = nullptr;                          // ... and without the holes
  uint64_t ord_patches = 0, ord_patched_keys = 0, ord_merges = 0; double last_patch_us = 0;
  // the view's PENDING patch: logical view = main - pd + pi (both sorted by (value, position); pi carries ids). A refresh merges its change run into these small
  // runs; the streaming merge into main runs when they have grown past ord_n / 16 keys. Two sets: a merge writes the other one.
  void* pd_v[2] = {nullptr, nullptr}; uint32_t* pd_p[2] = {nullptr, nullptr};
  void* pi_v[2] = {nullptr, nullptr}; uint32_t* pi_p[2] = {nullptr, nullptr}; uint64_t* pi_ids[2] = {nullptr, nullptr};
  uint8_t* pi_dead = nullptr;          // one byte per key of pi: set for the inserts a refresh's deleted keys cancel (scratch of the join)
  uint64_t npd = 0, npi = 0, pend_cap = 0; int pcur = 0 /* the current set of pd */, icur = 0 /* the current set of pi */;
  // the rewrite of main (main - pd + pi -> the second set of columns) runs BEHIND the answer of the query that found it due: in flight until its event has completed
  // and its error word has been looked at; until then (main, pd, pi) go on answering
  bool rewrite_due = false, rewrite_inflight = false; uint64_t rewrite_nz = 0;
  void release_pending();   // the pending patch's buffers; the patch is empty and no rewrite is due or in flight
  void release();           // every buffer (the pending patch's too): the view is stale until sorted again
};
struct Index {
  uint32_t field = 0;
  uint64_t n = 0, cap = 0;
  uint64_t* ids = nullptr; int64_t* v64 = nullptr; int32_t* v32 = nullptr;   // the columns (free_columns)
  bool fits32 = false;
  uint64_t version = ~0ull;  // table version it was built from
  bool has_pos = false;      // its rows' positions are in ctx->chg.slot_pos (it can be maintained from the change log)
  uint64_t content = 0;      // counts the refreshes that really changed something in the columns (a value, a new row, a rebuild)
  OrderedView view;
};
// What the views of one context share (bmx_view.inc).
struct ViewShared {
  // sort scratch of the view patches (view_kernels.h): two key arrays (value 8 B, position 4 B) the merge sort ping-pongs between
  void* vk_v[2] = {nullptr, nullptr}; uint32_t* vk_p[2] = {nullptr, nullptr}; uint64_t vk_cap = 0;
  void* vk_sv = nullptr; uint32_t* vk_sp = nullptr; uint32_t* vk_d0 = nullptr; uint32_t* vk_y0 = nullptr; uint64_t vk_tiles_cap = 0;   // per tile of the view: its first key (the sample), deleted indices / inserted keys in front of it
  uint32_t* err_host = nullptr; hipEvent_t ev = nullptr;      // a background rewrite's error word (page-locked host memory) and completion event
  bool patching = true;           // BMX_VIEW_PATCH=0: a change makes the view stale as in round 4 (A/B switch)
  int test_fail = 0;              // BMX_TEST_VIEW_FAIL (test hook): 1 = every patch reports failure (the view goes stale), 2 = every background rewrite reports failure (main + patch go on answering)
  bool own_sort = false;          // BMX_VIEW_SORT=own: a new view is sorted by the patch path's own kernels (tile sort + merge passes) instead of rocPRIM's radix sort (A/B switch)
  bool pending = true;            // BMX_VIEW_PENDING=0: every patch rewrites the view's main run at once (no pending patch; A/B switch)
  bool debug = false;             // BMX_VIEW_DEBUG: diagnostic prints to stderr (patches given up, rewrite and refresh timings)
  void read_env();                // the switches above, at create
  void release();
};

thread_local std::string g_err;
constexpr uint32_t PROF_MAX_CALLS = 64;

template <class T>
void dev_free(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}
// One all-or-nothing group of device buffers: what the pointers of the list hold goes back, then every one gets a new buffer, or none does (what was
// allocated goes back, the HIP error is cleared and handed to `err`). dev_alloc_all is the same for a context's entry points.
struct DevBuf { void** p; size_t bytes; template <class T> DevBuf(T*& q, size_t b) : p(reinterpret_cast<void**>(&q)), bytes(b) {} };
bool alloc_all(std::initializer_list<DevBuf> bufs, hipError_t* err = nullptr) {
  for (const DevBuf& b : bufs) dev_free(*b.p);
  for (const DevBuf* b = bufs.begin(); b != bufs.end(); b++) {
    const hipError_t e = hipMalloc(b->p, b->bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      *b->p = nullptr;
      for (const DevBuf* f = bufs.begin(); f != b; f++) dev_free(*f->p);
      if (err) *err = e;
      return false;
    }
  }
  return true;
}

// The merge's per-batch workspace (merge_core), grown on demand.
struct MergeWs {
  // what the compaction (K3) reads is kept per batch PARITY, so that the compaction of batch b can run on a second stream while the probe
  // kernel of batch b + 1 fills the other set ("deferred compaction", merge_core): winner bytes, the claimers' slots, the deltas' field
  // hashes (for the index change log) and the sharded counters
  // THREE sets: while batch k is probed the compactions of batches k - 1 (just released) and k - 2 (not waited for yet) may both still be reading theirs
  static constexpr uint32_t SETS = 3, BLK_SEGS = 4;
  uint32_t cap = 0;
  uint32_t* next = nullptr;
  uint8_t* wflag[SETS] = {nullptr, nullptr, nullptr};
  uint32_t* slot_of[SETS] = {nullptr, nullptr, nullptr};
  uint32_t* fld[SETS] = {nullptr, nullptr, nullptr};
  uint32_t par = 0;
  uint32_t* blk_info = nullptr;       // 4 x (cap/256 + 16) block summaries: batch k adds into segment k % 4 and k_probe_apply zeroes segment (k + 1) % 4 for batch k + 1;
                                      // four, because the compactions of batches k - 1 and k - 2 may still read theirs while batch k is probed
  uint32_t blk_half = 0, blk_seg = 0; bool blk_clean[BLK_SEGS] = {false, false, false, false};   // blk_clean[h]: segment h is known to be all zero
  uint32_t* blk_follow = nullptr;     // cap/256 epoch tags: a delta of the block got a follower on its row
  unsigned long long* shard_ctr = nullptr;  // SETS x CTR_SHARDS * CTR_STRIDE (one per workspace set), allocated at create
  int ensure(bmx_ctx* ctx, uint64_t n);     // room for a batch of n deltas
  void release() {
    dev_free(next); dev_free(blk_info); dev_free(blk_follow); dev_free(shard_ctr);
    for (uint32_t h = 0; h < SETS; h++) { dev_free(wflag[h]); dev_free(slot_of[h]); dev_free(fld[h]); }
    cap = 0;
  }
};

// Deferred compaction (merge_core): the compaction of a device-resident batch is not launched with the batch. If the next call is another such
// merge, it goes to a high-priority side stream behind a one-wave wait for that merge's probe kernel to START (= everything of this batch is
// done), and runs under that probe kernel; anything else launches it on the context's stream first (flush_pending).
struct Deferral {
  struct PendingK3 {
    bool on = false;
    const uint8_t* wflag = nullptr; const uint32_t* blk = nullptr; uint32_t n = 0; uint32_t* applied = nullptr;
    FinishMerge Fin{}; ChgLog L{}; uint32_t mark_created = 0; bool notify_after = false; uint64_t notify_seq = 0; uint64_t seq = 0;
  } pend;
  bool enabled = true;
  hipStream_t side = nullptr;
  bool side_is_callers = false;       // bmx_set_side_stream: the deferred compactions run on a stream the caller owns (the sharded pipeline's exchange stream)
  uint64_t seq = 0;                   // deferred merges so far (the sequence numbers in ds->seqw)
  uint64_t side_last = 0, side_prev = 0;   // sequence numbers of the last two compactions launched on the side stream (0: none this stream is not ordered behind already)
  uint64_t n_deferred = 0, n_side = 0;   // merges whose compaction was deferred / actually ran on the side stream (bmx_get_deferred_counts)
  void release() {                    // the side stream finishes; it is destroyed only if the library created it
    if (!side) return;
    (void)hipStreamSynchronize(side);
    if (!side_is_callers) (void)hipStreamDestroy(side);
    side = nullptr;
  }
};

// What exists only for BMX_MEM_HOST calls (bmx_host.inc): staging, copy streams, mapped host memory, the point reads' columns.
struct HostIO {
  // Two staging sets: batch b+1 is uploaded (copy stream) while batch b is merged (main stream); bmx_merge_submit / bmx_merge_collect
  struct Staging {
    uint32_t cap = 0;
    uint64_t* id = nullptr; uint32_t* field = nullptr; int64_t* ts = nullptr; int64_t* val = nullptr;
    uint32_t* applied = nullptr; uint8_t* flags = nullptr;
    unsigned long long* n_out = nullptr; bmx_merge_stats* stats = nullptr;   // device words of this set
    SmallOut* tail = nullptr;                                                 // the same, in mapped host memory (null: copied down instead)
    hipEvent_t up = nullptr, done = nullptr;                                  // inputs uploaded / kernels of the batch finished
    uint64_t n = 0; bool want_flags = false; bool busy = false; uint64_t ticket = 0;
  } stg[2];
  SmallOut* tails = nullptr;           // mapped host memory behind stg[i].tail
  // small host batches (<= SMALL_HOST_N deltas): inputs are packed into mapped host memory the kernels read directly, results are written
  // straight into mapped host memory: three launches and one stream synchronisation per call, no copies, no second stream
  uint8_t* pin_in = nullptr; uint8_t* pin_out = nullptr;
  hipStream_t copy_stream = nullptr;   // uploads
  hipStream_t down_stream = nullptr;   // downloads (PCIe is full duplex: results of batch b come back while batch b+1 goes up)
  uint64_t next_ticket = 1;
  volatile unsigned long long* hres = nullptr;   // mapped page-locked result words (HRES_*): counts the host waits for arrive without a download
  // persistent device buffers of the host-mode point reads and dumps (grow-only)
  uint64_t pr_cap = 0;
  uint64_t* pr_id = nullptr; uint32_t* pr_field = nullptr; int64_t* pr_ts = nullptr; int64_t* pr_val = nullptr; uint8_t* pr_found = nullptr;
  int create(bmx_ctx* ctx);            // at create: the staging sets' events, device words and mapped tails
  void release();                      // (after the context's stream has finished)
};

// Scratch of the scans and selects, grown on demand.
struct ScanScratch {
  uint64_t out_cap = 0; uint64_t* out = nullptr;       // a host-mode answer on its way down
  bool defer = false; uint64_t defer_cap = 0;          // host-mode scan split in two (bmx_comm_scan_*): enqueue now, scan_collect() later
  uint32_t* block_counts = nullptr;   // SEL_MAX_BLOCKS, allocated at create
  uint32_t* mask = nullptr;           // one match bit per index row
  uint32_t* counts = nullptr;         // matches per 8192-row block (+ total)
  uint64_t blocks_cap = 0;
  int ensure(bmx_ctx* ctx, uint64_t rows, uint64_t out_n);
  void release() { dev_free(out); dev_free(block_counts); dev_free(mask); dev_free(counts); out_cap = blocks_cap = 0; }
};

// incremental index maintenance (scan_kernels.h): slot -> position in its field's index, and the log of the winners' slots since the
// indices were last brought up to date. valid: the log is complete (every merge since then was logged and nothing moved the slots).
// Both exist from the first index build on (ensure_ix_maintenance).
struct ChangeLog {
  uint32_t* slot_pos = nullptr; uint64_t slot_pos_n = 0;
  uint2* log = nullptr; uint64_t cap = 0, ub = 0;
  bool valid = false; uint32_t par = 0;
  uint64_t full_builds = 0, incremental = 0;
  void release() { dev_free(slot_pos); slot_pos_n = 0; dev_free(log); cap = 0; ub = 0; valid = false; }
};

// Scratch of the partition kernels (partition_impl).
struct PartScratch {
  uint32_t* counts = nullptr;         // PART_MAX_SHARDS * PART_BLOCKS, allocated at create
  uint8_t* owner = nullptr;           // owner shard of every delta of the batch being partitioned
  uint64_t owner_cap = 0;
  void release() { dev_free(counts); dev_free(owner); owner_cap = 0; }
};

// Scratch of the reconciliation sweeps (bmx_sync.inc): what a BMX_MEM_HOST caller's digest vectors, bucket set and records pass through. Grow-only.
struct SyncScratch {
  unsigned long long* dig = nullptr;      // 2 x 2^16 words: sums and counts
  unsigned long long* bits = nullptr;     // 2^16 bits
  bmx_delta_rec* recs = nullptr; uint64_t recs_cap = 0;
  int cus = 0;                            // compute units of the context's device (the digest's grid)
  void release() { dev_free(dig); dev_free(bits); dev_free(recs); recs_cap = 0; }
};

// Scratch of the aggregate queries (bmx_agg.inc): one accumulator per group, which every query's last kernel leaves empty again (clean), and the records of a
// BMX_MEM_HOST answer on their way down. Grow-only: 1025 records at first, 65537 with the first query that has more groups.
struct AggScratch {
  AggRaw* raw = nullptr; bmx_agg* stage = nullptr; uint32_t cap = 0;
  bool clean = false;
  int cus = 0;                            // compute units of the context's device (the sweep's grid)
  void release() { dev_free(raw); dev_free(stage); cap = 0; clean = false; }
};

// bmx_timer_* events and the optional per-kernel profiling (bmx_profile_enable).
struct Profiling {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool on = false;
  uint32_t n = 0;
  std::vector<hipEvent_t> ev;         // 4 events per profiled call
  std::vector<hipEvent_t> scan_ev;    // 3 events per profiled scan call (before the mask pass, after it, after the emit pass)
  uint32_t scan_n = 0;
  void release() {
    for (auto e : ev) (void)hipEventDestroy(e);
    for (auto e : scan_ev) (void)hipEventDestroy(e);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    ev.clear(); scan_ev.clear(); ev0 = ev1 = nullptr;
  }
};

}  // namespace

struct bmx_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  Slot* slots = nullptr;
  uint64_t nslots = 0, capacity_rows = 0;
  uint32_t load_pct = 50;             // maximum load factor (percent) at capacity_rows: nslots = capacity_rows * 100 / load_pct
  DevScalars* ds = nullptr;
  MergeWs ws;
  Deferral defer;
  HostIO host;
  ScanScratch scan;
  ChangeLog chg;
  PartScratch part;
  SyncScratch sync;
  AggScratch agg;
  Profiling prof;
  ViewShared view;                    // what the indexes' value-ordered views share
  bool fixed_capacity = false;
  uint64_t nbatch = 0;
  uint32_t epoch = 0;
  uint64_t version = 0;
  uint64_t rows_ub = 0;               // host-side upper bound of resident rows
  // {rows, sequence number of the batch that produced them}, written by every merge's last workgroup into mapped host memory: the capacity
  // guard tightens rows_ub from it (rows seen + deltas of the batches enqueued since) instead of synchronising the stream every few batches
  unsigned long long* host_rows = nullptr;
  uint64_t batch_seq = 0;
  std::deque<std::pair<uint64_t, uint64_t>> inflight;   // (sequence number, deltas) of batches whose row count the host has not seen yet
  std::vector<Index> indexes;
  // bmx_merge_notify: words (possibly in other GPUs' memory) that every merge's last workgroup sets to the number of merges finished since
  SeqPtrs notify{}; uint32_t n_notify = 0; uint64_t notify_seq = 0;
  // bmx_merge_tail_wait: armed = the next default-path merge's resolve kernel polls these words before it ends; waited = a resolve kernel that did so has
  // been enqueued (the bmx_merge_records_after that asks for the same wait then launches no wait kernel)
  struct TailWait { const unsigned long long* words = nullptr; uint32_t n = 0; unsigned long long at_least = 0; } tail_armed, tail_waited;
  bool notify_armed = false;          // set by bmx_merge_records_after around ITS merge: only the merges of the slab protocol count up the peers' free words
  uint32_t placement_tries = 0, placement_tries_asked = 0; float placement_us_best = 0, placement_us_worst = 0;   // what alloc_table_tuned saw for the current table
  uint64_t n_row_waits = 0;           // merges that waited for a batch in flight to report its row count (wait_for_row_reports)
  int k1_waves = 8;                   // BMX_K1_WAVES (8, 6 or 5): resident waves per SIMD of the probe kernel
  std::string err;
};

namespace {

int fail(bmx_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  g_err = msg;
  return code;
}
inline hipMemcpyKind host_or_dev(int mem) { return mem == BMX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice; }
int fail_hip(bmx_ctx* c, hipError_t e, const char* what) {
  return fail(c, BMX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(call)                                                  \
  do {                                                                \
    hipError_t e__ = (call);                                          \
    if (e__ != hipSuccess) return fail_hip(ctx, e__, #call);          \
  } while (0)
#define LAUNCHCHK(name)                                               \
  do {                                                                \
    hipError_t e__ = hipGetLastError();                               \
    if (e__ != hipSuccess) return fail_hip(ctx, e__, "launch " name); \
  } while (0)

int dev_alloc_all(bmx_ctx* ctx, std::initializer_list<DevBuf> bufs) {   // (alloc_all) BMX_ERR_NOMEM on out-of-memory, BMX_ERR_HIP otherwise
  hipError_t e = hipSuccess;
  if (alloc_all(bufs, &e)) return BMX_OK;
  return fail(ctx, e == hipErrorOutOfMemory ? BMX_ERR_NOMEM : BMX_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
}
template <class T>
int dev_alloc(bmx_ctx* ctx, T** p, uint64_t count) { return dev_alloc_all(ctx, {{*p, std::max<uint64_t>(count, 1) * sizeof(T)}}); }
void free_columns(Index& ix) { dev_free(ix.ids); dev_free(ix.v64); dev_free(ix.v32); ix.cap = 0; }

// Pull the sticky device status; translate to an error code.
int check_status(bmx_ctx* ctx) {
  uint32_t st = 0;
  HIPCHK(hipMemcpyAsync(&st, &ctx->ds->status, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (!st) return BMX_OK;
  HIPCHK(hipMemsetAsync(&ctx->ds->status, 0, sizeof(uint32_t), ctx->stream));
  if (st & ST_SPIN) {
    unsigned long long d[3] = {0, 0, 0};
    (void)hipMemcpy(d, ctx->ds->seq_diag, sizeof(d), hipMemcpyDeviceToHost);
    (void)hipMemset(ctx->ds->seq_diag, 0, sizeof(d));
    if (d[0]) {
      char buf[200];
      snprintf(buf, sizeof(buf), "device protocol fault: bmx_seq_wait on word %p expired after ~60 s waiting for %llu (last seen %llu): the signalling stream or peer never got there",
               (void*)(uintptr_t)d[0], d[1], d[2]);
      return fail(ctx, BMX_ERR_INTERNAL, buf);
    }
    return fail(ctx, BMX_ERR_INTERNAL, "device protocol fault: bounded spin expired");
  }
  if (st & ST_FULL) return fail(ctx, BMX_ERR_FULL, "resident table is full");
  if (st & ST_SLAB) return fail(ctx, BMX_ERR_OVERFLOW, "an exchange slab was too small for the records routed to one shard: records were dropped, re-route the batch with bmx_partition_by_owner");
  return fail(ctx, BMX_ERR_RANGE, "delta out of domain: reserved key, ts outside [0, 2^53-1] or |val| > 2^53-1");
}

#include "bmx_merge.inc"
#include "bmx_host.inc"

Index* find_index(bmx_ctx* ctx, uint32_t field) {
  for (auto& ix : ctx->indexes)
    if (ix.field == field) return &ix;
  return nullptr;
}

constexpr size_t IX_MAINTAINED_MAX = PART_MAX_SHARDS / 2;   // two scratch words of DevScalars::part_totals per maintained index

// slot -> index position map (4 B per slot) and the change log; both exist from the first index build on
int ensure_ix_maintenance(bmx_ctx* ctx) {
  int rc;
  if (ctx->chg.slot_pos_n != ctx->nslots) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dev_free(ctx->chg.slot_pos); ctx->chg.slot_pos_n = 0;
    for (auto& ix : ctx->indexes) ix.has_pos = false;
    ctx->chg.valid = false;
    if (ctx->nslots >= (1ull << 31)) return BMX_OK;      // bit 31 of a log entry is the "created" mark: larger tables are rebuilt, not maintained
    if ((rc = dev_alloc(ctx, &ctx->chg.slot_pos, ctx->nslots))) { g_err.clear(); ctx->err.clear(); return BMX_OK; }   // no memory for it: fall back to rebuilds
    ctx->chg.slot_pos_n = ctx->nslots;
    HIPCHK(hipMemsetAsync(ctx->chg.slot_pos, 0xFF, ctx->nslots * sizeof(uint32_t), ctx->stream));
  }
  // the log is only used while it is shorter than max(nslots/8, 1M) entries (fresh_index): size it for that, not for the largest table
  const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(ctx->nslots / 4, 1u << 20) + (1u << 16), 1u << 26);   // 1M .. 64M entries of 8 B
  if (ctx->chg.cap < want) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->chg.cap = 0; ctx->chg.valid = false;
    if ((rc = dev_alloc(ctx, &ctx->chg.log, want))) { g_err.clear(); ctx->err.clear(); return BMX_OK; }
    ctx->chg.cap = want;
  }
  return BMX_OK;
}

// forget the log: every index is either fresh or about to be rebuilt
int reset_chg_log(bmx_ctx* ctx) {
  HIPCHK(hipMemsetAsync(ctx->ds->chg_n, 0, sizeof(ctx->ds->chg_n), ctx->stream));
  ctx->chg.par = 0; ctx->chg.ub = 0;
  return BMX_OK;
}

// (Re)build the dense columns of `field` from the table, in slot order. Synchronous.
int build_index(bmx_ctx* ctx, Index* ix) {
  int mrc = ensure_ix_maintenance(ctx);
  if (mrc) return mrc;
  PredSlotField P{ctx->slots, ix->field};
  SelGeom g = sel_geom<PredSlotField::E>(ctx->nslots);
  hipLaunchKernelGGL((k_sel_count<PredSlotField>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, ctx->nslots, g.tiles_per_block, ctx->scan.block_counts);
  LAUNCHCHK("k_sel_count(index)");
  hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.block_counts, g.blocks, &ctx->ds->n_out);
  LAUNCHCHK("k_sum_counts");
  unsigned long long n = 0;
  HIPCHK(hipMemcpyAsync(&n, &ctx->ds->n_out, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (n + (n >> 4) + (1u << 16) > ix->cap) {   // too little head room left for appended rows: a new set of columns
    free_columns(*ix);
    uint64_t cap = (n + n / 8 + (1u << 16) + 1023) & ~1023ull;   // head room: rows created later are appended
    if (int rc = dev_alloc_all(ctx, {{ix->ids, cap * sizeof(uint64_t)}, {ix->v64, cap * sizeof(int64_t)}, {ix->v32, (cap + 4) * sizeof(int32_t)}})) return rc;
    ix->cap = cap;
  }
  HIPCHK(hipMemsetAsync(&ctx->ds->wide, 0, sizeof(uint32_t), ctx->stream));
  EmitIndex Em{ctx->slots, ix->ids, ix->v64, ix->v32, &ctx->ds->wide, ctx->chg.slot_pos};
  FinishCount Fin{nullptr};
  hipLaunchKernelGGL((k_sel_write<PredSlotField, EmitIndex, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, Em, Fin, ctx->nslots,
                     g.tiles_per_block, ctx->scan.block_counts);
  LAUNCHCHK("k_sel_write(index)");
  uint32_t wide = 0;
  HIPCHK(hipMemcpyAsync(&wide, &ctx->ds->wide, sizeof(wide), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ix->n = n;
  ix->fits32 = wide == 0;
  ix->content++;             // every position may be another row's now
  ix->version = ctx->version;
  ix->has_pos = ctx->chg.slot_pos != nullptr;
  ctx->chg.full_builds++;
  // the log starts (or goes on) only if every index now knows its rows' positions and none is waiting for entries already logged
  if (ctx->chg.slot_pos && ctx->chg.log && !ctx->chg.valid && ctx->indexes.size() <= IX_MAINTAINED_MAX) {
    bool all = true;
    for (auto& o : ctx->indexes) all = all && o.has_pos && o.version == ctx->version;
    if (all) { int rc = reset_chg_log(ctx); if (rc) return rc; ctx->chg.valid = true; }
  }
  return BMX_OK;
}

#include "bmx_view.inc"

// Bring EVERY maintained index up to date from the change log (they share it), then forget the log. Per index: created rows of its field are
// appended in log order, then every logged row of the field gets its current value. One host sync at the end (appended counts, wide flags).
// An index whose value-ordered view is current goes on being current: the refresh captures the change run and the view is patched with it.
int refresh_from_log(bmx_ctx* ctx) {
  const auto dbg_t0 = std::chrono::steady_clock::now();
  auto dbg_us = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - dbg_t0).count(); };
  double dbg_sync = 0;
  const unsigned long long* n_dev = &ctx->ds->chg_n[ctx->chg.par];
  const uint64_t ub = ctx->chg.ub;
  struct Res { unsigned long long added; uint32_t wide; uint32_t changed; unsigned long long run; };     // (wide, changed: the two halves of one result word)
  std::vector<Res> res(ctx->indexes.size());
  std::vector<char> capture(ctx->indexes.size(), 0);
  // results of index k live in its own scratch words: part_totals[] is free between partitions (k < PART_MAX_SHARDS indexes are maintained)
  if (ctx->indexes.size() > IX_MAINTAINED_MAX) return fail(ctx, BMX_ERR_INTERNAL, "index maintenance with more indexes than result words");
  if (ub) {
    if (!ensure_hres(ctx)) return fail(ctx, BMX_ERR_NOMEM, "index maintenance: no page-locked memory for the result words");
    for (size_t k = 0; k < ctx->indexes.size(); k++) ctx->host.hres[HRES_RUN + k] = ~0ull;
    for (size_t k = 0; k < ctx->indexes.size(); k++) {
      Index& ix = ctx->indexes[k];
      OrderedView& v = ix.view;
      // the view is current and can stay so: capture the change run (needs room for one entry per log entry)
      if (ctx->view.patching && v.ordered_after && v.s_val && v.ord_content == ix.content && v.ord_fits32 == ix.fits32 && ix.n && ix.n < 0xFFFFFFFFull && ub <= VIEW_PATCH_MAX_LOG) {
        if (int crc = ensure_change_run(ctx, v, ub)) return crc;
        capture[k] = v.cl_cap >= ub;
      }
      unsigned long long* d_added = &ctx->ds->part_totals[2 * k];
      uint32_t* d_wide = reinterpret_cast<uint32_t*>(&ctx->ds->part_totals[2 * k + 1]);
      HIPCHK(hipMemsetAsync(d_added, 0, 2 * sizeof(unsigned long long), ctx->stream));
      PredLogCreated P{ctx->chg.log, n_dev, ix.field, ctx->chg.slot_pos};
      SelGeom g = sel_geom<PredLogCreated::E>(ub);
      hipLaunchKernelGGL((k_sel_count<PredLogCreated>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, ub, g.tiles_per_block, ctx->scan.block_counts);
      LAUNCHCHK("k_sel_count(log)");
      EmitAppend Em{ctx->chg.log, ctx->slots, ix.ids, ix.v64, ix.v32, d_wide, ctx->chg.slot_pos, ix.n, ix.cap};
      FinishCount Fin{d_added};
      hipLaunchKernelGGL((k_sel_write<PredLogCreated, EmitAppend, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, Em, Fin, ub, g.tiles_per_block,
                         ctx->scan.block_counts);
      LAUNCHCHK("k_sel_write(log)");
      const uint32_t ublocks = (uint32_t)std::min<uint64_t>((ub + 255) / 256, 4096);
      hipLaunchKernelGGL(k_ix_update, dim3(ublocks), dim3(256), 0, ctx->stream, (const uint2*)ctx->chg.log, n_dev, (const Slot*)ctx->slots, ix.field, (const uint32_t*)ctx->chg.slot_pos,
                         ix.v64, ix.v32, d_wide, capture[k] ? 2u : (v.ordered_after ? 1u : 0u), v.cl_pos, v.cl_old, (uint64_t)v.cl_cap);
      LAUNCHCHK("k_ix_update");
      if (capture[k]) {      // the change run without its holes, in log order (ordered select: no atomics), and its length
        PredChanged PC{v.cl_pos, n_dev};
        SelGeom gc = sel_geom<PredChanged::E>(ub);
        hipLaunchKernelGGL((k_sel_count<PredChanged>), dim3(gc.blocks), dim3(SEL_THREADS), 0, ctx->stream, PC, ub, gc.tiles_per_block, ctx->scan.block_counts);
        EmitChanged EC{v.cl_pos, v.cl_old, v.cl2_pos, v.cl2_old};
        FinishCount FC{const_cast<unsigned long long*>(&ctx->host.hres[HRES_RUN + k])};
        hipLaunchKernelGGL((k_sel_write<PredChanged, EmitChanged, FinishCount>), dim3(gc.blocks), dim3(SEL_THREADS), 0, ctx->stream, PC, EC, FC, ub, gc.tiles_per_block, ctx->scan.block_counts);
        LAUNCHCHK("k_sel_write(change run)");
      }
    }
    // one copy of the indexes' (added, wide | changed) words into the mapped result words; the change runs' lengths were written there by their selects
    HIPCHK(hipMemcpyAsync(const_cast<unsigned long long*>(&ctx->host.hres[HRES_TOTALS]), ctx->ds->part_totals, 2 * ctx->indexes.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dbg_sync = dbg_us();
    for (size_t k = 0; k < ctx->indexes.size(); k++) {
      res[k].added = ctx->host.hres[HRES_TOTALS + 2 * k];
      const unsigned long long wc = ctx->host.hres[HRES_TOTALS + 2 * k + 1];
      res[k].wide = (uint32_t)wc; res[k].changed = (uint32_t)(wc >> 32);
      res[k].run = capture[k] ? ctx->host.hres[HRES_RUN + k] : 0;
    }
  }
  int rc = reset_chg_log(ctx);
  if (rc) return rc;
  for (size_t k = 0; k < ctx->indexes.size(); k++) {
    Index& ix = ctx->indexes[k];
    if (ub && ix.n + res[k].added > ix.cap) {
      // The appended rows did not fit. The entries it missed are gone with the log, so this index must never be refreshed from a LATER log:
      // without its positions it can only come back through build_index(), and the log stops until every index is fresh again.
      ix.version = ~0ull; ix.has_pos = false; ctx->chg.valid = false;
      continue;
    }
    if (ub) {
      const uint64_t n0 = ix.n;
      ix.n += res[k].added; if (res[k].wide) ix.fits32 = false;
      const bool moved = res[k].added || res[k].changed || !ix.view.ordered_after;     // (no view: nobody compared, nobody cares)
      if (moved) ix.content++;
      if (moved && capture[k] && ix.fits32 == ix.view.ord_fits32 && res[k].run <= ix.view.cl_cap && ix.n < 0xFFFFFFFFull) {
        const int prc = ix.view.ord_fits32 ? patch_view_t<int32_t>(ctx, ix, res[k].run, n0, res[k].added) : patch_view_t<int64_t>(ctx, ix, res[k].run, n0, res[k].added);
        if (prc == 0) ix.view.ord_content = ix.content;       // the view equals a fresh sort of the columns as they are now
      }
    }
    ix.version = ctx->version;
  }
  ctx->chg.incremental++;
  if (ctx->view.debug) std::fprintf(stderr, "bmx: refresh from the log: columns up to date after %.1f us, patches done after %.1f us\n", dbg_sync, dbg_us());
  return BMX_OK;
}

int fresh_index(bmx_ctx* ctx, uint32_t field, Index** out) {
  Index* ix = find_index(ctx, field);
  if (!ix) {  // equals()/range() auto-create a missing index: src/bullet-query.js:194-196, 230-232
    if (ctx->indexes.size() >= IX_MAINTAINED_MAX) ctx->chg.valid = false;   // more indexes than the maintenance pass has result words for: they are rebuilt when stale
    ctx->indexes.emplace_back();
    ix = &ctx->indexes.back();
    ix->field = field;
  }
  if (ix->version != ctx->version) {
    // maintained: every index has its positions recorded, the log is complete, and it is shorter than a quarter of the table
    // (beyond that the rebuild's two sequential passes over the table are cheaper than the log's random accesses)
    bool inc = ctx->chg.valid && ix->has_pos && ctx->chg.ub <= std::max<uint64_t>(ctx->nslots / 8, 1u << 20);
    if (inc) for (auto& o : ctx->indexes) inc = inc && (o.has_pos || &o == ix);
    if (inc) {
      int rc = refresh_from_log(ctx);
      if (rc) return rc;
    }
    if (ix->version != ctx->version) {   // not maintained (or its appended rows did not fit): rebuild from the table
      ctx->chg.valid = false;
      int rc = build_index(ctx, ix);
      if (rc) return rc;
    }
  }
  *out = ix;
  return BMX_OK;
}

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

// Run one predicate over an index and deliver ids (POS = false: u64 node ids gathered from the id column) or index positions (POS = true: u32,
// no gather) / the count according to `mem`. `out` is uint64_t* or uint32_t* accordingly.
// a value column above this size is read with nontemporal loads: it cannot stay in the 256 MiB Infinity Cache between two scans anyway (scan_kernels.h)
constexpr uint64_t SCAN_NT_BYTES = 256ull << 20;
constexpr uint32_t SCAN_NTX_DEFAULT = 0;      // EmitIds::ntx (profiles/r05_scan_nt_emit_ab.log)

// ---- the view's sort (bmx.h bmx_index_set_ordered; the rest of the view is bmx_view.inc) ---- It stays behind refresh_from_log: kernel templates are laid
// out in the gfx950 code object in the order the source first uses them, and this sort's kernels follow the patch's (in front, they would land elsewhere).
// Is the view of `ix` usable for the query at hand? A stale one is sorted again by the ordered_after-th query since the columns last changed — the
// queries in front of that one scan the column as ever (one sort of a 100M-row column costs what ~20 scans cost) —, and never while it cannot be had
// (no memory: the index goes on without it). Synchronous where it sorts.
bool ensure_ordered_view(bmx_ctx* ctx, Index* ix) {
  OrderedView& v = ix->view;
  if (!v.ordered_after || ix->n == 0 || ix->n > 0xFFFFFFFFull) return false;
  if (v.ord_content == ix->content && v.s_val) { finish_rewrite(ctx, v, /*wait=*/false); return true; }   // (a finished rewrite becomes main; an unfinished one changes nothing)
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
  if (++v.stale_queries < after) return false;
  const auto t_sort = std::chrono::steady_clock::now();
  v.npd = v.npi = 0;                          // a fresh sort of the columns: whatever patch was pending is in them
  const uint64_t n = ix->n;
  const size_t vb = ix->fits32 ? sizeof(int32_t) : sizeof(int64_t);
  auto give_up = [&]() { (void)hipGetLastError(); v.release(); v.stale_queries = 0; return false; };
  auto sorted = [&]() { v.ord_n = n; v.ord_content = ix->content; v.stale_queries = 0; v.ord_sorts++; v.last_sort_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_sort).count(); return true; };
  if (n > v.ord_cap || v.ord_fits32 != ix->fits32) {
    v.release();
    const uint64_t cap = n + n / 8 + 1024;
    if (!alloc_all({{v.s_val, cap * vb}, {v.s_pos, cap * sizeof(uint32_t)}, {v.s_ids, cap * sizeof(uint64_t)}})) return give_up();
    v.ord_cap = cap; v.ord_fits32 = ix->fits32;
  }
  if (ctx->view.own_sort && n && n < 0xFFFFFFFFull) {
    // A/B arm: the whole column through the patch path's sort — (value, position) keys, 4096-key tiles in LDS, then log2(n / 4096) merge-path passes between
    // the view's columns and a scratch pair; a tombstone is the column type's minimum and sorts in front like every other value
    void* tv = nullptr; uint32_t* tp = nullptr;
    if (!alloc_all({{tv, n * vb}, {tp, n * sizeof(uint32_t)}})) return give_up();
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
    if (eo != hipSuccess) return give_up();
    return sorted();
  }
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
  if (e != hipSuccess) return give_up();
  if (mm[0] > mm[1]) { mm[0] = 0; mm[1] = 0; }                   // nothing but tombstones
  const unsigned long long span = (unsigned long long)mm[1] - (unsigned long long)mm[0] + 1ull;     // largest rebased key
  unsigned bits = 1; while (bits < 64 && (span >> bits)) bits++;
  bits = std::min<unsigned>(bits, ix->fits32 ? 32u : 64u);
  uint32_t* iota = nullptr; void* tmp = nullptr; size_t tmp_bytes = 0;
  e = ix->fits32 ? sort_pairs_i32(nullptr, &tmp_bytes, nullptr, 0, bits, nullptr, nullptr, nullptr, n, ctx->stream)
                 : sort_pairs_i64(nullptr, &tmp_bytes, nullptr, 0, bits, nullptr, nullptr, nullptr, n, ctx->stream);
  if (e != hipSuccess || !alloc_all({{iota, n * sizeof(uint32_t)}, {tmp, std::max<size_t>(tmp_bytes, 16)}})) return give_up();
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
  if (e != hipSuccess) return give_up();
  return sorted();
}

template <bool POS, class Pred>
int run_scan_t(bmx_ctx* ctx, const Pred& P, const Index* ix, void* out_v, uint64_t cap, uint64_t* n_out, int mem, bool ordered = false, int64_t olo = 0, int64_t ohi = 0) {
  using OutT = typename std::conditional<POS, uint32_t, uint64_t>::type;
  OutT* out_ids = static_cast<OutT*>(out_v);
  const bool host = mem == BMX_MEM_HOST;
  OutT* d_out = out_ids;
  uint64_t d_cap = cap;
  int rc;
  // small host-mode answers (count only, or room for at most SCAN_PIN_IDS ids) come back through mapped host memory: no download, one synchronisation
  constexpr uint64_t SCAN_PIN_IDS = 16384;
  static_assert(SCAN_PIN_IDS * 8 + 8 <= SMALL_OUT_BYTES, "pinned scan answer fits the small-call buffer");
  const bool pinned = host && !ctx->scan.defer && (!out_ids || std::min<uint64_t>(cap, ix->n) <= SCAN_PIN_IDS) && ensure_pinned(ctx);
  bool direct_host = false, staged = false;
  if (host && out_ids) {
    d_cap = std::min<uint64_t>(cap, ix->n);
    if (pinned) d_out = reinterpret_cast<OutT*>(ctx->host.pin_out);
    else {
      // a caller's buffer in page-locked memory (bmx_host_alloc, hipHostMalloc, a registered range) is written by the kernels themselves: no staging copy behind the answer
      hipPointerAttribute_t at{};
      if (!ctx->scan.defer && hipPointerGetAttributes(&at, out_ids) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) { d_out = static_cast<OutT*>(at.devicePointer); direct_host = true; }
      else {
        (void)hipGetLastError();
        staged = true;
      }
    }
  }
  if ((rc = ctx->scan.ensure(ctx, std::max<uint64_t>(ix->n, 1), staged ? std::max<uint64_t>(d_cap, 1) : 0))) return rc;
  if (staged) d_out = reinterpret_cast<OutT*>(ctx->scan.out);
  const bool hres_n = host && !pinned && !ctx->scan.defer && !(ordered && std::is_same<Pred, PredFilter>::value) /* (that one counts with atomics) */ && ensure_hres(ctx);       // the count of a larger host-mode answer: a mapped result word
  unsigned long long* d_n = host ? (pinned ? reinterpret_cast<unsigned long long*>(ctx->host.pin_out + SCAN_PIN_IDS * 8) : hres_n ? const_cast<unsigned long long*>(&ctx->host.hres[HRES_SCAN_N]) : &ctx->ds->n_out)
                                 : reinterpret_cast<unsigned long long*>(n_out);
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
    if (nb > SCAN_SUB8_BLOCKS)   // large column: an eighth of the workgroups, each sums the counts in front of it once (no offsets launch)
      hipLaunchKernelGGL((k_scan_emit<EmT, FinishCount, 8>), dim3((nb + 7) / 8), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.mask, ctx->scan.counts, ix->n, nb, Em, Fin);
    else
      hipLaunchKernelGGL((k_scan_emit<EmT, FinishCount, 1>), dim3(nb), dim3(SEL_THREADS), 0, ctx->stream, ctx->scan.mask, ctx->scan.counts, ix->n, nb, Em, Fin);
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
  if (host && ctx->scan.defer) { ctx->scan.defer_cap = out_ids ? d_cap : 0; return BMX_OK; }   // the caller fetches with scan_collect()
  if (pinned) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const unsigned long long m = *d_n;
    if (out_ids && m) std::memcpy(out_ids, d_out, std::min<uint64_t>(m, d_cap) * sizeof(OutT));
    if (n_out) *n_out = m;
    return BMX_OK;
  }
  if (host) {
    unsigned long long m = 0;
    if (!hres_n) HIPCHK(hipMemcpyAsync(&m, &ctx->ds->n_out, sizeof(m), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (hres_n) m = ctx->host.hres[HRES_SCAN_N];
    if (out_ids && m && !direct_host) HIPCHK(hipMemcpy(out_ids, ctx->scan.out, std::min<uint64_t>(m, d_cap) * sizeof(OutT), hipMemcpyDeviceToHost));
    if (n_out) *n_out = m;
  }
  return BMX_OK;
}

// second half of a deferred host-mode scan: wait for the scan enqueued with ctx->scan.defer set, deliver the count and up to `cap` ids
int scan_collect(bmx_ctx* ctx, uint64_t* out_ids, uint64_t cap, uint64_t* n_out) {
  if (int erc = enter(ctx)) return erc;
  unsigned long long m = 0;
  HIPCHK(hipMemcpyAsync(&m, &ctx->ds->n_out, sizeof(m), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t k = std::min<uint64_t>(std::min<uint64_t>(m, ctx->scan.defer_cap), cap);
  if (out_ids && k) HIPCHK(hipMemcpy(out_ids, ctx->scan.out, k * 8, hipMemcpyDeviceToHost));
  if (n_out) *n_out = m;
  return BMX_OK;
}

template <bool POS>
int scan_range_impl_t(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, void* out, uint64_t cap, uint64_t* n_out, int mem) {
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  Index* ix;
  int rc = fresh_index(ctx, field, &ix);
  if (rc) return rc;
  const bool ordered = (n_out || out) && ensure_ordered_view(ctx, ix);     // (it was sorted from columns of the width they have now: a widened index has a new `content`)
  if (ix->fits32) {
    // every value fits int32: scan the 4-byte column with bounds clamped into int32 (an empty range stays empty). INT32_MIN itself is what a
    // tombstone looks like in this column and is never matched (a real -2^31 makes the index wide: scan_kernels.h v32_of)
    int64_t l = std::max<int64_t>(lo, (int64_t)INT32_MIN + 1), h = std::min<int64_t>(hi, INT32_MAX);
    if (lo > INT32_MAX || hi < INT32_MIN) { l = 1; h = 0; }
    PredRange32 P{ix->v32, (int32_t)l, (int32_t)h, ix->n * sizeof(int32_t) > SCAN_NT_BYTES};
    rc = run_scan_t<POS>(ctx, P, ix, out, cap, n_out, mem, ordered, l, h);
  } else {
    PredRange64 P{ix->v64, std::max<int64_t>(lo, -VAL_MAX), hi, ix->n * sizeof(int64_t) > SCAN_NT_BYTES};    // values live in +-(2^53-1): the clamp changes no answer and keeps tombstones (INT64_MIN) out
    rc = run_scan_t<POS>(ctx, P, ix, out, cap, n_out, mem, ordered, P.lo, P.hi);
  }
  if (ordered && !rc) view_after_query(ctx, ix);
  return rc;
}
int scan_range_impl(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem) {
  return scan_range_impl_t<false>(ctx, field, lo, hi, out_ids, cap, n_out, mem);
}

// the mean time between consecutive events of the profiled calls: `per` events per call, per - 1 intervals
int profile_means(bmx_ctx* ctx, bool scan, float* ms_out, uint32_t* n_calls) {
  if (!ctx || !ms_out || !n_calls) return fail(ctx, BMX_ERR_INVALID, "bad arguments");
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const std::vector<hipEvent_t>& ev = scan ? ctx->prof.scan_ev : ctx->prof.ev;
  const uint32_t per = scan ? 3 : 4, calls = scan ? ctx->prof.scan_n : ctx->prof.n;
  double acc[3] = {0, 0, 0};
  for (uint32_t i = 0; i < calls; i++)
    for (uint32_t k = 0; k + 1 < per; k++) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, ev[per * i + k], ev[per * i + k + 1]));
      acc[k] += ms;
    }
  for (uint32_t k = 0; k + 1 < per; k++) ms_out[k] = calls ? (float)(acc[k] / calls) : 0.f;
  *n_calls = calls;
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_abi_version(void) { return BMX_ABI_VERSION; }

const char* bmx_last_error(const bmx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

uint32_t bmx_owner_of(uint64_t id, uint32_t nshards) { return (uint32_t)(((unsigned __int128)owner_hash(id) * nshards) >> 64); }

// bmx.h "bmx_selfcheck". Synchronous for the caller, on a stream of its own (nothing else on the device is waited for); allocates and frees 128 KB + 4 words.
int bmx_selfcheck(int device, uint64_t* reads_out, uint64_t* torn_out, uint64_t* control_torn_out) {
  bmx_ctx* ctx = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, BMX_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  if (device < 0 || device >= ndev) return fail(nullptr, BMX_ERR_INVALID, "bmx_selfcheck: device index out of range");
  HIPCHK(hipSetDevice(device));
  constexpr uint32_t NS = 4096, ITERS = 1500, BLOCKS = 1024;     // 4096 hot slots (128 KB: every line is written and read all the time), ~2*10^8 checked loads
  uint4* slots = nullptr; unsigned long long* d = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&slots), (size_t)NS * 32) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&d), 4 * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError(); if (slots) (void)hipFree(slots);
    return fail(nullptr, BMX_ERR_NOMEM, "bmx_selfcheck: out of device memory");
  }
  unsigned long long h[4] = {0, 0, 0, 0};
  hipStream_t cs = nullptr;       // a stream of its own: no device-wide synchronisation, nothing of another context or library is waited for
  const char* nul = std::getenv("BMX_SELFCHECK_NULL_STREAM");     // measurement switch (round 5): the device's null stream, as rounds 1-4 used
  hipError_t e = (nul && nul[0] == '1') ? hipSuccess : hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMemsetAsync(slots, 0, (size_t)NS * 32, cs);
  if (e == hipSuccess) e = hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), cs);
  if (e == hipSuccess) { hipLaunchKernelGGL(k_selfcheck_tear<false>, dim3(BLOCKS), dim3(256), 0, cs, slots, NS, ITERS, d, d + 1); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipMemsetAsync(slots, 0, (size_t)NS * 32, cs);
  if (e == hipSuccess) { hipLaunchKernelGGL(k_selfcheck_tear<true>, dim3(BLOCKS), dim3(256), 0, cs, slots, NS, ITERS / 4, d + 2, d + 3); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, cs);
  if (e == hipSuccess) e = hipStreamSynchronize(cs);
  if (cs) (void)hipStreamDestroy(cs);
  (void)hipFree(slots); (void)hipFree(d);
  if (e != hipSuccess) return fail_hip(nullptr, e, "bmx_selfcheck");
  if (reads_out) *reads_out = h[1];
  if (torn_out) *torn_out = h[0];
  if (control_torn_out) *control_torn_out = h[2];
  if (h[0]) {
    char buf[240];
    snprintf(buf, sizeof(buf), "self-check failed on device %d: %llu of %llu aligned 16-byte loads saw HALF of an aligned 16-byte store; the merge kernel's exactness needs them indivisible (DESIGN.md section 4)",
             device, h[0], h[1]);
    return fail(nullptr, BMX_ERR_INTERNAL, buf);
  }
  return BMX_OK;
}

int bmx_create(int device, uint64_t capacity_rows, uint32_t flags, bmx_ctx** out) {
  return bmx_create_ex(device, capacity_rows, 0, flags, out);
}

int bmx_create_ex(int device, uint64_t capacity_rows, uint32_t max_load_pct, uint32_t flags, bmx_ctx** out) {
  if (!out || capacity_rows == 0) return fail(nullptr, BMX_ERR_INVALID, "bmx_create: bad arguments");
  *out = nullptr;
  // argument checks come before the device is looked at: they hold on any machine
  if (max_load_pct == 0) max_load_pct = BMX_DEFAULT_LOAD_PCT;
  if (max_load_pct < 5 || max_load_pct > 90) return fail(nullptr, BMX_ERR_INVALID, "bmx_create_ex: max_load_pct must be 5..90 (0 = default)");
  if (!slots_for(capacity_rows, max_load_pct))
    return fail(nullptr, BMX_ERR_INVALID, "bmx_create: table would need more than 2^32 slots (slot indices are 32-bit): shard the graph over more contexts");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) return fail(nullptr, BMX_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  if (device < 0 || device >= ndev) return fail(nullptr, BMX_ERR_INVALID, "bmx_create: device index out of range");
  {  // Once per device and process, BEFORE any stream of this library exists: one empty launch on the device's NULL stream. Measured (profiles/r05_defer_timeline_*.txt,
     // r05_step_regression.log): the runtime gives the first stream that is USED in a process its first hardware queue, and a context stream that lands there does not
     // yield wave slots to the high-priority side stream — the deferred compaction then waits ~50 us per step for slots (k_seq_signal, one wave, 54 us; k_resolve_lists
     // 54 instead of 5 us; 141-147 us per step instead of 77-84). Rounds 1-4 used the null stream by accident (the self-check ran there), which is why the deferral
     // worked; with BMX_SKIP_SELFCHECK=1 it never did (round-4 tree, same box: 76.8 -> 140.9 us). The null stream takes that first queue and keeps it.
    static std::atomic<unsigned> touched[64];
    const char* no = std::getenv("BMX_NO_NULL_STREAM_TOUCH");
    if (device < 64 && !(no && no[0] == '1') && !touched[device].load()) {
      if (hipSetDevice(device) == hipSuccess) {
        hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, nullptr);
        (void)hipStreamSynchronize(nullptr);
      }
      (void)hipGetLastError();
      touched[device].store(1u);
    }
  }
  {  // once per device and process: the 16-byte load/store indivisibility the probe kernel relies on is checked on THIS box (BMX_SKIP_SELFCHECK=1 skips it)
    static std::atomic<unsigned> checked[64];
    const char* skip = std::getenv("BMX_SKIP_SELFCHECK");
    if (device < 64 && !(skip && skip[0] == '1') && !checked[device].load()) {
      int src = bmx_selfcheck(device, nullptr, nullptr, nullptr);
      if (src) return src;
      checked[device].store(1u);
    }
  }
  bmx_ctx* ctx = new (std::nothrow) bmx_ctx();
  if (!ctx) return fail(nullptr, BMX_ERR_NOMEM, "out of host memory");
  ctx->device = device;
  ctx->capacity_rows = capacity_rows;
  ctx->load_pct = max_load_pct;
  auto bail = [&](int rc) { std::string m = ctx->err; bmx_destroy(ctx); g_err = m; return rc; };
#define CR(call) do { hipError_t e2 = (call); if (e2 != hipSuccess) { fail_hip(ctx, e2, #call); return bail(BMX_ERR_HIP); } } while (0)
  CR(hipSetDevice(device));
  CR(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
  ctx->stream = ctx->own_stream;
  CR(hipEventCreate(&ctx->prof.ev0));
  CR(hipEventCreate(&ctx->prof.ev1));
  for (auto& S : ctx->host.stg) { CR(hipEventCreateWithFlags(&S.up, hipEventDisableTiming)); CR(hipEventCreateWithFlags(&S.done, hipEventDisableTiming)); }
  const uint64_t nslots = slots_for(capacity_rows, max_load_pct);
  ctx->nslots = nslots;
  ctx->placement_tries_asked = (flags >> 8) & 0xFu;         // BMX_CTX_PLACEMENT_TRIES(n): 0 = the default
  if (ctx->placement_tries_asked > 8) ctx->placement_tries_asked = 8;
  int rc;
  if ((rc = alloc_table_tuned(ctx, nslots, &ctx->slots))) return bail(rc);
  if ((rc = dev_alloc(ctx, &ctx->ds, 1))) return bail(rc);
  if ((rc = ctx->host.create(ctx))) return bail(rc);
  if ((rc = dev_alloc_all(ctx, {{ctx->scan.block_counts, SEL_MAX_BLOCKS * sizeof(uint32_t)}, {ctx->part.counts, PART_MAX_SHARDS * PART_BLOCKS * sizeof(uint32_t)},
                                {ctx->ws.shard_ctr, MergeWs::SETS * CTR_SHARDS * CTR_STRIDE * sizeof(unsigned long long)}})))
    return bail(rc);
  CR(hipMemsetAsync(ctx->ws.shard_ctr, 0, MergeWs::SETS * CTR_SHARDS * CTR_STRIDE * sizeof(unsigned long long), ctx->stream));
  // the row-count mirror is an optimisation: without mapped host memory the capacity guard simply synchronises as before
  if (hipHostMalloc(reinterpret_cast<void**>(&ctx->host_rows), 2 * sizeof(unsigned long long), hipHostMallocMapped) == hipSuccess) {
    ctx->host_rows[0] = 0; ctx->host_rows[1] = 0;
  } else { ctx->host_rows = nullptr; (void)hipGetLastError(); }
  ctx->fixed_capacity = (flags & BMX_CTX_FIXED_CAPACITY) != 0;
  ctx->defer.enabled = !launches_are_serialized();
  ctx->view.read_env();
  { const char* kw = std::getenv("BMX_K1_WAVES"); if (kw && kw[0] >= '3' && kw[0] <= '8' && kw[0] != '7' && !kw[1]) ctx->k1_waves = kw[0] - '0'; }
  CR(hipMemsetAsync(ctx->ds, 0, sizeof(DevScalars), ctx->stream));
  hipLaunchKernelGGL(k_init_slots, dim3(2048), dim3(256), 0, ctx->stream, ctx->slots, nslots);
  CR(hipGetLastError());
  CR(hipStreamSynchronize(ctx->stream));
#undef CR
  *out = ctx;
  return BMX_OK;
}

void bmx_destroy(bmx_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)flush_pending(ctx); // a compaction that was only recorded writes the CALLER's winner list and count: it runs before anything is freed
  (void)hipGetLastError();
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  ctx->defer.release();
  for (auto& ix : ctx->indexes) { free_columns(ix); ix.view.release(); }
  dev_free(ctx->slots); dev_free(ctx->ds);
  ctx->ws.release();
  ctx->host.release();     // (the copy and download streams finish before the staging goes back)
  ctx->chg.release();
  ctx->view.release();
  ctx->scan.release();
  ctx->part.release();
  ctx->sync.release();
  ctx->agg.release();
  ctx->prof.release();
  if (ctx->host_rows) (void)hipHostFree(ctx->host_rows);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

int bmx_sync(bmx_ctx* ctx) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  return check_status(ctx);
}

int bmx_set_stream(bmx_ctx* ctx, void* s) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;        // a recorded compaction belongs on the old stream
  HIPCHK(hipStreamSynchronize(ctx->stream));   // work already enqueued on the old stream finishes first
  ctx->stream = s ? reinterpret_cast<hipStream_t>(s) : ctx->own_stream;
  return BMX_OK;
}
void* bmx_get_stream(bmx_ctx* ctx) { return ctx ? reinterpret_cast<void*>(ctx->stream) : nullptr; }

int bmx_seq_signal(bmx_ctx* ctx, void* hip_stream, uint64_t* seq_dev, uint64_t value) {
  if (!ctx || !seq_dev) return fail(ctx, BMX_ERR_INVALID, "bmx_seq_signal: null context or sequence word");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->stream;
  // a signal on the context's own stream says "every merge enqueued before this is done, outputs included": a compaction that is only recorded
  // (or still on the side stream) is ordered in front of it (a consumer stream woken by the word read a stale n_applied)
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

int bmx_get_info(bmx_ctx* ctx, bmx_info* out) {
  if (!ctx || !out) return fail(ctx, BMX_ERR_INVALID, "bad arguments");
  if (int erc = enter(ctx)) return erc;
  int rc = refresh_rows(ctx);
  if (rc) return rc;
  out->capacity_rows = ctx->capacity_rows; out->n_slots = ctx->nslots; out->table_bytes = ctx->nslots * sizeof(Slot); out->n_rows = ctx->rows_ub;
  out->device = (uint32_t)ctx->device; out->abi_version = BMX_ABI_VERSION; out->n_indexes = (uint32_t)ctx->indexes.size(); out->epoch = ctx->epoch;
  return BMX_OK;
}

int bmx_row_count(bmx_ctx* ctx, uint64_t* n_out) {
  if (!ctx || !n_out) return fail(ctx, BMX_ERR_INVALID, "bad arguments");
  if (int erc = enter(ctx)) return erc;
  int rc = refresh_rows(ctx);
  if (rc) return rc;
  *n_out = ctx->rows_ub;
  return BMX_OK;
}

int bmx_reserve(bmx_ctx* ctx, uint64_t capacity_rows) {
  if (!ctx || capacity_rows == 0) return fail(ctx, BMX_ERR_INVALID, "bad arguments");
  if (int erc = enter(ctx)) return erc;
  return grow_table(ctx, capacity_rows);
}

int bmx_merge_batch(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val,
                    int insert_mode, int mem, uint32_t* applied_idx, uint64_t* n_applied, uint8_t* flags, bmx_merge_stats* stats) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (n && (!id || !field || !ts || !val)) return fail(ctx, BMX_ERR_INVALID, "null input column");
  MergeMode mode; if (const char* bad = merge_mode_of(insert_mode, &mode)) return fail(ctx, BMX_ERR_INVALID, bad);
  HIPCHK(hipSetDevice(ctx->device));
  const MergeIn in{n, id, field, ts, val, nullptr}; const MergeOut out{applied_idx, n_applied, flags, stats};
  if (mem == BMX_MEM_DEVICE) return merge_core(ctx, in, out, mode, /*defer=*/true);
  if (mem != BMX_MEM_HOST) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (n > MAX_BATCH) return fail(ctx, BMX_ERR_INVALID, BATCH_TOO_LARGE);   // before staging memory is sized
  return merge_host(ctx, in, mode, out);
}

int bmx_merge_submit(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val, int insert_mode,
                     int want_flags, uint64_t* ticket) {
  if (!ctx || !ticket) return fail(ctx, BMX_ERR_INVALID, "bmx_merge_submit: null context or ticket");
  if (n && (!id || !field || !ts || !val)) return fail(ctx, BMX_ERR_INVALID, "null input column");
  if (n > MAX_BATCH) return fail(ctx, BMX_ERR_INVALID, BATCH_TOO_LARGE);   // before staging memory is sized
  MergeMode mode; if (const char* bad = merge_mode_of(insert_mode, &mode)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = enter(ctx)) return erc;
  return submit_host(ctx, MergeIn{n, id, field, ts, val, nullptr}, mode, want_flags != 0, ticket, true);
}

int bmx_merge_collect(bmx_ctx* ctx, uint64_t ticket, uint32_t* applied_idx, uint64_t* n_applied, uint8_t* flags, bmx_merge_stats* stats) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  return collect_host(ctx, ticket, applied_idx, n_applied, flags, stats);
}

int bmx_merge_records(bmx_ctx* ctx, uint64_t n, const bmx_delta_rec* recs, int insert_mode, uint32_t* applied_idx, uint64_t* n_applied,
                      uint8_t* flags, bmx_merge_stats* stats) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (n && !recs) return fail(ctx, BMX_ERR_INVALID, "null records");
  MergeMode mode; if (const char* bad = merge_mode_of(insert_mode, &mode)) return fail(ctx, BMX_ERR_INVALID, bad);
  HIPCHK(hipSetDevice(ctx->device));
  return merge_core(ctx, MergeIn{n, nullptr, nullptr, nullptr, nullptr, recs}, MergeOut{applied_idx, n_applied, flags, stats}, mode, /*defer=*/true);
}

int bmx_merge_records_after(bmx_ctx* ctx, const uint64_t* wait_words_dev, uint32_t n_wait, uint64_t wait_at_least, uint64_t n, const bmx_delta_rec* recs,
                            int insert_mode, uint32_t* applied_idx, uint64_t* n_applied, uint8_t* flags, bmx_merge_stats* stats) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (wait_words_dev && n_wait) {
    const bool done = ctx->tail_waited.n == n_wait && ctx->tail_waited.words == reinterpret_cast<const unsigned long long*>(wait_words_dev) && ctx->tail_waited.at_least >= wait_at_least;
    ctx->tail_waited = bmx_ctx::TailWait{};
    if (!done) { int wrc = bmx_seq_wait_all(ctx, nullptr, wait_words_dev, n_wait, wait_at_least); if (wrc) return wrc; }   // (done: the resolve kernel of the merge before waited for exactly this)
  }
  ctx->notify_armed = true;      // THIS merge reads a receive slab set: it (and no other merge of the context) tells the origins when the set is free again
  const int rc = bmx_merge_records(ctx, n, recs, insert_mode, applied_idx, n_applied, flags, stats);
  ctx->notify_armed = false;
  return rc;
}

int bmx_load_rows(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val, int mem) { return load_rows(ctx, n, id, field, ts, val, mem, MODE_LOAD); }
int bmx_put_rows(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val, int mem) { return load_rows(ctx, n, id, field, ts, val, mem, MODE_PUT); }

int bmx_get_rows(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, int64_t* ts, int64_t* val, uint8_t* found, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (n == 0) return BMX_OK;
  if (!id || !field || !ts || !val || !found || n > 0xFFFFFFFFull) return fail(ctx, BMX_ERR_INVALID, "bad arguments");
  if (int erc = enter(ctx)) return erc;
  const uint32_t blocks = (uint32_t)((n + 255) / 256);
  if (mem == BMX_MEM_DEVICE) {
    hipLaunchKernelGGL(k_get_rows, dim3(blocks), dim3(256), 0, ctx->stream, ctx->slots, ctx->nslots, (uint32_t)n, id, field, ts, val, found);
    LAUNCHCHK("k_get_rows");
    return BMX_OK;
  }
  if (mem != BMX_MEM_HOST) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (n <= 8192 && ensure_pinned(ctx)) {   // few keys: keys and answers through mapped host memory, one launch and one synchronisation (25 us instead of 67)
    uint64_t* p_id = reinterpret_cast<uint64_t*>(ctx->host.pin_in);
    uint32_t* p_f = reinterpret_cast<uint32_t*>(ctx->host.pin_in + n * 8);
    int64_t* o_ts = reinterpret_cast<int64_t*>(ctx->host.pin_out);
    int64_t* o_val = reinterpret_cast<int64_t*>(ctx->host.pin_out + n * 8);
    uint8_t* o_found = ctx->host.pin_out + n * 16;
    std::memcpy(p_id, id, n * 8); std::memcpy(p_f, field, n * 4);
    hipLaunchKernelGGL(k_get_rows, dim3(blocks), dim3(256), 0, ctx->stream, ctx->slots, ctx->nslots, (uint32_t)n, (const uint64_t*)p_id, (const uint32_t*)p_f, o_ts, o_val, o_found);
    LAUNCHCHK("k_get_rows");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::memcpy(ts, o_ts, n * 8); std::memcpy(val, o_val, n * 8); std::memcpy(found, o_found, n);
    return BMX_OK;
  }
  int rc = ensure_point_read(ctx, n);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(ctx->host.pr_id, id, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->host.pr_field, field, n * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_get_rows, dim3(blocks), dim3(256), 0, ctx->stream, ctx->slots, ctx->nslots, (uint32_t)n, ctx->host.pr_id, ctx->host.pr_field, ctx->host.pr_ts, ctx->host.pr_val, ctx->host.pr_found);
  LAUNCHCHK("k_get_rows");
  HIPCHK(hipMemcpyAsync(ts, ctx->host.pr_ts, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(val, ctx->host.pr_val, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(found, ctx->host.pr_found, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return BMX_OK;
}

int bmx_get_row(bmx_ctx* ctx, uint64_t id, uint32_t field, int64_t* ts, int64_t* val) {
  uint8_t found = 0;
  int64_t t = 0, v = 0;
  int rc = bmx_get_rows(ctx, 1, &id, &field, &t, &v, &found, BMX_MEM_HOST);
  if (rc) return rc;
  if (found) { if (ts) *ts = t; if (val) *val = v; }
  return found ? 1 : 0;
}

int bmx_dump_rows(bmx_ctx* ctx, uint64_t cap, uint64_t* id, uint32_t* field, int64_t* ts, int64_t* val, uint64_t* n_out, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (cap && (!id || !field || !ts || !val)) return fail(ctx, BMX_ERR_INVALID, "null output column");
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (int erc = enter(ctx)) return erc;
  const bool host = mem == BMX_MEM_HOST;
  uint64_t* d_id = id; uint32_t* d_f = field; int64_t* d_ts = ts; int64_t* d_val = val;
  int rc = BMX_OK;
  if (host && cap) {   // persistent (grow-only) device columns: no allocation per call
    if ((rc = ensure_point_read(ctx, cap))) return rc;
    d_id = ctx->host.pr_id; d_f = ctx->host.pr_field; d_ts = ctx->host.pr_ts; d_val = ctx->host.pr_val;
  }
  PredSlotAny P{ctx->slots};
  EmitRows Em{ctx->slots, cap, d_id, d_f, d_ts, d_val};
  FinishCount Fin{host ? &ctx->ds->n_out : reinterpret_cast<unsigned long long*>(n_out)};
  SelGeom g = sel_geom<PredSlotAny::E>(ctx->nslots);
  hipLaunchKernelGGL((k_sel_count<PredSlotAny>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, ctx->nslots, g.tiles_per_block, ctx->scan.block_counts);
  hipLaunchKernelGGL((k_sel_write<PredSlotAny, EmitRows, FinishCount>), dim3(g.blocks), dim3(SEL_THREADS), 0, ctx->stream, P, Em, Fin, ctx->nslots,
                     g.tiles_per_block, ctx->scan.block_counts);
  hipError_t e = hipGetLastError();
  if (host) {
    unsigned long long m = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&m, &ctx->ds->n_out, sizeof(m), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    uint64_t k = std::min<uint64_t>(m, cap);
    if (e == hipSuccess && k) {
      e = hipMemcpy(id, d_id, k * 8, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(field, d_f, k * 4, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(ts, d_ts, k * 8, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(val, d_val, k * 8, hipMemcpyDeviceToHost);
    }
    if (n_out) *n_out = m;
  }
  if (e != hipSuccess) return fail_hip(ctx, e, "bmx_dump_rows");
  return BMX_OK;
}

int bmx_index_build(bmx_ctx* ctx, uint32_t field) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  return fresh_index(ctx, field, &ix);
}

int bmx_index_drop(bmx_ctx* ctx, uint32_t field) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < ctx->indexes.size(); i++)
    if (ctx->indexes[i].field == field) {
      free_columns(ctx->indexes[i]); ctx->indexes[i].view.release();
      ctx->indexes.erase(ctx->indexes.begin() + (long)i);
      if (ctx->indexes.empty()) ctx->chg.release();   // nothing left to maintain: the merges stop logging and the maintenance memory goes back
      return BMX_OK;
    }
  return fail(ctx, BMX_ERR_NO_INDEX, "no index on that field");
}

int bmx_index_size(bmx_ctx* ctx, uint32_t field, uint64_t* n_out) {
  if (!ctx || !n_out) return fail(ctx, BMX_ERR_INVALID, "bad arguments");
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  int rc = fresh_index(ctx, field, &ix);
  if (rc) return rc;
  *n_out = ix->n;
  return BMX_OK;
}

int bmx_index_refresh_counts(bmx_ctx* ctx, uint64_t* full_builds, uint64_t* incremental_updates) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (full_builds) *full_builds = ctx->chg.full_builds;
  if (incremental_updates) *incremental_updates = ctx->chg.incremental;
  return BMX_OK;
}

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

int bmx_scan_range(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  return scan_range_impl(ctx, field, lo, hi, out_ids, cap, n_out, mem);
}
int bmx_scan_equals(bmx_ctx* ctx, uint32_t field, int64_t value, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem) {
  return bmx_scan_range(ctx, field, value, value, out_ids, cap, n_out, mem);
}
int bmx_scan_count(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, uint64_t* n_out, int mem) {
  return bmx_scan_range(ctx, field, lo, hi, nullptr, 0, n_out, mem);
}

int bmx_scan_range_pos(bmx_ctx* ctx, uint32_t field, int64_t lo, int64_t hi, uint32_t* out_pos, uint64_t cap, uint64_t* n_out, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  return scan_range_impl_t<true>(ctx, field, lo, hi, out_pos, cap, n_out, mem);
}

int bmx_index_ids(bmx_ctx* ctx, uint32_t field, uint64_t first, uint64_t count, uint64_t* out_ids, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  int rc = fresh_index(ctx, field, &ix);
  if (rc) return rc;
  if (first > ix->n || count > ix->n - first) return fail(ctx, BMX_ERR_INVALID, "bmx_index_ids: range beyond the index (bmx_index_size)");
  if (count == 0) return BMX_OK;
  if (!out_ids) return fail(ctx, BMX_ERR_INVALID, "null output");
  HIPCHK(hipMemcpyAsync(out_ids, ix->ids + first, count * sizeof(uint64_t), host_or_dev(mem), ctx->stream));
  if (mem == BMX_MEM_HOST) HIPCHK(hipStreamSynchronize(ctx->stream));
  return BMX_OK;
}

int bmx_scan_filter(bmx_ctx* ctx, uint32_t nterms, const bmx_term* terms, uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (nterms == 0 || nterms > MAX_TERMS || !terms) return fail(ctx, BMX_ERR_INVALID, "filter needs 1..8 terms");
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (int erc = enter(ctx)) return erc;
  Index* ix;
  int rc = fresh_index(ctx, terms[0].field, &ix);
  if (rc) return rc;
  PredFilter P;
  P.v = ix->v64; P.ids = ix->ids; P.slots = ctx->slots; P.nslots = ctx->nslots; P.nterms = nterms;
  for (uint32_t k = 0; k < nterms; k++) { P.t[k] = terms[k]; P.t[k].lo = std::max<int64_t>(terms[k].lo, -VAL_MAX); }   // tombstones (INT64_MIN) match no term
  // with a value-ordered view of the first term's index: its run is the candidate list, the other terms are probed for those ids only (no order)
  if ((n_out || out_ids) && ensure_ordered_view(ctx, ix)) {
    const int src = run_scan_t<false>(ctx, P, ix, out_ids, cap, n_out, mem, true, P.t[0].lo, P.t[0].hi);
    if (!src) view_after_query(ctx, ix);
    return src;
  }
  return run_scan_t<false>(ctx, P, ix, out_ids, cap, n_out, mem);
}

static int partition_impl(bmx_ctx* ctx, uint64_t n, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val,
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

int bmx_host_alloc(uint64_t bytes, void** host_ptr) {
  if (!host_ptr || bytes == 0) return fail(nullptr, BMX_ERR_INVALID, "bmx_host_alloc: bad arguments");
  *host_ptr = nullptr;
  hipError_t e = hipHostMalloc(host_ptr, bytes, hipHostMallocPortable);
  if (e != hipSuccess) { (void)hipGetLastError(); *host_ptr = nullptr; return fail(nullptr, e == hipErrorOutOfMemory ? BMX_ERR_NOMEM : BMX_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
  return BMX_OK;
}
int bmx_host_free(void* host_ptr) {
  if (!host_ptr) return BMX_OK;
  hipError_t e = hipHostFree(host_ptr);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, BMX_ERR_HIP, std::string("hipHostFree: ") + hipGetErrorString(e)); }
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
  ctx->tail_armed.words = reinterpret_cast<const unsigned long long*>(words_dev); ctx->tail_armed.n = nwords; ctx->tail_armed.at_least = at_least;
  return BMX_OK;
}

int bmx_merge_notify(bmx_ctx* ctx, uint64_t* const* words, uint32_t nwords) {
  if (!ctx || nwords > PART_MAX_SHARDS || (nwords && !words)) return fail(ctx, BMX_ERR_INVALID, "bmx_merge_notify: at most 16 words");
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::memset(&ctx->notify, 0, sizeof(ctx->notify));
  for (uint32_t k = 0; k < nwords; k++) ctx->notify.p[k] = reinterpret_cast<unsigned long long*>(words[k]);
  ctx->n_notify = nwords; ctx->notify_seq = 0;
  return BMX_OK;
}

int bmx_set_deferred_compaction(bmx_ctx* ctx, int on) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  ctx->defer.enabled = on != 0 && !launches_are_serialized();    // (never where kernels run one at a time: see launches_are_serialized)
  return BMX_OK;
}
int bmx_set_wait_limit(bmx_ctx* ctx, double seconds) {
  if (!ctx || !(seconds >= 0.001) || seconds > 3600.0) return fail(ctx, BMX_ERR_INVALID, "bmx_set_wait_limit: 0.001 .. 3600 seconds");
  HIPCHK(hipSetDevice(ctx->device));
  const unsigned long long ticks = (unsigned long long)(seconds * 1.0e8);      // wall_clock64(): 100 MHz
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_wait_ticks), &ticks, sizeof(ticks), 0, hipMemcpyHostToDevice));
  return BMX_OK;
}
int bmx_set_side_stream(bmx_ctx* ctx, void* hip_stream) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;            // whatever is recorded or still on the old side stream is ordered into the context's stream first
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (ctx->defer.side) { HIPCHK(hipStreamSynchronize(ctx->defer.side)); if (!ctx->defer.side_is_callers) (void)hipStreamDestroy(ctx->defer.side); }
  ctx->defer.side = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : nullptr;    // nullptr: the next deferring merge creates the context's own again
  ctx->defer.side_is_callers = hip_stream != nullptr;
  return BMX_OK;
}
int bmx_merge_fence(bmx_ctx* ctx) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  return enter(ctx);
}
int bmx_get_deferred_counts(bmx_ctx* ctx, uint64_t* deferred, uint64_t* on_side_stream) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (deferred) *deferred = ctx->defer.n_deferred;
  if (on_side_stream) *on_side_stream = ctx->defer.n_side;
  return BMX_OK;
}

int bmx_set_probe_waves(bmx_ctx* ctx, int waves_per_simd) {
  if (!ctx || waves_per_simd < 3 || waves_per_simd > 8 || waves_per_simd == 7) return fail(ctx, BMX_ERR_INVALID, "bmx_set_probe_waves: 3, 4, 5, 6 or 8");
  ctx->k1_waves = waves_per_simd;
  return BMX_OK;
}

int bmx_get_placement(bmx_ctx* ctx, uint32_t* candidates, float* probe_us_chosen, float* probe_us_slowest) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (candidates) *candidates = ctx->placement_tries;
  if (probe_us_chosen) *probe_us_chosen = ctx->placement_us_best;
  if (probe_us_slowest) *probe_us_slowest = ctx->placement_us_worst;
  return BMX_OK;
}

int bmx_timer_start(bmx_ctx* ctx) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipEventRecord(ctx->prof.ev0, ctx->stream));
  return BMX_OK;
}

int bmx_timer_mark(bmx_ctx* ctx) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;          // the last batch's compaction is part of what is timed
  HIPCHK(hipEventRecord(ctx->prof.ev1, ctx->stream));
  return BMX_OK;
}
int bmx_timer_elapsed(bmx_ctx* ctx, float* ms_out) {
  if (!ctx || !ms_out) return fail(ctx, BMX_ERR_INVALID, "bad arguments");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipEventSynchronize(ctx->prof.ev1));
  HIPCHK(hipEventElapsedTime(ms_out, ctx->prof.ev0, ctx->prof.ev1));
  return BMX_OK;
}
int bmx_timer_stop(bmx_ctx* ctx, float* ms_out) {
  if (!ctx || !ms_out) return fail(ctx, BMX_ERR_INVALID, "bad arguments");
  if (int rc = bmx_timer_mark(ctx)) return rc;
  return bmx_timer_elapsed(ctx, ms_out);
}

int bmx_profile_enable(bmx_ctx* ctx, int on) {
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (on && ctx->prof.ev.empty()) {
    ctx->prof.ev.resize(4 * PROF_MAX_CALLS, nullptr);
    for (auto& ev : ctx->prof.ev) HIPCHK(hipEventCreate(&ev));
    ctx->prof.scan_ev.resize(3 * PROF_MAX_CALLS, nullptr);
    for (auto& ev : ctx->prof.scan_ev) HIPCHK(hipEventCreate(&ev));
  }
  ctx->prof.on = on != 0;
  ctx->prof.n = 0;
  ctx->prof.scan_n = 0;
  return BMX_OK;
}

int bmx_profile_read(bmx_ctx* ctx, float ms_out[3], uint32_t* n_calls) { return profile_means(ctx, false, ms_out, n_calls); }
int bmx_profile_read_scan(bmx_ctx* ctx, float ms_out[2], uint32_t* n_calls) { return profile_means(ctx, true, ms_out, n_calls); }

}  // extern "C"

#include "bmx_sync.inc"
#include "bmx_agg.inc"
#include "bmx_vc.inc"
#include "bmx_comm.inc"
