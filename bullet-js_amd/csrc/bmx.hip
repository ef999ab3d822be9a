// bmx.hip — C ABI (include/bmx.h) over the gfx950 kernels. One context = one GPU + one HIP stream.
// No CPU fallback exists: every entry point fails with BMX_ERR_NO_DEVICE / BMX_ERR_HIP when there is no GPU.
// This file: the state (bmx_ctx and its owned parts), the error and allocation helpers of all three handles (fail, HIPCHK_ON, dev_alloc_all: bmx_ctx here, bmx_vc in
// bmx_vc.inc, bmx_comm in bmx_comm.inc, each with its own last-error channel), check_status, bmx_selfcheck, create / destroy, the merge entry points, the point reads
// and the dump, the setters, timers and profiling. Everything else of the translation unit is the .inc files, by subject, in the two include lists below; what the
// queries set up alike in front of their launches (term checks and clamps, the int32 range clamp, the sweep grid) is bmx_query.inc, at the head of the first list.
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
#include "../../include/bmx_claim.h"
#include "merge_kernels.h"
#include "scan_kernels.h"
#include "select.h"
#include "slot.h"
#include "sync_kernels.h"
#include "view_kernels.h"
#include "agg_kernels.h"
#include "top_kernels.h"
#include "where_kernels.h"
#include "watch_kernels.h"
#include "where_agg_kernels.h"
#include "../../include/bmx_where_agg.h"
#include "group_kernels.h"
#include "rows_kernels.h"
#include "semi_kernels.h"
#include "quant_kernels.h"
#include "join_kernels.h"
#include "join_rows_kernels.h"
#include "update_kernels.h"
#include "mgroup_kernels.h"
#include "reach_kernels.h"
#include "first_kernels.h"
#include "gtop_kernels.h"
#include "expr_kernels.h"

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
// Its code is bmx_view.inc and bmx_view_sort.inc. Copied with its Index (ctx->indexes is a vector): no destructor, release() gives the buffers back.
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
  uint64_t layout = 0;       // stamp of the build that laid the columns out (build_index, from bmx_ctx::layout_seq: never 0, never repeated in a context); between two
                             // builds a row keeps its position and new rows are appended. Read by the standing queries (bmx_watch.inc) and handed to the callers of the row projection, whose cursors are positions (bmx_rows.inc)
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

// Each handle type keeps its own thread-local last-error word for the calls that have no handle to leave the text in:
// bmx_last_error(NULL), bmx_vc_last_error(NULL) and bmx_comm_last_error(NULL) are separate channels.
thread_local std::string g_err, g_vc_err, g_comm_err;
inline std::string& tls_err(const bmx_ctx*) { return g_err; }
inline std::string& tls_err(const bmx_vc*) { return g_vc_err; }
inline std::string& tls_err(const bmx_comm*) { return g_comm_err; }
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

// How the answer of one scan leaves the device (bmx_scan.inc: plan_delivery decides it in front of the launch, deliver carries it out behind it).
struct ScanDelivery {
  enum Route : uint8_t {
    DEVICE,          // BMX_MEM_DEVICE: the caller's device buffer and count word; nothing is waited for
    PINNED_SMALL,    // count only, or at most 16384 ids: through the mapped small-answer buffer (HostIO::pin_out), then a memcpy on the host
    CALLER_PINNED,   // the caller's buffer is page-locked: the kernels write it themselves
    STAGED,          // ScanScratch::out, then a download
    DEFERRED,        // ScanScratch::out, and the caller comes back with scan_collect (bmx_comm_scan_*)
  };
  enum CountHome : uint8_t { COUNT_CALLER /* DEVICE only */, COUNT_PIN_OUT /* the word behind the small answer's ids */, COUNT_HRES /* mapped result word HRES_SCAN_N */, COUNT_DEV_SCALAR /* ds->n_out: downloaded */ };
  Route route = DEVICE;
  void* d_out = nullptr; uint64_t d_cap = 0;            // where the kernels write ids (or positions), and how many at most; null: count only
  CountHome count = COUNT_CALLER; unsigned long long* d_n = nullptr;   // where the kernels write the count (null: a device-mode caller did not ask)
};

// Scratch of the scans and selects, grown on demand.
struct ScanScratch {
  uint64_t out_cap = 0; uint64_t* out = nullptr;       // a host-mode answer on its way down
  // what a scan on the deferred route (bmx_comm_scan_*: enqueue now, scan_collect() later) left for scan_collect: ids staged in `out`, and where the count is
  struct DeferredAnswer { uint64_t cap = 0; ScanDelivery::CountHome count = ScanDelivery::COUNT_DEV_SCALAR; } deferred;
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

// Scratch of the partition kernels (bmx_exchange.inc partition_impl).
struct PartScratch {
  uint32_t* counts = nullptr;         // PART_MAX_SHARDS * PART_BLOCKS, allocated at create
  uint8_t* owner = nullptr;           // owner shard of every delta of the batch being partitioned
  uint64_t owner_cap = 0;
  void release() { dev_free(counts); dev_free(owner); owner_cap = 0; }
};

// What the slab protocol of the cross-process exchange (bmx_exchange.inc) keeps between its calls and the merges they frame (read by bmx_merge.inc).
struct SlabProtocol {
  // bmx_merge_notify: words (possibly in other GPUs' memory) that every merge's last workgroup sets to the number of merges finished since
  SeqPtrs notify{}; uint32_t n_notify = 0; uint64_t notify_seq = 0;
  // bmx_merge_tail_wait: armed = the next default-path merge's resolve kernel polls these words before it ends; waited = a resolve kernel that did so has
  // been enqueued (the bmx_merge_records_after that asks for the same wait then launches no wait kernel)
  struct TailWait { const unsigned long long* words = nullptr; uint32_t n = 0; unsigned long long at_least = 0; } tail_armed, tail_waited;
  bool notify_armed = false;          // set by bmx_merge_records_after around ITS merge: only the merges of the slab protocol count up the peers' free words
};

// Scratch of the reconciliation sweeps (bmx_sync.inc): what a BMX_MEM_HOST caller's digest vectors, bucket set and records pass through. Grow-only.
struct SyncScratch {
  unsigned long long* dig = nullptr;      // 2 x 2^16 words: sums and counts
  unsigned long long* bits = nullptr;     // 2^16 bits
  bmx_delta_rec* recs = nullptr; uint64_t recs_cap = 0;
  void release() { dev_free(dig); dev_free(bits); dev_free(recs); recs_cap = 0; }
};

// Scratch of the aggregate queries (bmx_agg.inc): one accumulator per group, which every query's last kernel leaves empty again (clean), and the records of a
// BMX_MEM_HOST answer on their way down. Grow-only: 1025 records at first, 65537 with the first query that has more groups.
struct AggScratch {
  AggRaw* raw = nullptr; bmx_agg* stage = nullptr; uint32_t cap = 0;
  bool clean = false;
  void release() { dev_free(raw); dev_free(stage); cap = 0; clean = false; }
};

// Scratch of the ordered top-k queries (bmx_top.inc): the select's state record, which every query's last kernel leaves ready for the next (clean), the
// candidate list, and the counts + records of a BMX_MEM_HOST answer on their way down. Allocated by the first query.
struct TopScratch {
  TopState* state = nullptr; unsigned long long* cand_u = nullptr; unsigned long long* cand_id = nullptr; uint8_t* stage = nullptr;
  bool clean = false;
  void release() { dev_free(state); dev_free(cand_u); dev_free(cand_id); dev_free(stage); clean = false; }
};

// Scratch of the group-by over discovered values (bmx_group.inc): the open-addressed table (a key word and an accumulator per slot) and the state record, which
// every query's last kernel leaves empty again (clean), and the records + result record of a BMX_MEM_HOST answer on their way down. Grows to the largest cap
// asked so far, all or nothing; a query with a smaller cap uses the head of the table.
struct GroupScratch {
  long long* keys = nullptr; AggRaw* acc = nullptr; GroupState* state = nullptr; bmx_group_rec* stage = nullptr; bmx_group_res* stage_res = nullptr;
  uint64_t cap = 0, slots = 0;
  bool clean = false;
  void release() { dev_free(keys); dev_free(acc); dev_free(state); dev_free(stage); dev_free(stage_res); cap = 0; slots = 0; clean = false; }
};

// Scratch of the group-by over several fields (bmx_group_multi.inc): the tuple table (GroupScratch's shape, keyed by the packed word), the dictionaries
// (dict_words key words: nkeys tables of a query's slot count at the head), the state records (the tuple table's, then one per dictionary), which every query's
// last kernels leave empty again (clean), and the records + result record of a BMX_MEM_HOST answer on their way down. Grows to the largest cap and the most
// dictionary words asked so far, all or nothing.
struct MGroupScratch {
  long long* keys = nullptr; AggRaw* acc = nullptr; long long* dict = nullptr; GroupState* state = nullptr; bmx_mgroup_rec* stage = nullptr; bmx_group_res* stage_res = nullptr;
  uint64_t cap = 0, slots = 0, dict_words = 0;
  bool clean = false;
  void release() { dev_free(keys); dev_free(acc); dev_free(dict); dev_free(state); dev_free(stage); dev_free(stage_res); cap = 0; slots = 0; dict_words = 0; clean = false; }
};

// Scratch of the row projection (bmx_rows.inc): the columns and the result record of a BMX_MEM_HOST answer on their way down (`stage`: 8-byte words, grown on
// demand), and what a call's mask pass leaves its emit pass (the base index as the mask pass saw it; the sharded form enqueues every shard's mask pass first).
struct RowsScratch {
  unsigned long long* stage = nullptr; uint64_t stage_words = 0; bmx_rows_res* stage_res = nullptr;
  struct Masked { const uint64_t* ids = nullptr; const void* v = nullptr; uint64_t n = 0, layout = 0; bool fits32 = false; uint32_t nb = 0; } masked;
  void release() { dev_free(stage); dev_free(stage_res); stage_words = 0; }
};

// Scratch of the semi-joins (bmx_semi.inc): the open-addressed table of key words and the state record, which every query's last kernel leaves empty again
// (clean), and the staging of the host-mode and sharded forms: a list of values on its way up or of exported keys on its way down (stage_keys, `cap` words), the
// result record, and the ids of an answer on their way down (stage_ids, grown on demand; `staged`: how many the last staged query had room for). The table
// grows to the largest set_cap asked so far, all or nothing; a query with a smaller set_cap uses the head of the table.
struct SemiScratch {
  long long* keys = nullptr; SemiState* state = nullptr; long long* stage_keys = nullptr; bmx_semi_res* stage_res = nullptr;
  uint64_t* stage_ids = nullptr; uint64_t ids_cap = 0, staged = 0;
  uint64_t cap = 0, slots = 0;
  bool clean = false;
  void release() { dev_free(keys); dev_free(state); dev_free(stage_keys); dev_free(stage_res); dev_free(stage_ids); ids_cap = 0; staged = 0; cap = 0; slots = 0; clean = false; }
};

// Scratch of the lookup joins (bmx_join.inc): the open-addressed map of {key, attribute} pairs and its state record, which every query's last kernel leaves empty
// again (clean), and the staging of the host-mode and sharded forms: the pairs of a list on their way up or of an exported map on their way down (stage_keys,
// stage_vals, `cap` words each) and the result record. The map grows to the largest map_cap asked so far, all or nothing; a query with a smaller map_cap uses
// the head of the table. The records are aggregated in GroupScratch's table and come down through its staging.
struct JoinScratch {
  JoinPair* map = nullptr; JoinState* state = nullptr; long long* stage_keys = nullptr; long long* stage_vals = nullptr; bmx_join_res* stage_res = nullptr;
  uint64_t cap = 0, slots = 0;
  bool clean = false;
  void release() { dev_free(map); dev_free(state); dev_free(stage_keys); dev_free(stage_vals); dev_free(stage_res); cap = 0; slots = 0; clean = false; }
};

// Scratch of the quantiles (bmx_quant.inc): the select's state record, which every query's last kernel leaves empty again (clean), the position-indexed value
// scratch of a probed measure (8 bytes per index position, allocated by the first such query and grown with the index) and the records + result record of a
// BMX_MEM_HOST answer on their way down.
struct QuantScratch {
  QuantState* state = nullptr; int64_t* vals = nullptr; uint64_t vals_cap = 0; uint8_t* stage = nullptr;
  bool clean = false;
  void release() { dev_free(state); dev_free(vals); dev_free(stage); vals_cap = 0; clean = false; }
};

// Scratch of the computed measures (bmx_expr.inc): the two counters of bmx_expr_res, which every query's last kernel (k_expr_finish) leaves zero again (clean), and
// the record of a BMX_MEM_HOST or sharded answer on its way down.
struct ExprScratch {
  ExprState* state = nullptr; bmx_expr_res* stage = nullptr;
  bool clean = false;
  void release() { dev_free(state); dev_free(stage); clean = false; }
};

// Scratch of the update by query (bmx_update.inc): the staging slab of records the emit pass fills and the merge reads, the winners' indices and ids (`cap` of
// each, grown on demand), the words between the passes (counts: what the host waits for; ctr: the sharded counters of the mask pass, zero between two calls), the
// merge's count and stats, the record of a BMX_MEM_HOST answer on its way down, and what a call's mask pass leaves its emit pass (as RowsScratch::masked).
struct UpdScratch {
  bmx_delta_rec* recs = nullptr; uint32_t* applied = nullptr; uint64_t* ids = nullptr; uint64_t cap = 0;
  UpdCounts* counts = nullptr; unsigned long long* ctr = nullptr; unsigned long long* n_applied = nullptr; bmx_merge_stats* stats = nullptr; bmx_upd_res* stage_res = nullptr;
  RowsScratch::Masked masked;
  void release() { dev_free(recs); dev_free(applied); dev_free(ids); dev_free(counts); dev_free(ctr); dev_free(n_applied); dev_free(stats); dev_free(stage_res); cap = 0; }
};

// Scratch of the graph traversal (bmx_reach.inc): one link word and one depth byte per position of the base field's index (allocated by the first traversal and
// grown with the largest index seen, like QuantScratch::vals), the state record, which every call's last kernel leaves zero again (clean), and the ids, depths
// and result record of a BMX_MEM_HOST answer on their way down (`staged`: how many entries the last staged call had room for). The map is JoinScratch's.
// Nothing here survives a call, so an index laid out anew needs no care.
struct ReachScratch {
  long long* link = nullptr; uint8_t* depth = nullptr; uint64_t pos_cap = 0;
  ReachState* state = nullptr; bool clean = false;
  uint64_t* stage_ids = nullptr; uint8_t* stage_depth = nullptr; uint64_t stage_cap = 0, staged = 0; bmx_reach_res* stage_res = nullptr;
  void release() {
    dev_free(link); dev_free(depth); dev_free(state); dev_free(stage_ids); dev_free(stage_depth); dev_free(stage_res);
    pos_cap = 0; stage_cap = 0; staged = 0; clean = false;
  }
};

// Scratch of the first node per group (bmx_first.inc), beside GroupScratch, whose table it uses: one id word per slot, which every query's last kernel leaves at
// BMX_FIRST_NO_NODE again (clean), the two words per position of the base field's index that pass 1 leaves pass 2 (allocated by the first query and grown with
// the largest index seen, like ReachScratch::link), and the records, columns (8-byte words, grown on demand) and result record of a BMX_MEM_HOST answer on their
// way down. Nothing here survives a call, so an index laid out anew needs no care.
struct FirstScratch {
  unsigned long long* idw = nullptr; uint64_t slots = 0; bool clean = false;
  long long* gw = nullptr; long long* ow = nullptr; uint64_t pos_cap = 0;
  bmx_first_rec* stage = nullptr; unsigned long long* stage_cols = nullptr; bmx_first_res* stage_res = nullptr; uint64_t stage_cap = 0, stage_words = 0;
  void release() {
    dev_free(idw); dev_free(gw); dev_free(ow); dev_free(stage); dev_free(stage_cols); dev_free(stage_res);
    slots = 0; clean = false; pos_cap = 0; stage_cap = 0; stage_words = 0;
  }
};

// Scratch of the first N nodes per group (bmx_group_top.inc), beside GroupScratch and FirstScratch, whose table, id words and words per position it uses: per slot
// the previous winner, the round's extreme and the rank counter, which every query's last kernel leaves at rest again (clean), the rounds' counters, `per` winner
// pairs per slot (grown to the largest slots * per asked so far; read only below the rank counter, so they need no rest state), and the groups, rows, columns
// (8-byte words) and result record of a BMX_MEM_HOST answer on their way down. Nothing here survives a call.
struct GtopScratch {
  long long* pv = nullptr; unsigned long long* pid = nullptr; long long* ext = nullptr; uint32_t* rank = nullptr; GtopState* state = nullptr;
  uint64_t slots = 0; bool clean = false;
  bmx_gtop_row* win = nullptr; uint64_t win_rows = 0;
  bmx_gtop_grp* stage = nullptr; bmx_gtop_row* stage_rows = nullptr; unsigned long long* stage_cols = nullptr; bmx_gtop_res* stage_res = nullptr;
  uint64_t stage_cap = 0, stage_rows_cap = 0, stage_words = 0;
  void release() {
    dev_free(pv); dev_free(pid); dev_free(ext); dev_free(rank); dev_free(state); dev_free(win);
    dev_free(stage); dev_free(stage_rows); dev_free(stage_cols); dev_free(stage_res);
    slots = 0; clean = false; win_rows = 0; stage_cap = 0; stage_rows_cap = 0; stage_words = 0;
  }
};

// The standing queries of one context (bmx_watch.inc). A watch: its prepared program, its base field, `prev` (the committed set, one bit per position of the base
// field's index) and the stamp of the index layout that bitmap was sized and zeroed for (0: none yet). Shared by the watches: per watch the stamp of the layout it
// last COMMITTED under (device words: a device-mode poll commits without the host), the two scratch masks and three count arrays of a poll, its totals record
// (tot[0]; tot[1] is where a host-mode poll's record waits for its download when there is no mapped word), and what the first half of a poll leaves the second.
struct Watch {
  bool live = false; uint32_t base_field = 0; WhereProg W{};
  uint32_t* prev = nullptr; uint64_t prev_words = 0; uint64_t layout = 0;
};
struct WatchState {
  Watch w[BMX_WATCH_MAX];
  unsigned long long* committed = nullptr;   // [BMX_WATCH_MAX]
  uint32_t* entered = nullptr; uint32_t* left = nullptr; uint32_t* counts = nullptr; uint64_t blocks_cap = 0;   // masks: one allocation, 256 words per 8192-row block, `left` blocks_cap blocks behind `entered`; counts: 3 x blocks_cap
  WatchTotals* tot = nullptr;
  bmx_watch_res* hres = nullptr;             // mapped page-locked record of the host-mode polls
  struct Pending { bool on = false; uint32_t watch = 0; uint64_t n = 0; uint32_t nb = 0; const uint64_t* ids = nullptr; uint64_t layout = 0; } pend;
  int ensure(bmx_ctx* ctx, uint64_t nb);     // scratch for an index of nb blocks
  void release() {
    for (auto& x : w) { dev_free(x.prev); x.prev_words = 0; x.live = false; }
    dev_free(committed); dev_free(entered); left = nullptr; dev_free(counts); dev_free(tot); blocks_cap = 0; pend.on = false;
    if (hres) (void)hipHostFree(hres);
    hres = nullptr;
  }
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
  int cus = 1;                        // compute units of the device, looked up at create (sweep_grid)
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
  TopScratch top;
  GroupScratch group;
  RowsScratch rows;
  SemiScratch semi;
  QuantScratch quant;
  JoinScratch join;
  UpdScratch upd;
  MGroupScratch mgroup;
  ReachScratch reach;
  FirstScratch first;
  GtopScratch gtop;
  ExprScratch expr;
  WatchState watch;
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
  uint64_t layout_seq = 0;            // index builds so far (Index::layout)
  SlabProtocol slab;
  uint32_t placement_tries = 0, placement_tries_asked = 0; float placement_us_best = 0, placement_us_worst = 0;   // what alloc_table_tuned saw for the current table
  uint64_t n_row_waits = 0;           // merges that waited for a batch in flight to report its row count (wait_for_row_reports)
  bool claim_team = false;            // claim mode (BMX_CLAIM_MODE): a claimer swaps head, ts and val in one team request (team_claim) instead of exchange + store
  int k1_waves = 8;                   // BMX_K1_WAVES (8, 6 or 5): resident waves per SIMD of the probe kernel
  std::string err;
};

namespace {

// The error and allocation helpers of all three handles (bmx_ctx here, bmx_vc in bmx_vc.inc, bmx_comm in bmx_comm.inc): the text goes to the handle, if there
// is one, and to the handle type's own thread-local word. A bare nullptr means "no context".
template <class H>
int fail(H* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  tls_err(h) = msg;
  return code;
}
inline int fail(std::nullptr_t, int code, const std::string& msg) { return fail(static_cast<bmx_ctx*>(nullptr), code, msg); }
inline hipMemcpyKind host_or_dev(int mem) { return mem == BMX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice; }
template <class H>
int fail_hip(H* h, hipError_t e, const char* what) {
  return fail(h, BMX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// HIPCHK_ON(handle, call) returns BMX_ERR_HIP with the call's text from the enclosing function; HIPCHK(call) is the same for a function whose handle is `ctx`.
// HIPCHK_BAIL is for the create functions, which leave through their `bail` lambda (it destroys the half-built handle and keeps the text).
#define HIPCHK_ON(h, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail_hip(h, e__, #call); } while (0)
#define HIPCHK(call) HIPCHK_ON(ctx, call)
#define HIPCHK_BAIL(h, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return bail(fail_hip(h, e__, #call)); } while (0)
#define LAUNCHCHK(name)                                               \
  do {                                                                \
    hipError_t e__ = hipGetLastError();                               \
    if (e__ != hipSuccess) return fail_hip(ctx, e__, "launch " name); \
  } while (0)

template <class H>
int dev_alloc_all(H* h, std::initializer_list<DevBuf> bufs) {   // (alloc_all) BMX_ERR_NOMEM on out-of-memory, BMX_ERR_HIP otherwise
  hipError_t e = hipSuccess;
  if (alloc_all(bufs, &e)) return BMX_OK;
  return fail(h, e == hipErrorOutOfMemory ? BMX_ERR_NOMEM : BMX_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
}
template <class H, class T>
int dev_alloc(H* h, T** p, uint64_t count) { return dev_alloc_all(h, {{*p, std::max<uint64_t>(count, 1) * sizeof(T)}}); }
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

}  // namespace

// ---- the rest of this translation unit, by subject ----
// The ORDER of the two include lists is part of the build: kernel templates are laid out in the gfx950 code object in the order the source first uses them, and
// the code object is held byte-identical across refactors of the host side. So every file sits where its code always sat, which is why two subjects come in two
// files each: the index build in front of the view's patch and the refresh (which calls the patch) behind it, with the view's sort behind the refresh; the range
// scans in front of this file's own entry points (bmx_selfcheck and bmx_dump_rows launch kernel templates) and the position scan and the filter behind them.
#include "bmx_query.inc"   // (host arithmetic only: it launches nothing, so it has no place to keep)
#include "bmx_merge.inc"
#include "bmx_host.inc"
#include "bmx_index.inc"
#include "bmx_view.inc"
#include "bmx_index_refresh.inc"
#include "bmx_view_sort.inc"
#include "bmx_scan.inc"
#include "bmx_exchange.inc"

namespace {

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

}  // extern "C"

namespace {
// Both tear checks (k_selfcheck_tear: the 16-byte store, or with `team` the team swap, each followed by its control). Synchronous for the caller, on a stream of its
// own (nothing else on the device is waited for); allocates and frees 128 KB + 4 words. -> h = {torn, reads, control torn, control reads}
int run_tear_check(int device, bool team, unsigned long long (&h)[4]) {
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
  h[0] = h[1] = h[2] = h[3] = 0;
  hipStream_t cs = nullptr;       // a stream of its own: no device-wide synchronisation, nothing of another context or library is waited for
  const char* nul = std::getenv("BMX_SELFCHECK_NULL_STREAM");     // measurement switch (round 5): the device's null stream, as rounds 1-4 used
  hipError_t e = (nul && nul[0] == '1') ? hipSuccess : hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMemsetAsync(slots, 0, (size_t)NS * 32, cs);
  if (e == hipSuccess) e = hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), cs);
  if (e == hipSuccess) {
    if (team) hipLaunchKernelGGL((k_selfcheck_tear<false, true>), dim3(BLOCKS), dim3(256), 0, cs, slots, NS, ITERS, d, d + 1);
    else hipLaunchKernelGGL((k_selfcheck_tear<false>), dim3(BLOCKS), dim3(256), 0, cs, slots, NS, ITERS, d, d + 1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemsetAsync(slots, 0, (size_t)NS * 32, cs);
  if (e == hipSuccess) {
    if (team) hipLaunchKernelGGL((k_selfcheck_tear<true, true>), dim3(BLOCKS), dim3(256), 0, cs, slots, NS, ITERS / 4, d + 2, d + 3);
    else hipLaunchKernelGGL((k_selfcheck_tear<true>), dim3(BLOCKS), dim3(256), 0, cs, slots, NS, ITERS / 4, d + 2, d + 3);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, cs);
  if (e == hipSuccess) e = hipStreamSynchronize(cs);
  if (cs) (void)hipStreamDestroy(cs);
  (void)hipFree(slots); (void)hipFree(d);
  if (e != hipSuccess) return fail_hip(ctx, e, "bmx_selfcheck");
  return BMX_OK;
}
}  // namespace

extern "C" {

// bmx.h "bmx_selfcheck"
int bmx_selfcheck(int device, uint64_t* reads_out, uint64_t* torn_out, uint64_t* control_torn_out) {
  unsigned long long h[4];
  if (int rc = run_tear_check(device, false, h)) return rc;
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

// bmx_claim.h "bmx_selfcheck_claim". A torn pair is a result, not an error: the caller (bmx_create) keeps claim mode `store` then.
int bmx_selfcheck_claim(int device, uint64_t* reads_out, uint64_t* torn_out, uint64_t* control_torn_out) {
  unsigned long long h[4];
  if (int rc = run_tear_check(device, true, h)) return rc;
  if (reads_out) *reads_out = h[1];
  if (torn_out) *torn_out = h[0];
  if (control_torn_out) *control_torn_out = h[2];
  return BMX_OK;
}

int bmx_get_claim_mode(bmx_ctx* ctx) {
  if (!ctx) return fail(ctx, BMX_ERR_INVALID, "bmx_get_claim_mode: no context");
  return ctx->claim_team ? BMX_CLAIM_TEAM : BMX_CLAIM_STORE;
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
  bool team_checked = false;
  {  // once per device and process: the 16-byte load/store indivisibility the probe kernel relies on is checked on THIS box (BMX_SKIP_SELFCHECK=1 skips it)
    static std::atomic<unsigned> checked[64];
    const char* skip = std::getenv("BMX_SKIP_SELFCHECK");
    if (device < 64 && !(skip && skip[0] == '1') && !checked[device].load()) {
      int src = bmx_selfcheck(device, nullptr, nullptr, nullptr);
      if (src) return src;
      // the team swap's indivisibility, beside it: no torn pair AND a control that tore = claim mode `team` is sound on this box (2); anything else,
      // a failed run included, silently keeps `store` (1)
      uint64_t torn = 0, control = 0;
      const bool team_ok = bmx_selfcheck_claim(device, nullptr, &torn, &control) == BMX_OK && torn == 0 && control != 0;
      checked[device].store(team_ok ? 2u : 1u);
    }
    team_checked = device < 64 && checked[device].load() == 2u;
  }
  bmx_ctx* ctx = new (std::nothrow) bmx_ctx();
  if (!ctx) return fail(nullptr, BMX_ERR_NOMEM, "out of host memory");
  ctx->device = device;
  ctx->capacity_rows = capacity_rows;
  ctx->load_pct = max_load_pct;
  auto bail = [&](int rc) { std::string m = ctx->err; bmx_destroy(ctx); g_err = m; return rc; };
  HIPCHK_BAIL(ctx, hipSetDevice(device));
  HIPCHK_BAIL(ctx, hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, device));
  ctx->cus = std::max(ctx->cus, 1);
  HIPCHK_BAIL(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
  ctx->stream = ctx->own_stream;
  HIPCHK_BAIL(ctx, hipEventCreate(&ctx->prof.ev0));
  HIPCHK_BAIL(ctx, hipEventCreate(&ctx->prof.ev1));
  for (auto& S : ctx->host.stg) { HIPCHK_BAIL(ctx, hipEventCreateWithFlags(&S.up, hipEventDisableTiming)); HIPCHK_BAIL(ctx, hipEventCreateWithFlags(&S.done, hipEventDisableTiming)); }
  const uint64_t nslots = slots_for(capacity_rows, max_load_pct);
  ctx->nslots = nslots;
  ctx->placement_tries_asked = (flags >> 8) & 0xFu;         // BMX_CTX_PLACEMENT_TRIES(n): 0 = the default
  if (ctx->placement_tries_asked > 8) ctx->placement_tries_asked = 8;
  // claim mode: `team` where this process has seen the team swap checked on the device; BMX_CLAIM_MODE=store|team overrides it (set before the table is placed:
  // the placement probe issues the mode's request mix)
  ctx->claim_team = team_checked;
  { const char* cm = std::getenv("BMX_CLAIM_MODE"); if (cm && !std::strcmp(cm, "store")) ctx->claim_team = false; else if (cm && !std::strcmp(cm, "team")) ctx->claim_team = true; }
  int rc;
  if ((rc = alloc_table_tuned(ctx, nslots, &ctx->slots))) return bail(rc);
  if ((rc = dev_alloc(ctx, &ctx->ds, 1))) return bail(rc);
  if ((rc = ctx->host.create(ctx))) return bail(rc);
  if ((rc = dev_alloc_all(ctx, {{ctx->scan.block_counts, SEL_MAX_BLOCKS * sizeof(uint32_t)}, {ctx->part.counts, PART_MAX_SHARDS * PART_BLOCKS * sizeof(uint32_t)},
                                {ctx->ws.shard_ctr, MergeWs::SETS * CTR_SHARDS * CTR_STRIDE * sizeof(unsigned long long)}})))
    return bail(rc);
  HIPCHK_BAIL(ctx, hipMemsetAsync(ctx->ws.shard_ctr, 0, MergeWs::SETS * CTR_SHARDS * CTR_STRIDE * sizeof(unsigned long long), ctx->stream));
  // the row-count mirror is an optimisation: without mapped host memory the capacity guard simply synchronises as before
  if (hipHostMalloc(reinterpret_cast<void**>(&ctx->host_rows), 2 * sizeof(unsigned long long), hipHostMallocMapped) == hipSuccess) {
    ctx->host_rows[0] = 0; ctx->host_rows[1] = 0;
  } else { ctx->host_rows = nullptr; (void)hipGetLastError(); }
  ctx->fixed_capacity = (flags & BMX_CTX_FIXED_CAPACITY) != 0;
  ctx->defer.enabled = !launches_are_serialized();
  ctx->view.read_env();
  { const char* kw = std::getenv("BMX_K1_WAVES"); if (kw && kw[0] >= '3' && kw[0] <= '8' && kw[0] != '7' && !kw[1]) ctx->k1_waves = kw[0] - '0'; }
  HIPCHK_BAIL(ctx, hipMemsetAsync(ctx->ds, 0, sizeof(DevScalars), ctx->stream));
  hipLaunchKernelGGL(k_init_slots, dim3(2048), dim3(256), 0, ctx->stream, ctx->slots, nslots);
  HIPCHK_BAIL(ctx, hipGetLastError());
  HIPCHK_BAIL(ctx, hipStreamSynchronize(ctx->stream));
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
  ctx->top.release();
  ctx->group.release();
  ctx->rows.release();
  ctx->semi.release();
  ctx->quant.release();
  ctx->join.release();
  ctx->upd.release();
  ctx->mgroup.release();
  ctx->reach.release();
  ctx->first.release();
  ctx->gtop.release();
  ctx->expr.release();
  ctx->watch.release();
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

// ---- the second include list (the order constraint: see the first) ----
#include "bmx_scan_filter.inc"
#include "bmx_sync.inc"
#include "bmx_agg.inc"
#include "bmx_top.inc"
#include "bmx_vc.inc"
#include "bmx_comm.inc"
#include "bmx_vc_sync.inc"   // (behind everything that was here before it: its kernels follow the others in the code object)
#include "bmx_where.inc"     // (likewise; bmx_comm.inc declares the two functions of it that it calls. It also holds what every form below shares: the predicate, the
                             //  width dispatch of a sweep, the entry guards, the mask pass and the cursor steps of the paged sharded forms; the emit pass's
                             //  geometry, emit_dispatch, is bmx_scan.inc's)
#include "bmx_watch.inc"     // (likewise)
#include "bmx_where_agg.inc" // (likewise)
#include "bmx_group.inc"     // (likewise; it holds the collect, merge and sharded combine of every grouped answer)
#include "bmx_rows.inc"      // (likewise; it holds the staging growth and the column copy of every projected answer)
#include "bmx_semi.inc"      // (likewise)
#include "bmx_quant.inc"     // (likewise)
#include "bmx_join.inc"      // (likewise; it uses bmx_group.inc's scratch and grouped-answer steps and bmx_semi.inc's slot count)
#include "bmx_join_rows.inc" // (likewise; it uses bmx_join.inc's map scratch, bmx_rows.inc's mask pass, staging and column copy and bmx_where.inc's mask pass)
#include "bmx_update.inc"    // (likewise; it calls bmx_merge.inc's merge_core with records it made itself; its mask pass is bmx_where.inc's)
#include "bmx_group_multi.inc" // (likewise; it uses bmx_group.inc's slot count, finish grid, fold and grouped-answer steps, and a scratch of its own)
#include "bmx_reach.inc"     // (likewise; it uses bmx_join.inc's map scratch, bmx_semi.inc's grids and slot count and bmx_where.inc's mask pass)
#include "bmx_first.inc"     // (likewise; it uses bmx_group.inc's table, scratch and grouped-answer steps)
#include "bmx_group_top.inc" // (likewise; it uses bmx_first.inc's passes 1 and 2 and bmx_group.inc's grouped-answer steps)
#include "bmx_expr.inc"      // (likewise; it calls the enqueue, collect and combine steps of bmx_where_agg.inc, bmx_group.inc and bmx_quant.inc with a computed measure)
