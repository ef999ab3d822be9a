// update_kernels.h — update and delete by query (bmx_update.h bmx_where_update): a boolean filter's selection turned into 32-byte delta records on the device,
// which the merge then takes as any other batch of records, gfx950, wave64.
//
// The four ops come down to two questions, both uniform over the launch: where the value's source is (UPD_SRC_NONE: the operand alone, SET and DELETE;
// UPD_SRC_COLUMN: the base field's index column, COPY / ADD with src_field == base_field; UPD_SRC_PROBE: one agg_probe of src_field) and what is added to it
// (`operand`: 0 for COPY; for SET and DELETE it IS the value). They travel as kernel arguments and are tested in scalar branches; no per-lane array is indexed
// by the op (where_kernels.h on scratch).
//
// Pass 1 is select.h's k_scan_mask<PredUpd<T>, true>: rows_kernels.h's PredRowsFrom (the program behind a cursor) and, for a source that is read, one look at the
// source for each row the program selected. The bit is cleared when the source holds no data (absent or tombstone) or the sum leaves +-VAL_MAX, so the mask is
// exactly the WRITABLE nodes and pass 2 ranks dense records: no holes, no second compaction. The cleared bits are counted without an atomic per node:
// k_scan_mask calls mask() under a divergent branch (the lanes behind the column's end do not call), so the lanes' counts (0 .. E) are summed over the lanes
// that are there with three ballots, and the wave's first such lane adds the sum — if it is not zero — to one of UPD_CTR_SHARDS counter pairs, each in a 64-byte
// line of its own, picked by the workgroup's number: at most one non-returning atomic per wave and 64 * E rows, spread over 64 lines.
//
// Pass 2, k_upd_emit<T, SUB>, ranks exactly like k_rows_emit (the counts of the blocks in front, block_excl_scan, the loc[] transpose; SUB = 1 / 8) and writes,
// for the ranks below cap, one bmx_delta_rec per node into the staging slab as two 16-byte stores; consecutive lanes land on consecutive records. The source is
// read again (pass 1 keeps bits, not values); the table has not changed in between. The lane that meets the node of rank cap writes next_pos; the last
// workgroup sums the counter shards, puts them back to zero for the next call and writes the counts the host waits for (UpdCounts).
//
// k_upd_finish, behind the merge: out_ids[k] = recs[applied_idx[k] & BMX_APPLIED_INDEX].id for the n_applied winners (the compaction delivers them in batch
// order, which is index order), and the bmx_upd_res from UpdCounts and the merge's stats.
//
// No lane waits on a word another lane must write; every loop is bounded by the block, by the probe's slot count or by the grid stride.
#pragma once
#include "rows_kernels.h"
#include "../../include/bmx_update.h"

namespace bmx {

static_assert(sizeof(bmx_upd_res) == 72, "the record of bmx_update.h");
static_assert(sizeof(bmx_delta_rec) == 32, "a record is two 16-byte stores");
static_assert(BMX_UPD_MAX_CAP == MAX_BATCH, "cap is the merge's batch limit");

constexpr uint32_t UPD_SRC_NONE = 0u, UPD_SRC_COLUMN = 1u, UPD_SRC_PROBE = 2u;
constexpr uint32_t UPD_CTR_SHARDS = 64u, UPD_CTR_STRIDE = 8u;     // 64 lines of 64 bytes: word 0 = n_nosrc, word 1 = n_range

// how a node's value comes about (uniform over a launch)
struct UpdSrc {
  uint32_t kind, field;        // UPD_SRC_*; the probed field
  int64_t operand;             // NONE: the value itself; otherwise what is added to the source (0: COPY)
};

// what pass 2 leaves the host (one download, the call's one wait) and k_upd_finish
struct UpdCounts { unsigned long long n_writable, n_sent, n_nosrc, n_range, next_pos, layout; };

// the source value of the selected row at `pos` (kind != NONE) -> 0 = writable (y: the value to write), 1 = no data, 2 = the sum leaves the range
template <class T>
__device__ __forceinline__ uint32_t upd_value(const UpdSrc& S, const T* __restrict__ v, const uint64_t* __restrict__ ids, const Slot* __restrict__ slots, uint64_t nslots,
                                              uint64_t pos, int64_t& y) {
  if (S.kind == UPD_SRC_COLUMN) y = (int64_t)v[pos];                      // a selected row holds data
  else if (!agg_probe(slots, nslots, ids[pos], S.field, y) || y == VAL_DELETED) return 1u;
  y += S.operand;                                                          // |y|, |operand| <= 2^53 - 1: no overflow
  return (y < -VAL_MAX || y > VAL_MAX) ? 2u : 0u;
}

// the sum of c (0 .. 7) over the lanes of the wave that are here
__device__ __forceinline__ uint32_t upd_wave_sum(uint32_t c) {
  return (uint32_t)__popcll(__ballot((c & 1u) != 0u)) + 2u * (uint32_t)__popcll(__ballot((c & 2u) != 0u)) + 4u * (uint32_t)__popcll(__ballot((c & 4u) != 0u));
}

template <class T, bool CLOCKS>
struct PredUpd {   // the program behind a cursor AND (the node's record can be written)
  static constexpr int E = PredWhere<T>::E;
  static_assert(E < 8, "upd_wave_sum takes a lane's count in three bits");
  PredRowsFrom<T, CLOCKS> R;
  UpdSrc S;
  unsigned long long* ctr;                        // UPD_CTR_SHARDS x UPD_CTR_STRIDE words
  __device__ uint32_t mask(uint64_t first, uint64_t n) const {
    const uint32_t sel = R.mask(first, n);
    if (S.kind == UPD_SRC_NONE) return sel;       // (uniform) SET, DELETE: PredRowsFrom itself
    const T* v = R.P.v;
    uint32_t out = 0, nosrc = 0, range = 0;
    for (uint32_t m = sel; m; m &= m - 1u) {      // this lane's rows that the program selected
      const uint32_t e = (uint32_t)__ffs((int)m) - 1u;
      int64_t y;
      const uint32_t why = upd_value<T>(S, v, R.P.ids, R.P.slots, R.P.nslots, first + e, y);
      if (why == 0u) out |= 1u << e;
      nosrc += why == 1u ? 1u : 0u;
      range += why == 2u ? 1u : 0u;
    }
    const uint32_t w_nosrc = upd_wave_sum(nosrc), w_range = upd_wave_sum(range);
    const unsigned long long here = __ballot(true);
    if ((threadIdx.x & 63u) == (uint32_t)__ffsll((long long)here) - 1u) {
      unsigned long long* c = ctr + (size_t)(blockIdx.x & (UPD_CTR_SHARDS - 1u)) * UPD_CTR_STRIDE;
      if (w_nosrc) atomicAdd(c, (unsigned long long)w_nosrc);
      if (w_range) atomicAdd(c + 1, (unsigned long long)w_range);
    }
    return out;
  }
};

struct UpdArgs {
  const uint64_t* ids; const void* v;           // the base field's index columns (v: int32_t or int64_t, the kernel's T)
  const Slot* slots; uint64_t nslots;
  bmx_delta_rec* recs;                          // the staging slab: room for cap records
  UpdCounts* counts; unsigned long long* ctr;
  uint64_t cap, n, layout;
  int64_t ts;
  UpdSrc S;
  uint32_t target;
};

// `tot` writable nodes at rows base + loc[q], q = 0 .. tot - 1, whose ranks in the whole batch are running + q (loc[] complete and visible to the workgroup)
template <class T>
__device__ __forceinline__ void upd_emit_block(const UpdArgs& A, const uint16_t* loc, uint32_t tot, uint64_t base, uint64_t running) {
  if (running <= A.cap && A.cap - running < tot && threadIdx.x == 0) A.counts->next_pos = base + loc[A.cap - running];   // the first writable node that is not sent
  if (running >= A.cap) return;
  const uint32_t m = (uint32_t)(A.cap - running < tot ? A.cap - running : tot);
  const T* v = reinterpret_cast<const T*>(A.v);
  uint4* out = reinterpret_cast<uint4*>(A.recs + running);
  for (uint32_t q = threadIdx.x; q < m; q += SEL_THREADS) {
    const uint64_t pos = base + loc[q];
    const uint64_t id = A.ids[pos];
    int64_t y = A.S.operand;
    if (A.S.kind != UPD_SRC_NONE) (void)upd_value<T>(A.S, v, A.ids, A.slots, A.nslots, pos, y);     // (uniform) writable: pass 1 saw the same table
    out[2u * q] = make_uint4((uint32_t)id, (uint32_t)(id >> 32), A.target, 0u);
    out[2u * q + 1u] = make_uint4((uint32_t)(uint64_t)A.ts, (uint32_t)((uint64_t)A.ts >> 32), (uint32_t)(uint64_t)y, (uint32_t)((uint64_t)y >> 32));
  }
}

// SUB consecutive 8192-row blocks per workgroup, as k_rows_emit has them
template <class T, int SUB>
__global__ __launch_bounds__(SEL_THREADS) void k_upd_emit(const uint32_t* __restrict__ mask_words, const uint32_t* __restrict__ counts, uint32_t nblocks, UpdArgs A) {
  __shared__ uint32_t wsum[4];
  __shared__ uint16_t loc[SCAN_BLOCK_ELEMS];        // block-local row offsets of the writable nodes, in rank order
  const uint32_t b0 = blockIdx.x * (uint32_t)SUB;
  const bool last = blockIdx.x == gridDim.x - 1;
  uint32_t offset;
  {
    uint32_t part = strided_partial_sum(counts, b0);
    block_excl_scan(part, offset, wsum);
  }
  if ((uint64_t)offset > A.cap && !last) return;
  uint64_t running = offset;
  bool done = false;
  if (SUB > 1) {
    uint32_t mk[SUB];
    uint32_t cnt = 0;
#pragma unroll
    for (int q = 0; q < SUB; q++) {
      const uint64_t w = (uint64_t)b0 * SEL_THREADS + (uint64_t)threadIdx.x * SUB + q;
      mk[q] = (w << 5) < A.n ? mask_words[w] : 0u;
      cnt += __popc(mk[q]);
    }
    uint32_t tot;
    uint32_t r = block_excl_scan(cnt, tot, wsum);
    if (tot <= SCAN_BLOCK_ELEMS) {
#pragma unroll
      for (int q = 0; q < SUB; q++) {
        uint32_t m = mk[q];
        while (m) { const int e = __ffs((int)m) - 1; m &= m - 1; loc[r++] = (uint16_t)((threadIdx.x * SUB + q) * 32u + (uint32_t)e); }
      }
      __syncthreads();
      upd_emit_block<T>(A, loc, tot, (uint64_t)b0 * SCAN_BLOCK_ELEMS, running);
      running += tot;
      done = true;
    }
  }
  if (!done) {
#pragma unroll 1
    for (uint32_t k = 0; k < (uint32_t)SUB; k++) {
      const uint32_t blk = b0 + k;
      if (blk >= nblocks) break;
      const uint64_t w = (uint64_t)blk * SEL_THREADS + threadIdx.x;
      uint32_t mk = (w << 5) < A.n ? mask_words[w] : 0u;
      uint32_t tot;
      uint32_t r = block_excl_scan((uint32_t)__popc(mk), tot, wsum);
      while (mk) { const int e = __ffs((int)mk) - 1; mk &= mk - 1; loc[r++] = (uint16_t)(threadIdx.x * 32u + (uint32_t)e); }
      __syncthreads();
      upd_emit_block<T>(A, loc, tot, (uint64_t)blk * SCAN_BLOCK_ELEMS, running);
      running += tot;
      __syncthreads();
    }
  }
  if (last && threadIdx.x < 64u) {                  // (one whole wave) pass 1 is complete: its counters are final, and only this wave touches them now
    static_assert(UPD_CTR_SHARDS == 64u, "one shard per lane");
    unsigned long long* c = A.ctr + (size_t)threadIdx.x * UPD_CTR_STRIDE;
    unsigned long long nosrc = c[0], range = c[1];
    if (nosrc) c[0] = 0ull;
    if (range) c[1] = 0ull;
    for (int d = 32; d >= 1; d >>= 1) { nosrc += __shfl_xor(nosrc, d); range += __shfl_xor(range, d); }
    if (threadIdx.x == 0) {
      A.counts->n_writable = running; A.counts->n_sent = running < A.cap ? running : A.cap; A.counts->n_nosrc = nosrc; A.counts->n_range = range; A.counts->layout = A.layout;
      if (running <= A.cap) A.counts->next_pos = A.n;
    }
  }
}

constexpr int UPD_FIN_THREADS = 256;
// merged != 0: behind the merge of counts->n_sent records, which wrote applied_idx, n_applied and stats; merged == 0: nothing was sent, *row_count is the table's
__global__ __launch_bounds__(UPD_FIN_THREADS) void k_upd_finish(const bmx_delta_rec* __restrict__ recs, const uint32_t* __restrict__ applied_idx, const unsigned long long* __restrict__ n_applied,
                                                               const bmx_merge_stats* __restrict__ stats, const UpdCounts* __restrict__ counts,
                                                               const unsigned long long* __restrict__ row_count, uint64_t* __restrict__ out_ids, bmx_upd_res* __restrict__ res, uint32_t merged) {
  const uint64_t na = merged ? *n_applied : 0ull;
  if (out_ids)
    for (uint64_t k = (uint64_t)blockIdx.x * UPD_FIN_THREADS + threadIdx.x; k < na; k += (uint64_t)gridDim.x * UPD_FIN_THREADS)
      out_ids[k] = recs[applied_idx[k] & BMX_APPLIED_INDEX].id;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    res->n_match = counts->n_writable + counts->n_nosrc + counts->n_range; res->n_nosrc = counts->n_nosrc; res->n_range = counts->n_range;
    res->n_sent = counts->n_sent; res->n_applied = na; res->n_rows = merged ? stats->n_rows : *row_count;
    res->next_pos = counts->next_pos; res->layout = counts->layout; res->next_shard = 0u; res->reserved = 0u;
  }
}

}  // namespace bmx
