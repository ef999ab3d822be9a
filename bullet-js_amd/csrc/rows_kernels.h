// rows_kernels.h — row projection (bmx_rows.h bmx_where_rows): the ids of the nodes a boolean filter selects and, per requested field, a column of values (and
// clocks), gfx950, wave64.
//
// Pass 1 is select.h's k_scan_mask<PredRowsFrom<T>, true>: where_kernels.h's PredWhere behind a cursor. A lane whose 16 bytes lie wholly in front of the cursor
// loads nothing; a position in front of it enters the walk as "no candidate" and never probes. Every mask word and every block count is still written, as zero.
//
// Pass 2, k_rows_emit, ranks like k_scan_emit — the counts of the blocks in front (left by pass 1) summed by the workgroup itself, one mask word per thread,
// block_excl_scan, the loc[] transpose through LDS that puts consecutive lanes on consecutive ranks — and writes, for the ranks below cap, the id and the cells.
// The cells are written FIELD-OUTER: a loop over the requested fields whose counter is the same in every lane of the workgroup (the field hash comes out of the
// kernel arguments through a scalar load; no per-lane array is indexed by the field number, which would live in scratch), and inside it the lanes stride over
// the block's matches, so a lane has one probe in flight per field and match, the probes of one field are independent of each other, and consecutive lanes
// store to consecutive addresses of out_val[f * cap + rank]. The id of a match is re-read from the id column in every field's round: the block's part of that
// column is 64 KB that this workgroup has just read, so the re-read comes from L2, and LDS stays at the 16 KB of loc[] (keeping 8192 ids there would take
// 64 KB more and halve the workgroups a CU holds; DESIGN.md "Row projection").
//
// The lane that meets the match of rank cap writes next_pos; the last workgroup writes n_match, n_out, layout, and next_pos when nothing was cut off (total <=
// cap: then no match has rank cap, so the two writers exclude each other).
#pragma once
#include "where_kernels.h"
#include "../../include/bmx_rows.h"

namespace bmx {

constexpr uint32_t ROWS_MAX_FIELDS = BMX_ROWS_MAX_FIELDS;

template <class T, bool CLOCKS>
struct PredRowsFrom {   // PredWhere over the positions from `start` on
  static constexpr int E = PredWhere<T>::E;
  PredWhere<T, true, CLOCKS> P; uint64_t start;
  __device__ uint32_t mask(uint64_t first, uint64_t n) const {
    if (first + E <= start) return 0u;
    return P.mask_from(first, n, start);
  }
};

struct RowsArgs {
  const uint64_t* ids; const void* v;           // the base field's index columns (v: int32_t or int64_t, the kernel's T)
  const Slot* slots; uint64_t nslots;
  uint64_t* out_ids; int64_t* out_val; int64_t* out_ts; bmx_rows_res* res;
  uint64_t cap, n, layout;
  uint32_t nfields, base_field, with_ts, nt;    // nt: the output is larger than the Infinity Cache: nontemporal stores
  uint32_t field[ROWS_MAX_FIELDS];
};

template <class V>
__device__ __forceinline__ void rows_put(V* p, V x, bool nt) { if (nt) __builtin_nontemporal_store(x, p); else *p = x; }

// `tot` matches at rows base + loc[q], q = 0 .. tot - 1, whose ranks in the whole answer are running + q (loc[] complete and visible to the workgroup)
template <class T>
__device__ __forceinline__ void rows_emit_block(const RowsArgs& A, const uint16_t* loc, uint32_t tot, uint64_t base, uint64_t running) {
  if (running <= A.cap && A.cap - running < tot && threadIdx.x == 0) A.res->next_pos = base + loc[A.cap - running];   // the first match that is not delivered
  if (running >= A.cap) return;
  const uint32_t m = (uint32_t)(A.cap - running < tot ? A.cap - running : tot);
  const bool nt = A.nt != 0u;
  for (uint32_t q = threadIdx.x; q < m; q += SEL_THREADS) rows_put<unsigned long long>(reinterpret_cast<unsigned long long*>(A.out_ids + running + q), A.ids[base + loc[q]], nt);
  for (uint32_t f = 0; f < A.nfields; f++) {                       // (uniform over the workgroup)
    const uint32_t fh = A.field[f];
    int64_t* val = A.out_val + (uint64_t)f * A.cap + running;
    if (fh == A.base_field && !A.with_ts) {                         // the column value of a selected row: it holds data
      const T* v = reinterpret_cast<const T*>(A.v);
      for (uint32_t q = threadIdx.x; q < m; q += SEL_THREADS) rows_put<long long>(reinterpret_cast<long long*>(val + q), (long long)v[base + loc[q]], nt);
      continue;
    }
    int64_t* ts = A.out_ts + (uint64_t)f * A.cap + running;
    for (uint32_t q = threadIdx.x; q < m; q += SEL_THREADS) {
      const uint64_t id = A.ids[base + loc[q]];
      int64_t x = VAL_DELETED, t = BMX_ROWS_NO_CLOCK;               // what an absent row delivers
      agg_probe_ts(A.slots, A.nslots, id, fh, x, t);
      rows_put<long long>(reinterpret_cast<long long*>(val + q), (long long)x, nt);
      if (A.with_ts) rows_put<long long>(reinterpret_cast<long long*>(ts + q), (long long)t, nt);
    }
  }
}

// SUB consecutive 8192-row blocks per workgroup, as k_scan_emit has them: SUB = 1 up to SCAN_SUB8_BLOCKS blocks, SUB = 8 beyond.
template <class T, int SUB>
__global__ __launch_bounds__(SEL_THREADS) void k_rows_emit(const uint32_t* __restrict__ mask_words, const uint32_t* __restrict__ counts, uint32_t nblocks, RowsArgs A) {
  __shared__ uint32_t wsum[4];
  __shared__ uint16_t loc[SCAN_BLOCK_ELEMS];        // block-local row offsets of the matches, in rank order
  const uint32_t b0 = blockIdx.x * (uint32_t)SUB;
  const bool last = blockIdx.x == gridDim.x - 1;
  uint32_t offset;
  {
    uint32_t part = strided_partial_sum(counts, b0);
    block_excl_scan(part, offset, wsum);
  }
  // everything this workgroup holds lies behind rank cap, and the match of rank cap is some earlier workgroup's: nothing to write (the last one still reports the total)
  if ((uint64_t)offset > A.cap && !last) return;
  uint64_t running = offset;
  bool done = false;
  if (SUB > 1) {
    // at most 8192 matches in the SUB blocks: a thread owns SUB consecutive mask words and ONE block scan ranks them all (k_scan_emit's fast path)
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
      rows_emit_block<T>(A, loc, tot, (uint64_t)b0 * SCAN_BLOCK_ELEMS, running);
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
      rows_emit_block<T>(A, loc, tot, (uint64_t)blk * SCAN_BLOCK_ELEMS, running);
      running += tot;
      __syncthreads();
    }
  }
  if (last && threadIdx.x == 0) {
    A.res->n_match = running; A.res->n_out = running < A.cap ? running : A.cap; A.res->layout = A.layout; A.res->next_shard = 0; A.res->reserved = 0;
    if (running <= A.cap) A.res->next_pos = A.n;
  }
}

}  // namespace bmx
