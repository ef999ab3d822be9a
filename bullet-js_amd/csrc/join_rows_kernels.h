// join_rows_kernels.h — join projection (bmx_join_rows.h bmx_where_join_rows, bmx_where_map_rows): a map key -> inner NODE built on the device by one program,
// and the rows of a second program's selection delivered with fields of both nodes, gfx950, wave64.
//
// The map is join_kernels.h's (JoinPair, JoinState, join_insert, join_find, the context's JoinScratch) with the node id as the carried word: jrows_word(id) =
// (long long)(id ^ 2^63) keeps the UNSIGNED order of the ids under join_insert's signed atomicMin and maps the reserved id (BMX_JROWS_NO_NODE, which no row
// holds) onto JOIN_NO_ATTR, the word an unlowered slot carries. A key is only ever inserted together with an id, so once the build is complete every key's word
// is an id. k_jrows_finish leaves map and state record exactly as k_join_clear does: bmx_where_join_group and these calls interleave on one context.
//
// k_jrows_build<T>      : k_join_build's shape (top_sweep, PredWhere::row() called by every lane for all E rows of a unit). A selected inner row's key is the
//                         column value when key_field is the inner base field, otherwise one agg_probe, made after the match is known; the carried word comes
//                         from the id column. Selected rows and keyed rows are counted in the lane and leave the workgroup as one atomic each.
// k_jrows_insert        : the same insert from a list of (key, node id) pairs. A key outside +-VAL_MAX or the reserved id is skipped and not counted (ids do not
//                         obey the value domain, which is why k_join_insert cannot serve).
// PredJRowsFrom<T>      : the inner join's mask pass, for select.h's k_scan_mask: PredRowsFrom<T>'s walk over the lane's E rows first; then, for each row the
//                         outer program selected, the link value (the column, or one agg_probe) and a read-only walk of the map. The lanes loop over their own
//                         matched rows, no wave vote is involved. The map is complete before this pass by stream order alone. With the overflow state set every
//                         mask is 0. (The left join's mask pass is k_scan_mask<PredRowsFrom<T>, true> unchanged.)
// k_jrows_emit<T, SUB>  : k_rows_emit's ranking, and per block rows_emit_block for the outer columns followed by jrows_emit_inner: one round that resolves the
//                         inner id of every delivered row (the link read, one 16-byte map load per walk step) and writes out_in_ids, then FIELD-OUTER rounds with
//                         a workgroup-uniform counter that get the id back from out_in_ids[rank] — written by the same thread in round 0, so no second map walk
//                         and no per-lane array indexed by the field number — and make one agg_probe_ts keyed by the INNER id. Consecutive lanes sit on
//                         consecutive ranks; stores are nontemporal when the output exceeds the Infinity Cache. The joined rows are counted in the lane and leave
//                         the workgroup as one atomic (JoinState::nout, free here: k_join_export is not part of these calls' delivery). With the overflow state
//                         set nothing is ranked or written but the record's first four words (zero rows, next_pos = index size).
// k_jrows_finish        : the map back to empty; the workgroup that finishes last completes `res` (n_joined, the map's counts, flags) and puts the state record
//                         back. rows == 0 (the sharded form's phase 1, after k_join_export): the whole record, with no rows.
//
// No lane waits on a word another lane must write; every loop is bounded by `slots` (the walks), by the field count or by the block.
#pragma once
#include "join_kernels.h"
#include "rows_kernels.h"
#include "../../include/bmx_join_rows.h"

namespace bmx {

static_assert(sizeof(bmx_jrows_res) == 72, "the record of bmx_join_rows.h");
static_assert(sizeof(bmx_jrows_res) <= sizeof(bmx_join_res), "a host-mode answer's record comes down through JoinScratch::stage_res");
constexpr unsigned long long JROWS_BIAS = 1ull << 63;
__host__ __device__ inline long long jrows_word(unsigned long long id) { return (long long)(id ^ JROWS_BIAS); }
__host__ __device__ inline unsigned long long jrows_id(long long w) { return (unsigned long long)w ^ JROWS_BIAS; }
static_assert((unsigned long long)JOIN_NO_ATTR == (BMX_JROWS_NO_NODE ^ JROWS_BIAS), "the reserved id is the word of a slot without attribute");

// key_src: 0 = the inner base field's column, AGG_SRC_PROBE = one probe of key_field
template <class T, bool CLOCKS>
__global__ __launch_bounds__(AGG_THREADS) void k_jrows_build(uint64_t n, PredWhere<T, true, CLOCKS> P, JoinArgs A, uint32_t key_field, uint32_t key_src) {
  __shared__ unsigned long long s_n[TOP_WAVES], s_k[TOP_WAVES];
  unsigned long long cnt_l = 0, key_l = 0;
  where_sweep<T>(n, P, [&](int, T xe, uint64_t pos, bool sel) {
    if (!sel) return;
    cnt_l++;
    int64_t key = (int64_t)xe;
    if (!where_field(P, pos, key_src, key_field, key)) return;
    key_l++;
    join_insert(A, (long long)key, jrows_word(P.ids[pos]));
  });
  semi_count_end(cnt_l, s_n, TOP_WAVES, &A.S->n_inner);
  semi_count_end(key_l, s_k, TOP_WAVES, &A.S->n_keyed);
}

__global__ __launch_bounds__(JOIN_THREADS) void k_jrows_insert(const long long* __restrict__ keys, const unsigned long long* __restrict__ ids, uint64_t n, JoinArgs A) {
  __shared__ unsigned long long s_n[JOIN_THREADS / 64], s_k[JOIN_THREADS / 64];
  unsigned long long cnt_l = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * JOIN_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * JOIN_THREADS) {
    const long long k = keys[i];
    const unsigned long long id = ids[i];
    if (k < -VAL_MAX || k > VAL_MAX || id == BMX_JROWS_NO_NODE) continue;
    cnt_l++;
    join_insert(A, k, jrows_word(id));
  }
  semi_count_end(cnt_l, s_n, JOIN_THREADS / 64, &A.S->n_inner);
  semi_count_end(cnt_l, s_k, JOIN_THREADS / 64, &A.S->n_keyed);
}

// what the mask pass and the emit pass need of the map and the link
struct JRowsLink {
  const JoinPair* map; const JoinState* S;
  uint64_t mslots, mcap;
  uint32_t link, link_src;                        // link_src: 0 = the outer base field's column, AGG_SRC_PROBE = one probe of `link`
};

// the word the link value of the selected row at `pos` maps to; JOIN_NO_ATTR: no inner node
template <class T>
__device__ __forceinline__ long long jrows_resolve(const JRowsLink& L, const T* __restrict__ v, const uint64_t* __restrict__ ids, const Slot* __restrict__ slots, uint64_t nslots, uint64_t pos) {
  int64_t y = VAL_DELETED;
  bool have;
  if (L.link_src == 0u) { y = (int64_t)v[pos]; have = true; }           // a selected row holds data (not where_field: the column value is not at hand)
  else have = agg_probe(slots, nslots, ids[pos], L.link, y) && y != VAL_DELETED;
  long long w = JOIN_NO_ATTR;
  if (!have || !join_find(L.map, L.mslots, (long long)y, w)) w = JOIN_NO_ATTR;
  return w;
}

template <class T, bool CLOCKS>
struct PredJRowsFrom {   // the outer program behind a cursor AND (link value is a key of the map)
  static constexpr int E = PredWhere<T>::E;
  PredRowsFrom<T, CLOCKS> R;
  JRowsLink L;
  __device__ uint32_t mask(uint64_t first, uint64_t n) const {
    if (!join_map_fits(L.S, L.mcap)) return 0u;                         // (uniform)
    uint32_t out = 0;
    for (uint32_t m = R.mask(first, n); m; m &= m - 1u) {                // this lane's rows that the outer program selected
      const uint32_t e = (uint32_t)__ffs((int)m) - 1u;
      if (jrows_resolve<T>(L, R.P.v, R.P.ids, R.P.slots, R.P.nslots, first + e) != JOIN_NO_ATTR) out |= 1u << e;
    }
    return out;
  }
};

struct JRowsArgs {
  RowsArgs R;                                     // the outer side, as k_rows_emit takes it (R.res: the first four words of the bmx_jrows_res)
  JRowsLink L;
  uint64_t* out_in_ids; int64_t* out_in_val; int64_t* out_in_ts;
  unsigned long long* n_joined;                   // JoinState::nout
  uint32_t n_in_fields;
  uint32_t in_field[ROWS_MAX_FIELDS];
};

// behind rows_emit_block, for the same `tot` matches: the inner id and the inner cells of the ranks below cap
template <class T>
__device__ __forceinline__ void jrows_emit_inner(const JRowsArgs& A, const uint16_t* loc, uint32_t tot, uint64_t base, uint64_t running, unsigned long long& joined_l) {
  const RowsArgs& R = A.R;
  if (running >= R.cap) return;
  const uint32_t m = (uint32_t)(R.cap - running < tot ? R.cap - running : tot);
  const bool nt = R.nt != 0u;
  unsigned long long* iid = reinterpret_cast<unsigned long long*>(A.out_in_ids + running);
  const T* v = reinterpret_cast<const T*>(R.v);
  for (uint32_t q = threadIdx.x; q < m; q += SEL_THREADS) {
    const long long w = jrows_resolve<T>(A.L, v, R.ids, R.slots, R.nslots, base + loc[q]);
    joined_l += w != JOIN_NO_ATTR ? 1ull : 0ull;
    rows_put<unsigned long long>(iid + q, jrows_id(w), nt);              // (JOIN_NO_ATTR comes out as BMX_JROWS_NO_NODE)
  }
  for (uint32_t g = 0; g < A.n_in_fields; g++) {                         // (uniform over the workgroup)
    const uint32_t fh = A.in_field[g];
    int64_t* val = A.out_in_val + (uint64_t)g * R.cap + running;
    int64_t* ts = A.out_in_ts + (uint64_t)g * R.cap + running;
    for (uint32_t q = threadIdx.x; q < m; q += SEL_THREADS) {
      const unsigned long long id = iid[q];                              // this thread's own store of the round above
      int64_t x = VAL_DELETED, t = BMX_ROWS_NO_CLOCK;                    // what an absent row, and a row without inner node, delivers
      if (id != BMX_JROWS_NO_NODE) agg_probe_ts(R.slots, R.nslots, id, fh, x, t);
      rows_put<long long>(reinterpret_cast<long long*>(val + q), (long long)x, nt);
      if (R.with_ts) rows_put<long long>(reinterpret_cast<long long*>(ts + q), (long long)t, nt);
    }
  }
}

// SUB consecutive 8192-row blocks per workgroup, as k_rows_emit has them
template <class T, int SUB>
__global__ __launch_bounds__(SEL_THREADS) void k_jrows_emit(const uint32_t* __restrict__ mask_words, const uint32_t* __restrict__ counts, uint32_t nblocks, JRowsArgs A) {
  __shared__ uint32_t wsum[4];
  __shared__ unsigned long long s_j[SEL_THREADS / 64];
  __shared__ uint16_t loc[SCAN_BLOCK_ELEMS];        // block-local row offsets of the matches, in rank order
  const RowsArgs& R = A.R;
  const uint32_t b0 = blockIdx.x * (uint32_t)SUB;
  const bool last = blockIdx.x == gridDim.x - 1;
  if (!join_map_fits(A.L.S, A.L.mcap)) {            // (uniform: the build is complete) no row is delivered
    if (last && threadIdx.x == 0) { R.res->n_match = 0; R.res->n_out = 0; R.res->next_pos = R.n; R.res->layout = R.layout; }
    return;
  }
  uint32_t offset;
  {
    uint32_t part = strided_partial_sum(counts, b0);
    block_excl_scan(part, offset, wsum);
  }
  if ((uint64_t)offset > R.cap && !last) return;
  uint64_t running = offset;
  unsigned long long joined_l = 0;
  bool done = false;
  if (SUB > 1) {
    uint32_t mk[SUB];
    uint32_t cnt = 0;
#pragma unroll
    for (int q = 0; q < SUB; q++) {
      const uint64_t w = (uint64_t)b0 * SEL_THREADS + (uint64_t)threadIdx.x * SUB + q;
      mk[q] = (w << 5) < R.n ? mask_words[w] : 0u;
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
      rows_emit_block<T>(R, loc, tot, (uint64_t)b0 * SCAN_BLOCK_ELEMS, running);
      jrows_emit_inner<T>(A, loc, tot, (uint64_t)b0 * SCAN_BLOCK_ELEMS, running, joined_l);
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
      uint32_t mk = (w << 5) < R.n ? mask_words[w] : 0u;
      uint32_t tot;
      uint32_t r = block_excl_scan((uint32_t)__popc(mk), tot, wsum);
      while (mk) { const int e = __ffs((int)mk) - 1; mk &= mk - 1; loc[r++] = (uint16_t)(threadIdx.x * 32u + (uint32_t)e); }
      __syncthreads();
      rows_emit_block<T>(R, loc, tot, (uint64_t)blk * SCAN_BLOCK_ELEMS, running);
      jrows_emit_inner<T>(A, loc, tot, (uint64_t)blk * SCAN_BLOCK_ELEMS, running, joined_l);
      running += tot;
      __syncthreads();
    }
  }
  semi_count_end(joined_l, s_j, SEL_THREADS / 64, A.n_joined);
  if (last && threadIdx.x == 0) {
    R.res->n_match = running; R.res->n_out = running < R.cap ? running : R.cap; R.res->layout = R.layout;
    if (running <= R.cap) R.res->next_pos = R.n;
  }
}

// rows != 0: behind k_jrows_emit, which wrote n_match, n_out, next_pos and layout; rows == 0: no rows were asked for (the sharded form's phase 1)
__global__ __launch_bounds__(JOIN_THREADS) void k_jrows_finish(JoinArgs J, bmx_jrows_res* __restrict__ res, uint32_t rows) {
  JoinState* M = J.S;
  for (uint64_t s = (uint64_t)blockIdx.x * JOIN_THREADS + threadIdx.x; s < J.slots; s += (uint64_t)gridDim.x * JOIN_THREADS)
    if (J.map[s].key != JOIN_EMPTY) { JoinPair e; e.key = JOIN_EMPTY; e.val = JOIN_NO_ATTR; J.map[s] = e; }
  if (last_workgroup(&M->done) && threadIdx.x == 0) {                   // only this thread reads the state record in this kernel
    const bool mfits = join_map_fits(M, J.cap);
    if (!rows) { res->n_match = 0ull; res->n_out = 0ull; res->next_pos = 0ull; res->layout = 0ull; }
    res->n_joined = rows && mfits ? M->nout : 0ull;
    res->map_size = M->claims; res->n_inner = M->n_inner; res->n_keyed = M->n_keyed;
    res->flags = mfits ? 0u : BMX_JOIN_MAP_OVERFLOW; res->next_shard = 0u;
    join_state_reset(M);                                                // (`unmatched` was empty already: as k_join_clear leaves the record)
  }
}

}  // namespace bmx
