// reach_kernels.h — graph traversal (bmx_reach.h bmx_where_reach, bmx_where_reach_from): a level-synchronous breadth-first closure over the edges
// link_field -> key_field of the nodes one program selects, gfx950, wave64.
//
// The map is the lookup joins' (join_kernels.h: 16-byte {key, val} pairs, home slot and walk as there); `val` is the LEVEL of the value. The per-position
// scratch (ReachScratch) is one 8-byte link word and one depth byte per position of the base field's index.
//
// k_reach_seed<T>    : k_semi_build's shape. The seed program's selection inserts (value of the seed field, 0); the selected nodes are counted into n_seed.
// k_reach_list       : k_join_insert's shape. A list of values inserted at a given level: the list form's seeds (level 0, counted into n_seed), and every
//                      level's union in the sharded forms (not counted). A value outside +-VAL_MAX is skipped.
// k_reach_prepare<T> : ONE sweep of the base column (top_sweep, PredWhere::row() called by every lane for all E rows of a unit). A selected node's link is the
//                      column value or one agg_probe; link[pos] = the link, or REACH_NO_LINK = INT64_MIN for a position that is no edge node; depth[pos] = 0.
//                      The edge nodes are counted in the lane, reduced per workgroup and added to n_edges with one atomic. After it no round evaluates the program
//                      or probes a link again.
// k_reach_round<T>   : round r. Sweeps link[] and depth[] — 9 bytes per position: per lane one 16-byte load of two link words and one 2-byte load of their depth
//                      bytes, REACH_U of each in flight. A position with depth == 0 and a link makes ONE walk of the map with plain 16-byte loads and is reached
//                      iff the link is found with val <= r - 1. A reached position gets depth[pos] = r, fetches its key (the column, or one agg_probe: once per
//                      node in the whole call, since a reached node is never looked at again) and calls reach_insert(key, r). The workgroup raises `rounds` with
//                      one atomic. The kernel returns at once, on a uniform branch, when the overflow state is set or new_keys[r - 1] == 0: all max_depth rounds
//                      are enqueued blind, and the empty ones cost a launch each.
// PredReach          : the predicate of the answer's mask pass for select.h's k_scan_mask: depth[pos] != 0, sixteen depth bytes per lane and load; every mask
//                      is 0 with the overflow state set.
// k_reach_emit<SUB>  : ranks like k_rows_emit (the counts of the blocks in front summed by the workgroup itself, block_excl_scan, the loc[] transpose through
//                      LDS) and writes id and depth for the ranks below cap; the last workgroup leaves the total in the state record.
// k_reach_export     : the keys of one level compacted into a list by wave ballot + popcount (the sharded forms, after every round).
// k_reach_finish     : the map back to empty; the workgroup that finishes last writes `res` and puts both state records back.
//
// reach_insert is join_insert's two steps (join_slot, join_lower), with one addition: a successful claim made at level r adds one to new_keys[r] with a no-return
// atomic. A value is claimed in the round that first meets it, and every insert of round r carries r, so new_keys[r] is the number of values of level r: it
// drives the early-out of round r + 1, and new_keys[max_depth] != 0 is BMX_REACH_MORE.
//
// Why the round's lookups may be plain loads. A pair with val <= r - 1 was complete when the previous kernel ended, and the kernel boundary made it visible to
// every XCD. Linear probing never moves a key, so every slot on the walk to such a pair was occupied before round r began: the walk cannot end early on a slot
// that round r fills. Whatever round r itself writes carries val == r or JOIN_NO_ATTR ("none", between the claim and the minimum), and both fail the test
// val <= r - 1. So a stale or torn view of this round's writes cannot change an answer. No lane waits on a word another wave must write; every loop is bounded
// by `slots`.
#pragma once
#include "join_kernels.h"
#include "rows_kernels.h"
#include "../../include/bmx_reach.h"

namespace bmx {

constexpr long long REACH_NO_LINK = INT64_MIN;    // link[pos] of a position that is no edge node
static_assert(REACH_NO_LINK == VAL_DELETED && REACH_NO_LINK == JOIN_EMPTY, "the one value no row holds");
static_assert(sizeof(bmx_reach_res) == 40, "the record of bmx_reach.h");
constexpr uint32_t REACH_LEVELS = BMX_REACH_MAX_DEPTH + 1u;   // levels 0..255
constexpr int REACH_THREADS = 256;                // the round kernel
constexpr int REACH_U = 4;                        // loads of each array a lane of the round kernel has in flight
static_assert(REACH_LEVELS == (uint32_t)JOIN_THREADS, "k_reach_finish's last workgroup zeroes one level counter per thread");

// the state record of one traversal, in device memory; k_reach_finish leaves it all zero
struct ReachState {
  unsigned long long n_seed, n_edges;             // bmx_reach_res's
  unsigned long long n_match;                     // k_reach_emit's total
  unsigned long long nout;                        // k_reach_export's rank counter
  uint32_t rounds;                                // the largest round that reached a node
  uint32_t pad;
  uint32_t new_keys[REACH_LEVELS];                // values claimed at each level
};

struct ReachArgs {
  long long* link; uint8_t* depth;                // per position of the base field's index
  ReachState* S;
};

__device__ __forceinline__ void reach_insert(const JoinArgs& A, ReachState* R, long long key, uint32_t level) {
  uint64_t s; bool claimed;
  if (!join_slot(A, key, s, claimed)) return;
  if (claimed) atomicAdd(&R->new_keys[level], 1u);
  join_lower(A, s, (long long)level);
}

// is `key` in the map with a level <= max_level? One walk, plain 16-byte loads (the header comment: why that is exact while the round inserts).
__device__ __forceinline__ bool reach_has(const JoinPair* __restrict__ map, uint64_t slots, long long key, long long max_level) {
  const uint64_t mask = slots - 1u;
  uint64_t s = group_mix(key) & mask;
  for (uint64_t p = 0; p < slots; ++p, s = (s + 1u) & mask) {
    const join_ll2 kv = *reinterpret_cast<const join_ll2*>(map + s);
    if (kv.x == key) return kv.y <= max_level;
    if (kv.x == JOIN_EMPTY) return false;
  }
  return false;
}

// seed_src: 0 = the seed base field's column, AGG_SRC_PROBE = one probe of seed_field
template <class T, bool CLOCKS>
__global__ __launch_bounds__(AGG_THREADS) void k_reach_seed(uint64_t n, PredWhere<T, true, CLOCKS> P, JoinArgs J, ReachState* R, uint32_t seed_field, uint32_t seed_src) {
  __shared__ unsigned long long s_n[TOP_WAVES];
  unsigned long long cnt_l = 0;
  where_sweep<T>(n, P, [&](int, T xe, uint64_t pos, bool sel) {
    if (!sel) return;
    cnt_l++;
    int64_t key = (int64_t)xe;
    if (where_field(P, pos, seed_src, seed_field, key)) reach_insert(J, R, (long long)key, 0u);
  });
  semi_count_end(cnt_l, s_n, TOP_WAVES, &R->n_seed);
}

// count != 0: the listed values inside the domain are counted into n_seed
__global__ __launch_bounds__(JOIN_THREADS) void k_reach_list(const long long* __restrict__ values, uint64_t n, JoinArgs J, ReachState* R, uint32_t level, uint32_t count) {
  __shared__ unsigned long long s_n[JOIN_THREADS / 64];
  unsigned long long cnt_l = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * JOIN_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * JOIN_THREADS) {
    const long long v = values[i];
    if (v < -VAL_MAX || v > VAL_MAX) continue;                           // no row holds it (INT64_MIN is the empty word)
    cnt_l += count ? 1ull : 0ull;
    reach_insert(J, R, v, level);
  }
  semi_count_end(cnt_l, s_n, JOIN_THREADS / 64, &R->n_seed);
}

// link_src: 0 = the base field's column, AGG_SRC_PROBE = one probe of link_field. Writes link[0, n) and depth[0, n).
template <class T, bool CLOCKS>
__global__ __launch_bounds__(AGG_THREADS) void k_reach_prepare(uint64_t n, PredWhere<T, true, CLOCKS> P, ReachArgs A, uint32_t link_field, uint32_t link_src) {
  constexpr int E = PredWhere<T>::E;
  typedef T vec_t __attribute__((ext_vector_type(E)));
  __shared__ unsigned long long s_n[TOP_WAVES];
  unsigned long long cnt_l = 0;
  top_sweep<T>(P.v, n, P.nt ? 1u : 0u, [&](uint64_t unit, const vec_t& x, uint32_t cnt) {
    where_unit_rows<T>(P, unit, x, cnt, [&](int e, T xe, uint64_t pos, bool sel) {
      if ((uint32_t)e >= cnt) return;                                     // (beyond the column: nothing to write)
      int64_t y = (int64_t)xe;
      const bool have = sel && where_field(P, pos, link_src, link_field, y);      // (a selected row holds data)
      cnt_l += have ? 1ull : 0ull;
      A.link[pos] = have ? (long long)y : REACH_NO_LINK;
      A.depth[pos] = (uint8_t)0;
    });
  });
  semi_count_end(cnt_l, s_n, TOP_WAVES, &A.S->n_edges);
}

struct ReachKey {   // where a reached node's key comes from. key_src: 0 = the base field's column `v`, AGG_SRC_PROBE = one probe of key_field
  const uint64_t* ids; const void* v; const Slot* slots; uint64_t nslots;
  uint32_t key_field, key_src;
};

template <class T>
__global__ __launch_bounds__(REACH_THREADS) void k_reach_round(uint64_t n, ReachArgs A, JoinArgs J, ReachKey K, uint32_t r) {
  __shared__ uint32_t s_any;
  ReachState* S = A.S;
  if (!join_map_fits(J.S, J.cap) || S->new_keys[r - 1u] == 0u) return;     // (uniform: both were final when the previous kernel ended)
  if (threadIdx.x == 0) s_any = 0u;
  __syncthreads();
  const long long below = (long long)r - 1;
  const T* col = reinterpret_cast<const T*>(K.v);
  bool any = false;
  const uint64_t nu = (n + 1u) / 2u;                                       // units of two positions
  for (uint64_t b = (uint64_t)blockIdx.x * (REACH_THREADS * REACH_U); b < nu; b += (uint64_t)gridDim.x * (REACH_THREADS * REACH_U)) {
    join_ll2 lk[REACH_U];
    uint32_t dp[REACH_U];
#pragma unroll
    for (int u = 0; u < REACH_U; u++) {
      const uint64_t i = b + (uint64_t)u * REACH_THREADS + threadIdx.x, p0 = 2u * i;
      lk[u].x = REACH_NO_LINK; lk[u].y = REACH_NO_LINK; dp[u] = 0u;
      if (p0 + 2u <= n) { lk[u] = *reinterpret_cast<const join_ll2*>(A.link + p0); dp[u] = *reinterpret_cast<const uint16_t*>(A.depth + p0); }
      else if (p0 < n) { lk[u].x = A.link[p0]; dp[u] = A.depth[p0]; }
    }
#pragma unroll
    for (int u = 0; u < REACH_U; u++) {
      const uint64_t p0 = 2u * (b + (uint64_t)u * REACH_THREADS + threadIdx.x);
#pragma unroll
      for (uint32_t k = 0; k < 2u; k++) {
        const long long l = k ? lk[u].y : lk[u].x;
        if (l == REACH_NO_LINK || ((dp[u] >> (8u * k)) & 255u) != 0u) continue;
        if (!reach_has(J.map, J.slots, l, below)) continue;
        const uint64_t pos = p0 + k;
        A.depth[pos] = (uint8_t)r;
        any = true;
        int64_t key = 0;
        bool have;
        if (K.key_src == 0u) { key = (int64_t)col[pos]; have = true; }    // an edge node's base row holds data (no PredWhere here: not where_field)
        else have = agg_probe(K.slots, K.nslots, K.ids[pos], K.key_field, key) && key != VAL_DELETED;
        if (have) reach_insert(J, S, (long long)key, r);
      }
    }
  }
  if (any) s_any = 1u;                                                     // (every writer stores the same word)
  __syncthreads();
  if (threadIdx.x == 0 && s_any) atomicMax(&S->rounds, r);
}

struct PredReach {   // depth[pos] != 0, for k_scan_mask; `depth` is 16-byte aligned and `first` a multiple of 16
  static constexpr int E = 16;
  const uint8_t* depth; const JoinState* M; uint64_t cap;
  __device__ uint32_t mask(uint64_t first, uint64_t n) const {
    if (!join_map_fits(M, cap)) return 0u;                                // (uniform) nothing is delivered
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    uint32_t m = 0;
    if (first + 16u <= n) {
      const u4 w = *reinterpret_cast<const u4*>(depth + first);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t x = q == 0 ? w.x : (q == 1 ? w.y : (q == 2 ? w.z : w.w));
#pragma unroll
        for (int b = 0; b < 4; b++) m |= ((x >> (8 * b)) & 255u) ? 1u << (4 * q + b) : 0u;
      }
    } else {
      for (uint32_t e = 0; e < 16u && first + e < n; e++) m |= depth[first + e] ? 1u << e : 0u;
    }
    return m;
  }
};

struct ReachEmit {
  const uint64_t* ids; const uint8_t* depth;
  uint64_t* out_ids; uint8_t* out_depth; ReachState* S;
  uint64_t cap, n;
};

// `tot` matches at positions base + loc[q], q = 0 .. tot - 1, whose ranks in the whole answer are running + q (loc[] complete and visible to the workgroup)
__device__ __forceinline__ void reach_emit_block(const ReachEmit& A, const uint16_t* loc, uint32_t tot, uint64_t base, uint64_t running) {
  if (running >= A.cap) return;
  const uint32_t m = (uint32_t)(A.cap - running < tot ? A.cap - running : tot);
  for (uint32_t q = threadIdx.x; q < m; q += SEL_THREADS) {
    const uint64_t pos = base + loc[q];
    A.out_ids[running + q] = A.ids[pos];
    A.out_depth[running + q] = A.depth[pos];
  }
}

// SUB consecutive 8192-position blocks per workgroup, as k_rows_emit has them
template <int SUB>
__global__ __launch_bounds__(SEL_THREADS) void k_reach_emit(const uint32_t* __restrict__ mask_words, const uint32_t* __restrict__ counts, uint32_t nblocks, ReachEmit A) {
  __shared__ uint32_t wsum[4];
  __shared__ uint16_t loc[SCAN_BLOCK_ELEMS];        // block-local offsets of the matches, in rank order
  const uint32_t b0 = blockIdx.x * (uint32_t)SUB;
  const bool last = blockIdx.x == gridDim.x - 1;
  uint32_t offset;
  {
    uint32_t part = strided_partial_sum(counts, b0);
    block_excl_scan(part, offset, wsum);
  }
  if ((uint64_t)offset >= A.cap && !last) return;   // everything this workgroup holds lies behind rank cap (the last one still reports the total)
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
      reach_emit_block(A, loc, tot, (uint64_t)b0 * SCAN_BLOCK_ELEMS, running);
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
      reach_emit_block(A, loc, tot, (uint64_t)blk * SCAN_BLOCK_ELEMS, running);
      running += tot;
      __syncthreads();
    }
  }
  if (last && threadIdx.x == 0) A.S->n_match = running;
}

// `slots` is a multiple of 64: a wave's 64 lanes are inside the table or beyond it together. Writes nothing when the map does not fit.
__global__ __launch_bounds__(JOIN_THREADS) void k_reach_export(JoinArgs J, ReachState* R, long long level, long long* __restrict__ out) {
  if (!join_map_fits(J.S, J.cap)) return;                                // (uniform)
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t b = (uint64_t)blockIdx.x * JOIN_THREADS + (threadIdx.x & ~63u); b < J.slots; b += (uint64_t)gridDim.x * JOIN_THREADS) {
    const join_ll2 kv = *reinterpret_cast<const join_ll2*>(J.map + b + lane);
    const bool occ = kv.x != JOIN_EMPTY && kv.y == level;
    if (!__ballot(occ)) continue;                                        // (uniform)
    const unsigned long long rk = wave_rank(occ, &R->nout, lane);
    if (occ && rk < J.cap) out[rk] = kv.x;
  }
}

__global__ __launch_bounds__(JOIN_THREADS) void k_reach_finish(JoinArgs J, ReachState* R, bmx_reach_res* __restrict__ res, uint32_t max_depth) {
  JoinState* M = J.S;
  for (uint64_t s = (uint64_t)blockIdx.x * JOIN_THREADS + threadIdx.x; s < J.slots; s += (uint64_t)gridDim.x * JOIN_THREADS)
    if (J.map[s].key != JOIN_EMPTY) { JoinPair e; e.key = JOIN_EMPTY; e.val = JOIN_NO_ATTR; J.map[s] = e; }
  if (!last_workgroup(&M->done)) return;                                // (uniform) no other workgroup reads the state records any more
  if (threadIdx.x == 0) {
    const bool fits = join_map_fits(M, J.cap);
    bmx_reach_res o;
    o.n_match = fits ? R->n_match : 0ull; o.set_size = M->claims; o.n_seed = R->n_seed; o.n_edges = R->n_edges;
    o.rounds = fits ? R->rounds : 0u;
    o.flags = fits ? (R->new_keys[max_depth] ? BMX_REACH_MORE : 0u) : BMX_REACH_OVERFLOW;
    *res = o;
    join_state_reset(M);
    R->n_seed = 0ull; R->n_edges = 0ull; R->n_match = 0ull; R->nout = 0ull; R->rounds = 0u; R->pad = 0u;
  }
  __syncthreads();                                                      // (thread 0 has read new_keys[max_depth])
  R->new_keys[threadIdx.x] = 0u;
}

}  // namespace bmx
