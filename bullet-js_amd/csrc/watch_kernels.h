// watch_kernels.h — standing queries (bmx_watch.h bmx_watch_poll): the match mask of a predicate compared with the mask the watch committed last, gfx950.
//
// A watch keeps `prev`, one bit per position of the base field's dense index: the committed set. One poll is
//   k_watch_mask<Pred>  one read of the value column -> the match word of 32 rows (as select.h k_scan_mask packs it), compared at once with the same word of `prev`:
//                       entered = cur & ~prev and left = prev & ~cur go into two scratch masks, and the block leaves three counts (entered, left, matches);
//   k_watch_totals      one workgroup sums the three count arrays into the poll's record and looks up whether the watch was committed under this layout;
//   k_scan_emit         (select.h, as it is) once per list: ids from a mask at ranks from the counts of an earlier launch, position order;
//   k_watch_commit      reads the totals and the caps; if both lists fit it folds the two masks into `prev`, otherwise it leaves `prev` alone; writes bmx_watch_res.
// No atomics and no scratch memory anywhere; LDS only for the block scans. Workgroups never talk to each other inside a launch: what k_watch_commit decides on
// (the totals, the RESET bit) was written by k_watch_totals, a launch earlier.
#pragma once
#include "where_kernels.h"
#include "../../include/bmx_watch.h"

namespace bmx {

// The poll's record between its launches: the shape of bmx_watch_res, flags = BMX_WATCH_RESET or 0 (k_watch_commit adds BMX_WATCH_OVERFLOW on the way out).
struct WatchTotals { unsigned long long n_entered, n_left, n_match; uint32_t flags, pad; };
static_assert(sizeof(WatchTotals) == sizeof(bmx_watch_res), "the totals record is copied out as a bmx_watch_res");

// One 8192-row block per workgroup, the geometry of k_scan_mask: thread t of tile k owns rows [base + (256 k + t) E, + E); the 32 / E lanes that share a mask word
// OR their bits together and the first of them owns the word. That lane loaded the word of `prev` in front of the column (a word of `prev` whose first row is behind
// n has never been written to and is not read). Words of the block behind n are written as zero, so the passes behind this one never look at n again.
// `masks` = the entered mask, and blocks_cap blocks of words further on the left mask; `counts` = blocks_cap entered, left and match counts each (two pointers and a
// stride instead of five pointers: the predicate's program already fills most of the scalar registers that eight waves per SIMD leave a wave).
template <class Pred>
__global__ __launch_bounds__(SEL_THREADS) void k_watch_mask(Pred P, uint64_t n, const uint32_t* __restrict__ prev, uint32_t* __restrict__ masks, uint32_t* __restrict__ counts,
                                                             uint32_t blocks_cap) {
  constexpr int E = Pred::E;
  constexpr int TILES = 32 / E;   // tiles of 256*E elements per block
  constexpr int LPW = 32 / E;     // lanes that share one 32-bit mask word
  __shared__ uint32_t wsum[4];
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_BLOCK_ELEMS;
  const bool owner = (threadIdx.x & (LPW - 1)) == 0;
  uint32_t pw[TILES];
#pragma unroll
  for (int k = 0; k < TILES; k++) {
    const uint64_t first = base + (uint64_t)k * SEL_THREADS * E + (uint64_t)threadIdx.x * E;      // (the owner's first row is the word's first row)
    pw[k] = (owner && first < n) ? prev[first >> 5] : 0u;
  }
  uint32_t m[TILES];
#pragma unroll
  for (int k = 0; k < TILES; k++) {
    const uint64_t first = base + (uint64_t)k * SEL_THREADS * E + (uint64_t)threadIdx.x * E;
    m[k] = first < n ? P.mask(first, n) : 0u;
  }
  uint32_t c_m = 0, c_e = 0, c_l = 0;
#pragma unroll
  for (int k = 0; k < TILES; k++) {
    c_m += __popc(m[k]);
    uint32_t v = m[k] << (E * (threadIdx.x & (LPW - 1)));
#pragma unroll
    for (int d = 1; d < LPW; d <<= 1) v |= __shfl_xor(v, d);
    if (owner) {
      const uint32_t e = v & ~pw[k], l = pw[k] & ~v;
      const uint64_t w = (base + (uint64_t)k * SEL_THREADS * E + (uint64_t)threadIdx.x * E) >> 5;
      masks[w] = e; masks[(uint64_t)blocks_cap * (SCAN_BLOCK_ELEMS / 32) + w] = l;
      c_e += __popc(e); c_l += __popc(l);
    }
  }
  uint32_t t_e, t_l, t_m;
  block_excl_scan(c_e, t_e, wsum);
  block_excl_scan(c_l, t_l, wsum);
  block_excl_scan(c_m, t_m, wsum);
  if (threadIdx.x == 0) { counts[blockIdx.x] = t_e; counts[blocks_cap + blockIdx.x] = t_l; counts[2 * blocks_cap + blockIdx.x] = t_m; }
}

// One workgroup: the three totals, and RESET if the watch's committed set does not belong to the index layout this poll swept (`committed`: the stamp of the layout
// the watch last committed under, 0 = never; only k_watch_commit writes it).
__global__ __launch_bounds__(SEL_THREADS) void k_watch_totals(const uint32_t* __restrict__ cnt_entered, const uint32_t* __restrict__ cnt_left, const uint32_t* __restrict__ cnt_match,
                                                               uint32_t nblocks, const unsigned long long* __restrict__ committed, unsigned long long layout, WatchTotals* __restrict__ tot) {
  __shared__ uint32_t wsum[4];
  uint32_t t_e, t_l, t_m;
  block_excl_scan(strided_partial_sum(cnt_entered, nblocks), t_e, wsum);
  block_excl_scan(strided_partial_sum(cnt_left, nblocks), t_l, wsum);
  block_excl_scan(strided_partial_sum(cnt_match, nblocks), t_m, wsum);
  if (threadIdx.x == 0) { tot->n_entered = t_e; tot->n_left = t_l; tot->n_match = t_m; tot->flags = *committed != layout ? BMX_WATCH_RESET : 0u; tot->pad = 0u; }
}

// The commit. Every workgroup reads the totals (written a launch earlier) and takes the same decision. If both lists fit: prev = (prev | entered) & ~left over the
// `nquads` 16-byte units of the masks (whole 8192-row blocks: k_watch_mask wrote every word of them), skipped when nothing changed; thread 0 of workgroup 0 stamps
// the watch with the layout. It also writes the caller's record: the totals, RESET as k_watch_totals found it, OVERFLOW if a list did not fit.
__global__ __launch_bounds__(256) void k_watch_commit(const uint4* __restrict__ entered, const uint4* __restrict__ left, uint4* __restrict__ prev, uint64_t nquads,
                                                       const WatchTotals* __restrict__ tot, uint64_t cap_entered, uint64_t cap_left,
                                                       unsigned long long* __restrict__ committed, unsigned long long layout, bmx_watch_res* __restrict__ res) {
  const unsigned long long n_e = tot->n_entered, n_l = tot->n_left;
  const bool fits = n_e <= cap_entered && n_l <= cap_left;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    res->n_entered = n_e; res->n_left = n_l; res->n_match = tot->n_match;
    res->flags = tot->flags | (fits ? 0u : BMX_WATCH_OVERFLOW); res->reserved = 0u;
    if (fits) *committed = layout;
  }
  if (!fits || (n_e | n_l) == 0) return;
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < nquads; q += (uint64_t)gridDim.x * 256u) {
    const uint4 e = entered[q], l = left[q];
    if ((e.x | e.y | e.z | e.w | l.x | l.y | l.z | l.w) == 0u) continue;       // (most of a large index between two polls)
    uint4 p = prev[q];
    p.x = (p.x | e.x) & ~l.x; p.y = (p.y | e.y) & ~l.y; p.z = (p.z | e.z) & ~l.z; p.w = (p.w | e.w) & ~l.w;
    prev[q] = p;
  }
}

}  // namespace bmx
