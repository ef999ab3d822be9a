// semi_kernels.h — semi-joins (bmx_semi.h bmx_where_semijoin, bmx_where_in): a set of values built on the device by one program and tested by another, gfx950,
// wave64.
//
// k_semi_build<T> : one read of the inner base field's value column (top_sweep's shape: 16-byte loads, TOP_U in flight per lane, 512 threads); PredWhere::row()
//                   decides the inner selection exactly as k_group_sweep does, called by every lane for all E rows of a unit. A selected row's key is the
//                   column value when the key field is the base field, otherwise one agg_probe, made after the match is known. The key goes into the table
//                   (semi_insert); the selected rows are counted in the lane, reduced per workgroup and added to n_inner with one atomic.
// k_semi_insert   : the same insert from a list of values (bmx_where_in, and the union the sharded form sends to every shard). A value outside +-VAL_MAX is
//                   skipped and not counted.
// PredSemi<T>     : the predicate of the probe sweep, for select.h's k_scan_mask: a PredWhere<T> plus the table. It exposes E and mask(first, n), so run_scan_t
//                   delivers its answer like any scan's. Per lane: PredWhere's walk over its E rows first (mask_from: row() per element); then, for each row the
//                   outer program selected, the link value (the column, or one agg_probe) and a walk of the now read-only table with plain loads until the key
//                   or an empty word. The lanes loop over their own matched rows: no wave vote is involved, so a lane with one match does not wait for the E
//                   rounds of a fixed loop. With the overflow state set every mask is 0: nothing is written and the count is 0.
// k_semi_export   : the occupied slots compacted into a list by wave ballot + popcount (the sharded form's phase 1).
// k_semi_finish   : every occupied slot back to empty; the workgroup that finishes last writes `res` from the scan's count and the state record and puts the state
//                   record back to zero.
// k_semi_clear    : table and state to their empty state (new scratch, or a query that did not get as far as its last kernel).
//
// The table (device memory, SemiScratch): `slots` = max(64, next power of two >= 2 * set_cap) key words, SEMI_EMPTY = INT64_MIN = BMX_VAL_DELETED = empty, which
// is never a data value and never inserted. The HOME slot of a key is group_mix(key) & (slots - 1) — group_kernels.h's function, the 64-bit finalizer of
// MurmurHash3 — and probing is linear with wrap, so tests/group_model.py's mix / home / keys_with_home / walk describe this table too.
// Insert (group_kernels.h group_slot's walk; semi_insert says why it has a copy of its own): walk from the home slot reading key words with relaxed
// agent-scope atomic loads; stop at the key itself; claim an empty word with one 64-bit atomicCAS;
// on a lost CAS look at the word the CAS returned (it may be this key, claimed by another lane) before moving on. A key that is already present costs no atomic:
// an inner side of 10^7 nodes with 5 distinct keys sends 5 + a few lost CASes to memory, not 10^7. A successful claim adds one to the claim counter with a
// no-return add. No lane waits for another or spins on a word another lane must write; the only loop is the walk, bounded by `slots`. Once more than set_cap keys
// are claimed the answer is an overflow whatever else happens, so a walk gives up at every 64th step from then on and raises the overflow bit (k_group_sweep's
// rule); a walk that finds no room at all raises it too.
// Probe: the load factor is at most 0.5 when the set fits, so a walk meets an empty word; it is bounded by `slots` anyway.
#pragma once
#include "group_kernels.h"
#include "../../include/bmx_semi.h"

namespace bmx {

constexpr long long SEMI_EMPTY = INT64_MIN;
static_assert(SEMI_EMPTY == VAL_DELETED && SEMI_EMPTY == GROUP_EMPTY, "the empty key is the one value no row holds");
static_assert(sizeof(bmx_semi_res) == 32, "the record of bmx_semi.h");
constexpr int SEMI_THREADS = 256;                 // the list, export, finish and clear kernels

// the state record of one query, in device memory; k_semi_finish leaves it as k_semi_clear does
struct SemiState {
  unsigned long long claims;                      // slots claimed = distinct keys in the table
  unsigned long long n_inner;                     // inner nodes selected / listed values inside the domain
  unsigned long long n_match;                     // the probe sweep's count (run_scan_t's count word)
  unsigned long long nout;                        // k_semi_export's rank counter
  uint32_t overflow;                              // a walk found no room (or gave up behind set_cap)
  uint32_t done;                                  // k_semi_finish's workgroups that have finished
};

struct SemiArgs {
  long long* keys; SemiState* S;
  uint64_t slots, cap;                            // this query's: the head of a table that may be larger
};

__device__ __forceinline__ void semi_state_reset(SemiState* S) {
  S->claims = 0ull; S->n_inner = 0ull; S->n_match = 0ull; S->nout = 0ull; S->overflow = 0u; S->done = 0u;
}

// `key` into the table: group_slot's walk (group_kernels.h), in a copy of its own. Measured: every path that claims leaves the loop at once here, so the
// compiler puts the wave's one add to the claim counter BEHIND the loop; in one shared definition, where a claim falls through, the add sits inside the
// walk, and a build of 10^6 distinct keys takes 4.6 ms instead of 3.4 (profiles/kernel_sharing_timings.txt). A change to one of the walks goes into the
// others by hand.
__device__ __forceinline__ void semi_insert(const SemiArgs& A, long long key) {
  const uint64_t mask = A.slots - 1u;
  uint64_t s = group_mix(key) & mask;
  for (uint64_t p = 0; p < A.slots; ++p, s = (s + 1u) & mask) {
    long long k = __hip_atomic_load(&A.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == key) return;                                                // present: no atomic
    if (k == SEMI_EMPTY) {
      k = (long long)atomicCAS(reinterpret_cast<unsigned long long*>(&A.keys[s]), (unsigned long long)SEMI_EMPTY, (unsigned long long)key);
      if (k == SEMI_EMPTY) { atomicAdd(&A.S->claims, 1ull); return; }
      if (k == key) return;                                              // the lane that won the word brought the same key
    }
    if ((p & 63u) == 63u && __hip_atomic_load(&A.S->claims, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > A.cap) break;
  }
  atomicOr(&A.S->overflow, 1u);
}

// is `key` in the table? Plain loads: nobody writes the table while the probe sweep runs.
__device__ __forceinline__ bool semi_has(const long long* __restrict__ keys, uint64_t slots, long long key) {
  const uint64_t mask = slots - 1u;
  uint64_t s = group_mix(key) & mask;
  for (uint64_t p = 0; p < slots; ++p, s = (s + 1u) & mask) {
    const long long k = keys[s];
    if (k == key) return true;
    if (k == SEMI_EMPTY) return false;
  }
  return false;
}

// a lane's count -> one atomic per workgroup (every lane of the workgroup calls it; `part`: one word per wave)
__device__ __forceinline__ void semi_count_end(unsigned long long c, unsigned long long* part, uint32_t nwaves, unsigned long long* dst) {
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < nwaves; w++) t += part[w];
    if (t) atomicAdd(dst, t);
  }
}

// key_src: 0 = the inner base field's column, AGG_SRC_PROBE = one probe of key_field
template <class T, bool CLOCKS>
__global__ __launch_bounds__(AGG_THREADS) void k_semi_build(uint64_t n, PredWhere<T, true, CLOCKS> P, SemiArgs A, uint32_t key_field, uint32_t key_src) {
  __shared__ unsigned long long s_n[TOP_WAVES];
  unsigned long long cnt_l = 0;
  where_sweep<T>(n, P, [&](int, T xe, uint64_t pos, bool sel) {
    if (!sel) return;
    cnt_l++;
    int64_t key = (int64_t)xe;
    if (where_field(P, pos, key_src, key_field, key)) semi_insert(A, (long long)key);
  });
  semi_count_end(cnt_l, s_n, TOP_WAVES, &A.S->n_inner);
}

__global__ __launch_bounds__(SEMI_THREADS) void k_semi_insert(const long long* __restrict__ values, uint64_t n, SemiArgs A) {
  __shared__ unsigned long long s_n[SEMI_THREADS / 64];
  unsigned long long cnt_l = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * SEMI_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SEMI_THREADS) {
    const long long v = values[i];
    if (v < -VAL_MAX || v > VAL_MAX) continue;                           // no row holds it (INT64_MIN is the empty word)
    cnt_l++;
    semi_insert(A, v);
  }
  semi_count_end(cnt_l, s_n, SEMI_THREADS / 64, &A.S->n_inner);
}

template <class T, bool CLOCKS>
struct PredSemi {   // the outer program AND (link value in the set) / AND NOT (...)
  static constexpr int E = PredWhere<T>::E;
  PredWhere<T, true, CLOCKS> P;
  const long long* keys; uint64_t slots;
  const SemiState* S; uint64_t cap;               // the overflow state: the bit, or more claims than set_cap
  uint32_t link, link_src, anti;                  // link_src: 0 = the base field's column, AGG_SRC_PROBE = one probe of `link`

  __device__ uint32_t mask(uint64_t first, uint64_t n) const {
    if (S->overflow != 0u || S->claims > cap) return 0u;               // (uniform)
    uint32_t out = 0;
    for (uint32_t m = P.mask_from(first, n, 0); m; m &= m - 1u) {      // this lane's rows that the outer program selected
      const uint32_t e = (uint32_t)__ffs((int)m) - 1u;
      const uint64_t pos = first + e;
      int64_t y = VAL_DELETED;
      bool have;
      if (link_src == 0u) { y = (int64_t)P.v[pos]; have = true; }      // a selected row holds data
      else have = agg_probe(P.slots, P.nslots, P.ids[pos], link, y) && y != VAL_DELETED;
      const bool in = have && semi_has(keys, slots, (long long)y);
      if (in != (anti != 0u)) out |= 1u << e;
    }
    return out;
  }
};

// `slots` is a multiple of 64: a wave's 64 lanes are inside the table or beyond it together. Writes nothing when the set does not fit.
__global__ __launch_bounds__(SEMI_THREADS) void k_semi_export(SemiArgs A, long long* __restrict__ out) {
  SemiState* S = A.S;
  if (S->overflow != 0u || S->claims > A.cap) return;                    // (uniform)
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t b = (uint64_t)blockIdx.x * SEMI_THREADS + (threadIdx.x & ~63u); b < A.slots; b += (uint64_t)gridDim.x * SEMI_THREADS) {
    const long long k = A.keys[b + lane];
    const bool occ = k != SEMI_EMPTY;
    if (!__ballot(occ)) continue;                                        // (uniform)
    const unsigned long long r = wave_rank(occ, &S->nout, lane);
    if (occ && r < A.cap) out[r] = k;
  }
}

__global__ __launch_bounds__(SEMI_THREADS) void k_semi_finish(SemiArgs A, bmx_semi_res* __restrict__ res) {
  SemiState* S = A.S;
  for (uint64_t s = (uint64_t)blockIdx.x * SEMI_THREADS + threadIdx.x; s < A.slots; s += (uint64_t)gridDim.x * SEMI_THREADS)
    if (A.keys[s] != SEMI_EMPTY) A.keys[s] = SEMI_EMPTY;
  if (last_workgroup(&S->done) && threadIdx.x == 0) {                    // only this thread reads the state record in this kernel
    const bool fits = S->overflow == 0u && S->claims <= A.cap;
    bmx_semi_res o;
    o.n_match = fits ? S->n_match : 0ull; o.set_size = S->claims; o.n_inner = S->n_inner; o.flags = fits ? 0u : BMX_SEMI_OVERFLOW; o.reserved = 0u;
    *res = o;
    semi_state_reset(S);
  }
}

__global__ __launch_bounds__(SEMI_THREADS) void k_semi_clear(long long* __restrict__ keys, uint64_t slots, SemiState* __restrict__ S) {
  for (uint64_t s = (uint64_t)blockIdx.x * SEMI_THREADS + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * SEMI_THREADS) keys[s] = SEMI_EMPTY;
  if (blockIdx.x == 0 && threadIdx.x == 0) semi_state_reset(S);
}

}  // namespace bmx
