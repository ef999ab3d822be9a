// group_kernels.h — group-by over discovered values (bmx_group.h bmx_where_group): a hash aggregation behind a boolean filter, gfx950, wave64.
//
// k_group_sweep<T> : one read of the base field's value column (top_sweep's shape: 16-byte loads, TOP_U in flight per lane, 512 threads); PredWhere::row()
//                    decides the candidates exactly as k_where_agg does. A selected row's measure and group value are the column value when the field is the base
//                    field, otherwise one agg_probe each, made after the match is known. The row is added to `total` (and to `absent` when its group value is
//                    absent or tombstoned) in the lane's registers, and to the record of its key.
// k_group_finish   : one sweep of the table's slots. Occupied slots are ranked by wave ballot + popcount into one counter (top_kernels.h wave_rank); if the
//                    distinct keys fit the caller's cap the 128-bit sums are composed and the records written. Every slot goes back to its empty state; the
//                    workgroup that finishes last (last_workgroup) writes `res` and puts the state record back too (group_state_reset).
// k_group_clear    : table and state to their empty state (new scratch, or a query that did not get as far as its last kernel).
//
// The table (device memory, GroupScratch): `slots` = max(64, next power of two >= 2 * cap) entries of a key word and an AggRaw accumulator. An empty slot's key
// is GROUP_EMPTY = INT64_MIN = BMX_VAL_DELETED, which is never a data value. The HOME slot of a key is group_mix(key) & (slots - 1), group_mix = the 64-bit
// finalizer of MurmurHash3 (x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33); probing is linear with wrap. A claim is
// one 64-bit atomicCAS on the key word (and one no-return add to the claim counter). The accumulators are in their empty state before the launch, so any lane
// may add into a slot the moment it sees its key there: no lane ever waits for another lane or spins on a word another lane must write. The only loop is the
// probe walk, bounded by `slots`; a walk that finds no room raises the overflow bit and drops the row from the groups (it still counts in `total`). A walk also
// gives up at every 64th step once more keys than `cap` have been claimed: the answer is an overflow by then and only `absent` and `total` still matter.
//
// Pre-aggregation. A column with a handful of distinct values must not send one set of memory-side atomics per row to a handful of addresses. Each workgroup
// keeps a cache of GROUP_CACHE = 1024 {key, 40-byte partial} entries in LDS (48 KB, what G = 1 of agg_kernels.h spends): GROUP_SETS = 256 sets of GROUP_WAYS = 4.
// The set of a key is group_set(key) = (((uint32)key ^ (uint32)(key >> 32)) * 0x9E3779B1) >> 24 (Fibonacci hashing: consecutive values and strided values both
// spread evenly over the sets). A lane takes the first way of its set that holds its key or that it can claim (atomicCAS in LDS); the partials are LDS atomics
// as in G = 1. A row whose set is taken by four other keys BYPASSES the cache: it goes straight to the global table with the no-return atomics of agg_add<2>.
// Which of more than four keys of a set get its ways depends on who comes first; the answer does not. The occupied entries are flushed once behind the
// workgroup's last row: one find-or-claim and at most 6 memory-side atomics per key and workgroup. Within a wave, the lanes that hold the first selected
// lane's key add their count once (ballot + popcount, as k_top_digit does).
//
// One definition each, for this family and the ones built on it (first_, gtop_, mgroup_, semi_, join_, join_rows_, reach_kernels.h): group_row_put (the
// wave's key combine), group_cache_begin / group_cache_end (the LDS cache around a sweep: clear, flush, the two records' tail), last_workgroup and
// group_state_reset. The row walk and the field fetch are where_agg_kernels.h's. The find-or-claim walk has three copies (group_slot says why).
#pragma once
#include "where_agg_kernels.h"
#include "../../include/bmx_group.h"

namespace bmx {

constexpr uint32_t GROUP_WAYS = 4, GROUP_SETS = 256, GROUP_CACHE = GROUP_WAYS * GROUP_SETS;
constexpr long long GROUP_EMPTY = INT64_MIN;
static_assert(GROUP_EMPTY == VAL_DELETED, "the empty key is the one value no row holds");
static_assert(GROUP_SETS == 256, "group_set keeps the top 8 bits of the product");
static_assert(sizeof(bmx_group_rec) == 56 && sizeof(bmx_group_res) == 112, "the records of bmx_group.h");

// the state record of one query, in device memory; k_group_finish leaves it as k_group_clear does
struct GroupState {
  unsigned long long claims;                   // slots claimed = distinct keys in the table
  unsigned long long nout;                     // k_group_finish's rank counter
  uint32_t overflow;                           // a walk found no room (or gave up behind cap)
  uint32_t done;                               // k_group_finish's workgroups that have finished
  AggRaw absent, total;
};

struct GroupArgs {
  long long* keys; AggRaw* acc; GroupState* S;
  uint64_t slots, cap;
  uint32_t measure, group;                     // field hashes (read where m_src / g_src == AGG_SRC_PROBE)
  uint32_t m_src, g_src;                       // 0: the base field's column, AGG_SRC_PROBE, AGG_SRC_NONE (the measure alone)
};

__host__ __device__ inline uint64_t group_mix(int64_t key) {
  uint64_t x = (uint64_t)key;
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
__host__ __device__ inline uint32_t group_set(int64_t key) { return (((uint32_t)(uint64_t)key ^ (uint32_t)((uint64_t)key >> 32)) * 0x9E3779B1u) >> 24; }

struct GroupLds {
  long long key[GROUP_CACHE];
  uint32_t nm[GROUP_CACHE], n[GROUP_CACHE];
  long long mn[GROUP_CACHE], mx[GROUP_CACHE];
  unsigned long long slo[GROUP_CACHE]; long long shi[GROUP_CACHE];
  AggLds<0> w;                                 // the waves' partials of `total`, then of `absent`
};

constexpr AggRaw GROUP_RAW_EMPTY = AggRaw{0ull, 0ull, INT64_MAX, INT64_MIN, 0ull, 0ll};

__device__ __forceinline__ void group_state_reset(GroupState* S) {
  S->claims = 0ull; S->nout = 0ull; S->overflow = 0u; S->done = 0u; S->absent = GROUP_RAW_EMPTY; S->total = GROUP_RAW_EMPTY;
}

// The "last workgroup" step of a finish kernel, called by every thread behind its part of the sweep: a barrier (every thread of the workgroup has read the
// state record and done its slots), one count into `done`, -> true in every thread of the workgroup that counted last: nobody else reads the record any more.
__device__ __forceinline__ bool last_workgroup(uint32_t* done) {
  __shared__ uint32_t s_last;
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(done, 1u) == gridDim.x - 1u ? 1u : 0u;
  __syncthreads();
  return s_last != 0u;
}

// The slot of `key` in the global table, found or claimed; false: no room (the overflow bit is up). The find-or-claim walk of the family: from the key's home
// slot, linear with wrap; relaxed agent-scope load; an empty word is claimed with one CAS and one no-return add to the claim counter; the word a lost CAS
// returned is looked at before moving on (it may be this key, claimed by another lane); a key already present costs no atomic. The walk gives up at every
// 64th step once more than `cap` keys are claimed, and in a table without room. semi_insert and join_kernels.h's join_slot are the same walk over their own
// tables, each in a copy of its own, and a change to one goes into the others by hand. Measured: one shared definition (a claim that falls through to the
// k == key test, the stride a callable) leaves every figure of the resource table alone but spills 6 more scalar registers in k_group_sweep's computed
// builds, makes bmx_where_group 3 to 6 us slower where the walk is inlined on the bypass path of the row loop, and costs semi_insert a third of its speed.
__device__ __forceinline__ bool group_slot(const GroupArgs& A, long long key, uint64_t& slot) {
  const uint64_t mask = A.slots - 1u;
  uint64_t s = group_mix(key) & mask;
  for (uint64_t p = 0; p < A.slots; ++p, s = (s + 1u) & mask) {
    long long k = __hip_atomic_load(&A.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == GROUP_EMPTY) {
      k = (long long)atomicCAS(reinterpret_cast<unsigned long long*>(&A.keys[s]), (unsigned long long)GROUP_EMPTY, (unsigned long long)key);
      if (k == GROUP_EMPTY) { atomicAdd(&A.S->claims, 1ull); slot = s; return true; }
    }
    if (k == key) { slot = s; return true; }
    if ((p & 63u) == 63u && __hip_atomic_load(&A.S->claims, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > A.cap) break;
  }
  atomicOr(&A.S->overflow, 1u);
  return false;
}

// one contribution to the record of `key`: nm rows, and (have_m) one measured value
__device__ __forceinline__ void group_put(const GroupArgs& A, GroupLds& S, long long key, uint32_t nm, bool have_m, int64_t mval) {
  const unsigned long long lo = (unsigned long long)(uint32_t)mval; const long long hi = mval >> 32;
  const uint32_t n1 = (have_m && A.m_src == AGG_SRC_PROBE) ? 1u : 0u;   // (otherwise every match has its measure or none has: n is k_group_finish's)
  const uint32_t base = group_set(key) * GROUP_WAYS;
  uint32_t hit = GROUP_CACHE;
#pragma unroll
  for (uint32_t w = 0; w < GROUP_WAYS; w++) {
    if (hit != GROUP_CACHE) break;
    long long k = __hip_atomic_load(&S.key[base + w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == GROUP_EMPTY) {
      k = (long long)atomicCAS(reinterpret_cast<unsigned long long*>(&S.key[base + w]), (unsigned long long)GROUP_EMPTY, (unsigned long long)key);
      if (k == GROUP_EMPTY) k = key;
    }
    if (k == key) hit = base + w;
  }
  if (hit != GROUP_CACHE) {
    if (nm) atomicAdd(&S.nm[hit], nm);
    if (have_m) {
      if (n1) atomicAdd(&S.n[hit], 1u);
      atomicAdd(&S.slo[hit], lo);
      if (hi) atomicAdd(reinterpret_cast<unsigned long long*>(&S.shi[hit]), (unsigned long long)hi);
      atomicMin(&S.mn[hit], (long long)mval); atomicMax(&S.mx[hit], (long long)mval);
    }
    return;
  }
  uint64_t slot;                                                       // the bypass
  if (group_slot(A, key, slot))
    agg_flush_one(A.acc + slot, nm, n1, have_m ? (long long)mval : INT64_MAX, have_m ? (long long)mval : INT64_MIN, have_m ? lo : 0ull, have_m ? hi : 0ll);
}

__device__ __forceinline__ void group_lane_add(AggLane& L, bool have_m, int64_t mval) {
  L.nm++;
  if (have_m) { L.n++; L.slo += (unsigned long long)(uint32_t)mval; L.shi += mval >> 32; L.mn = mval < L.mn ? mval : L.mn; L.mx = mval > L.mx ? mval : L.mx; }
}

// the end of one row of every grouped sweep, called by every lane of the wave: the row (go = false: none) into the record of its key
__device__ __forceinline__ void group_row_put(const GroupArgs& A, bool go, int64_t gval, bool have_m, int64_t mval, uint32_t lane, GroupLds& S) {
  const unsigned long long act = __ballot(go);
  if (!act) return;                                                  // (uniform)
  // rows of one wave often share a key: the lanes that hold the first one's key add their count once
  const int first = __ffsll((long long)act) - 1;
  const long long k0 = __shfl((long long)gval, first);
  const unsigned long long same = __ballot(go && (long long)gval == k0);
  if (!go) return;
  uint32_t nm = 1u;
  if ((long long)gval == k0) nm = (int)lane == first ? (uint32_t)__popcll(same) : 0u;
  if (nm || have_m) group_put(A, S, (long long)gval, nm, have_m, mval);
}

// one row of the sweep, called by every lane of the wave (sel = false: the lane only keeps the wave's votes company). EXPR: where_agg_row's; `total` and
// `absent` take the node as its class says (the host sets A.m_src = AGG_SRC_PROBE: n is counted per row).
template <class T, bool CLOCKS, bool EXPR>
__device__ __forceinline__ void group_row(const PredWhere<T, true, CLOCKS>& P, const GroupArgs& A, const ExprArgs<EXPR>& X, bool sel, int64_t x, uint64_t pos, uint32_t lane,
                                          AggLane& Lt, AggLane& La, GroupLds& S, ExprWave& C) {
  int64_t mval = x, gval = x;
  bool have_m = A.m_src == 0u, have_g = A.g_src == 0u;
  uint32_t cls = EXPR_DEFINED;
  if (sel) {
    if constexpr (EXPR) have_m = expr_fetch(P.slots, P.nslots, P.ids, X, A.g_src, A.group, x, pos, mval, gval, have_g, cls);
    else where_two_fields(P, pos, A.m_src, A.measure, mval, have_m, A.g_src, A.group, gval, have_g);
    group_lane_add(Lt, have_m, mval);
    if (!have_g) group_lane_add(La, have_m, mval);
  }
  if constexpr (EXPR) expr_count(C, cls);
  group_row_put(A, sel && have_g, gval, have_m, mval, lane, S);
}

// a lane's record -> one set of no-return atomics per workgroup (agg_end<0>)
__device__ __forceinline__ void group_end(AggRaw* dst, AggLane& L, AggLds<0>& W) {
  AggArgs B;
  B.acc = dst;
  agg_end<0>(B, L, W);
}

// The workgroup's cache around a sweep, called by every thread. group_cache_begin: every entry empty, visible to the workgroup.
__device__ __forceinline__ void group_cache_begin(GroupLds& S) {
  for (uint32_t e = threadIdx.x; e < GROUP_CACHE; e += AGG_THREADS) {
    S.key[e] = GROUP_EMPTY; S.nm[e] = 0u; S.n[e] = 0u; S.mn[e] = INT64_MAX; S.mx[e] = INT64_MIN; S.slo[e] = 0ull; S.shi[e] = 0ll;
  }
  __syncthreads();
}
// group_cache_end, behind the workgroup's last row: the flush (every key the workgroup cached, once: one find-or-claim and one set of atomics), then the
// lanes' records of `total` and of `absent` through the one AggLds<0>, one after the other
__device__ __forceinline__ void group_cache_end(const GroupArgs& A, GroupLds& S, AggLane& Lt, AggLane& La) {
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < GROUP_CACHE; e += AGG_THREADS) {
    const long long k = S.key[e];
    const uint32_t nm = S.nm[e];
    uint64_t slot;
    if (k != GROUP_EMPTY && nm && group_slot(A, k, slot)) agg_flush_one(A.acc + slot, nm, S.n[e], S.mn[e], S.mx[e], S.slo[e], S.shi[e]);
  }
  group_end(&A.S->total, Lt, S.w);
  __syncthreads();                                                      // (thread 0 has read the waves' partials of `total`)
  group_end(&A.S->absent, La, S.w);
}

template <class T, bool CLOCKS, bool EXPR = false>      // (EXPR: a computed measure, bmx_expr.h; X is empty without one)
__global__ __launch_bounds__(AGG_THREADS) void k_group_sweep(uint64_t n, PredWhere<T, true, CLOCKS> P, GroupArgs A, ExprArgs<EXPR> X) {
  __shared__ GroupLds S;
  group_cache_begin(S);
  AggLane Lt, La;
  ExprWave C;
  const uint32_t lane = threadIdx.x & 63u;
  where_sweep<T>(n, P, [&](int, T xe, uint64_t pos, bool sel) { group_row<T>(P, A, X, sel, (int64_t)xe, pos, lane, Lt, La, S, C); });
  group_cache_end(A, S, Lt, La);
  expr_end(X, C);
}

__device__ __forceinline__ bmx_agg group_compose(const AggRaw& x, uint32_t n_is_match) {
  const __int128 s = ((__int128)x.shi << 32) + (__int128)x.slo;
  bmx_agg o;
  o.n_match = x.nm; o.n = n_is_match ? x.nm : x.n; o.min = x.mn; o.max = x.mx;
  o.sum_lo = (uint64_t)s; o.sum_hi = (int64_t)(s >> 64);
  return o;
}

// n_is_match: every match had its measure (or there is none): n = n_match. `slots` is a multiple of 64: a wave's 64 lanes are inside the table or beyond it together.
__global__ __launch_bounds__(256) void k_group_finish(GroupArgs A, bmx_group_rec* __restrict__ out, bmx_group_res* __restrict__ res, uint32_t n_is_match) {
  GroupState* S = A.S;
  const unsigned long long claims = S->claims;
  const bool fits = claims <= A.cap && S->overflow == 0u;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t b = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); b < A.slots; b += (uint64_t)gridDim.x * 256u) {
    const uint64_t s = b + lane;
    const long long k = A.keys[s];
    const bool occ = k != GROUP_EMPTY;
    if (!__ballot(occ)) continue;                                       // (uniform)
    if (fits) {
      const unsigned long long r = wave_rank(occ, &S->nout, lane);
      if (occ && r < A.cap) { bmx_group_rec o; o.key = k; o.agg = group_compose(A.acc[s], n_is_match); out[r] = o; }
    }
    if (occ) { A.keys[s] = GROUP_EMPTY; A.acc[s] = GROUP_RAW_EMPTY; }
  }
  if (last_workgroup(&S->done) && threadIdx.x == 0) {                   // no workgroup reads the state record any more
    bmx_group_res o;
    o.n_groups = claims; o.flags = fits ? 0u : BMX_GROUP_OVERFLOW; o.reserved = 0u;
    o.absent = group_compose(S->absent, n_is_match); o.total = group_compose(S->total, n_is_match);
    *res = o;
    group_state_reset(S);
  }
}

__global__ __launch_bounds__(256) void k_group_clear(long long* __restrict__ keys, AggRaw* __restrict__ acc, uint64_t slots, GroupState* __restrict__ S) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256u) { keys[s] = GROUP_EMPTY; acc[s] = GROUP_RAW_EMPTY; }
  if (blockIdx.x == 0 && threadIdx.x == 0) group_state_reset(S);
}

}  // namespace bmx
