// join_kernels.h — lookup joins (bmx_join.h bmx_where_join_group, bmx_where_map_group): a map key -> attribute built on the device by one program, and a second
// program's selection grouped by the attribute its link value maps to, gfx950, wave64.
//
// k_join_build<T>       : k_semi_build's shape (top_sweep, PredWhere::row() called by every lane for all E rows of a unit). A selected inner row's key and
//                         attribute are the column value when the field is the inner base field, otherwise one agg_probe each, made after the match is known
//                         (attr_field == key_field reuses the key). The pair goes into the map (join_insert); the selected rows and the ones that hold a key
//                         are counted in the lane, reduced per workgroup and added to n_inner / n_keyed with one atomic each.
// k_join_insert         : the same insert from a list of pairs (bmx_where_map_group, and the union the sharded form sends to every shard). A key outside
//                         +-VAL_MAX is skipped and not counted; a val outside +-VAL_MAX is "no attribute".
// k_join_group_sweep<T> : k_group_sweep's shape and LDS cache. Per selected row: the measure and the link (the column, or one agg_probe each), a read-only walk of
//                         the map with plain 16-byte loads, then `total` plus `absent` or `unmatched` in the lane's registers, or group_put with the mapped
//                         attribute as the key (group_row_put: the wave's same-key vote). The three lane records leave the workgroup one after another through
//                         the one AggLds<0>. With the map's overflow state set the kernel returns at once: nothing is grouped and every record stays empty.
// k_join_export         : the occupied pairs compacted into two lists by wave ballot + popcount (the sharded form's phase 1).
// k_join_finish         : the group records ranked and written as k_group_finish does; both tables back to empty; the workgroup that finishes last writes `res`
//                         and puts both state records back.
// k_join_clear          : the map and its state record to their empty state (new scratch, or a query that did not get as far as its last kernel).
//
// The map (device memory, JoinScratch): `slots` = max(64, next power of two >= 2 * map_cap) 16-byte {key, val} pairs: a lookup is one random access and one
// aligned 16-byte load brings both words. An empty key is JOIN_EMPTY = INT64_MIN = BMX_VAL_DELETED, a val of JOIN_NO_ATTR = INT64_MAX means "no attribute";
// neither is a data value. Home slot and walk are semi_insert's (group_mix(key) & (slots - 1), linear with wrap), so tests/group_model.py's home /
// keys_with_home / walk describe this table too. Insert: join_slot, group_slot's walk over the pairs' key words, as semi_insert (relaxed agent-scope loads,
// one atomicCAS on an empty word, the word the CAS returned looked at before moving on; a key already present costs no atomic), then the minimum: the val word
// of every slot is JOIN_NO_ATTR before the launch and only ever decreases, so an atomicMin is issued only when a relaxed agent-scope load of the word shows a
// value above the node's attribute — the skip is exact, and an inner side of 10^7 nodes with five keys does not send 10^7 atomics to five addresses. A lane may
// lower the val of a slot the moment it sees its key there: no lane waits for another or spins on a word another lane must write. The only loop is the walk,
// bounded by `slots`; it gives up at every 64th step once more than map_cap keys are claimed and raises the overflow bit, as semi_insert does.
#pragma once
#include "semi_kernels.h"
#include "../../include/bmx_join.h"

namespace bmx {

constexpr long long JOIN_EMPTY = INT64_MIN, JOIN_NO_ATTR = INT64_MAX;
static_assert(JOIN_EMPTY == SEMI_EMPTY && JOIN_EMPTY == GROUP_EMPTY, "the empty key is the one value no row holds");
static_assert(sizeof(bmx_join_res) == 184, "the record of bmx_join.h");
constexpr int JOIN_THREADS = SEMI_THREADS;        // the list, export, finish and clear kernels
constexpr uint32_t JOIN_SRC_KEY = 0xFDu;          // attr_src: the attribute is the key (attr_field == key_field)

struct alignas(16) JoinPair { long long key, val; };
typedef long long join_ll2 __attribute__((ext_vector_type(2)));
static_assert(sizeof(JoinPair) == 16 && sizeof(join_ll2) == 16, "one 16-byte load per step of a lookup");

// the state record of one query's map, in device memory; k_join_finish leaves it as k_join_clear does
struct JoinState {
  unsigned long long claims;                      // slots claimed = distinct keys in the map
  unsigned long long n_inner, n_keyed;            // inner nodes selected / of those, with key data (listed pairs inside the domain: both)
  unsigned long long nout;                        // k_join_export's rank counter
  uint32_t overflow;                              // a walk found no room (or gave up behind map_cap)
  uint32_t done;                                  // k_join_finish's workgroups that have finished
  AggRaw unmatched;                               // the third record of the group sweep (absent and total are GroupState's)
};

struct JoinArgs {
  JoinPair* map; JoinState* S;
  uint64_t slots, cap;                            // this query's: the head of a table that may be larger
};

__device__ __forceinline__ bool join_map_fits(const JoinState* S, uint64_t cap) { return S->overflow == 0u && S->claims <= cap; }

__device__ __forceinline__ void join_state_reset(JoinState* S) {
  S->claims = 0ull; S->n_inner = 0ull; S->n_keyed = 0ull; S->nout = 0ull; S->overflow = 0u; S->done = 0u; S->unmatched = GROUP_RAW_EMPTY;
}

// the slot of `key` in the map, for join_insert and reach_kernels.h's reach_insert: group_slot's find-or-claim walk over the pairs' key words, in a copy of its
// own (group_slot says why). false: no room (the overflow bit is up); claimed: by this lane, just now
__device__ __forceinline__ bool join_slot(const JoinArgs& A, long long key, uint64_t& slot, bool& claimed) {
  const uint64_t mask = A.slots - 1u;
  uint64_t s = group_mix(key) & mask;
  claimed = false;
  for (uint64_t p = 0; p < A.slots; ++p, s = (s + 1u) & mask) {
    long long k = __hip_atomic_load(&A.map[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == JOIN_EMPTY) {
      k = (long long)atomicCAS(reinterpret_cast<unsigned long long*>(&A.map[s].key), (unsigned long long)JOIN_EMPTY, (unsigned long long)key);
      if (k == JOIN_EMPTY) { atomicAdd(&A.S->claims, 1ull); claimed = true; k = key; }
    }
    if (k == key) { slot = s; return true; }                             // present (or just claimed, by this lane or another with the same key)
    if ((p & 63u) == 63u && __hip_atomic_load(&A.S->claims, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > A.cap) break;
  }
  atomicOr(&A.S->overflow, 1u);
  return false;
}
// the val of slot s down to `val` (the word only ever decreases: a value at or below val now stays there, and costs no atomic)
__device__ __forceinline__ void join_lower(const JoinArgs& A, uint64_t s, long long val) {
  if (__hip_atomic_load(&A.map[s].val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > val) atomicMin(&A.map[s].val, val);
}

// the pair (key, val) into the map: find or claim the key's slot, then lower its val (val == JOIN_NO_ATTR: the key alone)
__device__ __forceinline__ void join_insert(const JoinArgs& A, long long key, long long val) {
  uint64_t s; bool claimed;
  if (join_slot(A, key, s, claimed) && val != JOIN_NO_ATTR) join_lower(A, s, val);
}

// the val of `key` in the map; false: not a key. Plain loads: nobody writes the map while the group sweep runs.
__device__ __forceinline__ bool join_find(const JoinPair* __restrict__ map, uint64_t slots, long long key, long long& val) {
  const uint64_t mask = slots - 1u;
  uint64_t s = group_mix(key) & mask;
  for (uint64_t p = 0; p < slots; ++p, s = (s + 1u) & mask) {
    const join_ll2 kv = *reinterpret_cast<const join_ll2*>(map + s);
    if (kv.x == key) { val = kv.y; return true; }
    if (kv.x == JOIN_EMPTY) return false;
  }
  return false;
}

// key_src: 0 = the inner base field's column, AGG_SRC_PROBE = one probe of key_field; attr_src: likewise, or JOIN_SRC_KEY
template <class T, bool CLOCKS>
__global__ __launch_bounds__(AGG_THREADS) void k_join_build(uint64_t n, PredWhere<T, true, CLOCKS> P, JoinArgs A, uint32_t key_field, uint32_t key_src, uint32_t attr_field, uint32_t attr_src) {
  __shared__ unsigned long long s_n[TOP_WAVES], s_k[TOP_WAVES];
  unsigned long long cnt_l = 0, key_l = 0;
  where_sweep<T>(n, P, [&](int, T xe, uint64_t pos, bool sel) {
    if (!sel) return;
    cnt_l++;
    int64_t key = (int64_t)xe, attr = (int64_t)xe;
    bool have_k = key_src == 0u, have_a = attr_src == 0u;
    // the key (k = 0) and the attribute (k = 1) through ONE copy of the probe. Not where_two_fields: the skip of k = 1 depends on what k = 0 found in this lane.
#pragma unroll 1
    for (uint32_t k = 0; k < 2u; k++) {
      if ((k ? attr_src : key_src) != AGG_SRC_PROBE) continue;         // (uniform)
      if (k && !have_k) continue;                                       // (a keyless node's attribute is never looked at)
      int64_t y;
      if (agg_probe(P.slots, P.nslots, P.ids[pos], k ? attr_field : key_field, y) && y != VAL_DELETED) {
        if (k) { attr = y; have_a = true; } else { key = y; have_k = true; }
      }
    }
    if (!have_k) return;
    key_l++;
    if (attr_src == JOIN_SRC_KEY) { attr = key; have_a = true; }
    join_insert(A, (long long)key, have_a ? (long long)attr : JOIN_NO_ATTR);
  });
  semi_count_end(cnt_l, s_n, TOP_WAVES, &A.S->n_inner);
  semi_count_end(key_l, s_k, TOP_WAVES, &A.S->n_keyed);
}

__global__ __launch_bounds__(JOIN_THREADS) void k_join_insert(const long long* __restrict__ keys, const long long* __restrict__ vals, uint64_t n, JoinArgs A) {
  __shared__ unsigned long long s_n[JOIN_THREADS / 64], s_k[JOIN_THREADS / 64];
  unsigned long long cnt_l = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * JOIN_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * JOIN_THREADS) {
    const long long k = keys[i];
    if (k < -VAL_MAX || k > VAL_MAX) continue;                           // no row holds it (INT64_MIN is the empty word)
    long long v = vals[i];
    if (v < -VAL_MAX || v > VAL_MAX) v = JOIN_NO_ATTR;
    cnt_l++;
    join_insert(A, k, v);
  }
  semi_count_end(cnt_l, s_n, JOIN_THREADS / 64, &A.S->n_inner);
  semi_count_end(cnt_l, s_k, JOIN_THREADS / 64, &A.S->n_keyed);
}

// group_lane_add under a condition, with selects on the values: a branch per record invites the compiler to pick the RECORD by address, which puts two of the
// three lane records into scratch memory
__device__ __forceinline__ void join_lane_add(AggLane& L, bool on, bool have_m, int64_t mval) {
  const bool m = on && have_m;
  L.nm += on ? 1ull : 0ull; L.n += m ? 1ull : 0ull;
  L.slo += m ? (unsigned long long)(uint32_t)mval : 0ull; L.shi += m ? (long long)(mval >> 32) : 0ll;
  L.mn = (m && mval < L.mn) ? mval : L.mn; L.mx = (m && mval > L.mx) ? mval : L.mx;
}

// one row of the group sweep, called by every lane of the wave (sel = false: the lane only keeps the wave's votes company). A.group / A.g_src are the LINK's.
template <class T, bool CLOCKS>
__device__ __forceinline__ void join_row(const PredWhere<T, true, CLOCKS>& P, const GroupArgs& A, const JoinPair* __restrict__ map, uint64_t mslots, bool sel, int64_t x, uint64_t pos,
                                         uint32_t lane, AggLane& Lt, AggLane& La, AggLane& Lu, GroupLds& S) {
  int64_t mval = x, lval = x;
  long long gval = JOIN_NO_ATTR;
  bool have_m = A.m_src == 0u, have_l = A.g_src == 0u, go = false;
  if (sel) {
    where_two_fields(P, pos, A.m_src, A.measure, mval, have_m, A.g_src, A.group, lval, have_l);
    const bool in = have_l && join_find(map, mslots, (long long)lval, gval);
    group_lane_add(Lt, have_m, mval);
    join_lane_add(Lu, !in, have_m, mval);
    join_lane_add(La, in && gval == JOIN_NO_ATTR, have_m, mval);
    go = in && gval != JOIN_NO_ATTR;
  }
  group_row_put(A, go, gval, have_m, mval, lane, S);                   // (rows of one wave often map to one attribute)
}

template <class T, bool CLOCKS>
__global__ __launch_bounds__(AGG_THREADS) void k_join_group_sweep(uint64_t n, PredWhere<T, true, CLOCKS> P, GroupArgs A, JoinArgs J) {
  __shared__ GroupLds S;
  if (!join_map_fits(J.S, J.cap)) return;                                // (uniform: the build is complete) nothing is grouped, every record stays empty
  group_cache_begin(S);
  AggLane Lt, La, Lu;
  const uint32_t lane = threadIdx.x & 63u;
  const JoinPair* map = J.map;
  const uint64_t mslots = J.slots;
  where_sweep<T>(n, P, [&](int, T xe, uint64_t pos, bool sel) { join_row<T>(P, A, map, mslots, sel, (int64_t)xe, pos, lane, Lt, La, Lu, S); });
  group_cache_end(A, S, Lt, La);
  __syncthreads();
  group_end(&J.S->unmatched, Lu, S.w);
}

// `slots` is a multiple of 64: a wave's 64 lanes are inside the table or beyond it together. Writes nothing when the map does not fit.
__global__ __launch_bounds__(JOIN_THREADS) void k_join_export(JoinArgs A, long long* __restrict__ out_keys, long long* __restrict__ out_vals) {
  JoinState* S = A.S;
  if (!join_map_fits(S, A.cap)) return;                                  // (uniform)
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t b = (uint64_t)blockIdx.x * JOIN_THREADS + (threadIdx.x & ~63u); b < A.slots; b += (uint64_t)gridDim.x * JOIN_THREADS) {
    const join_ll2 kv = *reinterpret_cast<const join_ll2*>(A.map + b + lane);
    const bool occ = kv.x != JOIN_EMPTY;
    if (!__ballot(occ)) continue;                                        // (uniform)
    const unsigned long long r = wave_rank(occ, &S->nout, lane);
    if (occ && r < A.cap) { out_keys[r] = kv.x; out_vals[r] = kv.y; }
  }
}

// A.slots == 0: no group table to sweep (the sharded form's phase 1); A.S is read and put back all the same.
__global__ __launch_bounds__(JOIN_THREADS) void k_join_finish(GroupArgs A, JoinArgs J, bmx_group_rec* __restrict__ out, bmx_join_res* __restrict__ res, uint32_t n_is_match) {
  GroupState* S = A.S;
  JoinState* M = J.S;
  const unsigned long long claims = S->claims;
  const bool fits = claims <= A.cap && S->overflow == 0u;               // (a map that did not fit left the group table empty: fits, with nothing to write)
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t b = (uint64_t)blockIdx.x * JOIN_THREADS + (threadIdx.x & ~63u); b < A.slots; b += (uint64_t)gridDim.x * JOIN_THREADS) {
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
  for (uint64_t s = (uint64_t)blockIdx.x * JOIN_THREADS + threadIdx.x; s < J.slots; s += (uint64_t)gridDim.x * JOIN_THREADS)
    if (J.map[s].key != JOIN_EMPTY) { JoinPair e; e.key = JOIN_EMPTY; e.val = JOIN_NO_ATTR; J.map[s] = e; }
  if (last_workgroup(&M->done) && threadIdx.x == 0) {                   // no workgroup reads the state records any more
    const bool mfits = join_map_fits(M, J.cap);
    bmx_join_res o;
    o.n_groups = mfits ? claims : 0ull; o.map_size = M->claims; o.n_inner = M->n_inner; o.n_keyed = M->n_keyed;
    o.flags = (mfits ? 0u : BMX_JOIN_MAP_OVERFLOW) | (fits ? 0u : BMX_JOIN_GROUP_OVERFLOW); o.reserved = 0u;
    o.absent = group_compose(S->absent, n_is_match); o.unmatched = group_compose(M->unmatched, n_is_match); o.total = group_compose(S->total, n_is_match);
    *res = o;
    group_state_reset(S);
    join_state_reset(M);
  }
}

__global__ __launch_bounds__(JOIN_THREADS) void k_join_clear(JoinPair* __restrict__ map, uint64_t slots, JoinState* __restrict__ S) {
  for (uint64_t s = (uint64_t)blockIdx.x * JOIN_THREADS + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * JOIN_THREADS) { JoinPair e; e.key = JOIN_EMPTY; e.val = JOIN_NO_ATTR; map[s] = e; }
  if (blockIdx.x == 0 && threadIdx.x == 0) join_state_reset(S);
}

}  // namespace bmx
