// first_kernels.h — the first node per group (bmx_first.h bmx_where_group_first): an exact arg-min per discovered key under the total order (order value, then
// id as an unsigned number) behind a boolean filter, gfx950, wave64. There is no 128-bit atomic, so no single atomic can pick a (value, id) pair: the value is
// settled in one pass and the id in the next, with the kernel boundary between them.
//
// k_first_sweep<T>   : pass 1, k_group_sweep's shape and pieces: top_sweep over the base field's value column, PredWhere::row() evaluated once per candidate,
//                      the group and the order value from the column or from one agg_probe each (one probe for both when they are the same field), made after
//                      the match is known; the row then goes where a row of bmx_where_group goes with measure = order field (group_row_put, group_cache_begin
//                      and group_cache_end: the wave's count combine, the LDS cache, the bypass, the flush, the find-or-claim walk with its claim counter and
//                      give-up rule are group_kernels.h's, not copies). So per key the table holds n_match, n and BOTH extremes of the contenders' order values
//                      (64-bit atomic min and max). It also leaves, per index position, what pass 2 needs so that it probes nothing: a word gw[pos] when the
//                      group field is not the base column (the group value of a selected node that has one, else BMX_VAL_DELETED) and a word ow[pos] when the
//                      order field is not the base column (the order value of a selected node that has one, else BMX_VAL_DELETED). When both come from the
//                      column the order word is kept anyway: it is then the only record of which positions the program selected. A lane holds the words of its
//                      E positions in registers and stores them as whole 16-byte vectors behind the unit's last row, so consecutive lanes write consecutive
//                      addresses.
// k_first_resolve<T> : pass 2, a streaming sweep of those words (and of the column where a field is the base field). A position is a CONTENDER iff every word
//                      kept for it is not BMX_VAL_DELETED. A contender finds its key's slot with PLAIN loads and, if its value equals the slot's extreme
//                      (minimum, or maximum with BMX_FIRST_DESC), lowers the slot's id word with one unsigned 64-bit atomicMin of ids[pos] (behind a relaxed
//                      look at the word: it only ever falls, so a contender that is not below it has nothing to add).
// k_first_finish     : k_group_finish's ranking of the occupied slots; if they fit, the record of each and, field-outer (the loop counter is the same in every
//                      lane), the cells of its node through agg_probe_ts. Every slot, id word and the state record go back to empty; the workgroup that
//                      finishes last writes `res`.
// k_first_clear      : the id words to BMX_FIRST_NO_NODE (new scratch, or a query that did not get as far as its last kernel).
//
// Why this is exact. Pass 1's contributions to a key are exactly the rows with sel && have_g, and those with have_m among them are what min / max and n see:
// the contenders. Pass 2 starts behind the end of pass 1 (two kernels on one stream), so every key word, every minimum and maximum is final and visible when it
// is read, and plain loads suffice: no word pass 2 reads is written by pass 2, except the id word, which is only ever lowered by atomicMin. The words gw / ow
// reproduce pass 1's (sel, have_g, gval, have_m, mval) per position bit for bit, since BMX_VAL_DELETED is no data value; the program is not evaluated again and
// nothing is probed again, so a merge cannot slip between the two passes' views even in principle (and none can: they are one entry point's launches). The
// contenders whose value equals the final extreme are exactly the candidates for "first" under (value, then id); atomicMin over their ids as unsigned words
// gives the smallest, whatever the order of the lanes: the answer does not depend on positions, grid, cache hits or shards. A query that overflowed resolves
// nothing (the state record says so, uniformly, at the kernel's start): its table may lack keys, and no record is written anyway. Otherwise the table holds
// every key and at most cap <= slots / 2 of them, so the plain walk ends at the key. No lane waits for another lane anywhere: the loops are the sweeps and
// the walks, each bounded by its table or column.
//
// The table is GroupScratch's (keys + AggRaw + GroupState: measure = order field) plus one id word per slot of FirstScratch; both follow the "clean" protocol.
#pragma once
#include "group_kernels.h"
#include "rows_kernels.h"
#include "../../include/bmx_first.h"

namespace bmx {

constexpr unsigned long long FIRST_NO_NODE = BMX_FIRST_NO_NODE;
constexpr int FIRST_THREADS = 256;
static_assert(FIRST_NO_NODE == EMPTY_ID, "a record without a node carries the id no node has");
static_assert(sizeof(bmx_first_rec) == 40 && sizeof(bmx_first_res) == 40, "the records of bmx_first.h");

struct FirstArgs {
  GroupArgs G;                                  // the table and its state; G.measure / G.m_src: the order field
  unsigned long long* idw;                      // one id word per slot
  long long* gw; long long* ow;                 // the words per index position (nullptr: the base column says it / the group word says it)
  uint32_t same, desc;                          // same: order field == group field, both probed: ONE probe, and the group word is the order word
};

struct FirstOut {
  const Slot* slots; uint64_t nslots;
  bmx_first_rec* out; int64_t* out_val; int64_t* out_ts; bmx_first_res* res;
  uint32_t nfields, with_ts;
  uint32_t field[ROWS_MAX_FIELDS];
};

// one row of pass 1, called by every lane of the wave (sel = false: the lane only keeps the wave's votes company); gs / os: the row's words for pass 2
template <class T, bool CLOCKS>
__device__ __forceinline__ void first_row(const PredWhere<T, true, CLOCKS>& P, const FirstArgs& F, bool sel, int64_t x, uint64_t pos, uint32_t lane, AggLane& Lt, AggLane& La,
                                          GroupLds& S, long long& gs, long long& os) {
  const GroupArgs& A = F.G;
  int64_t mval = x, gval = x;
  bool have_m = A.m_src == 0u, have_g = A.g_src == 0u;
  if (sel) {
    // (same: the order field is the group field, which has the one probe)
    where_two_fields(P, pos, A.g_src, A.group, gval, have_g, F.same ? AGG_SRC_NONE : A.m_src, A.measure, mval, have_m);
    if (F.same) { mval = gval; have_m = have_g; }
    group_lane_add(Lt, have_m, mval);
    if (!have_g) group_lane_add(La, have_m, mval);
  }
  gs = sel && have_g ? (long long)gval : VAL_DELETED;
  os = sel && have_m ? (long long)mval : VAL_DELETED;
  group_row_put(A, sel && have_g, gval, have_m, mval, lane, S);
}

// a lane's E words of one unit: whole 16-byte vectors (the scratch is padded to whole units)
template <int E>
__device__ __forceinline__ void first_store_unit(long long* w, uint64_t unit, const long long (&q)[E], bool nt) {
  typedef long long ll2 __attribute__((ext_vector_type(2)));
  ll2* p = reinterpret_cast<ll2*>(w + unit * E);
#pragma unroll
  for (int k = 0; k < E / 2; k++) {
    ll2 v; v.x = q[2 * k]; v.y = q[2 * k + 1];
    if (nt) __builtin_nontemporal_store(v, p + k); else p[k] = v;
  }
}

template <class T, bool CLOCKS>
__global__ __launch_bounds__(AGG_THREADS) void k_first_sweep(uint64_t n, PredWhere<T, true, CLOCKS> P, FirstArgs F) {
  constexpr int E = PredWhere<T>::E;
  typedef T vec_t __attribute__((ext_vector_type(E)));
  __shared__ GroupLds S;
  group_cache_begin(S);
  AggLane Lt, La;
  const uint32_t lane = threadIdx.x & 63u;
  top_sweep<T>(P.v, n, P.nt ? 1u : 0u, [&](uint64_t unit, const vec_t& x, uint32_t cnt) {
    long long gq[E], oq[E];                                             // (indexed by unrolled counters only: registers)
#pragma unroll
    for (int k = 0; k < E; k++) { gq[k] = VAL_DELETED; oq[k] = VAL_DELETED; }
    where_unit_rows<T>(P, unit, x, cnt, [&](int e, T xe, uint64_t pos, bool sel) {
      long long gs, os;
      first_row<T>(P, F, sel, (int64_t)xe, pos, lane, Lt, La, S, gs, os);
#pragma unroll
      for (int k = 0; k < E; k++) { gq[k] = e == k ? gs : gq[k]; oq[k] = e == k ? os : oq[k]; }
    });
    if (cnt) {                                                          // a unit of the column (its rows beyond the column: "no contender", inside the padding)
      if (F.gw) first_store_unit<E>(F.gw, unit, gq, P.nt);
      if (F.ow) first_store_unit<E>(F.ow, unit, oq, P.nt);
    }
  });
  group_cache_end(F.G, S, Lt, La);
}

// the words kept for index position i, as loaded (VAL_DELETED where none is kept): is it a contender, and if so its group value and its order value (from the
// words, and from the column where a field is the base)
template <class T>
__device__ __forceinline__ bool first_decode(const FirstArgs& F, const T* __restrict__ col, uint64_t i, long long& key, long long& val) {
  bool ok = true;
  if (F.gw) ok = key != VAL_DELETED;
  if (F.ow) ok = ok && val != VAL_DELETED;
  if (!ok) return false;
  if (!F.gw || (!F.ow && !F.same)) {                                    // (uniform) a selected row: its column value is data
    const long long c = (long long)col[i];
    if (!F.gw) key = c;
    if (!F.ow && !F.same) val = c;
  }
  if (F.same) val = key;
  return true;
}

// what pass 1 left of index position i
template <class T>
__device__ __forceinline__ bool first_contender(const FirstArgs& F, const T* __restrict__ col, uint64_t i, long long& key, long long& val) {
  key = VAL_DELETED; val = VAL_DELETED;
  if (F.gw) key = __builtin_nontemporal_load(F.gw + i);
  if (F.ow) val = __builtin_nontemporal_load(F.ow + i);
  return first_decode<T>(F, col, i, key, val);
}

// the slot of `key` in the FINISHED table, with plain loads (behind the end of pass 1; false cannot happen without the overflow bit)
__device__ __forceinline__ bool first_find(const GroupArgs& A, long long key, uint64_t& s) {
  const uint64_t mask = A.slots - 1u;
  s = group_mix(key) & mask;
  for (uint64_t p = 0; p < A.slots; ++p, s = (s + 1u) & mask) {
    const long long k = A.keys[s];
    if (k == key) return true;
    if (k == GROUP_EMPTY) break;
  }
  return false;
}

template <class T>
__global__ __launch_bounds__(FIRST_THREADS) void k_first_resolve(const T* __restrict__ col, const uint64_t* __restrict__ ids, uint64_t n, FirstArgs F) {
  const GroupArgs& A = F.G;
  if (A.S->overflow != 0u || A.S->claims > A.cap) return;              // (uniform) no records will be written, and the table may lack keys
  for (uint64_t i = (uint64_t)blockIdx.x * FIRST_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FIRST_THREADS) {
    long long key, val;
    if (!first_contender<T>(F, col, i, key, val)) continue;
    uint64_t s;
    if (!first_find(A, key, s)) continue;
    const long long ext = F.desc ? A.acc[s].mx : A.acc[s].mn;
    if (val != ext) continue;
    const unsigned long long id = ids[i];
    if (__hip_atomic_load(&F.idw[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > id) atomicMin(&F.idw[s], id);
  }
}

// n_is_match: every member had its order value (the order field is the base field): n = n_match. `slots` is a multiple of 64.
__global__ __launch_bounds__(256) void k_first_finish(FirstArgs F, FirstOut O, uint32_t n_is_match) {
  const GroupArgs& A = F.G;
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
      const bool w = occ && r < A.cap;
      unsigned long long id = FIRST_NO_NODE;
      if (w) {
        const AggRaw a = A.acc[s];
        bmx_first_rec o;
        o.key = k; o.n_match = a.nm; o.n = n_is_match ? a.nm : a.n;
        if (o.n) id = F.idw[s];
        o.id = id; o.val = o.n ? (F.desc ? a.mx : a.mn) : VAL_DELETED;
        O.out[r] = o;
      }
      for (uint32_t f = 0; f < O.nfields; f++) {                        // (uniform) field-outer: one probe in flight per lane and field
        int64_t x = VAL_DELETED, t = BMX_ROWS_NO_CLOCK;                 // what an absent row, or a record without a node, delivers
        if (w && id != FIRST_NO_NODE) agg_probe_ts(O.slots, O.nslots, id, O.field[f], x, t);
        if (w) {
          O.out_val[(uint64_t)f * A.cap + r] = x;
          if (O.with_ts) O.out_ts[(uint64_t)f * A.cap + r] = t;
        }
      }
    }
    if (occ) { A.keys[s] = GROUP_EMPTY; A.acc[s] = GROUP_RAW_EMPTY; F.idw[s] = FIRST_NO_NODE; }
  }
  if (last_workgroup(&S->done) && threadIdx.x == 0) {                   // no workgroup reads the state record any more
    bmx_first_res o;
    o.n_groups = claims; o.flags = fits ? 0u : BMX_FIRST_OVERFLOW; o.reserved = 0u;
    o.total = S->total.nm; o.absent = S->absent.nm; o.n_ordered = S->total.n - S->absent.n;
    *O.res = o;
    group_state_reset(S);
  }
}

__global__ __launch_bounds__(256) void k_first_clear(unsigned long long* __restrict__ idw, uint64_t slots) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256u) idw[s] = FIRST_NO_NODE;
}

}  // namespace bmx
