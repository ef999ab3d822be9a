// mgroup_kernels.h — group-by over several fields (bmx_group_multi.h bmx_where_group_multi): group_kernels.h's hash aggregation keyed by a tuple of up to four
// values, each optionally bucketed, gfx950, wave64.
//
// k_mgroup_sweep<T> : k_group_sweep's sweep (one read of the base field's value column, PredWhere::row() decides the candidates). A selected row's key values
//                     are the column value when the field is the base field, otherwise one agg_probe each, made after the match is known; a row that lacks
//                     ANY of them goes to `absent` and touches no table. Every other row turns each value into a CODE through that key's dictionary, packs
//                     the codes into one word and is aggregated under that word by group_kernels.h's own machinery (group_row_put: the wave-level dedupe of
//                     the first lane's word; group_put: the LDS cache of 256 x 4 ways and the bypass; group_slot) in a tuple table of this call's own scratch.
// k_mgroup_finish   : k_group_finish over the tuple table. A record's keys are read back through the dictionaries: dict_j[code_j]. Every tuple slot goes back
//                     to its empty state; the workgroup that finishes last writes `res` and puts the tuple table's state record back.
// k_mgroup_clear    : the dictionaries and their state records to their empty state BEHIND the finish, which reads them (slots == 0); everything (new
//                     scratch, or a query that did not get as far as its last kernel) with the tuple table's slot count.
//
// Why dictionaries. k_group_sweep claims a slot with one 64-bit atomicCAS on the key word, which is why any lane may add into a slot the moment it sees its key
// there. A tuple of up to four 64-bit values cannot be claimed by one CAS, and a slot claimed by a first word and completed by further ones would make every
// other lane wait for the rest. So each key j has an open-addressed table dict_j of `slots` key words (slots = max(64, next power of two >= 2 * cap), the tuple
// table's size) with group_slot's find-or-claim, called as it stands on a GroupArgs that names dict_j and its own state record: relaxed agent-scope load, one
// CAS, linear probing with wrap, the give-up at every 64th step once that dictionary's claims exceed cap. The code of a value is the INDEX of the slot it ends
// up in: it is known to every lane the moment it sees the value there, so there is no second word to publish and nothing to wait for. A field has at most D
// distinct values among the rows that have every key (only those rows reach a dictionary), so a dictionary without room means D > cap: the overflow bit of its
// state record goes up and the row is dropped from the groups (it still counts in `total`).
// The packed word is sum of code_j << (j * log2 slots): 3 * 21 = 63 bits with cap <= 2^20, 4 * 15 = 60 bits with four keys and cap <= 2^14 (the cap rule of the
// header). It is never negative, hence never GROUP_EMPTY, and within one query it is injective on tuples: a value has exactly one slot in its dictionary.
// No lane waits for, or spins on, a word another lane must write; the only loops are group_slot's walks, bounded by `slots`.
//
// The bucket of a value is floor((v - origin) / width), toward minus infinity. width == 1 (uniform per key) takes no division. |v|, |origin| <= 2^53 - 1, so
// the difference cannot wrap and no key is GROUP_EMPTY.
#pragma once
#include "group_kernels.h"
#include "../../include/bmx_group_multi.h"

namespace bmx {

constexpr uint32_t MGROUP_KEYS = BMX_MGROUP_MAX_KEYS;
static_assert(sizeof(bmx_mgroup_rec) == 80 && sizeof(bmx_group_key) == 24, "the records of bmx_group_multi.h");
static_assert(MGROUP_KEYS == 4, "mgroup_row keeps the key values in four named registers");

struct MGroupKey { long long origin, width; uint32_t field, src; };   // src: 0 = the base field's column, AGG_SRC_PROBE = one probe of `field`

struct MGroupArgs {
  GroupArgs T;                                 // the tuple table and its state record; measure / m_src as in k_group_sweep (group / g_src are not read)
  long long* dict;                             // dictionary j: dict + j * T.slots
  GroupState* DS;                              // dictionary j's state record: DS + j (claims and overflow; the rest stays empty)
  uint32_t nkeys, shift;                       // shift = log2 T.slots
  MGroupKey k[MGROUP_KEYS];
};

// The workgroup's LDS: group_kernels.h's cache of partials under the packed word, and per key a direct-mapped, INSERT-ONLY cache value -> code of
// MGROUP_DSETS entries (12 KB for the four). A dictionary lookup is a round trip to L2 behind the probe's miss, and at low selectivity a wave's row step is
// that chain of latencies; a value the workgroup has met takes its code from LDS instead. The entry of a value is group_set(value). The first value to claim
// an entry (one CAS on the value word) keeps it for the workgroup's life and publishes its code with a second store; an entry whose code word is not yet
// written, or that holds another value, is a MISS (the lane asks the dictionary), never a wait. The only code ever stored beside a value is that value's.
constexpr uint32_t MGROUP_DSETS = GROUP_SETS, MGROUP_NOCODE = 0xFFFFFFFFu;
struct MGroupLds {
  GroupLds G;
  long long dval[MGROUP_KEYS * MGROUP_DSETS];
  uint32_t dcode[MGROUP_KEYS * MGROUP_DSETS];
};

// value -> code of key j: the LDS cache, else group_slot on the key's dictionary (false: no room, that dictionary's overflow bit is up)
__device__ __forceinline__ bool mgroup_code(const GroupArgs& D, MGroupLds& S, uint32_t j, long long v, uint64_t& code) {
  const uint32_t e = j * MGROUP_DSETS + group_set(v);
  long long cv = __hip_atomic_load(&S.dval[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (cv == v) {
    const uint32_t cc = __hip_atomic_load(&S.dcode[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cc != MGROUP_NOCODE) { code = cc; return true; }
  }
  if (!group_slot(D, v, code)) return false;
  if (cv == GROUP_EMPTY) {
    cv = (long long)atomicCAS(reinterpret_cast<unsigned long long*>(&S.dval[e]), (unsigned long long)GROUP_EMPTY, (unsigned long long)v);
    if (cv == GROUP_EMPTY) __hip_atomic_store(&S.dcode[e], (uint32_t)code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  return true;
}

__device__ __forceinline__ long long mgroup_bucket(long long v, long long origin, long long width) {
  const long long d = v - origin;
  if (width == 1) return d;                    // (uniform)
  long long q = d / width;
  if (d - q * width < 0) --q;                  // C++ truncates toward zero: one down where the remainder is negative
  return q;
}

// one row of the sweep, called by every lane of the wave (sel = false: the lane only keeps the wave's votes company)
template <class T, bool CLOCKS>
__device__ __forceinline__ void mgroup_row(const PredWhere<T, true, CLOCKS>& P, const MGroupArgs& A, bool sel, int64_t x, uint64_t pos, uint32_t lane, AggLane& Lt, AggLane& La, MGroupLds& S) {
  int64_t mval = x;
  long long k0 = 0, k1 = 0, k2 = 0, k3 = 0;
  bool have_m = A.T.m_src == 0u, have_g = true;
  if (sel) {
    // the keys (j < nkeys) and the measure (j == nkeys) through ONE copy of the probe (where_field); the values stay in named registers
#pragma unroll 1
    for (uint32_t j = 0; j <= A.nkeys; j++) {
      const bool is_m = j == A.nkeys;
      const uint32_t src = is_m ? A.T.m_src : A.k[j & 3u].src;        // (uniform)
      int64_t y = x;
      const bool have = where_field(P, pos, src, is_m ? A.T.measure : A.k[j & 3u].field, y);
      if (is_m) { if (src == AGG_SRC_PROBE && have) { mval = y; have_m = true; } continue; }
      if (!have) { have_g = false; continue; }
      const long long b = mgroup_bucket((long long)y, A.k[j].origin, A.k[j].width);
      k0 = j == 0u ? b : k0; k1 = j == 1u ? b : k1; k2 = j == 2u ? b : k2; k3 = j == 3u ? b : k3;
    }
    group_lane_add(Lt, have_m, mval);
    if (!have_g) group_lane_add(La, have_m, mval);
  }
  bool go = sel && have_g;
  if (!__ballot(go)) return;                                           // (uniform)
  // value -> code, key by key: only a row that has every key reaches a dictionary, so a dictionary never holds more values than there are tuples
  unsigned long long word = 0ull;
#pragma unroll 1
  for (uint32_t j = 0; j < A.nkeys; j++) {
    if (!go) continue;
    GroupArgs D{};
    D.keys = A.dict + (uint64_t)j * A.T.slots; D.S = A.DS + j; D.slots = A.T.slots; D.cap = A.T.cap;
    const long long v = j == 0u ? k0 : (j == 1u ? k1 : (j == 2u ? k2 : k3));
    uint64_t code;
    if (mgroup_code(D, S, j, v, code)) word |= (unsigned long long)code << (j * A.shift);
    else go = false;                                                   // (that dictionary's overflow bit is up)
  }
  group_row_put(A.T, go, (int64_t)word, have_m, mval, lane, S.G);      // (rows of one wave often share a tuple)
}

template <class T, bool CLOCKS>
__global__ __launch_bounds__(AGG_THREADS) void k_mgroup_sweep(uint64_t n, PredWhere<T, true, CLOCKS> P, MGroupArgs A) {
  __shared__ MGroupLds S;
  for (uint32_t e = threadIdx.x; e < MGROUP_KEYS * MGROUP_DSETS; e += AGG_THREADS) { S.dval[e] = GROUP_EMPTY; S.dcode[e] = MGROUP_NOCODE; }
  group_cache_begin(S.G);
  AggLane Lt, La;
  const uint32_t lane = threadIdx.x & 63u;
  where_sweep<T>(n, P, [&](int, T xe, uint64_t pos, bool sel) { mgroup_row<T>(P, A, sel, (int64_t)xe, pos, lane, Lt, La, S); });
  group_cache_end(A.T, S.G, Lt, La);
}

// k_group_finish over the tuple table; the keys of a record come back through the dictionaries. n_is_match and the wave / slots rule as there.
__global__ __launch_bounds__(256) void k_mgroup_finish(MGroupArgs A, bmx_mgroup_rec* __restrict__ out, bmx_group_res* __restrict__ res, uint32_t n_is_match) {
  GroupState* S = A.T.S;
  unsigned long long claims = S->claims, most = claims;
  bool fits = claims <= A.T.cap && S->overflow == 0u;
  for (uint32_t j = 0; j < A.nkeys; j++) {                              // (nobody writes the dictionaries' records in this kernel)
    const unsigned long long c = A.DS[j].claims;
    fits = fits && A.DS[j].overflow == 0u;
    most = c > most ? c : most;
  }
  // an overflow: the largest lower bound of D at hand (a field has at most D values). It is above cap: a walk gives up only in a full table or behind cap claims.
  if (!fits) claims = most;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t cmask = A.T.slots - 1u;
  for (uint64_t b = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); b < A.T.slots; b += (uint64_t)gridDim.x * 256u) {
    const uint64_t s = b + lane;
    const long long w = A.T.keys[s];
    const bool occ = w != GROUP_EMPTY;
    if (!__ballot(occ)) continue;                                       // (uniform)
    if (fits) {
      const unsigned long long r = wave_rank(occ, &S->nout, lane);
      if (occ && r < A.T.cap) {
        bmx_mgroup_rec o;
#pragma unroll
        for (uint32_t j = 0; j < MGROUP_KEYS; j++)
          o.key[j] = j < A.nkeys ? A.dict[(uint64_t)j * A.T.slots + (((uint64_t)w >> (j * A.shift)) & cmask)] : 0ll;
        o.agg = group_compose(A.T.acc[s], n_is_match);
        out[r] = o;
      }
    }
    if (occ) { A.T.keys[s] = GROUP_EMPTY; A.T.acc[s] = GROUP_RAW_EMPTY; }
  }
  if (last_workgroup(&S->done) && threadIdx.x == 0) {                   // no workgroup reads the state record any more
    bmx_group_res o;
    o.n_groups = claims; o.flags = fits ? 0u : BMX_GROUP_OVERFLOW; o.reserved = 0u;
    o.absent = group_compose(S->absent, n_is_match); o.total = group_compose(S->total, n_is_match);
    *res = o;
    group_state_reset(S);
  }
}

// dict_words words of dictionaries and their MGROUP_KEYS state records; with slots != 0 the tuple table and its state record too
__global__ __launch_bounds__(256) void k_mgroup_clear(long long* __restrict__ dict, uint64_t dict_words, GroupState* __restrict__ DS, long long* __restrict__ keys,
                                                      AggRaw* __restrict__ acc, uint64_t slots, GroupState* __restrict__ S) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x, step = (uint64_t)gridDim.x * 256u;
  for (uint64_t s = t; s < dict_words; s += step) dict[s] = GROUP_EMPTY;
  for (uint64_t s = t; s < slots; s += step) { keys[s] = GROUP_EMPTY; acc[s] = GROUP_RAW_EMPTY; }
  if (t <= MGROUP_KEYS) {
    GroupState* R = t < MGROUP_KEYS ? DS + t : S;
    if (t < MGROUP_KEYS || slots) group_state_reset(R);
  }
}

}  // namespace bmx
