// gtop_kernels.h — the first N nodes per group (bmx_group_top.h bmx_where_group_top): per discovered key the first `per` contenders under the total order (order
// value, then id as an unsigned number) behind a boolean filter, gfx950, wave64. Pass 1 is first_kernels.h's k_first_sweep as it is: per key the table holds
// n_match, n and both extremes, per index position the words gw / ow say who contends and with what. Then the winners come out in ROUNDS, one rank per round and
// group, each round settled the way the first node is: there is no 128-bit atomic, so a round settles the value in one sweep and the id in the next, with kernel
// boundaries between them. The kernels work on ov = desc ? -val : val; data values lie in +-(2^53 - 1), so the negation is exact and every comparison ascends.
//
// Per slot (GtopScratch): the previous winner (pv, pid), at rest (INT64_MIN, 0); the round's extreme ext, at rest INT64_MAX; the rank counter, at rest 0; `per`
// winner pairs (read only below the rank counter, so they have no rest state); and FirstScratch's id word idw, at rest NO_NODE.
//
// round 0          : the extreme is in the table (mn, or mx with BMX_GTOP_DESC) and k_first_resolve lowers idw to the smallest id on it.
// k_gtop_value<T>  : rounds >= 1, a streaming sweep of the words k_first_resolve reads, two positions per 16-byte load (first_decode, first_find: plain
//                    loads). A contender STRICTLY AFTER its group's previous winner (ov > pv || (ov == pv && id > pid), ids unsigned) lowers ext[s] with one 64-bit atomicMin behind a
//                    relaxed look (the word only ever falls within the kernel).
// k_gtop_id<T>     : the same sweep; a contender strictly after the previous winner whose ov equals ext[s] lowers idw[s] with an unsigned 64-bit atomicMin.
// k_gtop_advance   : over slots. If idw[s] is not NO_NODE, (idw, ext) is the group's winner of this round: it is recorded at the rank counter, becomes the
//                    previous winner, the counter goes up and idw and ext go back to rest. It also counts the groups that got a node this round (given[round]).
// k_gtop_finish    : k_first_finish's ranking of the occupied slots; if they fit, the group record, the `per` rows (padded with {NO_NODE, VAL_DELETED}) and,
//                    field-outer, the cells of every row through agg_probe_ts. Every slot and all per-slot state go back to rest; the workgroup that finishes
//                    last writes `res` and puts the state records back.
// k_gtop_clear     : the per-slot state and the state record to rest (new scratch, or a query that did not get as far as its last kernel).
//
// Why this is exact.
// (1) Plain loads suffice. Each kernel starts behind the end of the one before it (one stream). What k_gtop_value reads (keys, pv, pid) was last written by an
//     earlier kernel (the sweep, k_gtop_advance) and is not written by it; the only word it writes, ext, it only lowers with atomicMin. k_gtop_id reads keys,
//     pv, pid and the FINAL ext of this round and only lowers idw. k_gtop_advance touches slot s from one lane only. The words gw / ow are pass 1's and are
//     never written again, so every round sees the same contenders with the same values; nothing is probed and no program is evaluated again.
// (2) Every contender is visited exactly once, ties included. The order (ov, id) is total on a group's contenders, since ids are distinct. By induction the
//     previous winner after round j - 1 is the group's j-th contender c_j under the order (round 0: the smallest id on the table's extreme, which is
//     k_first_resolve's argument). In round j the contenders strictly after c_j are exactly c_{j+1}, c_{j+2}, ...: ext becomes the smallest ov among them,
//     which is c_{j+1}'s, and among those with that ov (all after c_j: a tied node qualifies through id > pid, and an already delivered node never does, since
//     it is not after c_j) the smallest id is c_{j+1}'s. "Strictly" keeps c_j itself out; comparing the id on equal values keeps its ties in.
//     atomicMin is commutative, so lanes, grid, cache hits and shard layout do not matter.
// (3) An exhausted group stays exhausted. If no contender is after (pv, pid), nobody lowers ext, it stays INT64_MAX, which no ov equals, so idw stays NO_NODE
//     and k_gtop_advance leaves (pv, pid), the counter and the rest state alone: the next round finds the same nothing. A group without contenders never
//     leaves rest at all (k_first_resolve finds nobody on its extreme).
// A query that overflowed runs no round (the state record says so, uniformly, at each kernel's start), and a round in front of which no group got a node ends
// at once for the same kind of uniform reason (given[round - 1] == 0: by (3) nothing can follow): device mode enqueues all rounds blind. No lane waits for
// another lane: the loops are the sweeps, the walks and the loops over `per` and the fields.
#pragma once
#include "first_kernels.h"
#include "../../include/bmx_group_top.h"

namespace bmx {

constexpr unsigned long long GTOP_NO_NODE = BMX_GTOP_NO_NODE;
constexpr uint32_t GTOP_MAX_PER = BMX_GTOP_MAX_PER;
static_assert(GTOP_NO_NODE == FIRST_NO_NODE && GTOP_NO_NODE == EMPTY_ID, "a row without a node carries the id no node has: idw's rest state");
static_assert(sizeof(bmx_gtop_grp) == 32 && sizeof(bmx_gtop_row) == 16 && sizeof(bmx_gtop_res) == 48, "the records of bmx_group_top.h");
static_assert(BMX_GTOP_DESC == BMX_FIRST_DESC && BMX_GTOP_OVERFLOW == BMX_FIRST_OVERFLOW, "one flag word for both forms");

// the state record of one query beside GroupState; k_gtop_finish leaves it as k_gtop_clear does
struct GtopState {
  uint32_t given[GTOP_MAX_PER];                 // groups that got a node in round j; their sum is the number of rows with a node
};

struct GtopArgs {
  long long* pv; unsigned long long* pid;       // the previous winner per slot (ov, id)
  long long* ext;                               // the round's extreme per slot (ov)
  uint32_t* rank;                               // winners recorded per slot
  bmx_gtop_row* win;                            // slot s, rank j: win[s * per + j] (the value as the caller sees it)
  GtopState* T;
  uint32_t per;
};

struct GtopOut {
  const Slot* slots; uint64_t nslots;
  bmx_gtop_grp* out; bmx_gtop_row* out_rows; int64_t* out_val; int64_t* out_ts; bmx_gtop_res* res;
  uint32_t nfields, with_ts;
  uint32_t field[ROWS_MAX_FIELDS];
};

// is this query without rounds (it overflowed), or is round `round` >= 1 one that nothing can reach any more? (uniform)
__device__ __forceinline__ bool gtop_idle(const GroupArgs& A, const GtopArgs& G, uint32_t round) {
  return A.S->overflow != 0u || A.S->claims > A.cap || (round && G.T->given[round - 1u] == 0u);
}

// one position of a round's sweep, its words already loaded: a contender strictly after its group's previous winner lowers the round's extreme (value
// sweep; the id is loaded only where the values tie) or, if it is on the round's extreme, the id word (ID sweep)
template <class T, bool ID>
__device__ __forceinline__ void gtop_visit(const FirstArgs& F, const GtopArgs& G, const T* __restrict__ col, const uint64_t* __restrict__ ids, uint64_t i, long long key,
                                           long long val) {
  if (!first_decode<T>(F, col, i, key, val)) return;
  uint64_t s;
  if (!first_find(F.G, key, s)) return;
  const long long ov = F.desc ? -val : val;
  const long long pv = G.pv[s];
  if (ov < pv) return;
  unsigned long long id = 0ull;
  if (ID || ov == pv) id = ids[i];
  if (ov == pv && id <= G.pid[s]) return;
  if (ID) {
    if (ov != G.ext[s]) return;
    if (__hip_atomic_load(&F.idw[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > id) atomicMin(&F.idw[s], id);
  } else if (__hip_atomic_load(&G.ext[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > ov) atomicMin(&G.ext[s], ov);
}

// A round's sweep over the words. A lane reads the words of two neighbouring positions as one 16-byte vector (the scratch is padded to whole units of pass 1,
// so the second word of the last pair is inside it; a position beyond the column is not visited) and has the vectors of two such pairs in flight before it
// looks at any of them: the sweep is a chain of dependent loads per position, and what hides their latency is loads in flight. Neither the column nor the
// ids are read beyond n.
template <class T, bool ID>
__device__ __forceinline__ void gtop_sweep(const T* __restrict__ col, const uint64_t* __restrict__ ids, uint64_t n, const FirstArgs& F, const GtopArgs& G) {
  typedef long long ll2 __attribute__((ext_vector_type(2)));
  const uint64_t pairs = (n + 1u) >> 1, step = (uint64_t)gridDim.x * FIRST_THREADS;
  const ll2* gw = reinterpret_cast<const ll2*>(F.gw);
  const ll2* ow = reinterpret_cast<const ll2*>(F.ow);
  for (uint64_t q = (uint64_t)blockIdx.x * FIRST_THREADS + threadIdx.x; q < pairs; q += 2u * step) {
    ll2 g[2], o[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint64_t p = q + (uint64_t)h * step;
      g[h].x = VAL_DELETED; g[h].y = VAL_DELETED; o[h] = g[h];
      if (p < pairs) {
        if (gw) g[h] = __builtin_nontemporal_load(gw + p);
        if (ow) o[h] = __builtin_nontemporal_load(ow + p);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint64_t p = q + (uint64_t)h * step;
      if (p >= pairs) continue;
      gtop_visit<T, ID>(F, G, col, ids, 2u * p, g[h].x, o[h].x);
      if (2u * p + 1u < n) gtop_visit<T, ID>(F, G, col, ids, 2u * p + 1u, g[h].y, o[h].y);
    }
  }
}

template <class T>
__global__ __launch_bounds__(FIRST_THREADS) void k_gtop_value(const T* __restrict__ col, const uint64_t* __restrict__ ids, uint64_t n, FirstArgs F, GtopArgs G, uint32_t round) {
  if (gtop_idle(F.G, G, round)) return;
  gtop_sweep<T, false>(col, ids, n, F, G);
}

template <class T>
__global__ __launch_bounds__(FIRST_THREADS) void k_gtop_id(const T* __restrict__ col, const uint64_t* __restrict__ ids, uint64_t n, FirstArgs F, GtopArgs G, uint32_t round) {
  if (gtop_idle(F.G, G, round)) return;
  gtop_sweep<T, true>(col, ids, n, F, G);
}

// round 0 takes the extreme from the table, the others from ext. `slots` is a multiple of 64.
__global__ __launch_bounds__(256) void k_gtop_advance(FirstArgs F, GtopArgs G, uint32_t round) {
  const GroupArgs& A = F.G;
  if (gtop_idle(A, G, round)) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t mine = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < A.slots; s += (uint64_t)gridDim.x * 256u) {
    const unsigned long long id = F.idw[s];
    if (id == GTOP_NO_NODE) continue;
    const long long ov = round ? G.ext[s] : (F.desc ? -A.acc[s].mx : A.acc[s].mn);
    const uint32_t j = G.rank[s];
    bmx_gtop_row w; w.id = id; w.val = F.desc ? -ov : ov;
    if (j < G.per) G.win[s * G.per + j] = w;                            // (always: a group gets one node per round)
    G.pv[s] = ov; G.pid[s] = id; G.rank[s] = j + 1u;
    F.idw[s] = GTOP_NO_NODE; G.ext[s] = INT64_MAX;
    mine++;
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d);
  if (lane == 0u && mine) atomicAdd(&G.T->given[round], mine);
}

// n_is_match: every member had its order value (the order field is the base field): n = n_match. `slots` is a multiple of 64.
__global__ __launch_bounds__(256) void k_gtop_finish(FirstArgs F, GtopArgs G, GtopOut O, uint32_t n_is_match) {
  const GroupArgs& A = F.G;
  GroupState* S = A.S;
  const unsigned long long claims = S->claims;
  const bool fits = claims <= A.cap && S->overflow == 0u;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t per = G.per;
  for (uint64_t b = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); b < A.slots; b += (uint64_t)gridDim.x * 256u) {
    const uint64_t s = b + lane;
    const long long k = A.keys[s];
    const bool occ = k != GROUP_EMPTY;
    if (!__ballot(occ)) continue;                                       // (uniform)
    if (fits) {
      const unsigned long long r = wave_rank(occ, &S->nout, lane);
      const bool w = occ && r < A.cap;
      uint32_t nr = 0;
      if (w) {
        const AggRaw a = A.acc[s];
        nr = min(G.rank[s], G.per);                                     // (a group gets one node per round: never above per)
        bmx_gtop_grp o;
        o.key = k; o.n_match = a.nm; o.n = n_is_match ? a.nm : a.n; o.n_rows = nr;
        O.out[r] = o;
      }
      for (uint32_t j = 0; j < G.per; j++) {                            // (uniform) one row per lane and step
        bmx_gtop_row x; x.id = GTOP_NO_NODE; x.val = VAL_DELETED;
        if (w && j < nr) x = G.win[s * per + j];
        if (w) O.out_rows[r * per + j] = x;
      }
      for (uint32_t f = 0; f < O.nfields; f++) {                        // (uniform) field-outer: one probe in flight per lane, field and row
        for (uint32_t j = 0; j < G.per; j++) {
          int64_t v = VAL_DELETED, t = BMX_ROWS_NO_CLOCK;               // what an absent row, or a row without a node, delivers
          if (w && j < nr) agg_probe_ts(O.slots, O.nslots, G.win[s * per + j].id, O.field[f], v, t);
          if (w) {
            const uint64_t at = (uint64_t)f * A.cap * per + r * per + j;
            O.out_val[at] = v;
            if (O.with_ts) O.out_ts[at] = t;
          }
        }
      }
    }
    if (occ) {
      A.keys[s] = GROUP_EMPTY; A.acc[s] = GROUP_RAW_EMPTY; F.idw[s] = GTOP_NO_NODE;
      G.pv[s] = INT64_MIN; G.pid[s] = 0ull; G.ext[s] = INT64_MAX; G.rank[s] = 0u;
    }
  }
  if (last_workgroup(&S->done) && threadIdx.x == 0) {                   // no workgroup reads the state records any more
    bmx_gtop_res o;
    o.n_groups = claims; o.flags = fits ? 0u : BMX_GTOP_OVERFLOW; o.per = G.per;
    o.total = S->total.nm; o.absent = S->absent.nm; o.n_ordered = S->total.n - S->absent.n;
    o.n_rows = 0ull;                                                    // the rounds' counts, final since the last k_gtop_advance (none ran on overflow: 0)
    for (uint32_t j = 0; j < GTOP_MAX_PER; j++) { o.n_rows += G.T->given[j]; G.T->given[j] = 0u; }
    *O.res = o;
    group_state_reset(S);
  }
}

__global__ __launch_bounds__(256) void k_gtop_clear(GtopArgs G, uint64_t slots) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256u) {
    G.pv[s] = INT64_MIN; G.pid[s] = 0ull; G.ext[s] = INT64_MAX; G.rank[s] = 0u;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (uint32_t j = 0; j < GTOP_MAX_PER; j++) G.T->given[j] = 0u;
}

}  // namespace bmx
