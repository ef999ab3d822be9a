// top_kernels.h — ordered, limited queries (bmx_top.h bmx_scan_top): the first k nodes, in (value, id) order behind a keyset cursor, of the nodes a declarative
// filter selects, gfx950.
//
// The selection is bmx_scan_filter's (term 0 on the index column, the other terms probed in the table). What differs is the end: no match list exists at any
// point. An exact radix select over the composite key (order-preserving key of the value, then the node id) finds the boundary of the first k eligible rows in
// sweeps of term 0's value column, one more sweep compacts the rows up to that boundary (at most TOP_CAND of them) and one workgroup sorts them.
//
// k_top_sweep0<T, PROBE> : pass 0. Counts the eligible rows and takes the minimum and maximum of their keys. PROBE = true (more than one term): probes the other
//                          terms and leaves one bit per index position (eligible or not) in the scans' mask scratch; every later pass reads that bit and probes
//                          nothing. PROBE = false is the single-term form: no probe code, and the id column is read only for rows whose value equals the cursor's.
// k_top_init             : the select's state from what pass 0 found. Done at once when every eligible row fits the candidate list.
// k_top_digit<T, PROBE>  : one digit (TOP_DIGIT_BITS bits) of the rows that share the prefix found so far: LDS histogram per workgroup (a wave whose rows all fall
//                          into one bin adds once), one no-return global atomic per non-empty bin and workgroup. Digits run over the value first, then over the id.
// k_top_find             : the bin that holds the row of rank k; prefix, rows below, done flag; clears the histogram.
// k_top_compact<T, PROBE>: every eligible row at or below the boundary -> {key, id}, ranked by wave ballot + popcount into one counter (wave_rank, which
//                          every finish and export kernel of the where family ranks with too).
// k_top_finish           : one workgroup, bitonic sort of the candidates in LDS, the first min(k, n_eligible) records with the key turned back into the value, the
//                          two counts, and the state left ready for the next query.
// Every pass behind "done" returns after reading the state record, so the host enqueues the worst-case chain and nothing comes back between the passes.
//
// The key of a value: u = (uint64)v ^ 2^63 (order-preserving), ~u with BMX_TOP_DESC. The digits run over u - min(u) (the minimum of the eligible rows, from pass 0):
// a field that holds -5..1000 has 10 digit bits, wherever its values sit in the 54-bit domain and whether or not they straddle zero.
#pragma once
#include "select.h"
#include "scan_kernels.h"
#include "agg_kernels.h"
#include "../../include/bmx_top.h"

namespace bmx {

constexpr int TOP_THREADS = 512;
constexpr int TOP_WAVES = TOP_THREADS / 64;
constexpr int TOP_U = 4;                          // 16-byte loads of the value column a lane has in flight
constexpr uint32_t TOP_DIGIT_BITS = 11;
constexpr uint32_t TOP_BINS = 1u << TOP_DIGIT_BITS;   // 8 KB of LDS per workgroup
constexpr uint32_t TOP_CAND = 4096;               // candidate capacity: k_top_finish sorts them in 64 KB of LDS
constexpr int TOP_SORT_THREADS = 1024;
static_assert(TOP_CAND >= BMX_TOP_MAX_K, "every answer fits the candidate list");
static_assert((TOP_CAND & (TOP_CAND - 1)) == 0, "the bitonic network wants a power of two");

// the select's state, in device memory; every query's last kernel leaves it as k_top_clear does
struct TopState {
  unsigned long long n_elig, kmin, kmax;          // pass 0: eligible rows, smallest and largest key among them
  unsigned long long kk;                          // min(k, n_elig): the rank looked for
  unsigned long long below;                       // rows known to lie below the current prefix
  unsigned long long pre, vfix;                   // the prefix in the current word (right-aligned); phase 1: the whole value word (key - kmin) the ids are told apart under
  unsigned long long ncand;                       // k_top_compact's counter
  uint32_t sh;                                    // bits of the current word not decided yet
  uint32_t phase;                                 // 0: value digits, 1: id digits
  uint32_t done, all;                             // all: every eligible row is a candidate
  uint32_t hist[TOP_BINS];
};

struct TopArgs {
  const uint64_t* ids;
  uint32_t* mask;                                 // PROBE: one bit per index position (written by pass 0, read behind it)
  const Slot* slots; uint64_t nslots;
  TopState* S;
  int64_t lo, hi;                                 // term 0, clamped as the scans clamp it
  unsigned long long au, aid; uint32_t has_after; // the cursor: key of its value, its id
  uint32_t desc;
  uint32_t nterms; bmx_term t[MAX_TERMS];         // t[k].lo >= -VAL_MAX: a tombstone matches no term
};

__device__ __forceinline__ unsigned long long top_key(int64_t v, uint32_t desc) {
  const unsigned long long u = (unsigned long long)v ^ 0x8000000000000000ull;
  return desc ? ~u : u;
}
__device__ __forceinline__ int64_t top_val(unsigned long long u, uint32_t desc) { return (int64_t)((desc ? ~u : u) ^ 0x8000000000000000ull); }

// One read of a value column: f(unit, x, cnt) for every 16-byte unit, cnt = rows of the unit that exist (the ragged last unit is loaded row by row). Every lane
// of a workgroup makes the same number of calls (cnt == 0 beyond the column), so f may use ballots and shuffles.
template <class T, class F>
__device__ __forceinline__ void top_sweep(const T* __restrict__ col, uint64_t n, uint32_t nt, F&& f) {
  constexpr int E = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(E)));
  const uint64_t nv = n / E, nu = (n + E - 1) / E;
  for (uint64_t b = (uint64_t)blockIdx.x * (TOP_THREADS * TOP_U); b < nu; b += (uint64_t)gridDim.x * (TOP_THREADS * TOP_U)) {
    vec_t x[TOP_U];
#pragma unroll
    for (int u = 0; u < TOP_U; u++) {
      const uint64_t i = b + (uint64_t)u * TOP_THREADS + threadIdx.x;
      const vec_t z = {};
      x[u] = z;
      if (i < nv) x[u] = nt ? __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(col) + i) : reinterpret_cast<const vec_t*>(col)[i];
      else if (i < nu) {
#pragma unroll
        for (int e = 0; e < E; e++) if (i * E + e < n) x[u][e] = col[i * E + e];
      }
    }
#pragma unroll
    for (int u = 0; u < TOP_U; u++) {
      const uint64_t i = b + (uint64_t)u * TOP_THREADS + threadIdx.x;
      const uint32_t cnt = i < nv ? (uint32_t)E : (i < nu ? (uint32_t)(n - nv * E) : 0u);
      f(i, x[u], cnt);
    }
  }
}

// Wave-ranked compaction, called by all 64 lanes of a wave of which at least one has occ set: lane 0 takes the wave's popcount out of `counter` with one
// atomic, and a lane with occ set gets that base plus the occ lanes below it (the others: a rank nobody uses).
__device__ __forceinline__ unsigned long long wave_rank(bool occ, unsigned long long* counter, uint32_t lane) {
  const unsigned long long bal = __ballot(occ);
  unsigned long long base = 0;
  if (lane == 0u) base = atomicAdd(counter, (unsigned long long)__popcll(bal));
  base = __shfl(base, 0);
  return base + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
}

// behind the cursor? (id_known: the caller has the row's id already)
__device__ __forceinline__ bool top_after(const TopArgs& A, unsigned long long u, uint64_t pos, bool id_known, uint64_t id) {
  if (!A.has_after) return true;
  if (u != A.au) return u > A.au;
  return (id_known ? id : A.ids[pos]) > A.aid;
}
// eligibility of row `pos` behind pass 0. E bits of the unit's rows come from the mask in the PROBE form.
template <bool PROBE>
__device__ __forceinline__ bool top_elig(const TopArgs& A, int64_t v, unsigned long long u, uint64_t pos, uint32_t bits, int e) {
  if (PROBE) return (bits >> e) & 1u;
  return v >= A.lo && v <= A.hi && top_after(A, u, pos, false, 0);
}
template <int E>
__device__ __forceinline__ uint32_t top_mask_bits(const TopArgs& A, uint64_t unit, uint32_t cnt) {
  if (!cnt) return 0u;
  const uint64_t first = unit * E;
  return (A.mask[first >> 5] >> (uint32_t)(first & 31u)) & ((1u << E) - 1u);
}

template <class T, bool PROBE>
__global__ __launch_bounds__(TOP_THREADS) void k_top_sweep0(const T* __restrict__ col, uint64_t n, uint32_t nt, TopArgs A) {
  constexpr int E = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(E)));
  __shared__ unsigned long long s_n[TOP_WAVES], s_mn[TOP_WAVES], s_mx[TOP_WAVES];
  unsigned long long cnt_l = 0, mn = ~0ull, mx = 0ull;
  const uint64_t nu = (n + E - 1) / E;
  top_sweep<T>(col, n, nt, [&](uint64_t unit, const vec_t& x, uint32_t cnt) {
    uint32_t nib = 0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int64_t v = (int64_t)x[e];
      bool ok = (uint32_t)e < cnt && v >= A.lo && v <= A.hi;
      const unsigned long long u = top_key(v, A.desc);
      if (PROBE) {
        if (ok) {
          const uint64_t id = A.ids[unit * E + e];
          for (uint32_t k = 1; k < A.nterms && ok; k++) {
            int64_t y;
            ok = agg_probe(A.slots, A.nslots, id, A.t[k].field, y) && y >= A.t[k].lo && y <= A.t[k].hi;
          }
          ok = ok && top_after(A, u, 0, true, id);
        }
        nib |= (uint32_t)ok << e;
      } else ok = ok && top_after(A, u, unit * E + e, false, 0);
      if (ok) { cnt_l++; mn = u < mn ? u : mn; mx = u > mx ? u : mx; }
    }
    if (PROBE) {   // 32 / E consecutive lanes hold one mask word (a unit index is a multiple of 32 / E where a lane index is)
      constexpr uint32_t L = 32 / E;
      uint32_t w = nib << (E * (threadIdx.x & (L - 1)));
#pragma unroll
      for (uint32_t d = 1; d < L; d <<= 1) w |= __shfl_xor(w, d);
      if ((threadIdx.x & (L - 1)) == 0 && unit < nu) A.mask[unit / L] = w;
    }
  });
  for (int d = 32; d >= 1; d >>= 1) {
    cnt_l += __shfl_xor(cnt_l, d);
    const unsigned long long a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
    mn = a < mn ? a : mn; mx = b > mx ? b : mx;
  }
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) { s_n[w] = cnt_l; s_mn[w] = mn; s_mx[w] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long c = 0, a = ~0ull, b = 0ull;
#pragma unroll
    for (int i = 0; i < TOP_WAVES; i++) { c += s_n[i]; a = s_mn[i] < a ? s_mn[i] : a; b = s_mx[i] > b ? s_mx[i] : b; }
    if (c) { atomicAdd(&A.S->n_elig, c); atomicMin(&A.S->kmin, a); atomicMax(&A.S->kmax, b); }
  }
}

__global__ void k_top_init(TopState* __restrict__ S, uint32_t k) {
  if (threadIdx.x || blockIdx.x) return;
  const unsigned long long n = S->n_elig;
  S->kk = n < k ? n : (unsigned long long)k;
  S->below = 0; S->ncand = 0; S->pre = 0; S->vfix = 0;
  if (n <= TOP_CAND) { S->all = 1u; S->done = 1u; S->phase = 0u; S->sh = 0u; return; }
  const unsigned long long d = S->kmax - S->kmin;
  S->all = 0u; S->done = 0u;
  if (d) { S->phase = 0u; S->sh = 64u - (uint32_t)__clzll((long long)d); }     // every eligible row has (key - kmin) >> sh == 0
  else { S->phase = 1u; S->sh = 64u; }                                         // one value: the ids decide, under the value word 0
}

template <class T, bool PROBE>
__global__ __launch_bounds__(TOP_THREADS) void k_top_digit(const T* __restrict__ col, uint64_t n, uint32_t nt, TopArgs A) {
  constexpr int E = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(E)));
  __shared__ uint32_t h[TOP_BINS];
  const TopState* S = A.S;
  if (S->done) return;
  const uint32_t phase = S->phase, sh = S->sh;
  const unsigned long long pre = S->pre, vfix = S->vfix, kmin = S->kmin;
  const uint32_t w = sh < TOP_DIGIT_BITS ? sh : TOP_DIGIT_BITS, nsh = sh - w;
  for (uint32_t b = threadIdx.x; b < TOP_BINS; b += TOP_THREADS) h[b] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  top_sweep<T>(col, n, nt, [&](uint64_t unit, const vec_t& x, uint32_t cnt) {
    const uint32_t bits = PROBE ? top_mask_bits<E>(A, unit, cnt) : 0u;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int64_t v = (int64_t)x[e];
      const uint64_t pos = unit * E + e;
      const unsigned long long u = top_key(v, A.desc);
      bool ok = (uint32_t)e < cnt && top_elig<PROBE>(A, v, u, pos, bits, e);
      unsigned long long word = u - kmin;
      if (ok) {
        if (phase == 0u) ok = sh >= 64u || (word >> sh) == pre;
        else if ((ok = word == vfix)) { word = A.ids[pos]; ok = sh >= 64u || (word >> sh) == pre; }
      }
      const uint32_t d = (uint32_t)(word >> nsh) & ((1u << w) - 1u);
      // rows that share a prefix often share the digit too: the lanes that hold the first one's digit add once
      const unsigned long long bal = __ballot(ok);
      if (bal) {
        const int first = __ffsll((long long)bal) - 1;
        const uint32_t d0 = __shfl(d, first);
        const unsigned long long same = __ballot(ok && d == d0);
        if ((int)lane == first) atomicAdd(&h[d0], (uint32_t)__popcll(same));
        else if (ok && d != d0) atomicAdd(&h[d], 1u);
      }
    }
  });
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < TOP_BINS; b += TOP_THREADS) {
    const uint32_t c = h[b];
    if (c) atomicAdd(&A.S->hist[b], c);
  }
}

__global__ __launch_bounds__(SEL_THREADS) void k_top_find(TopState* __restrict__ S) {
  __shared__ uint32_t wsum[4];
  static_assert(TOP_BINS == 8 * SEL_THREADS, "eight bins per thread");
  if (S->done) return;
  const uint32_t phase = S->phase, sh = S->sh;
  const uint32_t w = sh < TOP_DIGIT_BITS ? sh : TOP_DIGIT_BITS;
  uint32_t nsh = sh - w;
  const unsigned long long below = S->below, pre = S->pre;
  const unsigned long long r = S->kk - below;            // 1 .. rows that share the prefix
  uint32_t hb[8], s = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) { hb[j] = S->hist[threadIdx.x * 8 + j]; s += hb[j]; S->hist[threadIdx.x * 8 + j] = 0u; }
  uint32_t tot;
  const uint32_t off = block_excl_scan(s, tot, wsum);    // (fewer than 2^32 rows in an index)
  if ((unsigned long long)off < r && r <= (unsigned long long)off + s) {
    unsigned long long c = off; uint32_t bin = threadIdx.x * 8, in_bin = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (r <= c + hb[j]) { bin = threadIdx.x * 8 + j; in_bin = hb[j]; break; }
      c += hb[j];
    }
    const unsigned long long nb = below + c, np = (pre << w) | bin;
    S->below = nb; S->pre = np;
    uint32_t done = nb + in_bin <= TOP_CAND ? 1u : 0u;
    if (!done && nsh == 0u) {
      if (phase == 0u) { S->phase = 1u; S->vfix = np; S->pre = 0; nsh = 64u; }
      else done = 1u;                                    // (unreachable: the composite key is unique, the bin of a whole key holds one row)
    }
    S->sh = nsh; S->done = done;
  }
}

template <class T, bool PROBE>
__global__ __launch_bounds__(TOP_THREADS) void k_top_compact(const T* __restrict__ col, uint64_t n, uint32_t nt, TopArgs A, unsigned long long* __restrict__ cand_u,
                                                             unsigned long long* __restrict__ cand_id) {
  constexpr int E = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(E)));
  TopState* S = A.S;
  if (S->n_elig == 0) return;
  const uint32_t all = S->all, phase = S->phase, sh = S->sh;
  const unsigned long long pre = S->pre, vfix = S->vfix, kmin = S->kmin;
  const uint32_t lane = threadIdx.x & 63u;
  top_sweep<T>(col, n, nt, [&](uint64_t unit, const vec_t& x, uint32_t cnt) {
    const uint32_t bits = PROBE ? top_mask_bits<E>(A, unit, cnt) : 0u;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int64_t v = (int64_t)x[e];
      const uint64_t pos = unit * E + e;
      const unsigned long long u = top_key(v, A.desc);
      bool ok = (uint32_t)e < cnt && top_elig<PROBE>(A, v, u, pos, bits, e);
      if (ok && !all) {
        const unsigned long long word = u - kmin;
        if (phase == 0u) ok = sh >= 64u || (word >> sh) <= pre;
        else if (word != vfix) ok = word < vfix;
        else ok = sh >= 64u || (A.ids[pos] >> sh) <= pre;
      }
      if (__ballot(ok)) {                                      // (uniform)
        const unsigned long long at = wave_rank(ok, &S->ncand, lane);
        if (ok && at < TOP_CAND) { cand_u[at] = u; cand_id[at] = A.ids[pos]; }
      }
    }
  });
}

__device__ __forceinline__ void top_state_reset(TopState* S) {
  S->n_elig = 0; S->kmin = ~0ull; S->kmax = 0; S->kk = 0; S->below = 0; S->pre = 0; S->vfix = 0; S->ncand = 0;
  S->sh = 0; S->phase = 0; S->done = 0; S->all = 0;
}
__global__ __launch_bounds__(256) void k_top_clear(TopState* __restrict__ S) {
  for (uint32_t b = threadIdx.x; b < TOP_BINS; b += 256u) S->hist[b] = 0u;
  if (threadIdx.x == 0) top_state_reset(S);
}

// candidates -> records. One workgroup; the sort runs over the next power of two above the candidate count, padded with the largest key.
__global__ __launch_bounds__(TOP_SORT_THREADS) void k_top_finish(TopState* __restrict__ S, const unsigned long long* __restrict__ cand_u, const unsigned long long* __restrict__ cand_id,
                                                                 bmx_top_rec* __restrict__ out, unsigned long long* __restrict__ n_out, unsigned long long* __restrict__ n_eligible,
                                                                 uint32_t k, uint32_t desc) {
  __shared__ unsigned long long ku[TOP_CAND], ki[TOP_CAND];
  const unsigned long long ne = S->n_elig;
  const uint32_t nc = (uint32_t)(S->ncand < TOP_CAND ? S->ncand : TOP_CAND);
  uint32_t no = (uint32_t)(ne < k ? ne : (unsigned long long)k);
  no = no < nc ? no : nc;                                  // (nc >= min(k, n_eligible) by construction)
  uint32_t N2 = 2;
  while (N2 < nc) N2 <<= 1;
  for (uint32_t i = threadIdx.x; i < N2; i += TOP_SORT_THREADS) { ku[i] = i < nc ? cand_u[i] : ~0ull; ki[i] = i < nc ? cand_id[i] : ~0ull; }
  __syncthreads();
  for (uint32_t kk = 2; kk <= N2; kk <<= 1)
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < N2 / 2; t += TOP_SORT_THREADS) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const unsigned long long au = ku[i], ai = ki[i], bu = ku[p], bi = ki[p];
        const bool gt = au > bu || (au == bu && ai > bi);
        if (gt == ((i & kk) == 0)) { ku[i] = bu; ki[i] = bi; ku[p] = au; ki[p] = ai; }
      }
      __syncthreads();
    }
  for (uint32_t i = threadIdx.x; i < no; i += TOP_SORT_THREADS) { bmx_top_rec r; r.id = ki[i]; r.val = top_val(ku[i], desc); out[i] = r; }
  for (uint32_t b = threadIdx.x; b < TOP_BINS; b += TOP_SORT_THREADS) S->hist[b] = 0u;
  if (threadIdx.x == 0) {
    if (n_out) *n_out = no;
    if (n_eligible) *n_eligible = ne;
    top_state_reset(S);
  }
}

}  // namespace bmx
