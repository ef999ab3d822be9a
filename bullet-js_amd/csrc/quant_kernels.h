// quant_kernels.h — exact quantiles over boolean filters (bmx_quant.h bmx_where_quantiles): a radix select for up to QUANT_MAX ranks at once over the measure
// values of the nodes a program selects, gfx950, wave64.
//
// The answer of a quantile is a VALUE, so this is the simpler select of the two in the tree (top_kernels.h is the other): no id digits, no compaction, no sort.
// What is new against it: several ranks travel together (one LDS histogram per DISTINCT prefix the ranks still have in common), and the measure may be a probed
// field.
//
// k_quant0<T, PROBE> : pass 0, k_where_top0's shape (top_sweep over the base column, PredWhere::row() per row, the mask word composed by shuffles). PROBE = false:
//                      the measure is the base field, the column value is the sample value. PROBE = true: one agg_probe per SELECTED candidate; the value goes to
//                      a position-indexed scratch (int64 per index position, written only where the bit is set) that every later pass reads instead of probing.
//                      The bit left in the scans' mask scratch is "selected AND the measure holds data". Per workgroup one set of atomics: n_match, n, and the
//                      minimum and maximum of the biased key u = v ^ 2^63.
// k_quant_init       : the ranks from n, the digit bits from kmax - kmin (quant_sel_init), one workgroup.
// k_quant_digit<T>   : one digit (TOP_DIGIT_BITS bits) of the rows that share a LIVE prefix: a sweep of the mask plus the values — the base column (T = its
//                      width) or the value scratch (T = int64_t: the two 8-byte forms are one instantiation, the kernel cannot tell them apart and need not).
//                      NP x TOP_BINS x u32 of dynamic LDS, NP = distinct live prefixes; a wave whose rows fall into one (histogram, bin) adds once (k_top_digit's
//                      ballot + popcount), one no-return global atomic per non-empty bin and workgroup. With one live prefix (the first digit, and while the
//                      ranks stay together) the sweep is the one-compare form quant_digit_sweep<T, true>.
// k_quant_find       : for every rank the bin that holds it (block_excl_scan per live prefix, then quant_search / quant_step); rebuilds the list of distinct
//                      prefixes (quant_relist) and clears the histograms it read.
// k_quant_finish     : the records and the result, and the state record left empty for the next query (k_quant_clear does the same after a query that failed
//                      half-way).
// Every pass behind the last digit returns after one read of the state record, so the host enqueues the worst case and nothing comes back between the passes.
// The sharded form (bmx_quant.inc) runs pass 0 and the digit sweeps on every shard and quant_sel_init / quant_search / quant_step / quant_relist on the host:
// the same code, which is why they are __host__ __device__ and know nothing of threads.
#pragma once
#include "where_agg_kernels.h"
#include "../../include/bmx_quant.h"

namespace bmx {

constexpr uint32_t QUANT_MAX = BMX_QUANT_MAX;
static_assert(QUANT_MAX * TOP_BINS * sizeof(uint32_t) <= 65536, "the histograms of every rank fit the 64 KB of LDS one workgroup may ask for");

// the select of one call: plain data, the same on the device and on the host
struct QuantSel {
  unsigned long long n;                          // the sample's size
  unsigned long long kmin;                       // its smallest key; the digits run over key - kmin
  uint32_t nq, np;                               // ranks; distinct live prefixes (1 before the first digit)
  uint32_t sh;                                   // bits of key - kmin not decided yet; 0: done
  uint32_t pad;
  unsigned long long live[QUANT_MAX];            // the distinct prefixes, right-aligned, in order of first use by a rank
  unsigned long long rank[QUANT_MAX], prefix[QUANT_MAX], below[QUANT_MAX], n_equal[QUANT_MAX];   // per rank; below: sample elements under the prefix, n_equal: with it
  uint32_t slot[QUANT_MAX];                      // rank i's prefix is live[slot[i]]
};
// the state of one context, in device memory; every query's last kernel leaves it as k_quant_clear does
struct QuantState {
  unsigned long long n_match, n, kmin, kmax;     // pass 0 (this context's rows; Q.kmin is the whole sample's)
  QuantSel Q;
  unsigned long long hist[QUANT_MAX][TOP_BINS];  // [live prefix][bin]
};
struct QuantQs { bmx_quant_q q[QUANT_MAX]; };    // the caller's quantiles, by value

struct QuantArgs {
  uint32_t* mask;                                // one bit per index position: selected and measured
  int64_t* vals;                                 // PROBE: the measure value of every position whose bit is set
  QuantState* S;
  uint32_t measure;
};

// floor(num * (n - 1) / den), n >= 1
__host__ __device__ inline unsigned long long quant_rank(uint32_t num, uint32_t den, unsigned long long n) {
  // an index has fewer than 2^44 rows (32-bit slot indices, far fewer in fact) and den <= 2^20: the product stays below 2^64
  return (unsigned long long)num * (n - 1ull) / (unsigned long long)den;
}
__host__ __device__ inline uint32_t quant_bits(unsigned long long d) {
  uint32_t b = 0;
  while (d) { b++; d >>= 1; }
  return b;
}
// the width of the next digit
__host__ __device__ inline uint32_t quant_width(uint32_t sh) { return sh < TOP_DIGIT_BITS ? sh : TOP_DIGIT_BITS; }

__host__ __device__ inline void quant_sel_init(QuantSel& Q, unsigned long long n, unsigned long long kmin, unsigned long long kmax, uint32_t nq, const bmx_quant_q* qs) {
  Q.n = n; Q.kmin = kmin; Q.nq = nq; Q.np = 1; Q.pad = 0;
  Q.sh = n ? quant_bits(kmax - kmin) : 0u;       // every element has (key - kmin) >> sh == 0; all equal: no digit at all
  for (uint32_t i = 0; i < QUANT_MAX; i++) {
    Q.live[i] = 0; Q.slot[i] = 0; Q.prefix[i] = 0; Q.below[i] = 0;
    Q.rank[i] = (i < nq && n) ? quant_rank(qs[i].num, qs[i].den, n) : 0ull;
    Q.n_equal[i] = i < nq ? n : 0ull;
  }
}
// the bin of h[0 .. nb) that holds the element `target` (0-based) of the run that starts at count `off`: off + sum(h[0 .. bin)) <= target < ... + h[bin].
// -> false if the run does not hold it; *c = elements of the run in front of the bin (off included)
// and *in_bin = h[bin]
template <class H>
__host__ __device__ inline bool quant_search(const H* h, uint32_t nb, unsigned long long off, unsigned long long target, uint32_t* bin, unsigned long long* c,
                                             unsigned long long* in_bin) {
  unsigned long long at = off;
  if (target < at) return false;
  for (uint32_t b = 0; b < nb; b++) {
    const unsigned long long hb = (unsigned long long)h[b];
    if (target < at + hb) { *bin = b; *c = at; *in_bin = hb; return true; }
    at += hb;
  }
  return false;
}
// rank i found its bin of width-w digit: `c` elements of its prefix lie in front of the bin, in_bin in it
__host__ __device__ inline void quant_step(QuantSel& Q, uint32_t i, uint32_t bin, unsigned long long c, unsigned long long in_bin, uint32_t w) {
  Q.prefix[i] = (Q.prefix[i] << w) | (unsigned long long)bin;
  Q.below[i] += c;
  Q.n_equal[i] = in_bin;
}
// behind a digit: the distinct prefixes again, and the bits left
__host__ __device__ inline void quant_relist(QuantSel& Q, uint32_t nsh) {
  uint32_t np = 0;
  for (uint32_t i = 0; i < Q.nq; i++) {
    uint32_t j = 0;
    while (j < np && Q.live[j] != Q.prefix[i]) j++;
    if (j == np) Q.live[np++] = Q.prefix[i];
    Q.slot[i] = j;
  }
  Q.np = np; Q.sh = nsh;
}
// record i of the answer
__host__ __device__ inline bmx_quant_rec quant_record(const QuantSel& Q, uint32_t i) {
  bmx_quant_rec r;
  if (!Q.n) { r.value = 0; r.rank = 0; r.n_below = 0; r.n_equal = 0; return r; }
  r.value = (int64_t)((Q.kmin + Q.prefix[i]) ^ 0x8000000000000000ull);     // the bias undone
  r.rank = Q.rank[i]; r.n_below = Q.below[i]; r.n_equal = Q.n_equal[i];
  return r;
}
__host__ __device__ inline bmx_quant_res quant_result(unsigned long long n_match, unsigned long long n, unsigned long long kmin, unsigned long long kmax) {
  bmx_quant_res r;
  r.n_match = n_match; r.n = n;
  r.min = n ? (int64_t)(kmin ^ 0x8000000000000000ull) : INT64_MAX;
  r.max = n ? (int64_t)(kmax ^ 0x8000000000000000ull) : INT64_MIN;
  return r;
}

// EXPR (bmx_expr.h): the sample value is X's expression of two fields, computed per SELECTED candidate and left in the value scratch: PROBE's route, whatever
// the operands are. The bit is "selected AND the node is defined".
template <class T, bool PROBE, bool PAIRS, bool EXPR = false>      // (PAIRS: the program has a field pair; where_kernels.h PredWhere)
__global__ __launch_bounds__(TOP_THREADS) void k_quant0(uint64_t n, PredWhere<T, PAIRS> P, QuantArgs A, ExprArgs<EXPR> X) {
  static_assert(!EXPR || PROBE, "a computed measure goes through the value scratch");
  ExprWave C;
  constexpr int E = PredWhere<T>::E;
  typedef T vec_t __attribute__((ext_vector_type(E)));
  __shared__ unsigned long long s_m[TOP_WAVES], s_n[TOP_WAVES], s_mn[TOP_WAVES], s_mx[TOP_WAVES];
  unsigned long long cnt_m = 0, cnt_n = 0, mn = ~0ull, mx = 0ull;
  const uint64_t nu = (n + E - 1) / E;
  top_sweep<T>(P.v, n, P.nt ? 1u : 0u, [&](uint64_t unit, const vec_t& x, uint32_t cnt) {
    uint32_t nib = 0;
    // (its own copy of where_unit_rows' walk: through the helper the PROBE builds take 4 to 6 more VGPRs and two of them lose a wave of occupancy)
#pragma unroll 1
    for (int e = 0; e < E; e++) {
      const T xe = where_pick<T, E>(x, e);
      const uint64_t pos = unit * E + (uint64_t)e;
      const bool sel = P.row((uint32_t)e < cnt && xe != PredWhere<T>::TOMB, (int64_t)xe, pos);
      bool have = sel;
      int64_t v = (int64_t)xe;
      uint32_t cls = EXPR_DEFINED;
      if (PROBE && sel) {                                        // (pos < n: a selected row exists)
        int64_t y;
        if constexpr (EXPR) { bool hg = false; int64_t g = 0; have = expr_fetch(P.slots, P.nslots, P.ids, X, AGG_SRC_NONE, 0u, (int64_t)xe, pos, y, g, hg, cls); }
        else have = agg_probe(P.slots, P.nslots, P.ids[pos], A.measure, y) && y != VAL_DELETED;
        if (have) { v = y; A.vals[pos] = y; }
      }
      if constexpr (EXPR) expr_count(C, cls);
      nib |= (uint32_t)have << e;
      cnt_m += sel ? 1u : 0u;
      if (have) { const unsigned long long u = top_key(v, 0u); cnt_n++; mn = u < mn ? u : mn; mx = u > mx ? u : mx; }
    }
    // 32 / E consecutive lanes hold one mask word (a unit index is a multiple of 32 / E where a lane index is)
    constexpr uint32_t LW = 32 / E;
    uint32_t w = nib << (E * (threadIdx.x & (LW - 1)));
#pragma unroll
    for (uint32_t d = 1; d < LW; d <<= 1) w |= __shfl_xor(w, d);
    if ((threadIdx.x & (LW - 1)) == 0 && unit < nu) A.mask[unit / LW] = w;
  });
  for (int d = 32; d >= 1; d >>= 1) {
    cnt_m += __shfl_xor(cnt_m, d); cnt_n += __shfl_xor(cnt_n, d);
    const unsigned long long a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
    mn = a < mn ? a : mn; mx = b > mx ? b : mx;
  }
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) { s_m[w] = cnt_m; s_n[w] = cnt_n; s_mn[w] = mn; s_mx[w] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = 0, c = 0, a = ~0ull, b = 0ull;
#pragma unroll
    for (int i = 0; i < TOP_WAVES; i++) { m += s_m[i]; c += s_n[i]; a = s_mn[i] < a ? s_mn[i] : a; b = s_mx[i] > b ? s_mx[i] : b; }
    if (m) atomicAdd(&A.S->n_match, m);
    if (c) { atomicAdd(&A.S->n, c); atomicMin(&A.S->kmin, a); atomicMax(&A.S->kmax, b); }
  }
  expr_end(X, C);
}

__global__ void k_quant_init(QuantState* __restrict__ S, uint32_t nq, QuantQs qs) {
  if (threadIdx.x || blockIdx.x) return;
  quant_sel_init(S->Q, S->n, S->kmin, S->kmax, nq, qs.q);
}

// the sweep of one digit pass. ONE: a single live prefix (the first pass, and every pass of ranks that stayed together): one compare per row and no list of
// prefixes in registers
template <class T, bool ONE>
__device__ __forceinline__ void quant_digit_sweep(const T* __restrict__ col, uint64_t n, uint32_t nt, const uint32_t* __restrict__ mask, const QuantSel& Q, uint32_t* q_h) {
  constexpr int E = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(E)));
  const uint32_t sh = Q.sh, np = ONE ? 1u : Q.np;
  const unsigned long long kmin = Q.kmin;
  unsigned long long live[QUANT_MAX];                                     // (uniform; the loop over them below is unrolled)
#pragma unroll
  for (uint32_t j = 0; j < (ONE ? 1u : QUANT_MAX); j++) live[j] = Q.live[j];
  const uint32_t w = quant_width(sh), nsh = sh - w;
  const uint32_t lane = threadIdx.x & 63u;
  top_sweep<T>(col, n, nt, [&](uint64_t unit, const vec_t& x, uint32_t cnt) {
    uint32_t bits = 0;
    if (cnt) { const uint64_t first = unit * E; bits = (mask[first >> 5] >> (uint32_t)(first & 31u)) & ((1u << E) - 1u); }
    if (!__any(bits != 0u)) return;                                       // (a wave's 64 units without one sample element: common under a selective program)
#pragma unroll
    for (int e = 0; e < E; e++) {
      const unsigned long long word = top_key((int64_t)x[e], 0u) - kmin;
      const unsigned long long pre = sh >= 64u ? 0ull : word >> sh;
      uint32_t j = QUANT_MAX;
#pragma unroll
      for (uint32_t k = 0; k < (ONE ? 1u : QUANT_MAX); k++) j = (k < np && pre == live[k]) ? k : j;
      const bool ok = (uint32_t)e < cnt && ((bits >> e) & 1u) && j < QUANT_MAX;
      const uint32_t d = j * TOP_BINS + ((uint32_t)(word >> nsh) & ((1u << w) - 1u));
      // rows that share a prefix often share the digit too: the lanes that hold the first one's (histogram, bin) add once
      const unsigned long long bal = __ballot(ok);
      if (bal) {
        const int first = __ffsll((long long)bal) - 1;
        const uint32_t d0 = __shfl(d, first);
        const unsigned long long same = __ballot(ok && d == d0);
        if ((int)lane == first) atomicAdd(&q_h[d0], (uint32_t)__popcll(same));
        else if (ok && d != d0) atomicAdd(&q_h[d], 1u);
      }
    }
  });
}

template <class T>
__global__ __launch_bounds__(TOP_THREADS) void k_quant_digit(const T* __restrict__ col, uint64_t n, uint32_t nt, const uint32_t* __restrict__ mask, QuantState* __restrict__ S) {
  extern __shared__ __attribute__((aligned(16))) uint32_t q_h[];         // [np][TOP_BINS]; no static LDS beside it
  if (!S->Q.sh) return;
  const uint32_t np = S->Q.np;
  for (uint32_t b = threadIdx.x; b < np * TOP_BINS; b += TOP_THREADS) q_h[b] = 0u;
  __syncthreads();
  if (np == 1u) quant_digit_sweep<T, true>(col, n, nt, mask, S->Q, q_h);
  else quant_digit_sweep<T, false>(col, n, nt, mask, S->Q, q_h);
  __syncthreads();
  unsigned long long* hist = &S->hist[0][0];
  for (uint32_t b = threadIdx.x; b < np * TOP_BINS; b += TOP_THREADS) {
    const uint32_t c = q_h[b];
    if (c) atomicAdd(&hist[b], (unsigned long long)c);
  }
}

__global__ __launch_bounds__(SEL_THREADS) void k_quant_find(QuantState* __restrict__ S) {
  __shared__ uint32_t wsum[4];
  static_assert(TOP_BINS == 8 * SEL_THREADS, "eight bins per thread");
  const uint32_t sh = S->Q.sh;
  if (!sh) return;
  const uint32_t np = S->Q.np, nq = S->Q.nq;
  const uint32_t w = quant_width(sh);
  // every rank's target (0-based among the elements that share its prefix) and histogram, read by every thread in front of the first barrier: the one thread
  // that finds a rank's bin rewrites the rank's entry behind it
  unsigned long long target[QUANT_MAX]; uint32_t slot[QUANT_MAX];
#pragma unroll
  for (uint32_t i = 0; i < QUANT_MAX; i++) { target[i] = S->Q.rank[i] - S->Q.below[i]; slot[i] = i < nq ? S->Q.slot[i] : QUANT_MAX; }
  for (uint32_t j = 0; j < np; j++) {
    uint32_t hb[8], s = 0;                               // (fewer than 2^32 rows in one context's index)
#pragma unroll
    for (int k = 0; k < 8; k++) { hb[k] = (uint32_t)S->hist[j][threadIdx.x * 8 + k]; s += hb[k]; S->hist[j][threadIdx.x * 8 + k] = 0ull; }
    uint32_t tot;
    const uint32_t off = block_excl_scan(s, tot, wsum);
#pragma unroll
    for (uint32_t i = 0; i < QUANT_MAX; i++) {
      if (slot[i] != j) continue;                        // (uniform)
      uint32_t bin; unsigned long long c, in_bin;
      if (target[i] < (unsigned long long)off + s && quant_search(hb, 8u, off, target[i], &bin, &c, &in_bin)) quant_step(S->Q, i, threadIdx.x * 8 + bin, c, in_bin, w);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) quant_relist(S->Q, sh - w);
}

__device__ __forceinline__ void quant_state_reset(QuantState* S) {
  S->n_match = 0; S->n = 0; S->kmin = ~0ull; S->kmax = 0;
  S->Q.n = 0; S->Q.kmin = 0; S->Q.nq = 0; S->Q.np = 0; S->Q.sh = 0; S->Q.pad = 0;
}
__global__ __launch_bounds__(256) void k_quant_clear(QuantState* __restrict__ S) {
  unsigned long long* hist = &S->hist[0][0];
  for (uint32_t b = blockIdx.x * 256u + threadIdx.x; b < QUANT_MAX * TOP_BINS; b += gridDim.x * 256u) hist[b] = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) quant_state_reset(S);
}

// one workgroup. out == nullptr (the sharded form, which writes its records on the host): only the state is put back
__global__ __launch_bounds__(64) void k_quant_finish(QuantState* __restrict__ S, uint32_t nq, bmx_quant_rec* __restrict__ out, bmx_quant_res* __restrict__ res) {
  if (out && threadIdx.x < nq) out[threadIdx.x] = quant_record(S->Q, threadIdx.x);
  if (res && threadIdx.x == 0) *res = quant_result(S->n_match, S->n, S->kmin, S->kmax);
  __syncthreads();
  if (threadIdx.x == 0) quant_state_reset(S);
}

}  // namespace bmx
