// where_agg_kernels.h — aggregates and top-k over boolean filters (bmx_where_agg.h bmx_where_aggregate, bmx_where_top): the two sweeps that decide a
// candidate with where_kernels.h's PredWhere::row() and end like agg_kernels.h and top_kernels.h end, gfx950, wave64.
//
// k_where_agg<T, G> : one read of the base field's value column (top_sweep's shape: 16-byte loads, TOP_U in flight per lane, 512 threads). A candidate that
//                     the program selects goes through where_agg_row (agg_row's tail, with no terms): the measure and the group value are the column value
//                     when the field is the base field, otherwise one agg_probe each, made after the match is known. It probes through PredWhere's table
//                     pointer, not AggArgs' copy of it: the two are the same table, and one pair of scalar registers less is live across row()'s loops.
//                     agg_add<G>, the accumulators, agg_end<G> and k_agg_finish are bmx_scan_aggregate's (G = 0 / 1 / 2 as there).
// k_where_top0<T>   : pass 0 of the radix select for a program. Eligible = row() and behind the cursor. Counts the eligible rows, takes the minimum and maximum
//                     of their keys as k_top_sweep0 does, and leaves one bit per index position in the scans' mask scratch, composed as k_top_sweep0<T, true>
//                     composes it; k_top_digit<T, true> and k_top_compact<T, true> read that bit and know nothing of the program.
//
// row() walks its clauses in loops that end on wave votes, so every lane of a wave has to reach it the same number of times: top_sweep calls its functor once
// per unit in every lane (cnt == 0 beyond the column), and the functor calls row() for all E rows of the unit, with valid = false for a row beyond the column
// or a tombstoned position. As in PredWhere::mask, the E rows are one copy of the walk: the element is picked with selects, not with a run-time index.
// where_unit_rows is that walk and where_sweep the whole sweep, for every kernel of the family but k_where_top0 and k_quant0, which keep a copy and say why;
// where_field and where_two_fields fetch a selected node's fields.
#pragma once
#include "where_kernels.h"
#include "top_kernels.h"
#include "expr_kernels.h"

namespace bmx {

static_assert(AGG_THREADS == TOP_THREADS && AGG_U == TOP_U, "k_where_agg sweeps with top_sweep and reduces with agg_end: one workgroup shape");

// row e of a unit, without a run-time index into the vector
template <class T, int E, class V>
__device__ __forceinline__ T where_pick(const V& x, int e) {
  T xe = x[0];
#pragma unroll
  for (int k = 1; k < E; k++) xe = e == k ? x[k] : xe;
  return xe;
}

// The rows of one unit of top_sweep, in ONE copy of the walk: f(e, xe, pos, sel) for e = 0 .. E - 1, sel = the program selects the row at index position pos
// (never a row beyond the column or a tombstoned position). Every lane reaches row() and f E times: f may vote, or return at once on sel = false.
template <class T, class P, class V, class F>
__device__ __forceinline__ void where_unit_rows(const P& pred, uint64_t unit, const V& x, uint32_t cnt, F&& f) {
  constexpr int E = PredWhere<T>::E;
#pragma unroll 1
  for (int e = 0; e < E; e++) {
    const T xe = where_pick<T, E>(x, e);
    const uint64_t pos = unit * E + (uint64_t)e;
    f(e, xe, pos, pred.row((uint32_t)e < cnt && xe != PredWhere<T>::TOMB, (int64_t)xe, pos));
  }
}
// ... of every unit of the base field's value column: the whole sweep of a kernel with nothing to do per unit
template <class T, class P, class F>
__device__ __forceinline__ void where_sweep(uint64_t n, const P& pred, F&& f) {
  typedef T vec_t __attribute__((ext_vector_type(PredWhere<T>::E)));
  top_sweep<T>(pred.v, n, pred.nt ? 1u : 0u, [&](uint64_t unit, const vec_t& x, uint32_t cnt) { where_unit_rows<T>(pred, unit, x, cnt, f); });
}

// A field of the selected node at pos: src == 0, the base field, whose column value the caller has put into y; src == AGG_SRC_PROBE, one probe of `field`
// through the program's table; any other src: none. -> the node holds data there (y: the value)
template <class P>
__device__ __forceinline__ bool where_field(const P& pred, uint64_t pos, uint32_t src, uint32_t field, int64_t& y) {
  bool have = src == 0u;
  if (src == AGG_SRC_PROBE) have = agg_probe(pred.slots, pred.nslots, pred.ids[pos], field, y) && y != VAL_DELETED;      // (uniform)
  return have;
}
// Two such fields through ONE copy of the probe: a second inlined copy costs the grouped forms their last free scalar registers. The caller has set
// (y, have) of both for src == 0; field k is touched only where src_k == AGG_SRC_PROBE and the node holds data there.
template <class P>
__device__ __forceinline__ void where_two_fields(const P& pred, uint64_t pos, uint32_t src0, uint32_t field0, int64_t& y0, bool& have0, uint32_t src1, uint32_t field1,
                                                 int64_t& y1, bool& have1) {
#pragma unroll 1
  for (uint32_t k = 0; k < 2u; k++) {
    if ((k ? src1 : src0) != AGG_SRC_PROBE) continue;                // (uniform)
    int64_t y;
    if (agg_probe(pred.slots, pred.nslots, pred.ids[pos], k ? field1 : field0, y) && y != VAL_DELETED) {
      if (k) { y1 = y; have1 = true; } else { y0 = y; have0 = true; }
    }
  }
}

// a candidate the program selected: the measure and the group value (the column value x, or one probe each), then the add. The table is P's.
// EXPR (bmx_expr.h): the measure is X's expression of two fields, fetched with the group value through expr_fetch's one copy of the probe; a node that is
// undefined or out of range is a node without its measure; -> its class. The host sets A.m_src = AGG_SRC_PROBE for it: n is counted per row in every G.
template <int G, class T, bool CLOCKS, bool EXPR>
__device__ __forceinline__ uint32_t where_agg_row(const PredWhere<T, true, CLOCKS>& P, const AggArgs& A, const ExprArgs<EXPR>& X, int64_t x, uint64_t pos, AggLane& L,
                                                  AggLds<G>& S) {
  int64_t mval = x, gval = x;
  bool have_m = A.m_src == 0u, have_g = A.g_src == 0u;
  uint32_t cls = EXPR_DEFINED;
  if constexpr (EXPR) have_m = expr_fetch(P.slots, P.nslots, P.ids, X, A.g_src, A.group, x, pos, mval, gval, have_g, cls);
  else where_two_fields(P, pos, A.m_src, A.measure, mval, have_m, A.g_src, A.group, gval, have_g);
  uint32_t g = 0;
  if (G) {   // (the difference of two int64 is exact mod 2^64 once gval >= group_lo)
    const uint64_t d = (uint64_t)gval - (uint64_t)A.group_lo;
    g = (have_g && gval >= A.group_lo && d < (uint64_t)A.ngroups) ? (uint32_t)d : A.ngroups;
  }
  agg_add<G>(A, L, S, g, have_m, mval);
  return cls;
}

template <class T, int G, bool CLOCKS, bool EXPR = false>      // (EXPR: a computed measure, bmx_expr.h; X is empty without one)
__global__ __launch_bounds__(AGG_THREADS) void k_where_agg(uint64_t n, PredWhere<T, true, CLOCKS> P, AggArgs A, ExprArgs<EXPR> X) {
  __shared__ AggLds<G> S;
  AggLane L;
  ExprWave C;
  agg_begin<G>(A, S);
  where_sweep<T>(n, P, [&](int, T xe, uint64_t pos, bool sel) {
    uint32_t cls = EXPR_DEFINED;
    if (sel) cls = where_agg_row<G>(P, A, X, (int64_t)xe, pos, L, S);
    if constexpr (EXPR) expr_count(C, cls);
  });
  agg_end<G>(A, L, S);
  expr_end(X, C);
}

template <class T, bool PAIRS>      // (PAIRS: the program has a field pair; where_kernels.h PredWhere)
__global__ __launch_bounds__(TOP_THREADS) void k_where_top0(uint64_t n, PredWhere<T, PAIRS> P, TopArgs A) {
  constexpr int E = PredWhere<T>::E;
  typedef T vec_t __attribute__((ext_vector_type(E)));
  __shared__ unsigned long long s_n[TOP_WAVES], s_mn[TOP_WAVES], s_mx[TOP_WAVES];
  unsigned long long cnt_l = 0, mn = ~0ull, mx = 0ull;
  const uint64_t nu = (n + E - 1) / E;
  top_sweep<T>(P.v, n, P.nt ? 1u : 0u, [&](uint64_t unit, const vec_t& x, uint32_t cnt) {
    uint32_t nib = 0;
    // (its own copy of where_unit_rows' walk. Measured: through the helper, with the same register counts, bmx_where_top is 6 to 10 us slower at every
    // selectivity; with this copy it is level. profiles/kernel_sharing_timings.txt)
#pragma unroll 1
    for (int e = 0; e < E; e++) {
      const T xe = where_pick<T, E>(x, e);
      const uint64_t pos = unit * E + (uint64_t)e;
      const unsigned long long u = top_key((int64_t)xe, A.desc);
      bool ok = P.row((uint32_t)e < cnt && xe != PredWhere<T>::TOMB, (int64_t)xe, pos);
      ok = ok && top_after(A, u, pos, false, 0);               // (the id column is read only for a row whose value equals the cursor's)
      nib |= (uint32_t)ok << e;
      if (ok) { cnt_l++; mn = u < mn ? u : mn; mx = u > mx ? u : mx; }
    }
    // 32 / E consecutive lanes hold one mask word (a unit index is a multiple of 32 / E where a lane index is)
    constexpr uint32_t LW = 32 / E;
    uint32_t w = nib << (E * (threadIdx.x & (LW - 1)));
#pragma unroll
    for (uint32_t d = 1; d < LW; d <<= 1) w |= __shfl_xor(w, d);
    if ((threadIdx.x & (LW - 1)) == 0 && unit < nu) A.mask[unit / LW] = w;
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

}  // namespace bmx
