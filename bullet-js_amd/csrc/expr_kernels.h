// expr_kernels.h — computed measures (bmx_expr.h): what the three sweeps that take a measure share when the measure is value(a) op value(b) of the selected
// node, gfx950, wave64. The sweeps themselves are k_where_agg (where_agg_kernels.h), k_group_sweep (group_kernels.h) and k_quant0 (quant_kernels.h): each has a
// template flag EXPR, and its EXPR = false instantiations carry none of this (ExprArgs<false> is empty, the wave's counters are never touched).
//
// expr_fetch  : both operands, and the group value of the grouped sweeps, through ONE `#pragma unroll 1` copy of agg_probe (a second inlined copy costs the
//               grouped sweeps their last free scalar registers: where_agg_row). An operand that is the base field is the column value; b == a is a's value,
//               probed once.
// expr_value  : the node's class (bmx_expr.h: defined / undefined / out of range) and, defined, its value. + and - are exact in 64 bits (|operand| <= 2^53 - 1);
//               the product is decided by an overflow-checked multiply, never by its low 64 bits.
// expr_count  : the classes of a wave's lanes into the wave's two counters (ballot + popcount, in uniform control flow: scalar registers).
// expr_end    : the waves' counters -> the workgroup's (two LDS words) -> one pair of no-return atomics per workgroup into the context's ExprState.
// k_expr_finish : the last kernel of a computed-measure query: the two counters out, the state record back to zero (the `clean` protocol of the other forms).
//               The counters have a state record of their own, not two more words in AggRaw / GroupState / QuantState: those records and the kernels that
//               finish them (k_agg_finish, k_group_finish, k_quant_finish) serve the plain forms and stay as they are.
#pragma once
#include "agg_kernels.h"
#include "../../include/bmx_expr.h"

namespace bmx {

struct ExprState { unsigned long long n_undef, n_range; };
static_assert(sizeof(ExprState) == sizeof(bmx_expr_res) && sizeof(bmx_expr) == 16 && sizeof(bmx_expr_res) == 16, "the records of bmx_expr.h");

constexpr uint32_t EXPR_SRC_SAME = 0xFDu;       // ExprArgs::b_src: b is a's field (beside 0 = the base field's column and AGG_SRC_PROBE)

template <bool EXPR>
struct ExprArgs {};                             // a plain measure: nothing
template <>
struct ExprArgs<true> {
  ExprState* S;
  uint32_t a, b;                                // field hashes (read where a_src() / b_src() == AGG_SRC_PROBE)
  uint32_t mode;                                // a_src | b_src << 8 | op << 16 in ONE word: the sweeps have no scalar registers to spare for three
  __host__ __device__ uint32_t a_src() const { return mode & 0xFFu; }
  __host__ __device__ uint32_t b_src() const { return (mode >> 8) & 0xFFu; }
  __host__ __device__ uint32_t op() const { return mode >> 16; }      // BMX_EXPR_ADD / SUB / MUL
};

// The two counters of a WAVE, the same in all its lanes: they are added to in uniform control flow only (expr_count), so they live in scalar registers and
// cost the sweeps no vector register (two counters per lane cost the flat aggregate two waves of occupancy). (An index has fewer than 2^32 rows.)
struct ExprWave { uint32_t undef = 0, range = 0; };
constexpr uint32_t EXPR_DEFINED = 0u, EXPR_UNDEF = 1u, EXPR_RANGE = 2u;      // the class of a selected node (a lane without one: EXPR_DEFINED)

// called by every lane of the wave together: cls = the class of the lane's selected node
__device__ __forceinline__ void expr_count(ExprWave& C, uint32_t cls) {
  C.undef += (uint32_t)__popcll(__ballot(cls == EXPR_UNDEF));
  C.range += (uint32_t)__popcll(__ballot(cls == EXPR_RANGE));
}

// have: both operands hold data. -> the node is defined; r = its value then; cls = its class
__device__ __forceinline__ bool expr_value(uint32_t op, bool have, int64_t a, int64_t b, int64_t& r, uint32_t& cls) {
  long long p;
  bool in = true;
  if (op == BMX_EXPR_MUL) in = !__builtin_mul_overflow((long long)a, (long long)b, &p);     // (uniform)
  else p = op == BMX_EXPR_ADD ? (long long)a + (long long)b : (long long)a - (long long)b;  // (|a|, |b| <= VAL_MAX: exact)
  in = in && p >= -VAL_MAX && p <= VAL_MAX;
  cls = !have ? EXPR_UNDEF : (in ? EXPR_DEFINED : EXPR_RANGE);
  r = (int64_t)p;
  return have && in;
}

// the selected candidate at position pos with base value x. k = 0, 1: the operands; k = 2: the group field of the grouped sweeps (g_src == AGG_SRC_PROBE; the
// quantiles pass AGG_SRC_NONE). -> the node is defined, mval = its value; gval / have_g are touched only by a group probe that found data.
__device__ __forceinline__ bool expr_fetch(const Slot* __restrict__ slots, uint64_t nslots, const uint64_t* __restrict__ ids, const ExprArgs<true>& X, uint32_t g_src,
                                           uint32_t group, int64_t x, uint64_t pos, int64_t& mval, int64_t& gval, bool& have_g, uint32_t& cls) {
  int64_t a = x, b = x;
  bool have_a = X.a_src() == 0u, have_b = X.b_src() == 0u;
#pragma unroll 1
  for (uint32_t k = 0; k < 3u; k++) {
    if ((k == 0u ? X.a_src() : (k == 1u ? X.b_src() : g_src)) != AGG_SRC_PROBE) continue;      // (uniform)
    int64_t y;
    if (agg_probe(slots, nslots, ids[pos], k == 0u ? X.a : (k == 1u ? X.b : group), y) && y != VAL_DELETED) {
      if (k == 0u) { a = y; have_a = true; } else if (k == 1u) { b = y; have_b = true; } else { gval = y; have_g = true; }
    }
  }
  if (X.b_src() == EXPR_SRC_SAME) { b = a; have_b = have_a; }                                // (uniform)
  return expr_value(X.op(), have_a && have_b, a, b, mval, cls);
}

// every lane of the workgroup, once, behind its last row
__device__ __forceinline__ void expr_end(const ExprArgs<true>& X, const ExprWave& C) {
  __shared__ uint32_t s_x[2];
  if (threadIdx.x == 0) { s_x[0] = 0u; s_x[1] = 0u; }
  __syncthreads();
  if ((threadIdx.x & 63u) == 0) { if (C.undef) atomicAdd(&s_x[0], C.undef); if (C.range) atomicAdd(&s_x[1], C.range); }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_x[0]) atomicAdd(&X.S->n_undef, (unsigned long long)s_x[0]);
    if (s_x[1]) atomicAdd(&X.S->n_range, (unsigned long long)s_x[1]);
  }
}
__device__ __forceinline__ void expr_end(const ExprArgs<false>&, const ExprWave&) {}

// out == nullptr (a caller without an xres): only the state is put back
__global__ void k_expr_finish(ExprState* __restrict__ S, bmx_expr_res* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  if (out) { bmx_expr_res o; o.n_undef = S->n_undef; o.n_range = S->n_range; *out = o; }
  S->n_undef = 0ull; S->n_range = 0ull;
}

}  // namespace bmx
