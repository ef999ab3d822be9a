// where_kernels.h — boolean filters (bmx_where.h bmx_scan_where): a predicate for select.h's k_scan_mask / k_scan_emit, gfx950.
//
// The expression is in disjunctive normal form over range literals (1..8 clauses, 32 literals in all, 8 probed fields). The candidates are the positions of the
// base field's index whose row holds data; a literal on the base field is decided from the column value, every other field is looked up in the table with
// agg_probe — once per candidate at most, and only when a clause that is still alive for the lane asks for it.
//
// A lane keeps two words: `truth`, one bit per literal, and `known`, one bit per probed field. The first literal of a field that a live clause reaches probes
// the field and sets the truth bits of ALL its literals (WhereProg::flits), so later literals of that field — in this clause or another — are bit tests. There is
// no per-field value array: indexed at run time it would live in scratch.
// The clauses and literals are walked in loops whose counters are the same in every lane, so the literal constants come out of the kernel arguments through
// scalar loads; only the probe sits under a divergent branch. A lane drops out of a clause at its first false literal and out of the walk at its first true
// clause; the loops end early when no lane of the wave is left in them.
#pragma once
#include "agg_kernels.h"
#include "../../include/bmx_where.h"

namespace bmx {

constexpr uint32_t WHERE_MAX_CLAUSES = BMX_WHERE_MAX_CLAUSES, WHERE_MAX_LITS = BMX_WHERE_MAX_LITS, WHERE_MAX_FIELDS = BMX_WHERE_MAX_FIELDS;

// one literal as the kernel takes it: slot 0 = the base field (the column value), slot s > 0 = WhereProg::field[s - 1]; bounds clamped to +-VAL_MAX
struct WhereLit { uint32_t slot, neg; int64_t lo, hi; };
static_assert(sizeof(WhereLit) == sizeof(bmx_lit), "a literal stays 24 bytes");
// the prepared program (bmx_where.inc where_prepare): 888 bytes; PredWhere, the kernel argument that carries it, is 928
struct WhereProg {
  uint32_t nclauses, nfields;
  uint32_t base_lits;                       // bit l: literal l is on the base field
  uint32_t pad;
  uint32_t cbeg[WHERE_MAX_CLAUSES + 1];     // clause c = literals [cbeg[c], cbeg[c + 1]), those on the base field first
  uint32_t field[WHERE_MAX_FIELDS];         // the probed fields, in order of first use
  uint32_t flits[WHERE_MAX_FIELDS];         // bit l: literal l is on field[s]
  WhereLit lit[WHERE_MAX_LITS];
};

static_assert(sizeof(WhereProg) == 888, "the program stays far below the 4 KB of kernel arguments");

template <class T>
struct PredWhere {   // T = int32_t / int64_t: the width of the base field's value column; 16 bytes per lane and load
  static constexpr int E = 16 / (int)sizeof(T);
  static constexpr T TOMB = sizeof(T) == 4 ? (T)INT32_MIN : (T)INT64_MIN;      // what a tombstoned row looks like in the column (scan_kernels.h v32_of)
  const T* v; const uint64_t* ids; const Slot* slots; uint64_t nslots; bool nt;
  WhereProg W;

  // the candidate at position i with base value x (valid = false: no candidate; the lane only keeps the wave's loops company)
  __device__ __forceinline__ bool row(bool valid, int64_t x, uint64_t i) const {
    uint32_t truth = 0, known = 0;
    uint64_t id = 0;
    for (uint32_t bm = W.base_lits; bm; bm &= bm - 1u) {
      const uint32_t l = (uint32_t)__ffs((int)bm) - 1u;
      truth |= (uint32_t)((x >= W.lit[l].lo && x <= W.lit[l].hi) != (W.lit[l].neg != 0u)) << l;
    }
    bool match = false;
    for (uint32_t c = 0; c < W.nclauses; c++) {
      bool alive = valid && !match;
      for (uint32_t l = W.cbeg[c]; l < W.cbeg[c + 1]; l++) {
        const uint32_t s = W.lit[l].slot;
        if (s) {                                                   // (uniform)
          const uint32_t fb = 1u << (s - 1u);
          if (alive && !(known & fb)) {                            // the one divergent branch: this lane needs the field now
            if (!known) id = ids[i];
            int64_t y = VAL_DELETED;
            const bool have = agg_probe(slots, nslots, id, W.field[s - 1u], y);
            for (uint32_t bm = W.flits[s - 1u]; bm; bm &= bm - 1u) {
              const uint32_t j = (uint32_t)__ffs((int)bm) - 1u;    // (lo >= -VAL_MAX: a tombstone is inside no range)
              truth |= (uint32_t)((have && y >= W.lit[j].lo && y <= W.lit[j].hi) != (W.lit[j].neg != 0u)) << j;
            }
            known |= fb;
          }
        }
        alive = alive && ((truth >> l) & 1u);
        if (!__any(alive)) break;
      }
      match = match || alive;
      if (!__any(valid && !match)) break;
    }
    return match;
  }

  __device__ uint32_t mask(uint64_t first, uint64_t n) const { return mask_from(first, n, 0); }

  // ... of the positions from `from` on (rows_kernels.h: a page's cursor); a position in front of it is no candidate and its lane never probes
  __device__ __forceinline__ uint32_t mask_from(uint64_t first, uint64_t n, uint64_t from) const {
    typedef T vec_t __attribute__((ext_vector_type(E)));
    T x[E];
    if (first + E <= n) {
      const vec_t y = nt ? __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(v + first)) : *reinterpret_cast<const vec_t*>(v + first);
#pragma unroll
      for (int e = 0; e < E; e++) x[e] = y[e];
    } else {
#pragma unroll
      for (int e = 0; e < E; e++) x[e] = first + e < n ? v[first + e] : TOMB;
    }
    uint32_t m = 0;
#pragma unroll 1
    for (int e = 0; e < E; e++) {            // one copy of the walk: the element is picked with selects, not with a run-time index
      T xe = x[0];
#pragma unroll
      for (int k = 1; k < E; k++) xe = e == k ? x[k] : xe;
      if (row(xe != TOMB && first + (uint64_t)e >= from, (int64_t)xe, first + (uint64_t)e)) m |= 1u << e;
    }
    return m;
  }
};

}  // namespace bmx
