// where_kernels.h — boolean filters (bmx_where.h bmx_scan_where): a predicate for select.h's k_scan_mask / k_scan_emit, gfx950.
//
// The expression is in disjunctive normal form over range literals (1..8 clauses, 32 literals in all, 8 probed fields). The candidates are the positions of the
// base field's index whose row holds data; a literal on the base field is decided from the column value, every other field is looked up in the table with
// agg_probe — once per candidate at most, and only when a clause that is still alive for the lane asks for it.
//
// A lane keeps two words: `truth`, one bit per literal, and `known`, one bit per probed field. The first literal of a field that a live clause reaches probes
// the field and sets the truth bits of ALL its literals (WhereProg::flits), so later literals of that field — in this clause or another — are bit tests. There is
// no per-field value array: indexed at run time it would live in scratch.
// A slot of the field table is a probed field or an ordered pair of fields (A, B), whose literals range over A - B (bmx_where.h BMX_LIT_MINUS). The pair's
// two values are fetched inside the same divergent branch — each from the column value when it is the base field, from a probe otherwise — and the slot's
// truth bits are set from the difference as a plain slot's are from the value. Whether a slot is a pair is the same in every lane.
// A clock literal (bmx_where.h BMX_LIT_CLOCK, BMX_LIT_CLOCK_TOMB) ranges over the clock of its field's row. It sits on the field's plain slot next to the
// field's value literals: the slot's one probe (agg_probe_ts) returns whether the row exists, its value and its clock out of the same 32 bytes, and each
// literal of the slot takes the word it ranges over. A clock literal on the base field has a slot like any other field: the index column holds no clocks.
// Which slots carry a clock literal and which literals are one is the same in every lane and is read from the kernel arguments.
// The clauses and literals are walked in loops whose counters are the same in every lane, so the literal constants come out of the kernel arguments through
// scalar loads; only the probe sits under a divergent branch. A lane drops out of a clause at its first false literal and out of the walk at its first true
// clause; the loops end early when no lane of the wave is left in them.
#pragma once
#include "agg_kernels.h"
#include "../../include/bmx_where.h"

namespace bmx {

constexpr uint32_t WHERE_MAX_CLAUSES = BMX_WHERE_MAX_CLAUSES, WHERE_MAX_LITS = BMX_WHERE_MAX_LITS, WHERE_MAX_FIELDS = BMX_WHERE_MAX_FIELDS;

// one literal as the kernel takes it: slot 0 = the base field (the column value), slot s > 0 = WhereProg::field[s - 1] or the pair there; bounds clamped to
// +-VAL_MAX (a pair's and a clock literal's: as given); flags: WHERE_LIT_NOT, and for a clock literal the row states that qualify
struct WhereLit { uint32_t slot, flags; int64_t lo, hi; };
constexpr uint32_t WHERE_LIT_NOT = 1u, WHERE_LIT_CLOCK_DATA = 2u, WHERE_LIT_CLOCK_TOMB = 4u, WHERE_LIT_CLOCK = WHERE_LIT_CLOCK_DATA | WHERE_LIT_CLOCK_TOMB;
static_assert(sizeof(WhereLit) == sizeof(bmx_lit), "a literal stays 24 bytes");
// the prepared program (bmx_where.inc where_prepare): 920 bytes; PredWhere, the kernel argument that carries it, is 960
struct WhereProg {
  uint32_t nclauses, nfields;
  uint32_t base_lits;                       // bit l: literal l is on the base field
  uint32_t pairs;                           // per slot s: bit s = the slot is a pair (A, B) and its literals range over A - B; bit 8 + s = A is the base field
                                            // (the column value, no probe); bit 16 + s = B is; bit 24 + s = the (plain) slot has a clock literal
  uint32_t cbeg[WHERE_MAX_CLAUSES + 1];     // clause c = literals [cbeg[c], cbeg[c + 1]), those on the base field first
  uint32_t field[WHERE_MAX_FIELDS];         // the slots in order of first use: a probed field, or the A of a pair
  uint32_t field2[WHERE_MAX_FIELDS];        // the B of a pair slot
  uint32_t flits[WHERE_MAX_FIELDS];         // bit l: literal l is on slot s
  WhereLit lit[WHERE_MAX_LITS];
};
constexpr uint32_t WHERE_PAIR_A_BASE = 8u, WHERE_PAIR_B_BASE = 16u, WHERE_SLOT_CLOCK = 24u;      // shifts inside WhereProg::pairs

static_assert(sizeof(WhereProg) == 920, "the program stays far below the 4 KB of kernel arguments");

// PAIRS = false compiles the pair path and the clock literals out: for a program with neither (WhereProg::pairs == 0, the host's promise: bmx_where.inc
// where_plain_or_pairs). Only the kernels that would lose a wave of occupancy to those paths' registers are built both ways (k_watch_mask, k_quant0, k_where_top0); every other one takes the default.
// CLOCKS = false compiles the clock literals alone out: the walk of this predicate is bound by the instructions it issues, and a program without a clock
// literal runs measurably faster without their code. Every kernel that takes the program is built with and without them (its CLOCKS argument) and the host
// launches the build with them only for a program that has a clock literal (bmx_where.inc where_sweep_c, where_mask_pass, where_by_paths; DESIGN.md "Clock literals").
template <class T, bool PAIRS = true, bool CLOCKS = PAIRS>
struct PredWhere {   // T = int32_t / int64_t: the width of the base field's value column; 16 bytes per lane and load
  static constexpr int E = 16 / (int)sizeof(T);
  static constexpr bool HAS_CLOCKS = CLOCKS;
  static constexpr T TOMB = sizeof(T) == 4 ? (T)INT32_MIN : (T)INT64_MIN;      // what a tombstoned row looks like in the column (scan_kernels.h v32_of)
  const T* v; const uint64_t* ids; const Slot* slots; uint64_t nslots; bool nt;
  WhereProg W;

  // the candidate at position i with base value x (valid = false: no candidate; the lane only keeps the wave's loops company)
  __device__ __forceinline__ bool row(bool valid, int64_t x, uint64_t i) const {
    uint32_t truth = 0, known = 0;
    uint64_t id = 0;
    for (uint32_t bm = W.base_lits; bm; bm &= bm - 1u) {
      const uint32_t l = (uint32_t)__ffs((int)bm) - 1u;
      truth |= (uint32_t)((x >= W.lit[l].lo && x <= W.lit[l].hi) != ((W.lit[l].flags & WHERE_LIT_NOT) != 0u)) << l;
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
            // A, or the plain field: from a probe unless it is the base field of a pair. A probe that finds no row leaves VAL_DELETED, which is also what a
            // tombstoned row holds (agg_probe finds that one): no flag is kept across the second probe, each side is tested for VAL_DELETED behind it.
            // w, the slot's second word: the clock of a plain slot's row (for its clock literals; a clock is never negative, -1 = no row was found), the B of a
            // pair. A slot is never both, so one word does.
            int64_t y = x, w = -1;
            if (!PAIRS || !(W.pairs & (fb << WHERE_PAIR_A_BASE))) { y = VAL_DELETED; agg_probe_ts(slots, nslots, id, W.field[s - 1u], y, w); }      // (uniform)
            bool have = true;                                      // (a plain literal: lo >= -VAL_MAX keeps VAL_DELETED out of every range)
            if (PAIRS && (W.pairs & fb)) {                         // (uniform) a pair: both sides hold data, y = A - B (exact: |A|, |B| <= VAL_MAX)
              w = x;                                               // (the bounds of a pair literal are as given and keep nothing out: `have` does)
              if (!(W.pairs & (fb << WHERE_PAIR_B_BASE))) { w = VAL_DELETED; agg_probe(slots, nslots, id, W.field2[s - 1u], w); }
              have = y != VAL_DELETED && w != VAL_DELETED;
              y = (int64_t)((uint64_t)y - (uint64_t)w);
            }
            if (CLOCKS && (W.pairs & (fb << WHERE_SLOT_CLOCK))) {   // (uniform) a plain slot with a clock literal: each literal takes the word it ranges over
              for (uint32_t bm = W.flits[s - 1u]; bm; bm &= bm - 1u) {
                const uint32_t j = (uint32_t)__ffs((int)bm) - 1u;
                const uint32_t fl = W.lit[j].flags;
                bool ok = true;
                int64_t z = y;
                if (fl & WHERE_LIT_CLOCK) {                        // (uniform) the row is in a state the literal names, its clock in the bounds as given
                  ok = w >= 0 && (fl & (y != VAL_DELETED ? WHERE_LIT_CLOCK_DATA : WHERE_LIT_CLOCK_TOMB)) != 0u;
                  z = w;
                }
                truth |= (uint32_t)((ok && z >= W.lit[j].lo && z <= W.lit[j].hi) != ((fl & WHERE_LIT_NOT) != 0u)) << j;
              }
            } else {                                               // every other slot, as it always went: its literals carry no flag but WHERE_LIT_NOT
              for (uint32_t bm = W.flits[s - 1u]; bm; bm &= bm - 1u) {
                const uint32_t j = (uint32_t)__ffs((int)bm) - 1u;
                truth |= (uint32_t)((have && y >= W.lit[j].lo && y <= W.lit[j].hi) != ((W.lit[j].flags & WHERE_LIT_NOT) != 0u)) << j;
              }
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
