/* bmx_where.h — boolean filters: bmx_scan_where and bmx_comm_scan_where. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next to bmx.h.
 *
 * What it replaces in the reference: filter(path, fn) (src/bullet-query.js:270-283) calls a host predicate on every child. bmx_scan_filter answers one shape of
 * it on the device, an AND of inclusive ranges. docs/querying.md itself uses shapes that AND cannot say: `user.role !== "admin"` (a negation, true for a child
 * without a role), `categories.includes("electronics") || categories.includes("computers")` (a disjunction), `user.address && ...` (a presence test).
 * bmx_scan_where takes a boolean expression in disjunctive normal form over range literals, with NOT and with defined behaviour for absent and deleted fields,
 * and answers it in one sweep of one dense index column with table probes.
 *
 * Program: `lits` holds the literals of clause 0, then those of clause 1, and so on; clause c has clause_len[c] of them. A node MATCHES if some clause has all
 *   of its literals true. Presence of a field is the literal {field, 0, INT64_MIN, INT64_MAX}, absence the same with BMX_LIT_NOT.
 * Universe: the candidates are the nodes that hold data in base_field: the positions of that field's dense index (built or refreshed like any scan) whose row
 *   is not tombstoned. This stands for the children that filter(path, fn) iterates: the caller names a field that every child it cares about carries. A node
 *   without base_field is never returned, whatever the expression says (a program of negated literals alone included).
 * Literal truth: a positive literal is true iff the node's row of `field` holds data and lo <= value <= hi (both inclusive). A row that is absent or tombstoned
 *   (BMX_VAL_DELETED) makes it false. BMX_LIT_NOT is the exact complement: true for an absent or tombstoned field, like `undefined !== "admin"` on the
 *   reference. lo > hi: the positive literal is never true, the negated one always. Bounds outside +-(2^53 - 1) are clamped to the value domain, so a tombstone
 *   is never taken for a small value: {NOT, lo = INT64_MIN, hi = anything} is true on a tombstone because the field is absent. A literal on base_field is
 *   evaluated on the column value and costs no probe; every other distinct field is probed at most once per candidate, however many literals name it, and only
 *   for candidates whose answer still depends on it.
 * Field-to-field literals (`o.shipped > o.due`, `s.end - s.start <= 3600`): an entry with BMX_LIT_MINUS names field A and the bounds (and may carry
 *   BMX_LIT_NOT); the NEXT entry of the same clause names field B as {field = B, flags = BMX_LIT_SUBTRAHEND, lo = 0, hi = 0}. The two entries are one literal:
 *   true iff the node's rows of A and of B both hold data and lo <= value(A) - value(B) <= hi. With BMX_LIT_NOT it is the exact complement, so true when
 *   either side is absent or tombstoned (`undefined > x` is false on the reference). Values lie in +-(2^53 - 1), so the difference is exact in int64
 *   (|d| <= 2^54 - 2); the bounds are taken as given, not clamped: a == b is [0, 0], a != b the same with NOT, a > b is [1, INT64_MAX], a <= b + 5 is
 *   [INT64_MIN, 5], "both present" is [INT64_MIN, INT64_MAX]; lo > hi is never true and, negated, always. Either side may be base_field: it is then the
 *   column value and costs no probe. Both entries count toward clause_len (<= 8) and toward BMX_WHERE_MAX_LITS. An ordered pair (A, B) takes one of the
 *   BMX_WHERE_MAX_FIELDS slots that the distinct plain fields besides base_field also take; (A, B) and (B, A) are different slots; several literals on one
 *   pair share the slot and its probes. A field used both alone and inside a pair is probed in each of its slots (there is no cache across slots).
 * Clock literals ("written after clock T", "deleted since T", "exists in any state"): an entry with BMX_LIT_CLOCK, BMX_LIT_CLOCK_TOMB or both ranges over the
 *   CLOCK of the node's row of `field`, not over its value. It is true iff the row exists, its state is one the bits name (data for BMX_LIT_CLOCK, a tombstone,
 *   val == BMX_VAL_DELETED, for BMX_LIT_CLOCK_TOMB, either for both) and lo <= ts <= hi, both inclusive; ts is the clock bmx_get_rows reports (and the row
 *   projection with clocks). With BMX_LIT_NOT it is the exact complement: true for an absent row, for a row in a state the literal does not name and for a clock outside the
 *   range. The state decides and no sentinel is involved, so the bounds are taken as given, not clamped (clocks lie in 0..2^53 - 1,
 *   so no stored row could tell the difference); lo > hi is never true and, negated, always.
 *   {CLOCK_TOMB, INT64_MIN, INT64_MAX} is "the field is deleted", both bits over the full range "a row exists" (a plain literal cannot tell a tombstone from
 *   an absent row). The index column holds no clocks, so a clock literal on base_field is a probed literal: it takes a slot and reads the base field's own
 *   row; BMX_LIT_CLOCK_TOMB alone on base_field is never true, the candidates hold data. All plain and clock literals of one field share ONE slot and ONE
 *   probe: the clock lies in the 32 bytes the value comes from. Pair slots stay apart. A clock bit goes with neither BMX_LIT_MINUS nor BMX_LIT_SUBTRAHEND
 *   (differences of clocks are not offered).
 * Answer: node ids in position order of base_field's index columns (the order bmx_scan_filter gives without a view). *n_out is the number of matches even when
 *   cap is smaller; nothing is written at or beyond out_ids[cap]; out_ids == NULL counts only.
 * mem: as for bmx_scan_filter. BMX_MEM_HOST is synchronous; BMX_MEM_DEVICE takes out_ids and n_out as device pointers and only enqueues. An ordinary entry
 *   point: it orders behind a deferred compaction, sees the last merge, works after a growth and on an index that has switched to its int64 column.
 * Value-ordered views: with a view on base_field (bmx_index_set_ordered) the call still takes this column path and leaves the view's bookkeeping untouched, as
 *   bmx_scan_top does. Answering from the view when every clause bounds base_field is a follow-up.
 * BMX_ERR_INVALID, before any device work and without writing anything: nclauses outside 1..BMX_WHERE_MAX_CLAUSES, a clause_len of 0 or above 8, more than
 *   BMX_WHERE_MAX_LITS literals in all, more than BMX_WHERE_MAX_FIELDS distinct fields besides base_field, unknown flag bits, clause_len or lits NULL, a bad mem,
 *   a NULL context / communicator. And, each with a text of its own: a BMX_LIT_MINUS entry that ends its clause or is followed by anything but a
 *   BMX_LIT_SUBTRAHEND entry, a BMX_LIT_SUBTRAHEND entry not preceded by a BMX_LIT_MINUS entry, BMX_LIT_SUBTRAHEND together with any other bit or with
 *   lo / hi not 0, A == B, a pair that would need a ninth slot, a clock bit together with BMX_LIT_MINUS, a clock bit together with BMX_LIT_SUBTRAHEND. A
 *   clock literal that would need a ninth slot is refused as a ninth field is.
 * bmx_comm_scan_where (host memory): the shards' answers one after the other, the way bmx_comm_scan_filter works; every shard's sweep is enqueued before the
 *   first answer is fetched. A node's rows all live on the shard that owns its id, so the set equals the set one context holding the same rows gives. */
#ifndef BMX_WHERE_H
#define BMX_WHERE_H
#include "bmx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_lit { uint32_t field; uint32_t flags; int64_t lo, hi; } bmx_lit;   /* 24 bytes, same layout as bmx_term */
#define BMX_LIT_NOT           1u
#define BMX_LIT_MINUS         4u    /* this entry is A, lo, hi [, NOT]; the NEXT entry names B */
#define BMX_LIT_SUBTRAHEND    8u    /* {field = B, flags = exactly this, lo = 0, hi = 0} */
#define BMX_LIT_CLOCK         16u   /* the literal ranges over the row's clock; a row that holds data qualifies */
#define BMX_LIT_CLOCK_TOMB    32u   /* the literal ranges over the row's clock; a tombstoned row qualifies */
#define BMX_WHERE_MAX_CLAUSES 8u
#define BMX_WHERE_MAX_LITS    32u   /* over all clauses */
#define BMX_WHERE_MAX_FIELDS  8u    /* slots: distinct fields other than base_field, and ordered field pairs */

int bmx_scan_where(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                   uint64_t* out_ids, uint64_t cap, uint64_t* n_out, int mem);
int bmx_comm_scan_where(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                        uint64_t* out_ids, uint64_t cap, uint64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif
