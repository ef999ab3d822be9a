/* bmx_where_agg.h — aggregates and top-k over boolean filters: bmx_where_aggregate, bmx_where_top and their sharded forms. Additions to the C ABI of bmx.h
 * (ABI 4, unchanged); include it next to bmx.h. It brings bmx_where.h (the program: bmx_lit) and bmx_top.h (bmx_top_rec, BMX_TOP_*) with it.
 *
 * What it replaces in the reference: docs/querying.md follows its filters with reductions — "count users by role among the active non-admins", "total inventory
 * value of products in electronics OR computers", "the 20 youngest users who are not admins". bmx_scan_aggregate and bmx_scan_top answer such questions on the
 * device for an AND of ranges; a program with an OR, a NOT or a presence test could only be run through bmx_scan_where, which returns every matching id (8 bytes
 * per match) for the host to fetch and reduce. These calls reduce on the device: nothing proportional to the match count is written anywhere.
 *
 * Selection (both calls): exactly bmx_scan_where's. The program is its `nclauses, clause_len, lits` (disjunctive normal form over range literals; see
 *   bmx_where.h for literal truth, BMX_LIT_NOT, clamping and the limits). The candidates are the positions of base_field's dense index (built or refreshed like
 *   any scan) whose row holds data: a node whose base_field is absent or tombstoned is never selected, whatever the program says. A literal on base_field is
 *   decided on the column value; every other field is probed at most once per candidate.
 *
 * bmx_where_aggregate: measure, grouping, the record (bmx_agg, 48 bytes), BMX_AGG_NO_FIELD, BMX_AGG_MAX_GROUPS and the exact 128-bit sum are
 *   bmx_scan_aggregate's (bmx.h "aggregate queries"). ngroups == 0: out[0] is the one record. ngroups > 0: out[g] for group value group_lo + g,
 *   g < ngroups, and out[ngroups] for the selected nodes whose group value is absent, tombstoned or outside the window: ngroups + 1 records. A selected node
 *   whose measure row is absent or tombstoned counts in n_match but not in n. measure_field and group_field may each be base_field (the value comes from the
 *   column, no probe), a field of the program, or a field the program does not name; in the last two cases the field is probed once more for the candidates
 *   the program selected, after the match is known. min / max of a record with n == 0 are INT64_MAX / INT64_MIN.
 *
 * bmx_where_top: order, BMX_TOP_DESC, the keyset cursor, k and the counts are bmx_scan_top's (bmx_top.h). The order field is base_field: by its value, then by
 *   node id as an unsigned 64-bit number ("the 20 youngest users who are not admins" has base_field = age). `after` is a HOST pointer in both mem modes, read at
 *   call time; NULL: from the beginning; it need not name an existing row. A node is ELIGIBLE if it is selected and comes strictly after *after. out[0 ..
 *   min(k, n_eligible)) = the first eligible nodes in order, *n_out = records written, *n_eligible = eligible nodes; both may be NULL. k is 1..BMX_TOP_MAX_K.
 *   Cost: pass 0 runs the program (one sweep with its probes) and leaves one bit per index position; the digit and compaction sweeps of bmx_scan_top's
 *   multi-term form follow and read that bit.
 *
 * mem (both): BMX_MEM_HOST is synchronous. BMX_MEM_DEVICE takes the outputs (out; n_out, n_eligible) as device pointers and only enqueues. The records of an
 *   aggregate are written fully, in stream order, whatever out held. Ordinary entry points: they order behind a deferred compaction, see the last merge, work
 *   after a growth and on an index that has switched to its int64 column.
 * Value-ordered views: with a view on base_field (bmx_index_set_ordered) the calls still take the column path and leave the view's bookkeeping untouched, as
 *   bmx_scan_where and bmx_scan_top do. Answering from the view is a follow-up.
 * BMX_ERR_INVALID, before any device work and without writing anything: every refusal of bmx_scan_where's program (nclauses outside 1..8, a clause_len of 0 or
 *   above 8, more than 32 literals, more than 8 fields besides base_field, unknown literal flag bits, clause_len or lits NULL); out NULL; ngroups above
 *   BMX_AGG_MAX_GROUPS; ngroups > 0 with group_field == BMX_AGG_NO_FIELD; k == 0 or k > BMX_TOP_MAX_K; unknown top flag bits; a bad mem; a NULL context /
 *   communicator.
 * bmx_comm_where_aggregate, bmx_comm_where_top (host memory): the program is checked and prepared once and enqueued on every shard before the first answer
 *   is fetched. A node's rows all live on the shard that owns its id, so the shards' answers combine exactly, as bmx_comm_scan_aggregate's (counts and
 *   128-bit sums add, minima and maxima fold) and bmx_comm_scan_top's (merged into the first k, n_eligible added up) do. */
#ifndef BMX_WHERE_AGG_H
#define BMX_WHERE_AGG_H
#include "bmx.h"
#include "bmx_where.h"
#include "bmx_top.h"

#ifdef __cplusplus
extern "C" {
#endif

int bmx_where_aggregate(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                        uint32_t measure_field, uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* out, int mem);
int bmx_where_top(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                  uint32_t flags, const bmx_top_rec* after, uint32_t k, bmx_top_rec* out, uint64_t* n_out, uint64_t* n_eligible, int mem);
int bmx_comm_where_aggregate(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                             uint32_t measure_field, uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* out);
int bmx_comm_where_top(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                       uint32_t flags, const bmx_top_rec* after, uint32_t k, bmx_top_rec* out, uint64_t* n_out, uint64_t* n_eligible);

#ifdef __cplusplus
}
#endif
#endif
