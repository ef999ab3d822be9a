/* bmx_group.h — group-by over discovered values: bmx_where_group and its sharded form. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next to
 * bmx.h. It brings bmx_where.h (the program: bmx_lit) with it.
 *
 * What it replaces in the reference: "count users by role" (docs/querying.md, src/bullet-query.js:293-313) is one count() per key of the index, and the index
 * there is a Map keyed by value: the distinct values are the index's keys and nobody has to know them in advance. bmx_scan_aggregate and bmx_where_aggregate
 * group over a dense window group_lo .. group_lo + ngroups - 1 of at most 65536 consecutive values that the caller must already know; a field whose values are
 * sparse (category codes, bucketed timestamps, hashed foreign keys), lie anywhere in +-(2^53 - 1) or have an unknown range could only be grouped on the host.
 * bmx_where_group is a hash aggregation on the device: the records of bmx_where_aggregate, one per distinct value of the group field that actually occurs among
 * the selected nodes.
 *
 * Selection: exactly bmx_scan_where's. The program is its `nclauses, clause_len, lits` (disjunctive normal form over range literals; see bmx_where.h for literal
 *   truth, BMX_LIT_NOT, clamping and the limits). The candidates are the positions of base_field's dense index (built or refreshed like any scan) whose row holds
 *   data. A one-clause program is an AND of ranges: there is no separate scan_ form.
 * Group value: the value of group_field on the selected node. When group_field is base_field the value comes from the column and costs no probe; otherwise it
 *   costs one probe, made after the match is known. group_field == BMX_AGG_NO_FIELD is refused.
 * Measure: measure_field behaves as in bmx_where_aggregate. BMX_AGG_NO_FIELD: no measure — n = n_match, the sum is 0, min / max keep their empty values
 *   (INT64_MAX / INT64_MIN). The record is bmx_agg with the same exact 128-bit sum. A selected node whose measure row is absent or tombstoned counts in n_match
 *   but not in n.
 * res->absent aggregates the selected nodes whose group value is absent or tombstoned, res->total every selected node. Always:
 *   sum of out[i].agg.n_match + absent.n_match == total.n_match, and the same for n and for the sum.
 *
 * The answer. Let D be the number of distinct group values among the selected nodes.
 *   D <= cap: res->n_groups == D, res->flags == 0, out[0 .. D) holds one record per value, nothing is written at or beyond out[D]. With BMX_MEM_HOST the
 *     records are sorted ascending by key (the library sorts the at most cap records on the host after the download). With BMX_MEM_DEVICE the order of the
 *     records is unspecified; the set and every byte of every record are exact.
 *   D > cap: res->flags == BMX_GROUP_OVERFLOW, res->n_groups is some number > cap that is a lower bound of D, `out` is not written at all; absent and total are
 *     still exact. The caller retries with more room or a narrower program: the "commit only if it fits" rule of bmx_watch_poll.
 *   cap is 1..BMX_GROUP_MAX_CAP. The context keeps an open-addressed table of max(64, next power of two >= 2 * cap) slots of 56 bytes for the largest cap asked
 *     so far, and cap records of staging.
 *
 * mem: BMX_MEM_HOST is synchronous. BMX_MEM_DEVICE takes out and res as device pointers and only enqueues; res is written fully, in stream order. An ordinary
 *   entry point: it orders behind a deferred compaction, sees the last merge, works after a growth and on an index that has switched to its int64 column.
 * Value-ordered views: with a view on base_field (bmx_index_set_ordered) the call still takes the column path and leaves the view's bookkeeping untouched.
 * BMX_ERR_INVALID, before any device work and without writing anything: every refusal of bmx_scan_where's program (nclauses outside 1..8, a clause_len of 0 or
 *   above 8, more than 32 literals, more than 8 fields besides base_field, unknown literal flag bits, clause_len or lits NULL); res NULL; out NULL with cap > 0;
 *   cap == 0 or cap > BMX_GROUP_MAX_CAP; group_field == BMX_AGG_NO_FIELD; a bad mem; a NULL context / communicator.
 * bmx_comm_where_group (host memory): the program is checked and prepared once and enqueued on every shard, with the caller's cap, before the first answer is
 *   fetched. A node's rows all live on the shard that owns its id, so the shards' sorted lists merge exactly by key: counts and 128-bit sums add, minima and
 *   maxima fold; absent and total combine the same way. BMX_GROUP_OVERFLOW if any shard overflowed or the union has more than cap keys; nothing is written to
 *   `out` then, and n_groups is the largest lower bound known (the union's size when no shard overflowed). */
#ifndef BMX_GROUP_H
#define BMX_GROUP_H
#include "bmx.h"
#include "bmx_where.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_group_rec { int64_t key; bmx_agg agg; } bmx_group_rec;                    /* 56 bytes */
typedef struct bmx_group_res {
  uint64_t n_groups; uint32_t flags; uint32_t reserved;
  bmx_agg absent; bmx_agg total;
} bmx_group_res;                                                                             /* 112 bytes */
#define BMX_GROUP_OVERFLOW 1u
#define BMX_GROUP_MAX_CAP (1u << 20)

int bmx_where_group(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                    uint32_t measure_field, uint32_t group_field, bmx_group_rec* out, uint64_t cap, bmx_group_res* res, int mem);
int bmx_comm_where_group(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                         uint32_t measure_field, uint32_t group_field, bmx_group_rec* out, uint64_t cap, bmx_group_res* res);

#ifdef __cplusplus
}
#endif
#endif
