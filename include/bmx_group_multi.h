/* bmx_group_multi.h — group-by over several fields: bmx_where_group_multi and its sharded form. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it
 * next to bmx.h. It brings bmx_where.h (the program: bmx_lit) and bmx_group.h (bmx_agg's record per group, bmx_group_res, BMX_GROUP_OVERFLOW) with it.
 *
 * What it replaces in the reference: "orders by status and country", "revenue by customer tier and product category", "orders per day", "sessions per hour and
 * region" (docs/querying.md) are a filter() followed by a reduce into a Map keyed by a string the caller glues together from the fields, the time stamp divided
 * by a bucket width first. bmx_where_group groups by the raw value of exactly one field; a tuple of fields, or a key derived from a value, could only be grouped
 * on the host. bmx_where_group_multi is the same hash aggregation on the device, keyed by up to four fields, each optionally bucketed: one record per distinct
 * key tuple that actually occurs among the selected nodes. Nobody has to know the values in advance and no id list leaves the device.
 *
 * Selection: exactly bmx_where_group's (bmx_scan_where's program `nclauses, clause_len, lits` over the positions of base_field's dense index).
 * Measure, res->total, mem: exactly bmx_where_group's. measure_field == BMX_AGG_NO_FIELD: n = n_match, the sum is 0, min / max keep their empty values
 *   (INT64_MAX / INT64_MIN). The result record is bmx_group_res with the flag BMX_GROUP_OVERFLOW.
 * keys: nkeys = 1..BMX_MGROUP_MAX_KEYS descriptions in HOST memory in both mem modes, like lits.
 * Key j of a selected node: let v be the node's value of keys[j].field — from the column when the field is base_field, otherwise through one probe made after
 *   the match is known. The key is floor((v - origin) / width), floor toward minus infinity (Python's //): v = -1, origin = 0, width = 10 gives -1, not 0.
 *   origin = 0, width = 1 is the value itself (no division is made for width == 1). The same field may appear twice with different widths ("per hour and per
 *   day"). flags is reserved and must be 0.
 * Absent: a selected node for which ANY key field is absent or tombstoned lands in res->absent and in no record. Always:
 *   sum of out[i].agg.n_match + absent.n_match == total.n_match, and the same for n and for the sum.
 * Records: bmx_mgroup_rec, 80 bytes; key[j] for j >= nkeys is 0.
 *
 * The answer. Let D be the number of distinct key tuples among the selected nodes that have every key.
 *   D <= cap: res->n_groups == D, res->flags == 0, out[0 .. D) holds one record per tuple, nothing is written at or beyond out[D]. With BMX_MEM_HOST the
 *     records are sorted lexicographically by (key[0], key[1], ...), each signed ascending (the library sorts the at most cap records on the host after the
 *     download). With BMX_MEM_DEVICE the order of the records is unspecified; the set and every byte of every record are exact.
 *   D > cap: res->flags == BMX_GROUP_OVERFLOW, res->n_groups is some number > cap that is a lower bound of D, `out` is not written at all; absent and total are
 *     still exact. The caller retries with more room or a narrower program: the "commit only if it fits" rule of bmx_where_group.
 *   cap is 1..BMX_GROUP_MAX_CAP with one to three keys and 1..BMX_MGROUP_MAX_CAP4 with four: a tuple is aggregated under one 64-bit word that packs, per key,
 *     the number of a slot of that key's dictionary (log2 slots bits each, slots = max(64, next power of two >= 2 * cap)): 3 * 21 = 63 and 4 * 15 = 60 bits.
 *     The context keeps, for the largest call so far, a tuple table of `slots` entries of 56 bytes, nkeys dictionaries of `slots` words and cap records of
 *     staging; they are its own, bmx_where_group's table is not touched.
 *
 * mem: BMX_MEM_HOST is synchronous. BMX_MEM_DEVICE takes out and res as device pointers and only enqueues; res is written fully, in stream order. An ordinary
 *   entry point: it orders behind a deferred compaction, sees the last merge, works after a growth and on an index that has switched to its int64 column.
 * Value-ordered views: with a view on base_field the call still takes the column path and leaves the view's bookkeeping untouched.
 * BMX_ERR_INVALID, before any device work and without writing anything, each with its own text: every refusal of bmx_scan_where's program; res NULL; out NULL;
 *   keys NULL; nkeys outside 1..BMX_MGROUP_MAX_KEYS; a key field equal to BMX_AGG_NO_FIELD; a key's flags != 0; a width outside 1..2^53 - 1; an origin outside
 *   +-(2^53 - 1); cap == 0, cap > BMX_GROUP_MAX_CAP, or cap > BMX_MGROUP_MAX_CAP4 with four keys; a bad mem; a NULL context / communicator.
 * bmx_comm_where_group_multi (host memory): the program and the keys are checked and prepared once and enqueued on every shard, with the caller's cap, before
 *   the first answer is fetched. A node's rows all live on the shard that owns its id, so the shards' sorted lists merge exactly by tuple: counts and 128-bit
 *   sums add, minima and maxima fold; absent and total combine the same way. BMX_GROUP_OVERFLOW if any shard overflowed or the union has more than cap tuples;
 *   nothing is written to `out` then, and n_groups is the largest lower bound known (the union's size when no shard overflowed). */
#ifndef BMX_GROUP_MULTI_H
#define BMX_GROUP_MULTI_H
#include "bmx.h"
#include "bmx_where.h"
#include "bmx_group.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMX_MGROUP_MAX_KEYS 4u
#define BMX_MGROUP_MAX_CAP4 (1u << 14)      /* the largest cap of a 4-key call; 1..3 keys: BMX_GROUP_MAX_CAP */
typedef struct bmx_group_key  { uint32_t field; uint32_t flags; int64_t origin; int64_t width; } bmx_group_key;   /* 24 bytes */
typedef struct bmx_mgroup_rec { int64_t key[4]; bmx_agg agg; } bmx_mgroup_rec;                                    /* 80 bytes */

int bmx_where_group_multi(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                          uint32_t measure_field, uint32_t nkeys, const bmx_group_key* keys,
                          bmx_mgroup_rec* out, uint64_t cap, bmx_group_res* res, int mem);
int bmx_comm_where_group_multi(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                               uint32_t measure_field, uint32_t nkeys, const bmx_group_key* keys,
                               bmx_mgroup_rec* out, uint64_t cap, bmx_group_res* res);

#ifdef __cplusplus
}
#endif
#endif
