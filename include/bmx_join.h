/* bmx_join.h — lookup joins: bmx_where_join_group, bmx_where_map_group and their sharded forms. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it
 * next to bmx.h. It brings bmx_where.h (the program: bmx_lit) and bmx_group.h (the records: bmx_group_rec, bmx_agg) with it.
 *
 * What it is for: an aggregate grouped by an attribute of a LINKED node. "Revenue by the customer's country, over the paid orders of active customers", "posts
 * per author's team". bmx_where_semijoin crosses an edge but only tests existence: nothing is carried over from the inner node. bmx_where_group groups, but only
 * by a field of the selected node itself. Here one program builds a map M (key -> attribute) on the device, and a second program's selection is grouped by the
 * attribute its link value maps to; no list leaves the device in between.
 *
 * The map M.
 *   bmx_where_join_group: over the nodes the INNER program (in_base_field, in_nclauses, in_clause_len, in_lits) selects. The inner program is a bmx_scan_where
 *     program over in_base_field's dense index. An inner node whose key_field row is absent or tombstoned counts in res->n_inner only. Otherwise its key is in M
 *     and it counts in res->n_keyed. The attribute of a key is the MINIMUM of the attr_field data values over the selected inner nodes that hold that key; a key
 *     none of whose nodes holds attribute data is in M with "no attribute". (The minimum is independent of order and is one memory-side atomic; together with
 *     n_keyed - map_size it lets a caller who expects unique keys see that they were not.) key_field or attr_field equal to in_base_field reads the column and
 *     costs no probe; attr_field == key_field reuses the key; anything else costs one probe per selected inner node, made after the match is known.
 *   bmx_where_map_group: M is the `npairs` (1..BMX_JOIN_MAX_MAP) pairs (keys[i], vals[i]) given; npairs takes the place of map_cap, so this form never overflows
 *     the map. A pair whose key is outside +-(2^53 - 1) is skipped and not counted (no row holds such a value; INT64_MIN is the table's empty word). A val
 *     outside +-(2^53 - 1) means "no attribute" (INT64_MAX is the table's word for it). Duplicate keys take the minimum of their in-domain vals.
 *     res->n_inner == res->n_keyed == the pairs counted.
 * Selection and grouping: the OUTER program (base_field, nclauses, clause_len, lits) selects exactly as bmx_scan_where does. Every selected node lands in exactly
 *   one of three places:
 *     res->unmatched : its link_field row is absent or tombstoned, or its value is not a key of M;
 *     res->absent    : the key is in M with no attribute;
 *     the record of the key's attribute value.
 *   res->total aggregates every selected node. Always: sum of the records + absent + unmatched == total, for n_match, n and the 128-bit sum.
 *   measure_field behaves as in bmx_where_group, BMX_AGG_NO_FIELD included. link_field == base_field reads the column and costs no probe; any other link_field
 *   costs one probe per selected node.
 * The answer: exactly bmx_where_group's. Let D be the number of distinct attribute values among the selected nodes.
 *   D <= cap: res->n_groups == D, out[0 .. D) holds one record per value, nothing is written at or beyond out[D]. With BMX_MEM_HOST the records are sorted
 *     ascending by key; with BMX_MEM_DEVICE they come in any order.
 *   D > cap: BMX_JOIN_GROUP_OVERFLOW, res->n_groups is a lower bound of D above cap, `out` is not written at all; absent, unmatched and total are still exact.
 *   More than map_cap (1..BMX_JOIN_MAX_MAP) distinct keys: BMX_JOIN_MAP_OVERFLOW (and never BMX_JOIN_GROUP_OVERFLOW with it: no node is grouped). `out` is not
 *     written, n_groups is 0, absent, unmatched and total are empty records (n_match 0, min INT64_MAX, max INT64_MIN, sum 0), n_inner and n_keyed are exact and
 *     map_size is a lower bound above map_cap.
 *   The context keeps a map of max(64, next power of two >= 2 * map_cap) 16-byte {key, attribute} pairs for the largest map_cap asked so far and 2 * map_cap words
 *   of staging; the records are aggregated in bmx_where_group's table (cap 1..BMX_GROUP_MAX_CAP).
 * mem: BMX_MEM_HOST is synchronous; keys and vals are then host arrays. BMX_MEM_DEVICE takes out, res, keys and vals as device pointers and only enqueues: the
 *   group sweep reads the map's overflow state on the device, so no host round trip lies anywhere, and res is written fully by the call's last kernel, in stream
 *   order. An ordinary entry point: it orders behind a deferred compaction, sees the last merge, works after a growth and on an index that has switched to its
 *   int64 column, on either side.
 * Value-ordered views: with a view on base_field or in_base_field the call still takes the column path and leaves the view's bookkeeping untouched.
 * BMX_ERR_INVALID, before any device work and without writing anything: every refusal of bmx_scan_where's program, for either program (the text says "outer
 *   program" or "inner program"); res NULL; out NULL; cap outside 1..BMX_GROUP_MAX_CAP; map_cap or npairs outside 1..BMX_JOIN_MAX_MAP; keys or vals NULL;
 *   link_field, key_field or attr_field == BMX_AGG_NO_FIELD; a bad mem; a NULL context / communicator.
 * The sharded forms (host memory). A key may be held by inner nodes of several shards, and the node that links to it may live on yet another: M has to be the
 *   union. Phase 1 (bmx_comm_where_join_group alone): every shard builds its own map with the caller's map_cap and exports its pairs, all shards enqueued before
 *   the first list is fetched; the lists are united on the host (sorted by key, the minimum of the attributes of equal keys); n_inner and n_keyed add up.
 *   BMX_JOIN_MAP_OVERFLOW if any shard overflowed or the union has more than map_cap keys; map_size is then the largest lower bound known. Phase 2: the union
 *   goes to every shard as bmx_where_map_group's pairs do, every shard's sweep is enqueued before the first answer is fetched, and the shards' sorted record
 *   lists merge by key as bmx_comm_where_group's do; absent, unmatched and total fold the same way. BMX_JOIN_GROUP_OVERFLOW if any shard overflowed or the
 *   record union has more than cap keys. bmx_comm_where_map_group is phase 2 alone. */
#ifndef BMX_JOIN_H
#define BMX_JOIN_H
#include "bmx.h"
#include "bmx_where.h"
#include "bmx_group.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_join_res {
  uint64_t n_groups;   /* distinct attribute values among the selected outer nodes (a lower bound > cap on BMX_JOIN_GROUP_OVERFLOW; 0 on BMX_JOIN_MAP_OVERFLOW) */
  uint64_t map_size;   /* distinct keys in the map (a lower bound > map_cap on BMX_JOIN_MAP_OVERFLOW) */
  uint64_t n_inner;    /* join_group: inner nodes selected, key present or not; map_group: listed pairs whose key is inside +-(2^53-1) */
  uint64_t n_keyed;    /* of those, the ones whose key row holds data: n_keyed - map_size = inner nodes that share a key with another */
  uint32_t flags;      /* BMX_JOIN_MAP_OVERFLOW | BMX_JOIN_GROUP_OVERFLOW */
  uint32_t reserved;   /* 0 */
  bmx_agg absent, unmatched, total;
} bmx_join_res;        /* 184 bytes */
#define BMX_JOIN_MAP_OVERFLOW   1u
#define BMX_JOIN_GROUP_OVERFLOW 2u
#define BMX_JOIN_MAX_MAP (1u << 20)

int bmx_where_join_group(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                         uint32_t link_field, uint32_t measure_field,
                         uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits,
                         uint32_t key_field, uint32_t attr_field, uint64_t map_cap,
                         bmx_group_rec* out, uint64_t cap, bmx_join_res* res, int mem);
int bmx_where_map_group(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                        uint32_t link_field, uint32_t measure_field, const int64_t* keys, const int64_t* vals, uint64_t npairs,
                        bmx_group_rec* out, uint64_t cap, bmx_join_res* res, int mem);
int bmx_comm_where_join_group(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                              uint32_t link_field, uint32_t measure_field,
                              uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits,
                              uint32_t key_field, uint32_t attr_field, uint64_t map_cap,
                              bmx_group_rec* out, uint64_t cap, bmx_join_res* res);
int bmx_comm_where_map_group(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                             uint32_t link_field, uint32_t measure_field, const int64_t* keys, const int64_t* vals, uint64_t npairs,
                             bmx_group_rec* out, uint64_t cap, bmx_join_res* res);

#ifdef __cplusplus
}
#endif
#endif
