/* bmx_join_rows.h — join projection: bmx_where_join_rows, bmx_where_map_rows and their sharded forms. Additions to the C ABI of bmx.h (ABI 4, unchanged);
 * include it next to bmx.h. It brings bmx_rows.h (the outer side: program, columns, cursor) and bmx_join.h (the map: its limits and its overflow flag) with it.
 *
 * What it is for: a join that hands back ROWS. "The paid orders of active customers, each with its amount and date and with the customer's name, country and
 * tier." bmx_where_rows fetches fields of the selected node only; bmx_where_join_group crosses the edge but aggregates. Here one program builds a map M
 * (key -> inner NODE) on the device, and every row of a second program's selection comes with the id of the inner node its link value maps to and with the
 * requested fields of that node; no list leaves the device in between.
 *
 * The map M (key -> inner node).
 *   bmx_where_join_rows: built exactly as bmx_where_join_group builds its map — the same inner program (in_base_field, in_nclauses, in_clause_len, in_lits), the
 *     same n_inner / n_keyed / map_size, the same map_cap limits (1..BMX_JOIN_MAX_MAP), the same table size — but the word a key carries is the ID of the inner
 *     node. Where several selected inner nodes hold one key it carries the SMALLEST id, compared as unsigned 64-bit: independent of order, one memory-side
 *     minimum, and n_keyed - map_size still shows the sharing. The map is rebuilt on every call, so on every page; a caller who pages a lot takes the pairs once
 *     (a first page's out_in_ids, or a query of its own) and uses the list form.
 *   bmx_where_map_rows: M is the `npairs` (1..BMX_JOIN_MAX_MAP) pairs (keys[i], node_ids[i]) given; npairs takes the place of map_cap, so this form never
 *     overflows. A pair whose key is outside +-(2^53 - 1) or whose node id is BMX_JROWS_NO_NODE is skipped and not counted. Duplicate keys take the smallest id.
 *     res->n_inner == res->n_keyed == the pairs counted.
 * Selection, order, cursor, paging, cap == 0: bmx_where_rows's, on the OUTER program (base_field, nclauses, clause_len, lits).
 *   The default is a LEFT join: every selected outer node is delivered. A node whose link_field row is absent or tombstoned, or whose link value is not a key of
 *   M, gets out_in_ids = BMX_JROWS_NO_NODE and every inner cell in the absent state (BMX_VAL_DELETED, BMX_ROWS_NO_CLOCK).
 *   With BMX_JROWS_INNER in `flags` such nodes are not selected at all: they do not count in n_match, take no rank, and next_pos skips them (the link lookup is
 *   part of the mask pass).
 * Output: column-major with stride cap. out_ids, out_val[f * cap + r], out_ts[f * cap + r] for the outer node's `fields`: exactly bmx_where_rows's.
 *   out_in_ids[r] is the inner node's id; out_in_val[g * cap + r] / out_in_ts[g * cap + r] are the three-state cells (bmx_rows.h) of in_fields[g] read on the
 *   INNER node. 0..BMX_ROWS_MAX_FIELDS fields on either side, repeats allowed; `fields` may name base_field or link_field, in_fields may name key_field or
 *   in_base_field. BMX_ROWS_TS governs both clock buffers; without it neither is read or written. With n_in_fields == 0, out_in_ids alone is the join. Nothing is
 *   written in rows n_out .. cap of any column, nor beyond row cap.
 * The result record: n_match, n_out, next_pos, layout as bmx_rows_res (layout: the stamp of the OUTER base field's index layout); n_joined = of the delivered
 *   rows, those that have an inner node; map_size, n_inner, n_keyed as bmx_join_res.
 * Map overflow (more than map_cap distinct keys): BMX_JOIN_MAP_OVERFLOW in res->flags; no output column is written; n_match = n_out = n_joined = 0, next_pos =
 *   the index size, layout is filled; n_inner and n_keyed are exact, map_size is a lower bound above map_cap.
 * mem: BMX_MEM_HOST is synchronous, passes through staging columns of the context like bmx_where_rows, and takes keys / node_ids as host arrays. BMX_MEM_DEVICE
 *   takes every output, res, keys and node_ids as device pointers and only enqueues: the kernels read the map's overflow state on the device and res is complete
 *   when the call's last kernel has run. An ordinary entry point: it orders behind a deferred compaction, sees the last merge, works after a growth and on an
 *   index that has switched to its int64 column, on either side.
 * Value-ordered views: with a view on base_field or in_base_field the call still takes the column path and leaves the view's bookkeeping untouched.
 * Cost: the build (one sweep of the inner column, bmx_where_join_group's); bmx_where_rows's mask pass (with BMX_JROWS_INNER plus, per row the program selects,
 *   the link read and one map walk); then per delivered row its id, one probe per outer field, the link read, a walk of the map with one 16-byte load per step,
 *   and one probe per inner field keyed by the inner id.
 * BMX_ERR_INVALID, before any device work and without writing anything: every refusal of bmx_scan_where's program, for either program (the text says "outer
 *   program" or "inner program"); nfields or n_in_fields above BMX_ROWS_MAX_FIELDS; fields / in_fields NULL with a count > 0; unknown flag bits; res NULL; with
 *   cap > 0: out_ids or out_in_ids NULL, out_val / out_in_val NULL with fields on that side, out_ts / out_in_ts NULL with BMX_ROWS_TS and fields on that side;
 *   map_cap or npairs outside 1..BMX_JOIN_MAX_MAP; keys or node_ids NULL; link_field or key_field == BMX_AGG_NO_FIELD; a bad mem; a NULL context /
 *   communicator; for the comm forms start_shard >= the number of shards.
 * The sharded forms (host memory). Phase 1 (bmx_comm_where_join_rows alone): every shard builds its own map with the caller's map_cap and exports its (key, id)
 *   pairs, all shards enqueued before the first list is fetched; the host unites them by key with the smallest id; n_inner and n_keyed add up.
 *   BMX_JOIN_MAP_OVERFLOW if any shard overflowed or the union has more than map_cap keys; next_shard / next_pos are then the last shard and its index size.
 *   Phase 2: the union goes to every shard as the list form's pairs; the shards deliver in bmx_comm_where_rows's order and cursor (start_shard, start_pos,
 *   next_shard, the summed layout) the outer cells and out_in_ids; every shard's mask pass is enqueued before the first answer is fetched. Phase 3: an inner node
 *   lives on bmx_owner_of(inner id), usually another shard than the row that links to it, so the inner cells of the delivered rows are fetched through
 *   bmx_comm_get_rows's point reads, one request per inner field: not found is absent, found with BMX_VAL_DELETED is a tombstone with its clock.
 *   bmx_comm_where_map_rows is phases 2 and 3. */
#ifndef BMX_JOIN_ROWS_H
#define BMX_JOIN_ROWS_H
#include "bmx.h"
#include "bmx_rows.h"
#include "bmx_join.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_jrows_res {
  uint64_t n_match;    /* selected outer nodes at or behind the cursor (BMX_JROWS_INNER: of those, the joined ones), however small cap is */
  uint64_t n_out;      /* rows written = min(n_match, cap) */
  uint64_t next_pos;   /* as bmx_rows_res */
  uint64_t layout;     /* as bmx_rows_res: stamp of the OUTER base field's index layout */
  uint64_t n_joined;   /* of the n_out delivered rows, those that have an inner node (BMX_JROWS_INNER: == n_out) */
  uint64_t map_size;   /* as bmx_join_res */
  uint64_t n_inner;    /* as bmx_join_res */
  uint64_t n_keyed;    /* as bmx_join_res */
  uint32_t flags;      /* BMX_JOIN_MAP_OVERFLOW */
  uint32_t next_shard; /* comm forms: shard of next_pos; 0 for a context */
} bmx_jrows_res;       /* 72 bytes */
#define BMX_JROWS_INNER   2u                      /* in `flags`, next to BMX_ROWS_TS (1u): deliver only the outer nodes that have an inner node */
#define BMX_JROWS_NO_NODE 0xFFFFFFFFFFFFFFFFull   /* out_in_ids of a row without inner node: the table's reserved id */

int bmx_where_join_rows(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                        uint32_t link_field, uint32_t nfields, const uint32_t* fields,
                        uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits,
                        uint32_t key_field, uint32_t n_in_fields, const uint32_t* in_fields, uint64_t map_cap,
                        uint32_t flags, uint64_t start_pos, uint64_t cap,
                        uint64_t* out_ids, int64_t* out_val, int64_t* out_ts,
                        uint64_t* out_in_ids, int64_t* out_in_val, int64_t* out_in_ts, bmx_jrows_res* res, int mem);
int bmx_where_map_rows(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                       uint32_t link_field, uint32_t nfields, const uint32_t* fields,
                       const int64_t* keys, const uint64_t* node_ids, uint64_t npairs,
                       uint32_t n_in_fields, const uint32_t* in_fields,
                       uint32_t flags, uint64_t start_pos, uint64_t cap,
                       uint64_t* out_ids, int64_t* out_val, int64_t* out_ts,
                       uint64_t* out_in_ids, int64_t* out_in_val, int64_t* out_in_ts, bmx_jrows_res* res, int mem);
int bmx_comm_where_join_rows(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                             uint32_t link_field, uint32_t nfields, const uint32_t* fields,
                             uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits,
                             uint32_t key_field, uint32_t n_in_fields, const uint32_t* in_fields, uint64_t map_cap,
                             uint32_t flags, uint32_t start_shard, uint64_t start_pos, uint64_t cap,
                             uint64_t* out_ids, int64_t* out_val, int64_t* out_ts,
                             uint64_t* out_in_ids, int64_t* out_in_val, int64_t* out_in_ts, bmx_jrows_res* res);
int bmx_comm_where_map_rows(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                            uint32_t link_field, uint32_t nfields, const uint32_t* fields,
                            const int64_t* keys, const uint64_t* node_ids, uint64_t npairs,
                            uint32_t n_in_fields, const uint32_t* in_fields,
                            uint32_t flags, uint32_t start_shard, uint64_t start_pos, uint64_t cap,
                            uint64_t* out_ids, int64_t* out_val, int64_t* out_ts,
                            uint64_t* out_in_ids, int64_t* out_in_val, int64_t* out_in_ts, bmx_jrows_res* res);

#ifdef __cplusplus
}
#endif
#endif
