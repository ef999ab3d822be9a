/* bmx_group_top.h — the first N nodes per group: bmx_where_group_top and its sharded form. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next
 * to bmx.h. It brings bmx_where.h (the program: bmx_lit) and bmx_rows.h (the cells: BMX_ROWS_TS, BMX_ROWS_NO_CLOCK, BMX_ROWS_MAX_FIELDS) with it.
 *
 * What it replaces in the reference: "the 3 latest messages of every conversation", "the 5 cheapest offers per product", "each user's last 10 logins with ip
 * and device" are a filter() followed by a host sort over every match (SQL: ROW_NUMBER() OVER (PARTITION BY g ORDER BY o) <= N). The first-node-per-group form
 * tells which ONE node comes first per group; bmx_where_top orders one global list and knows no groups. bmx_where_group_top answers, per distinct value of
 * group_field among the selected nodes, WHICH `per` nodes come first under a total order, in that order, and fetches fields of each, without an id list leaving
 * the device.
 *
 * Selection, universe, group value, contenders, order: word for word those of the first-node-per-group form. The program (`nclauses, clause_len, lits`) is
 *   bmx_scan_where's (bmx_where.h); a view on base_field is neither read nor touched. The group value is the value of group_field on the selected node (the
 *   column value when group_field is base_field, otherwise one probe made after the match is known); a selected node whose group value is absent or tombstoned
 *   counts in res->absent and in no group. Only the members of a group whose order cell holds data are CONTENDERS. The order is the value of order_field, then
 *   the node id as an UNSIGNED 64-bit number; with BMX_GTOP_DESC the value is descending and the id is STILL ascending. The order is total and knows nothing of
 *   index positions, rebuilds or shards. order_field may be base_field, group_field, a field of the program or a field the program does not name.
 *   BMX_AGG_NO_FIELD is refused for either field.
 * The groups: out[g] = {key, n_match, n, n_rows}, one per distinct group value among the selected nodes: n_match = the selected members, n = the contenders
 *   among them, n_rows = min(per, n).
 * The rows: out_rows[g * per + j] for j < out[g].n_rows are the group's first n_rows contenders in order, as (id, order value); for n_rows <= j < per the row
 *   is {BMX_GTOP_NO_NODE, BMX_VAL_DELETED}. With per == 1 row g is what the first-node-per-group form's record g holds.
 * Projection: out_val[f * cap * per + g * per + j] is the cell of fields[f] on the node of row j of group g, out_ts at the same index its clock (written only
 *   with BMX_ROWS_TS), with the three states of bmx_rows.h (data / tombstone / absent). A row without a node gets absent cells (BMX_VAL_DELETED,
 *   BMX_ROWS_NO_CLOCK). `fields` may name the base, group or order field and may repeat; nfields <= BMX_ROWS_MAX_FIELDS. With nfields == 0 out_val and out_ts
 *   are not looked at.
 * res: n_groups, total (every selected node), absent and n_ordered (the contenders of all groups) as in the first-node-per-group form; per echoes the argument;
 *   n_rows = sum of out[g].n_rows. Always: sum of out[g].n_match + absent == total, and sum of out[g].n == n_ordered.
 * The answer. Let D be the number of distinct group values among the selected nodes.
 *   D <= cap: res->n_groups == D, res->flags == 0; nothing is written at or beyond group D of `out`, at or beyond row D * per of out_rows or of any column.
 *   D > cap: res->flags == BMX_GTOP_OVERFLOW, res->n_groups is some number > cap that is a lower bound of D; out, out_rows, out_val and out_ts are not written
 *     at all; total, absent and n_ordered are still exact; res->n_rows is 0. The caller retries with more room or a narrower program.
 *   cap is 1..BMX_GTOP_MAX_CAP, per is 1..BMX_GTOP_MAX_PER, cap * per at most BMX_GTOP_MAX_ROWS. The context uses bmx_where_group's table (max(64, next power
 *     of two >= 2 * cap) slots of 56 bytes) plus 36 + 16 * per bytes per slot, and one or two 8-byte words per position of base_field's index (allocated by the
 *     first call, grown with the index).
 * mem: BMX_MEM_HOST is synchronous and sorts the groups ascending by key, their rows and cells with them. BMX_MEM_DEVICE takes out, out_rows, out_val, out_ts
 *   and res as device pointers and only enqueues: the order of the groups is unspecified, but block g of every array belongs to out[g]; res is written by the
 *   last kernel and nothing returns to the host between the kernels. An ordinary entry point: it orders behind a deferred compaction, sees the last merge,
 *   works after a growth and on an index that has switched to its int64 column.
 * BMX_ERR_INVALID, before any device work and without writing anything, each with a text of its own: every refusal of bmx_scan_where's program; res NULL; cap
 *   outside 1..BMX_GTOP_MAX_CAP; per outside 1..BMX_GTOP_MAX_PER; cap * per above BMX_GTOP_MAX_ROWS; out NULL; out_rows NULL; nfields above
 *   BMX_ROWS_MAX_FIELDS; fields NULL with nfields > 0; out_val NULL with nfields > 0; out_ts NULL with BMX_ROWS_TS and nfields > 0; flag bits other than
 *   BMX_ROWS_TS | BMX_GTOP_DESC; group_field or order_field == BMX_AGG_NO_FIELD; a bad mem; a NULL context / communicator.
 * bmx_comm_where_group_top (host memory): the program is prepared once and enqueued on every shard, with the caller's cap and per, before the first answer is
 *   fetched. A node's rows all live on the shard that owns its id, so the shards' sorted lists merge exactly by key: n_match and n add, the merged rows of a
 *   key are the first per of the union of the shards' rows under the order (no node beyond a shard's first per can be among the union's first per), and each
 *   row brings ITS shard's cells; n_rows is recomputed; total, absent and n_ordered add. BMX_GTOP_OVERFLOW if any shard overflowed or the union has more than
 *   cap keys; nothing is written to the outputs then, and n_groups is the largest lower bound known (the union's size when no shard overflowed). */
#ifndef BMX_GROUP_TOP_H
#define BMX_GROUP_TOP_H
#include "bmx.h"
#include "bmx_where.h"
#include "bmx_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_gtop_grp { int64_t key; uint64_t n_match; uint64_t n; uint64_t n_rows; } bmx_gtop_grp;   /* 32 bytes */
typedef struct bmx_gtop_row { uint64_t id; int64_t val; } bmx_gtop_row;                                     /* 16 bytes */
typedef struct bmx_gtop_res {
  uint64_t n_groups; uint32_t flags; uint32_t per;
  uint64_t total; uint64_t absent; uint64_t n_ordered; uint64_t n_rows;
} bmx_gtop_res;                                                                                             /* 48 bytes */
#define BMX_GTOP_DESC     2u                      /* flags of the call: the order value descending (next to BMX_ROWS_TS, 1u) */
#define BMX_GTOP_OVERFLOW 1u                      /* flags of bmx_gtop_res */
#define BMX_GTOP_NO_NODE  0xFFFFFFFFFFFFFFFFull   /* id of a row without a node: the table's reserved id */
#define BMX_GTOP_MAX_CAP  (1u << 20)
#define BMX_GTOP_MAX_PER  16u
#define BMX_GTOP_MAX_ROWS (1u << 22)              /* cap * per */

int bmx_where_group_top(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                        uint32_t group_field, uint32_t order_field, uint32_t per, uint32_t nfields, const uint32_t* fields, uint32_t flags,
                        uint64_t cap, bmx_gtop_grp* out, bmx_gtop_row* out_rows, int64_t* out_val, int64_t* out_ts, bmx_gtop_res* res, int mem);
int bmx_comm_where_group_top(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                             uint32_t group_field, uint32_t order_field, uint32_t per, uint32_t nfields, const uint32_t* fields, uint32_t flags,
                             uint64_t cap, bmx_gtop_grp* out, bmx_gtop_row* out_rows, int64_t* out_val, int64_t* out_ts, bmx_gtop_res* res);

#ifdef __cplusplus
}
#endif
#endif
