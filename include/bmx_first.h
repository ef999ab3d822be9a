/* bmx_first.h — the first node per group: bmx_where_group_first and its sharded form. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next to
 * bmx.h. It brings bmx_where.h (the program: bmx_lit) and bmx_rows.h (the cells: BMX_ROWS_TS, BMX_ROWS_NO_CLOCK, BMX_ROWS_MAX_FIELDS) with it.
 *
 * What it replaces in the reference: "the latest message of every conversation", "the cheapest offer per product", "one representative per category" are a
 * filter() followed by a host reduce over every match (SQL: DISTINCT ON / ROW_NUMBER() = 1). bmx_where_group tells the minimum and maximum of a measure per
 * discovered key but not the node that holds it; bmx_where_top orders one global list and knows no groups. bmx_where_group_first answers, per distinct value
 * of group_field among the selected nodes, WHICH node comes first under a total order, and fetches fields of that node, without an id list leaving the device.
 *
 * Selection, universe, candidates: exactly bmx_scan_where's (`nclauses, clause_len, lits`; see bmx_where.h). A view on base_field is neither read nor touched.
 * Group value: the value of group_field on the selected node: the column value when group_field is base_field, otherwise one probe made after the match is
 *   known. A selected node whose group value is absent or tombstoned counts in res->absent and in no record.
 * Order: by the value of order_field, then by node id as an UNSIGNED 64-bit number. With BMX_FIRST_DESC the value is descending and the id is STILL ascending
 *   (bmx_scan_top's order). The order is total and knows nothing of index positions, rebuilds or shards. Only the members of a group whose order cell holds
 *   data are CONTENDERS. order_field may be base_field, group_field, a field of the program or a field the program does not name. With order_field ==
 *   group_field every member ties and the answer is the smallest id: one representative per group. BMX_AGG_NO_FIELD is refused for either field.
 * The records: one per distinct group value among the selected nodes. n_match = the selected members, n = the contenders among them, id and val = the first
 *   contender and its order value; with n == 0 they are BMX_FIRST_NO_NODE and BMX_VAL_DELETED.
 * res: total = every selected node, absent as above, n_ordered = the contenders of all groups. Always: sum of out[i].n_match + absent == total, and sum of
 *   out[i].n == n_ordered.
 * Projection: out_val[f * cap + r] is the cell of fields[f] on node out[r].id, out_ts[f * cap + r] its clock (written only with BMX_ROWS_TS), with the three
 *   states of bmx_rows.h (data / tombstone / absent). A record without a node gets absent cells (BMX_VAL_DELETED, BMX_ROWS_NO_CLOCK). `fields` may name the
 *   base, group or order field and may repeat; nfields <= BMX_ROWS_MAX_FIELDS. With nfields == 0 out_val and out_ts are not looked at.
 * The answer. Let D be the number of distinct group values among the selected nodes.
 *   D <= cap: res->n_groups == D, res->flags == 0; nothing is written at or beyond row D of `out` or of any column.
 *   D > cap: res->flags == BMX_FIRST_OVERFLOW, res->n_groups is some number > cap that is a lower bound of D; out, out_val and out_ts are not written at all;
 *     total, absent and n_ordered are still exact. The caller retries with more room or a narrower program.
 *   cap is 1..BMX_FIRST_MAX_CAP. The context uses bmx_where_group's table (max(64, next power of two >= 2 * cap) slots of 56 bytes) plus one id word per
 *     slot, and one or two 8-byte words per position of base_field's index (allocated by the first call, grown with the index).
 * mem: BMX_MEM_HOST is synchronous and sorts the records ascending by key, their cells with them. BMX_MEM_DEVICE takes out, out_val, out_ts and res as device
 *   pointers and only enqueues: the order of the records is unspecified, but row r of every column belongs to out[r]; res is written by the last kernel and
 *   nothing returns to the host between the passes. An ordinary entry point: it orders behind a deferred compaction, sees the last merge, works after a growth
 *   and on an index that has switched to its int64 column.
 * BMX_ERR_INVALID, before any device work and without writing anything, each with a text of its own: every refusal of bmx_scan_where's program; res NULL; cap
 *   outside 1..BMX_FIRST_MAX_CAP; out NULL; nfields above BMX_ROWS_MAX_FIELDS; fields NULL with nfields > 0; out_val NULL with nfields > 0; out_ts NULL with
 *   BMX_ROWS_TS and nfields > 0; flag bits other than BMX_ROWS_TS | BMX_FIRST_DESC; group_field or order_field == BMX_AGG_NO_FIELD; a bad mem; a NULL
 *   context / communicator.
 * bmx_comm_where_group_first (host memory): the program is prepared once and enqueued on every shard, with the caller's cap, before the first answer is
 *   fetched. A node's rows all live on the shard that owns its id, so the shards' sorted lists merge exactly by key: n_match and n add, the better (val, id)
 *   under the order wins and brings ITS shard's cells; total, absent and n_ordered add. BMX_FIRST_OVERFLOW if any shard overflowed or the union has more than
 *   cap keys; nothing is written to the outputs then, and n_groups is the largest lower bound known (the union's size when no shard overflowed). */
#ifndef BMX_FIRST_H
#define BMX_FIRST_H
#include "bmx.h"
#include "bmx_where.h"
#include "bmx_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_first_rec { int64_t key; uint64_t id; int64_t val; uint64_t n_match; uint64_t n; } bmx_first_rec;   /* 40 bytes */
typedef struct bmx_first_res {
  uint64_t n_groups; uint32_t flags; uint32_t reserved;
  uint64_t total; uint64_t absent; uint64_t n_ordered;
} bmx_first_res;                                                                                                       /* 40 bytes */
#define BMX_FIRST_DESC     2u                      /* flags of the call: the order value descending (next to BMX_ROWS_TS, 1u) */
#define BMX_FIRST_OVERFLOW 1u                      /* flags of bmx_first_res */
#define BMX_FIRST_NO_NODE  0xFFFFFFFFFFFFFFFFull   /* id of a record without a contender: the table's reserved id, as BMX_JROWS_NO_NODE */
#define BMX_FIRST_MAX_CAP  (1u << 20)

int bmx_where_group_first(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                          uint32_t group_field, uint32_t order_field, uint32_t nfields, const uint32_t* fields, uint32_t flags,
                          uint64_t cap, bmx_first_rec* out, int64_t* out_val, int64_t* out_ts, bmx_first_res* res, int mem);
int bmx_comm_where_group_first(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                               uint32_t group_field, uint32_t order_field, uint32_t nfields, const uint32_t* fields, uint32_t flags,
                               uint64_t cap, bmx_first_rec* out, int64_t* out_val, int64_t* out_ts, bmx_first_res* res);

#ifdef __cplusplus
}
#endif
#endif
