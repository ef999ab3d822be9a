/* bmx_rows.h — row projection: bmx_where_rows and bmx_comm_where_rows. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next to bmx.h. It brings
 * bmx_where.h (the program: bmx_lit) with it.
 *
 * What it replaces in the reference: equals, range and filter return BulletNodes and the next thing a caller does is read .value(); map(path, fn)
 * (src/bullet-query.js:322-333) exists for nothing else. bmx_scan_where hands back ids; the fields of those nodes then cost the id list a trip to the host and
 * one bmx_get_rows per field with the same ids on their way back. bmx_where_rows selects and fetches in one call: the ids of the selected nodes and, per
 * requested field, a column of values (and clocks), without an id list leaving the device in between.
 *
 * Selection, universe, order: exactly bmx_scan_where's — the same program (`nclauses, clause_len, lits`; see bmx_where.h for literal truth, BMX_LIT_NOT,
 *   clamping and the limits), the same candidates (the positions of base_field's dense index whose row holds data), the answers in position order of
 *   base_field's index columns. Positions below start_pos are not candidates: their fields are never probed.
 * Output: column-major with stride cap. out_ids[r] is the id of the r-th delivered node, out_val[f * cap + r] the value of fields[f] on that node,
 *   out_ts[f * cap + r] its clock. One cell has three states:
 *       data       out_val = the value            out_ts = its clock
 *       tombstone  out_val = BMX_VAL_DELETED      out_ts = the tombstone's clock
 *       absent     out_val = BMX_VAL_DELETED      out_ts = BMX_ROWS_NO_CLOCK
 *   Without BMX_ROWS_TS out_ts is neither read nor written and may be NULL. `fields` may name base_field (without BMX_ROWS_TS that value comes from the column
 *   and costs no probe), may name fields of the program, and may repeat a field: every entry gets its own column. nfields == 0 delivers ids alone; the answer
 *   then equals bmx_scan_where's with the same cap. Nothing is written at or beyond row cap of any column, nor in rows n_out .. cap.
 * The result record: n_match = the selected nodes at or behind the cursor, however small cap is; n_out = min(n_match, cap) rows written; next_pos = the index
 *   position of the first selected node that was NOT delivered, the index size when all were; layout = the stamp of the index layout the positions refer to.
 * cap == 0: no output pointer is looked at; res is still filled, and next_pos is then the position of the first selected node: counting and seeking are the
 *   same call.
 * Paging: pass res.next_pos (and next_shard) of the previous page as start_pos (start_shard). The pages of one layout concatenate to the one-shot answer. A
 *   cursor is good only while res.layout does not change: if it differs from the previous page's, the index was laid out anew (a rebuild after a growth, say) and
 *   the caller starts over. Between two layouts a row keeps its position and new rows are appended. A start_pos at or beyond the index size selects nothing and
 *   returns next_pos = index size.
 * mem: BMX_MEM_HOST is synchronous. BMX_MEM_DEVICE takes out_ids, out_val, out_ts and res as device pointers and only enqueues; res is written by the last
 *   kernel, and no host round trip happens between the passes. An ordinary entry point: it orders behind a deferred compaction, sees the last merge, works after
 *   a growth and on an index that has switched to its int64 column.
 * Value-ordered views: with a view on base_field (bmx_index_set_ordered) the call still takes the column path and leaves the view's bookkeeping untouched.
 * Cost: one sweep of base_field's value column with the program's probes (bmx_scan_where's mask pass), then per delivered node one read of its id and one table
 *   probe per requested field. A field that the program already probed in the first pass is probed again in the second: the first pass keeps one bit per row,
 *   not values. A BMX_MEM_HOST answer passes through a staging buffer of the context (1 + nfields x (1 or 2) columns of min(cap, index size) rows, grown on
 *   demand) and is downloaded column by column.
 * BMX_ERR_INVALID, before any device work and without writing anything: every refusal of bmx_scan_where's program (nclauses outside 1..8, a clause_len of 0 or
 *   above 8, more than 32 literals, more than 8 fields besides base_field, unknown literal flag bits, clause_len or lits NULL); nfields above
 *   BMX_ROWS_MAX_FIELDS; fields NULL with nfields > 0; unknown flag bits; res NULL; with cap > 0: out_ids NULL, out_val NULL with nfields > 0, out_ts NULL with
 *   BMX_ROWS_TS and nfields > 0; a bad mem; a NULL context / communicator; for the comm form start_shard >= the number of shards.
 * bmx_comm_where_rows (host memory): the shards are taken in order from the cursor on, the first from start_pos, the later ones from 0; every shard's mask
 *   pass is enqueued before the first answer is fetched. A shard's rows land behind those of the shards before it, in the same columns of stride cap; shards
 *   that no longer fit are counted only. n_match is the sum of the shards' counts (shards in front of start_shard are not candidates); layout is the sum of ALL
 *   shards' stamps — each stamp only ever grows, so the sum changes when any of them does; next_shard / next_pos name the first node not delivered, and are
 *   nshards - 1 and that shard's index size when everything was delivered. A node's rows all live on the shard that owns its id, so every cell comes from the
 *   shard that selected the node. */
#ifndef BMX_ROWS_H
#define BMX_ROWS_H
#include "bmx.h"
#include "bmx_where.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_rows_res {
  uint64_t n_match;     /* selected nodes at or behind the cursor, however small cap is */
  uint64_t n_out;       /* rows written = min(n_match, cap) */
  uint64_t next_pos;    /* cursor of the next page: index position of the first selected node NOT delivered; the index size when all were */
  uint64_t layout;      /* stamp of the index layout the positions refer to; a cursor is good only while this does not change */
  uint32_t next_shard;  /* bmx_comm_where_rows: shard of next_pos; 0 for a context */
  uint32_t reserved;    /* 0 */
} bmx_rows_res;         /* 40 bytes */
#define BMX_ROWS_MAX_FIELDS 8u
#define BMX_ROWS_TS         1u          /* also deliver the clocks */
#define BMX_ROWS_NO_CLOCK   (-1)        /* out_ts of an absent row (clocks are >= 0) */

int bmx_where_rows(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                   uint32_t nfields, const uint32_t* fields, uint32_t flags, uint64_t start_pos, uint64_t cap,
                   uint64_t* out_ids, int64_t* out_val, int64_t* out_ts, bmx_rows_res* res, int mem);
int bmx_comm_where_rows(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                        uint32_t nfields, const uint32_t* fields, uint32_t flags, uint32_t start_shard, uint64_t start_pos, uint64_t cap,
                        uint64_t* out_ids, int64_t* out_val, int64_t* out_ts, bmx_rows_res* res);

#ifdef __cplusplus
}
#endif
#endif
