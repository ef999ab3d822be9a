/* bmx_update.h — update and delete by query: bmx_where_update and bmx_comm_where_update. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next to
 * bmx.h. It brings bmx_where.h (the program: bmx_lit) with it.
 *
 * What it replaces in the reference: filter(...) / map(path, fn) followed by one put per node ("set status = archived on every order older than X that is not
 * paid", "delete the session field of every banned user", "copy price into last_price", "add 1 to strikes for the users selected by ..."). With the calls that
 * were here before, the ids of the selection go down to the host (bmx_scan_where), come up again for bmx_get_rows of the source field, and go up a second time
 * with bmx_merge_batch or bmx_put_rows. bmx_where_update selects, computes and writes in one call; no id list leaves the device.
 *
 * Selection, universe, order: exactly bmx_where_rows's (bmx_rows.h) — the same program, the same candidates (the positions of base_field's dense index whose
 *   row holds data), taken in position order of base_field's index columns. Positions in front of start_pos are not candidates and are never probed.
 * Snapshot: the selection and every source value are taken from the state BEFORE the call, also when target_field is base_field, a field of the program, or
 *   src_field ("add 1 to x where x < 5" adds 1 once to every node that had x < 5). Each node appears at most once, so the batch the call hands to the merge has
 *   no duplicate keys by construction.
 * The record of a node is {id, target_field, ts, val}. val is `operand` (BMX_UPD_SET), BMX_VAL_DELETED (BMX_UPD_DELETE), the value of src_field on the same
 *   node (BMX_UPD_COPY) or that value + operand (BMX_UPD_ADD). With src_field == base_field the value comes from the index column without a probe; a selected
 *   row holds data, so such a node is never counted in n_nosrc. A selected node whose src_field holds no data (absent or tombstone) is counted in n_nosrc, one
 *   whose sum leaves +-(2^53 - 1) in n_range; neither is ever written. What remains are the WRITABLE nodes. src_field and operand are ignored where the op does
 *   not read them (SET: src_field; DELETE: both; COPY: operand).
 * Default mode (flags == 0): the state afterwards is what bmx_merge_batch(ids, target_field, ts, vals, BMX_INSERT_DELTA) would leave: the lexicographic
 *   maximum of (ts, val) wins, a tombstone loses to ts >= its clock, an absent row is created with clock ts.
 * BMX_UPD_FORCE: the state afterwards is what bmx_put_rows would leave: every record is stored as given. That is the only way to a tombstone:
 *   BMX_UPD_DELETE without BMX_UPD_FORCE is BMX_ERR_INVALID.
 * What follows the write: maintained indexes, value-ordered views and standing queries follow through the change log, as after any merge.
 * out_ids: optional (NULL: not wanted), capacity cap. It receives the ids of the n_applied nodes whose row changed, in index order. Nothing is written at or
 *   behind n_applied.
 * cap: at most cap records are handed to the merge, the first cap writable nodes from the cursor on. cap == 0 counts and seeks and writes nothing (out_ids is
 *   not looked at; next_pos is then the position of the first writable node). cap > BMX_UPD_MAX_CAP (the merge's batch limit) is BMX_ERR_INVALID.
 * Paging: as in bmx_where_rows: pass res.next_pos (and next_shard) as the next start_pos (start_shard). The pages of one layout add up to the one-shot call,
 *   because the program is evaluated per node and a node's fields are only ever written by its own record. A growth of the table during the merge lays the index
 *   out anew: the NEXT page's res.layout then differs from the previous one's (the stamp is taken before the write) and the caller starts over. Starting over is
 *   harmless for SET, DELETE and COPY from another field — the same records are produced again and lose or tie. It is NOT harmless for BMX_UPD_ADD onto its own
 *   source (target_field == src_field): the nodes of the pages already done would be added to a second time. Reserve first (bmx_reserve(rows + n_match), with
 *   n_match from a cap == 0 call), so that no page grows the table; the Python helper Engine.where_update_all does exactly that. (A context with more indexes
 *   than the change log maintains — eight — rebuilds a stale index at its next use, so there every write ends the layout and pages cannot be chained.)
 * Synchronisation and mem: the call is NOT enqueue-only, whatever mem says. The merge's grid, its workspace and a possible growth of the table are sized on the
 *   host by the batch size, so the call downloads the counts once between the emit pass and the merge and waits there for the stream. mem only says where
 *   out_ids and res live: BMX_MEM_HOST: host memory, complete on return. BMX_MEM_DEVICE: device memory, written by the call's last kernel and valid after
 *   bmx_sync() or in stream order.
 * Errors after the device work began: what the merge can return (BMX_ERR_FULL on a BMX_CTX_FIXED_CAPACITY context that cannot take the batch, BMX_ERR_NOMEM);
 *   the table is then as it was before the call and res / out_ids are not written.
 * Refusals, before any device work and without writing anything: every refusal of bmx_scan_where's program -> BMX_ERR_INVALID; an unknown op or flag bit,
 *   BMX_UPD_DELETE without BMX_UPD_FORCE, cap > BMX_UPD_MAX_CAP -> BMX_ERR_INVALID; res NULL, a bad mem, a NULL context / communicator, for the comm form
 *   start_shard >= the number of shards -> BMX_ERR_INVALID; ts outside 0 .. 2^53 - 1 -> BMX_ERR_RANGE; |operand| > 2^53 - 1 for SET and ADD -> BMX_ERR_RANGE.
 * Cost: bmx_where_rows's mask pass (for COPY / ADD from a probed field with one more probe per selected node), an emit pass that probes the source again (the
 *   first pass keeps bits, not values) and writes one 32-byte record per node, one wait, the merge of n_sent records, and a gather of n_applied ids.
 * bmx_comm_where_update (host memory): a node's rows all live on the shard that owns its id, so every shard updates its own nodes. The shards are taken in
 *   order from the cursor on (the first from start_pos, the later ones from 0), each with the room that is left of cap; the counts are summed and a shard's ids
 *   land behind those of the shards before it. layout is the sum of ALL shards' stamps, next_shard / next_pos name the first writable node not sent, and are
 *   nshards - 1 and that shard's index size when all were, as in bmx_comm_where_rows. */
#ifndef BMX_UPDATE_H
#define BMX_UPDATE_H
#include "bmx.h"
#include "bmx_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMX_UPD_SET    0u   /* val = operand */
#define BMX_UPD_DELETE 1u   /* val = BMX_VAL_DELETED (a tombstone); needs BMX_UPD_FORCE */
#define BMX_UPD_COPY   2u   /* val = value of src_field on the same node */
#define BMX_UPD_ADD    3u   /* val = value of src_field on the same node + operand */
#define BMX_UPD_FORCE  1u   /* flags: store as given, like bmx_put_rows; default: through conflict resolution like bmx_merge_batch with BMX_INSERT_DELTA */
#define BMX_UPD_MAX_CAP (1ull << 24)   /* the merge's batch limit */

typedef struct bmx_upd_res {
  uint64_t n_match;    /* nodes the program selects at or behind the cursor, however small cap is */
  uint64_t n_nosrc;    /* of those: COPY/ADD whose src_field holds no data on the node (absent or tombstone): never written */
  uint64_t n_range;    /* of those: ADD whose result leaves +-(2^53 - 1): never written */
  uint64_t n_sent;     /* records handed to the merge = min(cap, n_match - n_nosrc - n_range) */
  uint64_t n_applied;  /* of those, the rows whose stored (ts, val) changed; with BMX_UPD_FORCE == n_sent */
  uint64_t n_rows;     /* resident rows after the call (bmx_merge_stats.n_rows) */
  uint64_t next_pos;   /* index position of the first writable node NOT sent; the index size when all were */
  uint64_t layout;     /* stamp of the index layout the positions refer to, taken BEFORE the write */
  uint32_t next_shard, reserved;   /* bmx_comm_where_update: shard of next_pos; 0 for a context. reserved: 0 */
} bmx_upd_res;         /* 72 bytes */

int bmx_where_update(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                     uint32_t target_field, uint32_t op, uint32_t src_field, int64_t operand, int64_t ts, uint32_t flags,
                     uint64_t start_pos, uint64_t cap, uint64_t* out_ids, bmx_upd_res* res, int mem);
int bmx_comm_where_update(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                          uint32_t target_field, uint32_t op, uint32_t src_field, int64_t operand, int64_t ts, uint32_t flags,
                          uint32_t start_shard, uint64_t start_pos, uint64_t cap, uint64_t* out_ids, bmx_upd_res* res);

#ifdef __cplusplus
}
#endif
#endif
