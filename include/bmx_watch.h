/* bmx_watch.h — standing queries: bmx_watch_* and bmx_comm_watch_*. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next to bmx.h.
 *
 * What it replaces: a client that keeps the answer of a query live (the reference's node.on(): src/bullet.js:227-250, 710-716 calls every listener of a path and of its parent with the
 * written value, and the listener filters on the host) had to run bmx_scan_where again after every batch of merges, pull the whole id list and diff two lists on the host. A watch keeps
 * the last answer on the device, one bit per position of the base field's dense index, and a poll hands back only the ids that ENTERED and LEFT the answer.
 *
 * Program: exactly a bmx_scan_where program (bmx_where.h): base_field, nclauses, clause_len, lits. It is checked and prepared once, by bmx_watch_create.
 * Committed set: a watch owns a set C of positions of base_field's index. C is empty at create.
 * Poll: brings the index up to date exactly as bmx_scan_where does (it orders behind a deferred compaction and sees the last merge), evaluates the program over the
 *   column — universe, literal truth, clamping and absence as in bmx_where.h — to the match set M, and writes
 *     entered = the ids of M \ C, left = the ids of C \ M, both in position order of base_field's index,
 *     res->n_entered, res->n_left (the TRUE counts, whatever the caps), res->n_match = |M|, res->flags.
 *   Nothing is written at or beyond entered[cap_entered] or left[cap_left].
 * Commit: if n_entered <= cap_entered and n_left <= cap_left the poll commits, C := M. Otherwise it sets BMX_WATCH_OVERFLOW, leaves C as it was (what the lists hold
 *   below their caps is then a prefix to be thrown away), and the next poll reports the same changes net of whatever happened since. A NULL list needs a cap of 0; a
 *   poll with both caps 0 and no change commits (trivially).
 * Net changes: a node that entered and left between two committed polls is in neither list; a value that changed inside the program's truth is in neither list.
 * What goes into `left`: a node whose base row was tombstoned, a node whose probed field was tombstoned under a positive literal, a node whose value moved out of
 *   range. A node created since the last poll gets an appended position and can only enter.
 * BMX_WATCH_RESET: the lists are relative to the EMPTY set — entered is all of M, left is empty, and the caller replaces its set with entered. C is emptied
 *   whenever base_field's index is laid out anew, because state keyed by position means nothing afterwards: after a growth of the table (bmx_reserve or a merge that
 *   rehashes), after a change log longer than the maintenance limit, after appended rows that did not fit the columns' head room, with more indexes than are
 *   maintained, and after bmx_index_drop followed by a rebuild. The first poll of a watch is a RESET poll too. The flag is reported by every poll until one commits.
 *   The switch of an index from its int32 to its int64 column moves no position and is no RESET.
 * Value-ordered views: with a view on base_field the poll takes the column path and leaves the view's bookkeeping untouched, as bmx_scan_where does.
 * mem: BMX_MEM_HOST is synchronous. BMX_MEM_DEVICE takes entered, left and res as device pointers and only enqueues: the overflow decision and the commit are made on
 *   the device.
 * BMX_ERR_INVALID, before any device work and without writing anything, with a NULL context / communicator too: every program error of bmx_scan_where
 *   (bmx_watch_create), a bad mem, a NULL watch_out or res, a NULL list with a non-zero cap. With a context: an unknown or destroyed watch id, and a watch beyond
 *   BMX_WATCH_MAX live ones. Destroyed ids are reused. bmx_destroy frees every watch.
 * bmx_comm_watch_* (host memory): one watch id is valid on every shard. A poll enqueues the comparison on all shards, then reads the shards' counts. If their sums fit
 *   the caps every shard writes its part of the lists, shard after shard (position order inside a shard), and commits; if not, no shard commits, nothing is written
 *   to the lists and BMX_WATCH_OVERFLOW is reported. res holds the sums; flags the OR of the shards' RESET bits — one shard may have been rebuilt alone, and its part of
 *   entered is then its whole match set. A node's rows all live on the shard that owns its id, so the union is the answer of one context holding the same rows. */
#ifndef BMX_WATCH_H
#define BMX_WATCH_H
#include "bmx_where.h"                 /* bmx_lit: a watch takes a bmx_scan_where program */

#ifdef __cplusplus
extern "C" {
#endif

#define BMX_WATCH_MAX      16u         /* live watches per context */
#define BMX_WATCH_RESET    1u
#define BMX_WATCH_OVERFLOW 2u
typedef struct bmx_watch_res { uint64_t n_entered, n_left, n_match; uint32_t flags, reserved; } bmx_watch_res;  /* 32 bytes */

int bmx_watch_create (bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t* watch_out);
int bmx_watch_poll   (bmx_ctx* ctx, uint32_t watch, uint64_t* entered, uint64_t cap_entered, uint64_t* left, uint64_t cap_left, bmx_watch_res* res, int mem);
int bmx_watch_destroy(bmx_ctx* ctx, uint32_t watch);
int bmx_comm_watch_create (bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t* watch_out);
int bmx_comm_watch_poll   (bmx_comm* comm, uint32_t watch, uint64_t* entered, uint64_t cap_entered, uint64_t* left, uint64_t cap_left, bmx_watch_res* res);
int bmx_comm_watch_destroy(bmx_comm* comm, uint32_t watch);

#ifdef __cplusplus
}
#endif
#endif
