/* bmx_reach.h — graph traversal: bmx_where_reach, bmx_where_reach_from and their sharded forms. Additions to the C ABI of bmx.h (ABI 4, unchanged); include
 * it next to bmx.h. It brings bmx_where.h (the program: bmx_lit) with it.
 *
 * What it is for: the transitive query. "Everybody who reports to this manager, directly or not, with their level", "the whole thread below this post", "every
 * folder under this folder", "every part that goes into this assembly" — and the mirror image, "the chain of managers above these people". Every other query
 * form crosses at most one edge: bmx_where_semijoin and the lookup joins build one set or map and test a field against it once. Here the set grows level by
 * level on the device: a breadth-first closure over the edges link_field -> key_field of the nodes one program selects, with no list leaving the device between
 * two levels.
 *
 * Candidates. The EDGE program (base_field, nclauses, clause_len, lits) is a bmx_scan_where program: its universe is the positions of base_field's dense index
 *   whose row holds data, literal truth and limits as in bmx_where.h. The nodes it selects are the only nodes that can be reached and the only nodes that pass a
 *   value on.
 * Fields of an edge node. Of a selected node, link_field is what gets tested and key_field is what the node contributes once reached. Each of them is the column
 *   value when it equals base_field and costs no probe then; any other field costs one probe: the link once per selected node in the whole call, the key once per
 *   reached node in the whole call. BMX_AGG_NO_FIELD is refused for both.
 * Edge nodes and leaves. A selected node whose link row is absent or tombstoned is no edge node: it is never reached. A reached node whose key row is absent or
 *   tombstoned is in the answer and passes nothing on.
 * Definition. The answer is the least fixed point of
 *     level(v) = 0                                   for every seed value v,
 *     level(v) = min depth(x) over the edge nodes x with key(x) == v          otherwise,
 *     depth(x) = 1 + level(link(x))                  where that level is defined,
 *   and consists of the edge nodes with depth <= max_depth. Nothing in it depends on an order of evaluation.
 *   - A node on a cycle is reached once, at its first level.
 *   - A node with link == key is reached only from outside.
 *   - Seeds are VALUES, not nodes: a node whose key is a seed value is in the answer only if its own link is reached.
 *   - Swapping link_field and key_field walks the edges the other way (toward the ancestors in a parent-pointer forest) with no other change.
 * Seeds.
 *   bmx_where_reach: the values of seed_field on the nodes the SEED program (seed_base_field, seed_nclauses, seed_clause_len, seed_lits) selects. A seed node
 *     whose seed_field row is absent or tombstoned counts in res->n_seed and adds nothing, as in bmx_where_semijoin. seed_field == seed_base_field reads the
 *     column.
 *   bmx_where_reach_from: the `nvalues` values given (1..BMX_REACH_MAX_SET). Duplicates are allowed. A value outside +-(2^53 - 1) is no value any row can hold:
 *     it is skipped and not counted in res->n_seed, as in bmx_where_in.
 * Limits. max_depth is 1..BMX_REACH_MAX_DEPTH. set_cap is 1..BMX_REACH_MAX_SET and bounds, in both forms, the seeds plus every value the reached nodes
 *   contribute. `flags` must be 0.
 * BMX_REACH_MORE is set exactly when some value has level == max_depth: a frontier is then left unexplored and the closure may be incomplete. res->rounds is the
 *   largest depth delivered.
 * The answer. out_ids holds the ids of the answer in position order of base_field's index, out_depth their depths (1..max_depth) in the same order; at most
 *   `cap` of each are written and nothing at or beyond [min(n_match, cap)]. cap == 0 with both pointers NULL counts only. res->n_match is exact whatever cap is.
 * Overflow: more than set_cap distinct values. res->flags == BMX_REACH_OVERFLOW (BMX_REACH_MORE is cleared), res->n_match == 0 and res->rounds == 0,
 *   res->set_size is some number > set_cap that is a lower bound of the distinct values, res->n_seed and res->n_edges are still exact, and nothing is written to
 *   either buffer: the "commit only if it fits" rule of bmx_where_semijoin and the lookup joins.
 *   The context uses the lookup joins' map (max(64, next power of two >= 2 * set_cap) pairs for the largest cap asked so far) and 9 bytes per position of the
 *   largest index traversed so far.
 *
 * mem: BMX_MEM_HOST is synchronous; `values` is then a host array. BMX_MEM_DEVICE takes out_ids, out_depth, res and values as device pointers and only enqueues:
 *   all max_depth rounds are enqueued blind, a round with nothing to do returns at once on the device, res is written fully by the call's last kernel, and no
 *   host round trip lies anywhere in the call. An ordinary entry point: it orders behind a deferred compaction, sees the last merge, works after a growth and on
 *   an index that has switched to its int64 column. Value-ordered views are neither read nor touched.
 * Why a level is exact. The val word of the map carries a value's level and is lowered with an exact atomic minimum. A round r reaches a node only if its link
 *   is found with a level <= r - 1. Such a pair was complete when the previous kernel ended; linear probing never moves a key, so every slot on the walk to it
 *   was occupied before the round began; and whatever round r itself writes carries the level r or "none", which both fail the test. A stale or torn view of the
 *   round's own writes therefore cannot change an answer, and the lookups are plain loads.
 * BMX_ERR_INVALID, before any device work and without writing anything: every refusal of bmx_scan_where's program, for either program (the text says "edge
 *   program" or "seed program"); res NULL; set_cap, nvalues or max_depth out of range; values NULL; out_ids or out_depth NULL with cap > 0; nonzero flags;
 *   link_field or key_field == BMX_AGG_NO_FIELD, and seed_field == BMX_AGG_NO_FIELD in the program form ("no seed field"); a bad mem; a NULL context /
 *   communicator.
 * The sharded forms (host memory). A key may be held on another shard than the node that links to it, so the levels have to agree across the shards: the host
 *   steps the rounds. Every shard seeds and prepares; round r is enqueued on every shard; every shard exports the values of level r; the host unites them and
 *   subtracts what is known; more than set_cap values in the union is an overflow, also when no shard overflowed; an empty union or r == max_depth ends the loop;
 *   otherwise the union goes to every shard at level r. Every shard's answer is enqueued before the first one is fetched. Ids and depths are concatenated in
 *   shard order, as bmx_comm_scan_where's ids are; n_match and n_edges add up, n_seed adds up in the program form and is the list's own count in the list form,
 *   set_size is the union's size and rounds the maximum: bit for bit what one context holding the same rows gives. */
#ifndef BMX_REACH_H
#define BMX_REACH_H
#include "bmx.h"
#include "bmx_where.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_reach_res {
  uint64_t n_match;   /* nodes reached (depth >= 1), however small cap is; 0 on overflow */
  uint64_t set_size;  /* distinct values in the set at the end, seeds included; on overflow some number > set_cap, a lower bound */
  uint64_t n_seed;    /* program form: seed nodes selected (seed value present or not); list form: listed values inside +-(2^53-1), duplicates counted */
  uint64_t n_edges;   /* nodes the edge program selects whose link row holds data */
  uint32_t rounds;    /* the largest depth in the answer; 0 when nothing was reached and on overflow */
  uint32_t flags;     /* BMX_REACH_OVERFLOW | BMX_REACH_MORE */
} bmx_reach_res;      /* 40 bytes */
#define BMX_REACH_OVERFLOW  1u
#define BMX_REACH_MORE      2u
#define BMX_REACH_MAX_SET   (1u << 20)
#define BMX_REACH_MAX_DEPTH 255u

int bmx_where_reach(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                    uint32_t link_field, uint32_t key_field, uint32_t flags,
                    uint32_t seed_base_field, uint32_t seed_nclauses, const uint32_t* seed_clause_len, const bmx_lit* seed_lits, uint32_t seed_field,
                    uint32_t max_depth, uint64_t set_cap, uint64_t* out_ids, uint8_t* out_depth, uint64_t cap, bmx_reach_res* res, int mem);
int bmx_where_reach_from(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                         uint32_t link_field, uint32_t key_field, uint32_t flags, const int64_t* values, uint64_t nvalues,
                         uint32_t max_depth, uint64_t set_cap, uint64_t* out_ids, uint8_t* out_depth, uint64_t cap, bmx_reach_res* res, int mem);
int bmx_comm_where_reach(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                         uint32_t link_field, uint32_t key_field, uint32_t flags,
                         uint32_t seed_base_field, uint32_t seed_nclauses, const uint32_t* seed_clause_len, const bmx_lit* seed_lits, uint32_t seed_field,
                         uint32_t max_depth, uint64_t set_cap, uint64_t* out_ids, uint8_t* out_depth, uint64_t cap, bmx_reach_res* res);
int bmx_comm_where_reach_from(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                              uint32_t link_field, uint32_t key_field, uint32_t flags, const int64_t* values, uint64_t nvalues,
                              uint32_t max_depth, uint64_t set_cap, uint64_t* out_ids, uint8_t* out_depth, uint64_t cap, bmx_reach_res* res);

#ifdef __cplusplus
}
#endif
#endif
